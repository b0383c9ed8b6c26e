/*
 * p3d.h -- C ABI of the MI355X-native 2D->3D pose-lifting MLP (libp3d.so).
 *
 * This is the drop-in boundary for the hot path of EsauPR/3d-pose-baseline:
 * the TF1 graph of src/linear_model.py (LinearModel.__init__ :34-151,
 * two_linear :154-201, step :203-245) and the MPJPE arithmetic of
 * src/predict_3dpose.py:evaluate_batches (:352-444).  The reference has no
 * FFI of its own (it is 100% Python over TensorFlow); each entry point below
 * replaces the TensorFlow op group named in its comment, and the Python host
 * (3d-pose-baseline_amd/linear_model.py) binds them through ctypes exactly as
 * INTEGRATION.md shows.
 *
 * Conventions
 *   - Plain C: int status return (P3D_OK = 0), message via p3d_last_error().
 *   - The library owns parameters, optimizer slots and workspace (device memory).
 *     The caller owns every I/O buffer passed in; all I/O pointers are DEVICE
 *     pointers, row-major, fp32 unless stated.
 *   - `stream` is a hipStream_t passed as void* (NULL = legacy default stream).
 *     Every call is asynchronous on that stream.
 *   - One model handle per stream/thread; calls on one handle are not thread-safe.
 */
#ifndef P3D_H_
#define P3D_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_OK 0
#define P3D_ERR_ARG 1      /* bad argument / shape (TF: InvalidArgumentError) */
#define P3D_ERR_HIP 2      /* HIP runtime failure                            */
#define P3D_ERR_STATE 3    /* call out of order (e.g. backward before fwd)   */
#define P3D_ERR_NOTFOUND 4 /* unknown parameter name                         */

/* p3d_forward ctr value meaning "use the device-resident global_step" (graph-capturable) */
#define P3D_CTR_GLOBAL_STEP 0xFFFFFFFFFFFFFFFFull

#define P3D_DTYPE_F32 0
#define P3D_DTYPE_BF16 1   /* bf16 weights/activations, fp32 accumulate + BN */
#define P3D_DTYPE_F64 2    /* float64 (data-pipeline entry points only)            */

typedef struct p3d_cfg {
  int32_t linear_size;  /* LinearModel(linear_size)            linear_model.py:35 */
  int32_t num_layers;   /* number of two_linear blocks          linear_model.py:36 */
  int32_t residual;     /* two_linear residual add              linear_model.py:199 */
  int32_t batch_norm;   /* tf.layers.batch_normalization        linear_model.py:112 */
  int32_t max_norm;     /* tf.clip_by_norm(w, 1)                linear_model.py:108 */
  int32_t input_size;   /* HUMAN_2D_SIZE = 32                   linear_model.py:62  */
  int32_t output_size;  /* HUMAN_3D_SIZE = 48 (42 if predict_14) linear_model.py:72 */
  int32_t dtype;        /* P3D_DTYPE_*                                              */
  int32_t max_batch;    /* largest B any call will use (workspace sizing)           */
  float bn_eps;         /* 1e-3 (TF default)                                        */
  float bn_momentum;    /* 0.99 (TF default)                                        */
} p3d_cfg;

typedef struct p3d_model p3d_model;

/* Last error message of the calling thread ("" if none). */
const char* p3d_last_error(void);

/* Build a model: allocates trainables (TF creation order), BN moving stats,
 * Adam slots, gradients and activation workspace.  Replaces the variable
 * creation + tf.global_variables_initializer of linear_model.py:84-151
 * (values are zero/one; the host writes kaiming weights via p3d_param_ptr). */
int p3d_create(const p3d_cfg* cfg, p3d_model** out);
int p3d_destroy(p3d_model* m);

/* Parameter table.  Names are TF1 variable names, e.g. "linear_model/w1",
 * "linear_model/two_linear_0/batch_normalization10/moving_mean".  Weights are
 * stored [in, out] row-major exactly like the TF variables (linear_model.py:103).
 * kind: 0 = trainable, 1 = BN moving statistic.  Indexing is 0..count-1. */
int p3d_param_count(const p3d_model* m, int32_t* count);
int p3d_param_info(const p3d_model* m, int32_t idx, const char** name, int64_t* numel,
                   int32_t* kind, int64_t* offset);
int p3d_param_ptr(p3d_model* m, const char* name, void** dptr, int64_t* numel);

/* Flat device buffers (trainables in TF order, 256-byte aligned segments):
 * params/grads/adam_m/adam_v share one layout; `numel` is the padded length.
 * grads is what data-parallel training all-reduces. */
int p3d_flat_ptr(p3d_model* m, int32_t which /*0 params,1 grads,2 adam_m,3 adam_v,4 moving*/,
                 void** dptr, int64_t* numel);

/* Must be called after the host writes parameters through p3d_param_ptr /
 * p3d_flat_ptr (refreshes derived device layouts, e.g. transposed weights). */
int p3d_params_updated(p3d_model* m, void* stream);

/* Bring the TF-layout weight masters (params buffer, p3d_param_ptr) up to date on `stream`.
 * The optimizers of a model without --max_norm read each weight from its packed data-gradient
 * copy and do not write the TF-layout master (4 of the 32 bytes per weight element of the fused
 * step's optimizer); call this before the host reads or writes weights through
 * p3d_param_ptr / p3d_flat_ptr(0).  No device work when the masters are current.
 * p3d_params_updated refuses (P3D_ERR_STATE) while they are behind. */
int p3d_params_sync(p3d_model* m, void* stream);

/* The parameters changed on the device without this library's host code issuing the change
 * (e.g. a replayed HIP graph of training steps, LinearModel.step's cached training graph):
 * host-scheduled derived tables (k_serve6's epilogue constants) are re-formed at their next
 * use.  Host-only, no device work.  Replaces nothing in the reference (TF re-reads variables
 * on every session.run). */
int p3d_params_changed(p3d_model* m);

/* Forward pass: y[B, output_size] = MLP(x[B, input_size]).
 *   training=0: BN uses moving statistics (isTraining=False, linear_model.py:239-245);
 *               at B <= 4 (env P3D_GEMV_MAXB) every layer is a weight-streaming GEMV kernel
 *               (the per-frame step of src/openpose_3dpose_sandbox.py:353-356); results
 *               equal the MFMA path's to fp32 rounding, rows independent of B.
 *   training=1: BN uses batch statistics, updates the moving averages
 *               (UPDATE_OPS, linear_model.py:138-140) and caches activations
 *               for p3d_backward.  Requires B <= max_batch.
 *   keep_prob:  tf.nn.dropout keep probability (1 = identity); the mask is
 *               Philox4x32-10 keyed by (seed, ctr, site, row_offset + row, col).
 * Replaces the forward ops of linear_model.py:103-128. */
int p3d_forward(p3d_model* m, const float* x, int64_t B, float* y, int32_t training,
                float keep_prob, uint64_t seed, uint64_t ctr, int64_t row_offset, void* stream);

/* p3d_forward on workspace rows [ws_row, ws_row + B) (ws_row a multiple of 16,
 * inference only): independent batches issued on different streams with disjoint
 * workspace rows run concurrently; results are bit-identical to p3d_forward. */
int p3d_forward_ex(p3d_model* m, const float* x, int64_t B, float* y, int32_t training,
                   float keep_prob, uint64_t seed, uint64_t ctr, int64_t row_offset, int64_t ws_row,
                   void* stream);

/* Evaluation forward of B rows as ceil(B/64) independent batch-64 steps -- the
 * per-batch LinearModel.step(isTraining=False) loop of predict_3dpose.py:evaluate_batches
 * (:352-444, step at :396) -- in ONE persistent launch (k_serve): each XCD runs whole
 * steps (all layers) out of its own L2, steps dealt round-robin over the XCDs.  Eval BN,
 * keep_prob 1; x [B, input_size], y [B, output_size] device pointers.  fp32 models with
 * linear_size % 128 == 0, input_size <= 64, output_size <= 64, at most 7 blocks.
 * Results equal p3d_forward's to fp32 rounding (the output layer sums 32-column partials
 * in fixed order; deterministic).  The launch is one workgroup per CU and needs all of
 * them resident together: do not run two p3d_serve launches concurrently on one device
 * (other kernels merely delay it).  A launch whose workgroups could not all synchronise
 * stops within ~0.5 s and is reported by the next p3d_serve_check (P3D_ERR_HIP). */
int p3d_serve(p3d_model* m, const float* x, int64_t B, float* y, void* stream);
/* p3d_serve with the evaluation loss of src/linear_model.py:129 (the `loss` output of the eval
 * step(), :239-245) fused into the launch: *loss = mean((y - t)^2) over B x output_size, t [B,
 * output_size] row-major.  x, y, t and loss may be pinned (mapped) host memory: the kernel reads
 * and writes them directly, so LinearModel.step(isTraining=False) is ONE launch from numpy.
 * B <= 4 (the batch-1 front end's evaluation): the persistent small-batch forward p3d_forward
 * runs at that batch, its last output workgroup reducing the loss -- y then has p3d_forward's
 * bits and *loss p3d_mse's on that y; it shares workspace slot 0 with the model's other batch
 * <= 4 calls, so keep those on one stream.  P3D_ERR_ARG where no form covers the launch (> 32
 * batch-64 steps, or a model shape it is not built for): the caller uses p3d_serve + p3d_mse
 * there. */
int p3d_serve_mse(p3d_model* m, const float* x, int64_t B, float* y, const float* t, float* loss, void* stream);
/* p3d_serve_mse that returns once y and *loss hold the results, for outputs in pinned host memory
 * (the reference's session.run returns its fetches: src/linear_model.py:239-245).  The launch's last
 * output tile stores the call's sequence number into a pinned completion word after every row and
 * the loss are system-visible, and the host waits on that word rather than on the runtime's
 * completion signal; the stream itself is not synchronised (later work on it is ordered behind the
 * launch).  Not capturable (P3D_ERR_STATE on a capturing stream).  Errors as p3d_serve_mse, plus
 * P3D_ERR_HIP when the launch ends without storing the word or when a kernel's error word is set
 * (p3d_error_flags reports which). */
int p3d_serve_mse_sync(p3d_model* m, const float* x, int64_t B, float* y, const float* t, float* loss, void* stream);
/* 0 if every p3d_serve launch so far completed its synchronisation (synchronises the device,
 * then reads the kernels' pinned error word).  After a failure p3d_serve refuses new launches
 * (P3D_ERR_HIP) until this call reports it once; the failed launch's rows hold NaN, never
 * unwritten or stale values.  NaN rows alone do not mean failure: a non-finite input row gives a
 * NaN output row (and a NaN loss) on every path, as in the reference, with the error words clean
 * -- NaN rows with a set error word are a failed launch, NaN rows without one are bad input.
 * k_serve6 launches pick their sync-word bank on the device, so a
 * captured p3d_serve replays correctly (its epilogue-constant table is re-formed in the graph). */
int p3d_serve_check(p3d_model* m);

/* 0 if every BN-train exchange so far completed (synchronises, then reads the pinned error word).
 * Training layers with batch norm run as one launch each whose row-tile workgroups swap their
 * column statistics inside the launch; a spin that ran out (workgroups not
 * co-resident, e.g. another persistent kernel holding CUs) sets a word this reports once, as
 * P3D_ERR_HIP. */
int p3d_sync_check(p3d_model* m);

/* The kernels' error words without any device round trip or synchronisation: they live in
 * pinned, mapped host memory the kernels write directly, so a caller reads them after a
 * synchronisation it makes anyway (a loss read, an output copy).  *flags: bit 0 a BN-train
 * exchange timed out, bit 1 a p3d_serve spin ran out, bit 2 a p3d_serve placement the launch
 * was not sized for.  clear != 0 resets what was reported (a serve error also re-zeroes the
 * serve sync words, which synchronises).  Replaces no reference interface: TF raised op
 * errors from session.run (src/linear_model.py:236,244). */
int p3d_error_flags(p3d_model* m, int32_t* flags, int32_t clear);

/* MSE loss of linear_model.py:129 and its gradient: loss = mean((y-t)^2) over
 * B*D, dy = (1/(B*D)) * 2*(y-t).  loss_dev: one device float (may be NULL),
 * dy may be NULL. */
int p3d_mse(const float* y, const float* t, int64_t B, int32_t D, float* loss_dev, float* dy,
            void* stream);

/* Backward pass of the last training forward: gradients of every trainable
 * into the flat grads buffer (opt.compute_gradients, linear_model.py:143). */
int p3d_backward(p3d_model* m, const float* dy, int64_t B, void* stream);

/* p3d_forward(training = 1, ctr = P3D_CTR_GLOBAL_STEP) + p3d_mse + p3d_backward in one
 * call (session.run of the train op up to compute_gradients, linear_model.py:129,143):
 * x [B,32], t [B,48] device row-major, 1 <= B <= max_batch; outputs y [B,48]; loss_dev = mean((y-t)^2);
 * gradients in the flat grads buffer.  The MSE runs in the output layer's epilogue. */
int p3d_train_fwd_bwd(p3d_model* m, const float* x, const float* t, int64_t B, float* y,
                      float keep_prob, uint64_t seed, int64_t row_offset, float* loss_dev,
                      void* stream);

/* Gradient-ready buckets for a data-parallel all-reduce that overlaps the backward (the DP
 * form of opt.compute_gradients -> apply_gradients, linear_model.py:143-145).
 * p3d_grad_buckets(m, n, lowest): bucket k covers the layers from the previous bucket's lowest
 * minus one down to lowest[k] (layers 0 = input .. 2N+1 = output; buckets in backward order,
 * lowest[] strictly decreasing, lowest[n-1] == 0; n == 0 turns the buckets off).  Every later
 * p3d_backward / p3d_train_fwd_bwd[_lr] then runs the weight gradients of bucket k as ONE
 * k_wgrad_multi launch as soon as its layers' dZ and BN-parameter gradients exist (right after
 * the data-gradient launch of the layer above lowest[k]) and records bucket k's event, so the
 * bucket's flat range (p3d_layer_grad_range of its layers, contiguous) is final at that event
 * and its all-reduce overlaps the rest of the backward.  p3d_stream_wait_grad makes another
 * stream wait for bucket k's event of the last backward.  p3d_grad_events(m, 1) = one bucket
 * per layer.  (--max_norm models: every event after the clip's gradient, i.e. at the end.) */
int p3d_grad_buckets(p3d_model* m, int32_t n, const int32_t* lowest);
int p3d_grad_events(p3d_model* m, int32_t enable);
int p3d_layer_grad_range(const p3d_model* m, int32_t layer, int64_t* begin, int64_t* end);
int p3d_stream_wait_grad(p3d_model* m, int32_t bucket, void* stream);

/* The data-parallel step (session.run of the train op with the gradient averaged over the
 * replicas, linear_model.py:137-145 + SURVEY 8e) in two calls around the caller's all-reduce of
 * the flat grads buffer: p3d_train_fwd_bwd_lr = p3d_train_fwd_bwd whose first backward launch
 * also forms the step's Adam alpha (lr0 * decay_rate^(global_step / decay_steps), TF1 bias
 * correction, from the device step state); p3d_adam_apply = TF1 ApplyAdam + weight re-pack with
 * that alpha, the step state (global_step, beta powers) advanced in the same launch.  Both are
 * graph-capturable (all step state on the device). */
int p3d_train_fwd_bwd_lr(p3d_model* m, const float* x, const float* t, int64_t B, float* y, float keep_prob,
                         uint64_t seed, int64_t row_offset, float lr0, float decay_steps, float decay_rate,
                         float* loss_dev, void* stream);
int p3d_adam_apply(p3d_model* m, void* stream);

/* p3d_adam_apply split by gradient bucket (p3d_grad_buckets), each part issued on the stream of
 * that bucket's all-reduce right after it: the stream waits until the last backward has issued
 * the last reader of the bucket's parameters (the data-gradient launch of its lowest layer),
 * then Adam + re-pack of the bucket's tensors; the last bucket's launch advances the step
 * state.  Every bucket exactly once per step, in bucket order on one stream; bit-identical
 * to p3d_adam_apply.  The optimizer then overlaps the rest of the backward.  max_norm models:
 * P3D_ERR_STATE (they take p3d_adam_apply). */
int p3d_adam_apply_bucket(p3d_model* m, int32_t bucket, void* stream);

/* ---------------------------------------------------------------------------------------
 * Data-parallel training with the gradient all-reduce issued by this library (the
 * reference is single-process, its step is one session.run of the train op, src/linear_model.py:
 * 230-237, with one optimizer step per batch, :137-145).  librccl is resolved at run time from
 * the library the process already uses (pass torch's librccl path; NULL = "librccl.so.1"):
 * libp3d.so has no link-time dependency on it.  The ranks build a communicator from a unique id
 * rank 0 draws and broadcasts over the caller's own channel (torch.distributed), attach it to a
 * model, and p3d_train_step_dp then runs the whole DP step -- forward, backward, the bucketed
 * all-reduce of the flat gradient on a library-owned stream overlapping the backward, TF1 Adam +
 * re-pack, step advance -- holding no object of the caller's runtime, so one HIP graph captures it
 * whole.  The reduction is the replica mean (one rank: the identity).
 * ------------------------------------------------------------------------------------- */
typedef struct p3d_comm p3d_comm;
int p3d_comm_load(const char* librccl_path);
int p3d_comm_unique_id(uint8_t* id, int64_t id_len /* >= 128 */);
int p3d_comm_create(const uint8_t* id, int64_t id_len, int32_t nranks, int32_t rank, p3d_comm** out);
int p3d_comm_destroy(p3d_comm* c);
/* in-place all-reduce of n elements (dtype P3D_DTYPE_F32 / F64; op 0 sum, 1 mean, 2 max) on `stream` */
int p3d_comm_allreduce(p3d_comm* c, void* buf, int64_t n, int32_t dtype, int32_t op, void* stream);
/* the communicator the model's data-parallel step reduces over (NULL detaches; not owned) */
int p3d_dp_attach(p3d_model* m, p3d_comm* c);
/* One data-parallel training step.  With gradient buckets (p3d_grad_buckets) bucket k's
 * all-reduce runs on the library's comm stream as soon as the backward recorded its event and its
 * TF1 Adam follows on `stream` (env P3D_DP_ADAM: 1 default; 0 one optimizer pass after the last
 * bucket; 2 each bucket's optimizer on the comm stream); without buckets one all-reduce after the
 * backward.  Arguments as p3d_train_fwd_bwd_lr.  Graph-capturable (the comm stream is forked from
 * and joined to `stream`). */
int p3d_train_step_dp(p3d_model* m, const float* x, const float* t, int64_t B, float* y, float keep_prob,
                      uint64_t seed, int64_t row_offset, float lr0, float decay_steps, float decay_rate,
                      float* loss_dev, void* stream);

/* One whole single-GPU TF1 training step (linear_model.py:225-237): p3d_train_fwd_bwd then
 * the TF1 Adam update, global_step += 1.  By default (env P3D_FUSE_ADAM=1 at p3d_create) the
 * update runs inside the batched weight-gradient launch (k_wgrad_multi: no separate optimizer
 * pass; the flat grads buffer then holds the bias and BN gradients, not dW), bit-identical to
 * the unfused sequence (tests/test_gpu_parity.py) and faster at cfg3;
 * P3D_FUSE_ADAM=0 runs k_adam_pack after the backward.
 * lr = lr0 * decay_rate^(global_step / decay_steps) on the device.  Equivalent to
 * p3d_train_fwd_bwd + p3d_adam_step_decay (which --max_norm models use internally).
 * Graph-capturable; data-parallel training uses the unfused calls around its all-reduce. */
int p3d_train_step(p3d_model* m, const float* x, const float* t, int64_t B, float* y,
                   float keep_prob, uint64_t seed, float lr0, float decay_steps, float decay_rate,
                   float* loss_dev, void* stream);

/* One TF1 ApplyAdam over all trainables (linear_model.py:137,145):
 *   alpha = lr*sqrt(1-beta2_power)/(1-beta1_power); m += (g-m)(1-b1);
 *   v += (g^2-v)(1-b2); w -= (m*alpha)/(sqrt(v)+eps)
 * then global_step += 1 and the beta powers advance.  The step state lives on the
 * device.  p3d_adam_step takes the already-decayed lr; p3d_adam_step_decay computes
 * tf.train.exponential_decay (lr0 * rate^(global_step/steps), linear_model.py:88-90)
 * on the device, so a whole training step can be captured in a HIP graph. */
int p3d_adam_step(p3d_model* m, float lr, void* stream);
int p3d_adam_step_decay(p3d_model* m, float lr0, float decay_steps, float decay_rate, void* stream);

/* Adam bookkeeping (for checkpoints): global_step and beta1/beta2 powers.  Both
 * synchronise the device (the state is device-resident). */
int p3d_get_step(const p3d_model* m, int64_t* global_step, float* beta1_power, float* beta2_power);
int p3d_set_step(p3d_model* m, int64_t global_step, float beta1_power, float beta2_power);

/* Fused MPJPE accumulation of src/predict_3dpose.py:399-430 for one batch:
 *   pred_n [B, 48] fp32 network outputs, gt_n [B, 48] fp32 normalized targets,
 *   mean96/std96 [96] fp64 (data_mean_3d / data_std_3d), dims48 [48] int32
 *   (dim_to_use_3d).  Un-normalizes both (x*std+mean, fp64, root dims = mean),
 *   takes the 17 joints [0,1,2] + dims48, and ADDS per-joint L2 sums (fp64) into
 *   joint_sum17[17]. */
int p3d_mpjpe_accum(const float* pred_n, const float* gt_n, const double* mean96,
                    const double* std96, const int32_t* dims48, int64_t B, double* joint_sum17,
                    void* stream);

/* General form (src/predict_3dpose.py:383,399-430 with FLAGS.predict_14 / FLAGS.procrustes):
 *   D = 48, n_joints = 17: the 17-joint protocol above (root joint prepended);
 *   D = 42, n_joints = 14: --predict_14 (dims = the 42 dim_to_use_3d, no root);
 *   procrustes != 0: per-frame similarity alignment of the prediction onto the target
 *   (src/procrustes.py:2-63, compute_optimal_scale=True) before the per-joint L2.
 * ADDS into joint_sum[n_joints]; if sq_sum is non-null also adds sum((pred_n - gt_n)^2)
 * over the B x D batch (the loss of src/linear_model.py:129 times B*D, fp64 sum). */
int p3d_mpjpe_accum_ex(const float* pred_n, const float* gt_n, int32_t D, const double* mean96,
                       const double* std96, const int32_t* dims, int64_t B, int32_t n_joints,
                       int32_t procrustes, double* joint_sum, double* sq_sum, void* stream);

/* rocprofv3 name of the kernel used for `what` under the model's tiling variants:
 * 0 = inference hidden layer at B <= 64, 1 = inference hidden layer at large M,
 * 2 = BN-train hidden-layer GEMM, 3 = the kernel of the last p3d_serve launch,
 * 4 = inference hidden layer at B <= 4 (weight-streaming GEMV), 5 = the kernel of the last bf16
 * hidden layer (empty before one ran), 6 = the optimizers' weight source: "packed" (W read from its
 * packed Wd copy, the TF-layout master not written) or "master".  (Measurement plumbing for bench.py.) */
int p3d_kernel_name(const p3d_model* m, int32_t what, char* out, int64_t out_len);
/* The kernel p3d_serve (with_loss != 0: p3d_serve_mse) would launch for B rows of a model of this
 * shape on a device of `cus` compute units, under the P3D_SERVE6* environment as it is at the call:
 * its name as p3d_kernel_name(3) reports it after that launch, and in shape[5], when non-null,
 * {groups per XCD (0: not k_serve6), row tiles per unit, column tiles per contraction, ring depth,
 * units}.  P3D_ERR_ARG where those calls refuse the shape or the launch.  Needs no model and touches
 * no GPU; the batch <= 4 path of p3d_serve_mse is not modelled. */
int p3d_serve_plan(const p3d_cfg* cfg, int32_t cus, int64_t B, int32_t with_loss, char* name, int64_t name_len,
                   int32_t* shape);

/* Host-binding plumbing: a DLPack v0.8 DLManagedTensor aliasing `data` (no copy; the
 * memory stays owned by its model), with a C deleter that frees only the record.  Wrap
 * it in a "dltensor" PyCapsule for torch.utils.dlpack.from_dlpack.  NULL on bad input. */
void* p3d_dlpack_alias(void* data, int32_t ndim, const int64_t* shape, int32_t device_id,
                       int32_t dtype_code, int32_t bits);

/* Live kernel timing (bench.py's roofline): while active, every kernel the model
 * launches is bracketed by a hipEvent pair.  p3d_profile_stop synchronises and writes
 * one line per kernel tag: "tag\tcount\ttotal_us\tmin_us\tmax_us\n". */
int p3d_profile_start(p3d_model* m, int32_t max_launches);
int p3d_profile_stop(p3d_model* m, char* out, int64_t out_len);

/* Host-overhead probe (bench.py's accounting of the timed region beyond the kernel): one launch
 * of an empty kernel of `grid` 256-thread workgroups on `stream`, through the same launch path as
 * the model's kernels (with the model's event pair while p3d_profile_start is active). */
int p3d_empty_launch(p3d_model* m, int32_t grid, void* stream);

/* Completion of a captured sequence without the runtime's completion signal (the reference's
 * session.run returns its fetches; LinearModel.step(isTraining=True) from numpy): p3d_host_signal
 * enqueues one small kernel that advances the model's signal counter and stores the new count into
 * a pinned word (system-scope release); it is capturable, and each replay of a graph holding it
 * signals once.  p3d_host_wait(m, count, stream) returns once the count has reached `count` (a count
 * already passed included: the 32-bit counter wraps, and the comparison is of the signed difference) -- the
 * kernels before the signal have completed and their writes to coherent host memory are visible --
 * then reports a set kernel error word as P3D_ERR_HIP (p3d_error_flags says which); it polls the
 * stream now and then, so a failed launch is reported instead of waited for.  The stream itself
 * is not synchronised.  A caller waits for the count of its OWN signal: waiting for a smaller count
 * returns as soon as that earlier signal was stored, whatever is still running behind it.
 * p3d_host_alloc / p3d_host_free: coherent pinned host memory (mapped, not
 * cached on the device), where kernels' host-memory outputs must live for p3d_host_wait to cover
 * them. */
int p3d_host_signal(p3d_model* m, void* stream);
int p3d_host_wait(p3d_model* m, uint32_t count, void* stream);
void* p3d_host_alloc(int64_t bytes);
int p3d_host_free(void* p);

/* Roofline timing hook: `reps` back-to-back launches of hidden layer `layer`
 * (1 .. 2*num_layers) of the inference forward over workspace rows [0, B). */
int p3d_time_layer(p3d_model* m, int32_t layer, int64_t B, int32_t reps, void* stream);

/* ---------------------------------------------------------------------------------------
 * H3.6M data pipeline: float64 like the reference's numpy, row-major,
 * device pointers, asynchronous on `stream`.  These replace the per-sequence numpy loops of
 * the loaders; results are bit-identical to the reference.
 * A camera record is 21 float64: R row-major (9; X_cam = R (P - T)), T (3), f (2), c (2),
 * k (3), p (2) -- the tuple of src/cameras.py:92-140 (load_camera_params / load_cameras).
 * ------------------------------------------------------------------------------------- */

/* Rigid camera transforms of n points for each of C cameras into out [C, n, 3].
 * inverse = 0: world -> camera, src/cameras.py:55-72 (world_to_camera_frame; the batched
 *   form of data_utils.transform_world_to_camera, src/data_utils.py:233-257);
 * inverse = 1: camera -> world, src/cameras.py:74-90 (camera_to_world_frame).
 * P is [n, 3] shared by all cameras (in_cam_stride = 0) or [C, n, 3] (in_cam_stride = 3n). */
int p3d_cam_transform(const double* P, int64_t n, int64_t in_cam_stride, const double* cams,
                      int32_t C, int32_t inverse, double* out, void* stream);

/* Pinhole projection with radial (k1..k3) and tangential (p1, p2) distortion of n world
 * points for each of C cameras, src/cameras.py:13-53 (project_point_radial; the batched form
 * of data_utils.project_to_cameras, src/data_utils.py:339-364).  proj [C, n, 2]; depth,
 * radial, tan, r2 [C, n] are optional (NULL = not written). */
int p3d_cam_project(const double* P, int64_t n, const double* cams, int32_t C, double* proj,
                    double* depth, double* radial, double* tan, double* r2, void* stream);

/* Root-centring, src/data_utils.py:474-494 (postprocess_3d): out = poses - tile(poses[:, :3]),
 * root [F, 3] = poses[:, :3] (may be NULL).  width = 3 * joints; out must not alias poses. */
int p3d_root_center(const double* poses, int64_t F, int32_t width, double* out, double* root,
                    void* stream);

/* src/data_utils.py:260-280 (normalize_data): out [F, U] = (x[:, use] - mean[use]) / std[use]
 * from x [F, D]; out_dtype P3D_DTYPE_F64, or P3D_DTYPE_F32 (the float64 result rounded, as
 * feeding it to the model's float32 placeholders does). */
int p3d_normalize(const double* x, int64_t F, int32_t D, const double* mean, const double* stdv,
                  const int32_t* dims_to_use, int32_t U, void* out, int32_t out_dtype, void* stream);

/* src/data_utils.py:283-311 (unNormalizeData): scatter xn [F, U] (P3D_DTYPE_F32 or F64; the
 * reference rounds it to float32) into zeros [F, D], then out = that * std + mean (float64).
 * D <= 256. */
int p3d_unnormalize(const void* xn, int32_t in_dtype, int64_t F, int32_t U, const double* mean,
                    const double* stdv, const int32_t* dims_to_use, int32_t D, double* out,
                    void* stream);

/* The numbers behind sample(), src/predict_3dpose.py:512-546, for N rows in one launch.  Per row,
 * in float64 with every product and sum rounded on its own:
 *   1. scatter yn's U values (P3D_DTYPE_F32, or F64 rounded to float32) into 96 zeros;
 *   2. * std96 + mean96 (unNormalizeData, :512-514);
 *   3. + the row's root on all 32 joints, when root [N, 3] is given (:526; NULL: skipped);
 *   4. R^T X + T per joint with camera cam_of_row[row] of cams [C, 21] (:539; NULL: camera 0);
 *   5. minus the transformed joint 0 on every joint (:542).
 * out [N, 96] holds the bits of p3d_unnormalize -> + root -> p3d_cam_transform(inverse = 1) ->
 * p3d_root_center without their intermediates.  1 <= N <= 2^20, 1 <= U <= 96, 1 <= C <= 64; out
 * 16-byte aligned, root 8-byte aligned (else P3D_ERR_ARG, before any GPU work).  dims_to_use
 * entries are in 0..95 and cam_of_row entries in 0..C-1: the caller checks them (an entry of
 * dims_to_use outside 0..95 is dropped; a camera index outside 0..C-1 gives undefined values
 * in that row).  Asynchronous on stream and capturable. */
int p3d_sample_world(const void* yn, int32_t in_dtype, int64_t N, int32_t U, const double* mean96,
                     const double* std96, const int32_t* dims_to_use, const double* root,
                     const double* cams, int32_t C, const int32_t* cam_of_row, double* out,
                     void* stream);

/* src/openpose_3dpose_sandbox.py:347-356 per call (normalize_data of the mapped 2D rows, the
 * float32 placeholder cast, model.step at is_training False / keep 1, unNormalizeData): raw
 * [B, D2] float64 -> out [B, D3] float64.  U2 / U3 must equal the model's input / output size.
 * One launch where the batch <= 4 persistent chain runs, else p3d_normalize + p3d_forward_ex +
 * p3d_unnormalize; the same bits as those three calls either way.  Float32 models. */
int p3d_lift(p3d_model* m, const double* raw, int64_t B, int32_t D2, const double* mean2, const double* std2,
             const int32_t* use2, int32_t U2, const double* mean3, const double* std3, const int32_t* use3,
             int32_t U3, int32_t D3, double* out, void* stream);
/* p3d_lift that returns once out holds the results (pinned host rows; the per-frame call of
 * src/openpose_3dpose_sandbox.py:353-356): on the one-launch chain form the launch's output
 * workgroups store a completion word the host waits on, as p3d_serve_mse_sync; on the three-step
 * form the stream is synchronised.  Not capturable. */
int p3d_lift_sync(p3d_model* m, const double* raw, int64_t B, int32_t D2, const double* mean2, const double* std2,
                  const int32_t* use2, int32_t U2, const double* mean3, const double* std3, const int32_t* use3,
                  int32_t U3, int32_t D3, double* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * A whole OpenPose clip (src/openpose_3dpose_sandbox.py): raw keypoints [N, 36] float64 (18 joints,
 * x / y interleaved, rows in the order of the sorted file names) to the arrays the sandbox
 * exports.  All arithmetic float64 in the reference's operation order, bit for bit.  1 <= N <=
 * 2^20 frames.  `work` is device memory of at least p3d_clip_workspace(N) bytes, 8-byte aligned;
 * every call is a fixed set of launches on `stream` (capturable), never waiting between
 * workgroups inside a launch: a workgroup owns p3d_clip_chunk() consecutive frames, and what a
 * hold carries across chunks goes through a second launch.
 * ------------------------------------------------------------------------------------- */
int32_t p3d_clip_chunk(void);
int64_t p3d_clip_workspace(int64_t N);

/* read_openpose_json's smoothing, src/openpose_3dpose_sandbox.py:140-227, then the per-frame input
 * of :319-351.  smooth != 0 and N >= 9: per coordinate the median of positions i..i+3 (first four
 * positions), i-3..i (last four) or i-3..i+3, a window of four giving (a + b) / 2 of its middle
 * values; then the hold in position order: a median equal to 0.0 at position i > 0 takes the
 * smoothed value of position i - 1 (NaN is not zero).  smooth == 0 or N == 1: xy_s = xy.
 * 2 <= N <= 8 with smooth != 0: P3D_ERR_ARG (the reference raises, :145-146).
 *   xy_s [N, 36] float64: the smoothed, held rows (must not alias xy);
 *   x [N, U2] float32: normalize_data (:348-351) of the joint mapping (:332-342: `order` of :25,
 *     Hip, Neck/Nose, Thorax) of xy_s over the 64-wide row, rounded to float32 -- the bits of
 *     p3d_normalize(..., P3D_DTYPE_F32) on the mapped rows, which are never stored.  mean2 / std2
 *     [64], use2 [U2 <= 64] entries in 0..63 (an entry outside gives NaN). */
int p3d_clip_prepare(const double* xy, int64_t N, int32_t smooth, const double* mean2, const double* std2,
                     const int32_t* use2, int32_t U2, float* x, double* xy_s, void* work, int64_t work_bytes,
                     void* stream);

/* The sandbox's output side, src/openpose_3dpose_sandbox.py:359-417, from the network's rows
 * y [N, U3] float32 and xy_s: unNormalizeData (:359; (double)v * std + mean as p3d_unnormalize),
 * per frame over its 32 joints the y / z swap, _max = max(0, max z'), _min = min(10000, min z')
 * (strict compares, :366-377), z'' = (_max - z') + _min, x += spine_x - 630, z'' += 500 - spine_y
 * (:379-383; spine = columns 2, 3 of xy_s).  cache_on_fail != 0 (:389-417): a frame whose minimum
 * over its 96 values is < -1000 (a NaN minimum is not) shows the previous frame's exported pose,
 * 96 zeros where there is none.  The un-post-processed rows are never stored.
 *   poses [N, D3 = 96] float64; src [N] int32 (may be NULL): the position each exported pose came
 *   from, -1 for zeros.  mean3 / std3 [96], use3 [U3 <= 96]. */
int p3d_clip_finish(const float* y, int64_t N, const double* xy_s, const double* mean3, const double* std3,
                    const int32_t* use3, int32_t U3, int32_t D3, int32_t cache_on_fail, double* poses,
                    int32_t* src, void* work, int64_t work_bytes, void* stream);

/* The clip loop of src/openpose_3dpose_sandbox.py:317-417 as one call: p3d_clip_prepare, the eval
 * forward (keep 1, :353-356) in tiles of max_batch rows through the forward of p3d_lift's
 * three-step form -- a tile's rows carry p3d_lift's bits at that batch -- and p3d_clip_finish,
 * all on `stream`.  U2 / U3 must equal the model's input / output size; float32 models.  `work`:
 * p3d_clip_lift_workspace(N, U2, U3) bytes of device memory, 256-byte aligned (the scan's
 * summaries and the network's input and output rows).  Capturable. */
int64_t p3d_clip_lift_workspace(int64_t N, int32_t U2, int32_t U3);
int p3d_clip_lift(p3d_model* m, const double* xy, int64_t N, int32_t smooth, const double* mean2,
                  const double* std2, const int32_t* use2, int32_t U2, const double* mean3, const double* std3,
                  const int32_t* use3, int32_t U3, int32_t D3, int32_t cache_on_fail, double* xy_s, double* poses,
                  int32_t* src, void* work, int64_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * A BATCH of S clips stored one after another: rows [N, 36] and clip offsets [S + 1] (clip s is
 * rows off[s] .. off[s + 1] - 1).  The same kernels' segmented forms: every
 * position-dependent rule -- the four-frame windows of the first and last four positions, the
 * never-flagged position 0, the hold's and the held pose's look-back -- uses the position inside
 * its clip, and no window or carry reads a neighbouring clip.  Every clip's rows carry the bits of
 * the single-clip call on that clip alone; a one-frame clip passes through unsmoothed.
 *   clip_off_host: host int64 [S + 1], read at the call to validate and to size the grids (no copy,
 *     no device round trip: the calls stay asynchronous and capturable);
 *   clip_off_dev: the same values in device memory, read by the kernels (and by the filter as its
 *     seq_off), clamped into [0, N]: a mismatch gives wrong rows, never an access outside the buffers.
 * 1 <= S <= N <= 2^20, every clip at least one frame.  P3D_ERR_ARG without touching the GPU: a null
 * argument; offsets that do not start at 0, decrease or do not end at N; an empty clip; a clip of
 * 2-8 frames with smooth != 0 ("min 9 frames"); a short or misaligned workspace (8 bytes;
 * p3d_clips_lift: 256); and what the single-clip calls refuse.  src holds row indices into the
 * batch (-1: zeros: the clip has no good frame before).
 * ------------------------------------------------------------------------------------- */
int64_t p3d_clips_workspace(int64_t N, int64_t S);
int p3d_clips_prepare(const double* xy, const int64_t* clip_off_host, const int64_t* clip_off_dev, int64_t S, int64_t N,
                      int32_t smooth, const double* mean2, const double* std2, const int32_t* use2, int32_t U2,
                      float* x, double* xy_s, void* work, int64_t work_bytes, void* stream);
int p3d_clips_finish(const float* y, const int64_t* clip_off_host, const int64_t* clip_off_dev, int64_t S, int64_t N,
                     const double* xy_s, const double* mean3, const double* std3, const int32_t* use3, int32_t U3,
                     int32_t D3, int32_t cache_on_fail, double* poses, int32_t* src, void* work, int64_t work_bytes,
                     void* stream);

/* p3d_clip_lift over the batch, with the temporal VAE filter (p3d_vae_seq_filter; K >= 1:
 * p3d_vae_seq_filter_mc) between the forward and the post-processing: prepare; the eval forward in
 * tiles of max_batch rows that START AGAIN AT EVERY CLIP'S FIRST FRAME (the lifter picks its
 * kernels by the batch size, so its bits depend on the tiling: with this rule clip s carries the
 * bits of p3d_clip_lift on clip s alone; the price is a launch-bound forward on batches of very
 * short clips); with v != NULL the filter over the clips as its sequences (seq_off = clip_off_dev,
 * fresh state, eps [N, latent] / [K, N, latent] or NULL with ctr and eps_row0 as there) into a ref
 * [N, U3] area of the workspace; finish on ref; and with poses_unfiltered != NULL a second finish
 * on the network's own rows, its cache_on_fail judged on its own poses.  xy_s does not depend on
 * the filter.  ref_var [N, U3] float32 (or NULL) receives the K samples' variance.
 * P3D_ERR_ARG as above and: D3 != 96; dimension sets that do not match the model; a bf16 model;
 * with a filter: v not a sequence filter with out == U3 and in == seq_len * U3, a bones filter, K
 * outside 0 .. 64 (0: one draw through p3d_vae_seq_filter), ref_var with K == 0; without one:
 * ref_var or the unfiltered outputs asked for.  `work`: p3d_clips_lift_workspace bytes, 256-byte
 * aligned: the batch's summaries | x [N, U2] | y [N, U3] | ref [N, U3] (with_filter), each area
 * 256-byte aligned. */
int64_t p3d_clips_lift_workspace(int64_t N, int64_t S, int32_t U2, int32_t U3, int32_t with_filter);
struct p3d_vae;   /* the VAE pose filter's handle (below) */
int p3d_clips_lift(p3d_model* m, struct p3d_vae* v /* or NULL */, int32_t K, const float* eps, uint64_t ctr, int64_t eps_row0,
                   const double* xy, const int64_t* clip_off_host, const int64_t* clip_off_dev, int64_t S, int64_t N,
                   int32_t smooth, const double* mean2, const double* std2, const int32_t* use2, int32_t U2,
                   const double* mean3, const double* std3, const int32_t* use3, int32_t U3, int32_t D3,
                   int32_t cache_on_fail, double* xy_s, double* poses, int32_t* src,
                   double* poses_unfiltered /* or NULL */, int32_t* src_unfiltered /* or NULL */,
                   float* ref_var /* or NULL */, void* work, int64_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * S LIVE OpenPose streams lifted frame by frame with carried state (DESIGN.md 8d;
 * src/openpose_3dpose_sandbox_realtime.py).  A session has S slots; each tick the caller pushes at
 * most one raw frame (36 float64) to any subset of them and may close others; the tick returns the
 * rows that became final.  For every stream the rows of its lifetime, concatenated, are xy_s / x /
 * poses / src of the clip calls above on the stream's whole frame list, bit for bit (src: the
 * stream-local frame, -1 with a zero pose while the stream has no good frame), up to the forward's
 * tiling (a tick's rows, in slot order, are forwarded in tiles of max_batch rows) and the filter's
 * noise keys (ctr, eps_row0 of the tick).  With smoothing a frame is final four pushes after its
 * own (the median looks three frames ahead, and the last four frames of a stream take another
 * window), at close for the last four; without, at once.
 *
 * p3d_live_plan is that rule, host only: count [S] (frames received, updated in place), push / close
 * [S] (non-zero: the slot gets a frame / is closed; never both) -> row_off [S + 1], row_slot /
 * row_frame / row_kind [<= 5 S] (kind 0 the frame itself, 1 head window f .. f+3, 2 middle f-3 ..
 * f+3, 3 tail f-3 .. f), push_frame [S] (the pushed frame's number, -1), is_short [S] (closed with
 * 2 .. 8 frames under smoothing: the stream is refused as a clip of that length is) and *n_rows.
 *
 * The tick's table -- xy_in [S, 36] (row s: the frame pushed to slot s), push_frame, row_off,
 * row_frame, row_kind -- is PINNED HOST memory that the host checks at the call and the kernels read
 * in place (no upload: the calls stay asynchronous); it must stay unchanged until the tick has
 * run.  The device clamps every offset into [0, N] and masks every ring index.  `state`:
 * p3d_live_state_bytes(S, U3) bytes of device memory, 8-byte aligned, reset by p3d_live_reset
 * (slot < 0: all slots) before a slot's first frame.  1 <= S <= 65536, 0 <= N <= 5 S.
 * P3D_ERR_ARG without touching the GPU: a null argument, S or N out of range, a row_off that does
 * not start at 0, decreases, gives a slot more than 5 rows or does not end at N, a negative frame,
 * a kind outside 0 .. 3 (or non-zero without smoothing), a misaligned state, U2 / U3 / D3 as at the
 * clip calls, and at p3d_live_push what p3d_clips_lift refuses of the model, the filter, K and the
 * workspace (p3d_live_push_workspace bytes, 256-byte aligned).
 * ------------------------------------------------------------------------------------- */
int p3d_live_plan(int64_t S, int32_t smooth, int32_t* count, const uint8_t* push, const uint8_t* close,
                  int64_t* row_off, int32_t* row_slot, int32_t* row_frame, int32_t* row_kind, int32_t* push_frame,
                  int32_t* is_short, int64_t* n_rows);
int64_t p3d_live_state_bytes(int64_t S, int32_t U3);
int p3d_live_reset(void* state, int64_t S, int64_t slot_or_minus1, void* stream);
/* k_live_in: the pushed frames into the slots' rings; per row the window median, the hold from the
 * slot's last smoothed row (never at frame 0), xy_s [N, 36] and x [N, U2] float32. */
int p3d_live_prepare(const double* xy_in, const int32_t* push_frame, const int64_t* row_off, const int32_t* row_frame,
                     const int32_t* row_kind, int64_t S, int64_t N, int32_t smooth, const double* mean2,
                     const double* std2, const int32_t* use2, int32_t U2, void* state, float* x, double* xy_s,
                     void* stream);
/* k_live_out: per row of y [N, U3] p3d_clip_finish's arithmetic from that row's xy_s; with
 * cache_on_fail a failing row shows the slot's last good pose and its frame (zeros and -1 where
 * there is none) and a good row becomes it.  src may be NULL. */
int p3d_live_finish(const float* y, const int64_t* row_off, const int32_t* row_frame, int64_t S, int64_t N,
                    const double* xy_s, const double* mean3, const double* std3, const int32_t* use3, int32_t U3,
                    int32_t D3, int32_t cache_on_fail, void* state, double* poses, int32_t* src, void* stream);
/* One tick on `stream`: prepare; the eval forward of the tick's rows in tiles of max_batch; with
 * v != NULL p3d_vae_seq_filter (K >= 1: p3d_vae_seq_filter_mc) over the slots as its sequences
 * (seq_off = row_off, slots without rows empty) on the carried filter_state / filter_started
 * ([S, (seq_len - 1) * U3] float32, [S] int32, as at p3d_vae_seq_filter; a reopened slot needs
 * filter_started[slot] = 0) with the library's noise at (ctr, eps_row0 + row); finish on the refined
 * rows.  ref_var [N, U3] float32 or NULL (needs K >= 1).  N == 0: the rings only. */
int64_t p3d_live_push_workspace(int64_t S, int32_t U2, int32_t U3, int32_t with_filter);
int p3d_live_push(p3d_model* m, struct p3d_vae* v /* or NULL */, int32_t K, uint64_t ctr, int64_t eps_row0,
                  void* state, float* filter_state, int32_t* filter_started, const double* xy_in,
                  const int32_t* push_frame, const int64_t* row_off, const int32_t* row_frame, const int32_t* row_kind,
                  int64_t S, int64_t N, const double* mean2, const double* std2, const int32_t* use2, int32_t U2,
                  const double* mean3, const double* std3, const int32_t* use3, int32_t U3, int32_t D3,
                  int32_t cache_on_fail, int32_t smooth, double* xy_s, double* poses, int32_t* src,
                  float* ref_var /* or NULL */, void* work, int64_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Lifted rows as a RIGID SKELETON: constant bone lengths per clip, one rotation per
 * bone and frame, Euler angles for BVH, and the pose with the constant lengths.  `poses` [N, 96]
 * float64 are rows as the clip, clips and live calls write them (32 joints, exported coordinates),
 * S clips one after another under clip offsets as at the clips calls (host copy: validated, sizes
 * the grids; device copy: read by the kernels, clamped into [0, N]; S = 1 with {0, N}: one clip).
 * The 17 skeleton joints are H3.6M joints {0,1,2,3,6,7,8,12,13,14,15,17,18,19,25,26,27}, joint 0
 * the hip, in skeleton coordinates (X, Y, Z) = (x, z, -y) (Y up); the 16 bones are the bones
 * filter's (bone b from joint ja(b) to jb(b), parent bone pb(b)); the rest direction r_b is -X for
 * the right hip / shoulder / elbow / wrist, +X for the left ones, -Y for knees and feet, +Y for
 * spine, thorax, neck and head.  All arithmetic float64.  src [N] int32 is the clip calls' (row
 * indices into the batch, -1: zeros) or NULL (every row carries its own pose).  The calls need no
 * model, are asynchronous and capturable, and give the same bits on every run; a clip inside a
 * batch carries the bits of the call on that clip alone.
 *
 * p3d_skel_lengths: lengths [S, 16] = per clip and bone the mean of |J[jb] - J[ja]| over the clip's
 * frames n with src[n] == n whose 17 joints are all finite; n_used [S] int64 their number (0: 16
 * zeros).  A workgroup owns p3d_skel_chunk() consecutive frames of one clip and a second launch
 * folds a clip's partial sums in a fixed order (no atomics).  `work`: p3d_skel_workspace(N, S)
 * bytes of device memory, 8-byte aligned.
 *
 * p3d_skel_pose, per frame and bone with d_b the bone's unit direction (a zero-length bone: r_b,
 * and the identity for g_b; a row with src[n] < 0 counts as zeros whatever it holds):
 *   quat  [N, 16, 4]  q_b = conj(g_pb) (x) g_b (w, x, y, z), g_b the shortest arc from r_b to d_b,
 *                     normalize(1 + r.d, r x d), or (0, 0, 0, 1) where 1 + r.d < 1e-12; a hip bone: g_b.
 *                     The twist about the bone is not determined by positions and stays the arc's;
 *   euler [N, 16, 3]  (Z, X, Y) degrees of q_b with R = Rz Rx Ry -- BVH's Zrotation Xrotation Yrotation;
 *   rigid [N, 17, 3]  P[0] = J[0], P[jb(b)] = P[ja(b)] + lengths[b] d_b;
 *   root  [N, 3]      J[0].
 * Each output may be NULL, not all.  lengths [S, 16] is device memory: p3d_skel_lengths' or the
 * caller's own (a known actor, a live stream).  A non-finite joint gives what the arithmetic gives.
 *
 * P3D_ERR_ARG ("p3d_skel_lengths: ..." / "p3d_skel_pose: ...") without touching the GPU: a null
 * poses, lengths, n_used or offsets; all four outputs null; N or S outside 1 <= S <= N <= 2^20;
 * offsets that do not start at 0, decrease, hold an empty clip or do not end at N; a null, short
 * or misaligned (8 bytes) workspace.
 * ------------------------------------------------------------------------------------- */
int32_t p3d_skel_chunk(void);
int64_t p3d_skel_workspace(int64_t N, int64_t S);
int p3d_skel_lengths(const double* poses, const int32_t* src /* or NULL */, const int64_t* clip_off_host,
                     const int64_t* clip_off_dev, int64_t S, int64_t N, double* lengths /* [S, 16] */,
                     int64_t* n_used /* [S] */, void* work, int64_t work_bytes, void* stream);
int p3d_skel_pose(const double* poses, const int32_t* src /* or NULL */, const int64_t* clip_off_host,
                  const int64_t* clip_off_dev, int64_t S, int64_t N, const double* lengths /* [S, 16], device */,
                  double* quat, double* euler, double* rigid, double* root /* each may be NULL, not all */,
                  void* stream);

/* ---------------------------------------------------------------------------------------
 * SPLINE-RESAMPLED clips (the reference's --interpolation --multiplier 1/R,
 * src/openpose_3dpose_sandbox.py:240-291).  Each of a clip's 36 smoothed tracks y over the frames
 * 0 .. m - 1 is fitted as scipy's UnivariateSpline(frame, y, k=3) followed by
 * set_smoothing_factor((max(y) - min(y)) * 125) fits it: FITPACK's curfit with s = m, then again with
 * iopt = 1 CONTINUING from the first call's knots and saved state (not a fresh fit).  The spline is
 * sampled at j * (1.0 / R), j = 0 .. R m - 1 (the last R - 1 positions extrapolate the last piece),
 * and the samples, renumbered from 0, are the clip the lifter sees.  All float64, no contraction,
 * + - * / sqrt fabs only, one fixed operation order: the same bits on every run, and a clip inside a
 * batch carries the bits of the call on that clip alone.  A non-finite sample follows the arithmetic.
 *
 * p3d_clips_resample: xy_s [N, 36] (p3d_clips_prepare's) under clip offsets as at the clips calls ->
 *   xy_r [R N, 36]; x [R N, U2] float32, the bits of p3d_clips_prepare(xy_r, smooth = 0);
 *   off_out_dev [S + 1] = R * off (device, clamped as read); info [S, 36, 5] int32 or NULL: per curve
 *   n after stage 1, n after stage 2, FITPACK's ier of either stage (-2 the least-squares polynomial,
 *   -1 the interpolating spline, 0 the smoothing spline, 2 / 3 the p search gave up or ran out of its
 *   20 iterations: the fit stands as FITPACK returns it; 5, ours: no knot interval could take a knot),
 *   and the p iterations of stage 2.
 *   `work`: p3d_clips_resample_workspace(N, S, R) bytes of device memory, 8-byte aligned:
 *   t f64 [36 (N + 4 S)] | c f64 [36 (N + 4 S)] | info i32 [S, 36, 5] | the state of curves too long for
 *   LDS, every area 256-byte aligned; the curve of clip s (rows lo .., m frames) and column col keeps
 *   its n knots and coefficients at 36 (lo + 4 s) + col (m + 4) of t and c.
 * p3d_clips_lift_resampled: p3d_clips_lift with the resampling between prepare and the forward; xy_s
 *   [N, 36] stays the smoothed rows, xy_r [R N, 36], poses [R N, 96], src [R N] (and the unfiltered
 *   outputs, ref_var [R N, U3], eps [R N, latent]) are rows of the resampled clips, whose forward
 *   tiles start again at every clip's first resampled row and whose filter sequences are off_out_dev:
 *   p3d_clips_lift on the xy_r clips with smooth = 0, bit for bit.
 * P3D_ERR_ARG without touching the GPU, the message starting with the call's name: a null argument;
 * R outside 1 .. 16; a clip under 4 frames (FITPACK needs m > k) or over 65,536; R N > 2^20; what the
 * clips calls refuse of N, S and the offsets; a null, short or misaligned workspace (8 bytes;
 * p3d_clips_lift_resampled: 256); aliased xy / xy_s / xy_r; and at p3d_clips_lift_resampled everything
 * p3d_clips_lift refuses.
 * ------------------------------------------------------------------------------------- */
int64_t p3d_clips_resample_workspace(int64_t N, int64_t S, int32_t R);
int p3d_clips_resample(const double* xy_s, const int64_t* clip_off_host, const int64_t* clip_off_dev, int64_t S,
                       int64_t N, int32_t R, const double* mean2, const double* std2, const int32_t* use2, int32_t U2,
                       float* x, double* xy_r, int64_t* off_out_dev, int32_t* info /* or NULL */, void* work,
                       int64_t work_bytes, void* stream);
int64_t p3d_clips_lift_resampled_workspace(int64_t N, int64_t S, int32_t R, int32_t U2, int32_t U3, int32_t with_filter);
int p3d_clips_lift_resampled(p3d_model* m, struct p3d_vae* v /* or NULL */, int32_t K, const float* eps, uint64_t ctr,
                             int64_t eps_row0, const double* xy, const int64_t* clip_off_host,
                             const int64_t* clip_off_dev, int64_t S, int64_t N, int32_t smooth, const double* mean2,
                             const double* std2, const int32_t* use2, int32_t U2, const double* mean3,
                             const double* std3, const int32_t* use3, int32_t U3, int32_t D3, int32_t cache_on_fail,
                             double* xy_s, double* poses, int32_t* src, double* poses_unfiltered /* or NULL */,
                             int32_t* src_unfiltered /* or NULL */, float* ref_var /* or NULL */, int32_t R,
                             double* xy_r, int64_t* off_out_dev, int32_t* info /* or NULL */, void* work,
                             int64_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * The ROOT TRAJECTORY of lifted rows: per frame the translation T = (Tx, Ty, Tz) in
 * the camera's frame (x right, y down, z forward, the 3D statistics' unit) that puts the
 * root-relative 3D joints of a `poses` row onto the 2D joints of an `xy_s` row under a pinhole
 * camera (focal length `focal`, principal point (cx, cy), pixels), in closed form.  `poses` [N, 96]
 * and `xy_s` [N, 36] float64 are rows as the clip, clips and live calls write them, S clips one after
 * another under clip offsets as at p3d_skel_pose (host copy: validated; device copy: read by the
 * kernels, clamped into [0, N]; no loads for it at S = 1); src [N] int32 is the clip calls' (row
 * indices into the batch) or NULL (every row its own).  Row n with s = src[n] takes its 3D from
 * poses[n] and its 2D from xy_s[s] (read clamped to N - 1); s < 0: T = 0, resid = 0, valid = 0.
 *
 * The 13 joints j of H3.6M {0,1,2,3,6,7,8,17,18,19,25,26,27} (hip, legs, arms), their 2D (u, v) the
 * OpenPose joint of the clip calls' mapping, the hip's (RHip + LHip) / 2; with P = poses[n]:
 *   x = P[3j] - P[0], z = P[3j+1] - P[1], y = P[2] - P[3j+2]   (camera frame, the export's offsets cancel)
 *   a = (u - cx) / focal, b = (v - cy) / focal, p = a z - x, q = b z - y
 *   am, bm, pm, qm = sum / 13; da = a - am, db = b - bm; D = sum(da da + db db), Nn = sum(da p + db q)
 *   D < 1e-12 (the 2D joints coincide): T = 0, resid = 0, valid = 0.  Else valid = 1 and
 *   Tz = -Nn / D, Tx = pm + am Tz, Ty = qm + bm Tz
 *   resid = sqrt(sum(eu eu + ev ev) / 13), eu = focal ((x + Tx) / (z + Tz)) - (u - cx), ev alike (pixels).
 * Every sum is one pairwise tree over 16 slots (13 joints and three +0.0), every operation float64
 * and rounded on its own; a non-finite value follows the arithmetic (a NaN D is not below the bound).
 * A joint behind the camera is not special: the residual shows it.
 *
 *   traj_raw [N, 3]  T;  resid [N];  valid [N] int32
 *   traj     [N, 3]  smooth_half = h: the sum, in ascending frame order, of the valid raw rows at most
 *                    h frames away inside the row's clip, divided by their number; zeros where the row
 *                    itself is not valid.  h = 0: the raw rows, byte for byte.
 * Each output may be NULL, not all.  `work`: p3d_root_trajectory_workspace(N, smooth_half) bytes of
 * device memory, 8-byte aligned (0 bytes at h = 0: NULL is fine): where the raw rows and the flags
 * stand when traj is asked for and they are not.  p3d_root_trajectory_rows(): the rows one solve
 * workgroup owns.  The call needs no model, is asynchronous and capturable (the solve's launch and,
 * with h > 0 and traj, the smoothing's behind it), and gives the same bits on every run; a clip
 * inside a batch carries the bits of the call on that clip alone.  It cannot know whether the rows
 * are in the camera's frame (a model trained with --camera_frame) or whether focal / cx / cy are the
 * video's: the caller vouches for both.
 *
 * P3D_ERR_ARG ("p3d_root_trajectory: ...") without touching the GPU: a null poses, xy_s or offsets;
 * all four outputs null; N or S outside 1 <= S <= N <= 2^20; offsets that do not start at 0,
 * decrease, hold an empty clip or do not end at N; focal not finite or <= 0; cx or cy not finite;
 * smooth_half outside 0 .. 32; with smooth_half > 0 a null, short or misaligned (8 bytes) workspace.
 * ------------------------------------------------------------------------------------- */
int64_t p3d_root_trajectory_workspace(int64_t N, int32_t smooth_half);
int32_t p3d_root_trajectory_rows(void);
int p3d_root_trajectory(const double* poses, const double* xy_s, const int32_t* src /* or NULL */,
                        const int64_t* clip_off_host, const int64_t* clip_off_dev, int64_t S, int64_t N,
                        double focal, double cx, double cy, int32_t smooth_half, double* traj, double* traj_raw,
                        double* resid, int32_t* valid /* each may be NULL, not all */, void* work,
                        int64_t work_bytes, void* stream);

/* np.mean / np.std (population) over axis 0 of x [F, D], D <= 256 -- the statistics of
 * src/data_utils.py:210-211 (normalization_stats).  Deterministic two-level column sums;
 * `work` must hold p3d_moments_workspace(F, D) bytes of device memory. */
int64_t p3d_moments_workspace(int64_t F, int32_t D);
int p3d_moments(const double* x, int64_t F, int32_t D, double* mean, double* stdv, void* work,
                int64_t work_bytes, void* stream);

/* CRC-32C (Castagnoli) of host memory -- TF tensor-bundle checksums (checkpoint interop,
 * src/predict_3dpose.py:165-181,328 save/restore through tf.train.Saver).  crc = 0 starts a
 * buffer; pass a previous result to continue it.  Host only, no device work. */
uint32_t p3d_crc32c(const void* data, int64_t n, uint32_t crc);

/* ------------------------------------------------------------------------------------------
 * The VAE pose filter on top of the frozen lifter: src/top_vae_3d_pose/models.py:12-91 (VAE),
 * src/top_vae_3d_pose/losses.py:12-109 (ELBO) and src/3d_pose_vae_filter.py:188-196
 * (train_step_vae).  A dense net in -> enc_dims (ReLU) -> {mean, log_varianze} [latent] ->
 * z = eps exp(0.5 log_var) + mean -> dec_dims (ReLU) -> out, whose whole parameter set lives in
 * one workgroup's LDS (csrc/p3d_vae.h).  All pointers are device pointers (`factors`: three host
 * floats, read at the call), every call is asynchronous on `stream` and capturable; argument
 * errors answer without a GPU.
 * ------------------------------------------------------------------------------------------ */
typedef struct p3d_vae p3d_vae;

/* keras.Model construction of models.py:25-52.  in <= 2048; 1-4 hidden layers each side, widths
 * <= 256; latent <= 64; out <= 64; every width a multiple of 8; max_batch <= 2^20 bounds the
 * rows of the loss / gradient / training calls; the parameters and the working space of four
 * 16-row tiles must fit one workgroup's LDS.  Anything else: P3D_ERR_ARG and a message.
 * in > 256 is the WIDE form (csrc/p3d_vae_wide.h; models.py:485-540 with use_2d and
 * use_effnet_ouptut: in = 32 + 48 + 1280): layer 0's kernel [in, enc_dims[0]] and bias stay in
 * their master buffer and are read through L2, every other layer keeps the packed LDS copy, and a
 * call is three launches ordered by the stream (layer 0 forward; the filter behind it; layer 0's
 * weight gradient and optimizer).  The parameter table, the names and the flat buffers are laid
 * out alike in both forms.  The weight gradient of layer 0 is one accumulator chain over the B
 * rows in row order: no per-block partial of it exists, and every gradient sum stays associated
 * by the row index alone.  p3d_vae_seq_filter refuses a wide filter.
 * Parameters start at zero (the host writes Glorot kernels through the parameter table);
 * `seed` keys the eps stream. */
int p3d_vae_create(int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent, int32_t n_dec,
                   const int32_t* dec_dims, int32_t out, int32_t max_batch, uint64_t seed, p3d_vae** v);
int p3d_vae_destroy(p3d_vae* v);
/* Bytes of LDS a workgroup of this shape's kernels uses (the packed parameters + four 16-row
 * tiles of activations), as p3d_vae_create lays them out; 0 for a shape it refuses for another
 * reason.  A wide shape answers what its largest workgroup uses: the filter behind layer 0 (the
 * layer-0 kernels use no LDS).  Host only. */
int64_t p3d_vae_lds_bytes(int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent, int32_t n_dec,
                          const int32_t* dec_dims, int32_t out);

/* The BONES filter (models.py:544-573 VAEBones, losses.py:113-156 loss_bones): the encoder and the
 * reparametrisation of p3d_vae_create, the decoder dec_dims (ReLU) -> mag1 (16, ReLU) -> {mag2 (16),
 * cos2 (48)}, both linear heads on mag1's output; out = 64 = [mag | cos], the layout of
 * p3d_bones_from_joints.  (The reference also constructs a layer "cos1"; its output is overwritten
 * before keras.Model is formed, so it is not part of the model and has no weights.)  The limits
 * of p3d_vae_create apply, in > 256 is the wide form.  The parameter table ends
 * "dec_f_<units>/...", "mag1/kernel", "mag1/bias", "mag2/...", "cos2/...".  Every p3d_vae_* call
 * takes the handle; where a bones filter differs it is said at the call's declaration. */
int p3d_vae_create_bones(int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent, int32_t n_dec,
                         const int32_t* dec_dims, int32_t max_batch, uint64_t seed, p3d_vae** v);
/* p3d_vae_lds_bytes for a bones filter.  Host only. */
int64_t p3d_vae_bones_lds_bytes(int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent, int32_t n_dec,
                                const int32_t* dec_dims);
/* 0: p3d_vae_create's filter (ELBO), 1: a bones filter; -1 for a null handle. */
int32_t p3d_vae_kind(const p3d_vae* v);

/* joints [B, 48] float32 (hip-centred, joint k >= 1 in columns 3 (k - 1) ..) -> out64 [B, 64] =
 * [bone lengths (16) | direction cosines (16 x 3)] over the bones
 *   from 0 1 2 0 4 5 0 7 8  9  9 14 15  9 11 12
 *   to   1 2 3 4 5 6 7 8 9 10 14 15 16 11 12 13   (bones.py:74-75).
 * precise = 1 is bones.py:101-121 convert_to_bones (float64 arithmetic, one rounding to float32),
 * precise = 0 bones.py:71-98 convert_to_bones_tf (float32 throughout, sum of squares left to
 * right); sqrt and divide correctly rounded, no FMA contraction.  A zero-length bone gives NaN
 * cosines.  B in 1 .. 2^20; asynchronous, capturable; argument errors answer without a GPU. */
int p3d_bones_from_joints(const float* joints, int64_t B, int32_t precise, float* out64, void* stream);
/* bones.py:124-153 convert_to_joints: bones64 [B, 64] -> joints_f64 [B, 48] float64, in bone order
 * J[to] = J[from] + (double)(cos * mag), the product float32.  Same limits. */
int p3d_bones_to_joints(const float* bones64, int64_t B, double* joints_f64, void* stream);

/* Parameter table in Keras order and names (model.get_weights(), models.py:29-49):
 * "enc_h_<units>/kernel", "enc_h_<units>/bias", ..., "mean/kernel", "mean/bias",
 * "log_varianze/kernel", "log_varianze/bias", "dec_f_<units>/kernel", ..., "dec_f_out/bias".
 * Kernels are [rows = in, cols = out] row-major masters, biases [1, cols]; `offset` is the
 * tensor's place in the flat buffers. */
int p3d_vae_param_count(const p3d_vae* v, int32_t* count);
int p3d_vae_param_info(const p3d_vae* v, int32_t idx, const char** name, int64_t* numel, int32_t* rows,
                       int32_t* cols, int64_t* offset);
int p3d_vae_param_ptr(p3d_vae* v, const char* name, void** dptr, int64_t* numel);
/* Flat device buffers sharing the parameter table's layout (0 params, 1 grads, 2 adam_m,
 * 3 adam_v), and 4: the workspace of per-block partial gradients, 5: the packed copy. */
int p3d_vae_flat_ptr(p3d_vae* v, int32_t which, void** dptr, int64_t* numel);
/* Re-derive the packed copy after the host wrote parameters (model.set_weights). */
int p3d_vae_params_updated(p3d_vae* v, void* stream);

/* VAE.call (models.py:62-80): y [B, out] from x [B, in], any B up to 2^20.  eps [B, latent] is
 * the caller's, or (null) drawn from the library's Philox stream keyed (seed, ctr, row, column)
 * -- tf.random.normal's own stream is not reproducible.  mean, log_var, z [B, latent] are
 * written when non-null; with a target [B, out], row_terms [B, 3] receives per row the mean
 * square likelihood, the KCS error (out == 48 only, else 0) and the KL divergence of
 * losses.py:29-32.  ctr = P3D_CTR_GLOBAL_STEP reads the device step counter.
 * Bones filter: y and target are [B, 64] = [mag | cos]; row_terms is [B, 4]: mean_16 (tm - pm)^2,
 * 3 mean_48 (tc - pc)^2, the KL divergence, mean_16x16 |G(tc) - G(pc)| (losses.py:127-152). */
int p3d_vae_forward(p3d_vae* v, const float* x, int64_t B, const float* eps, uint64_t ctr, float* y, float* mean,
                    float* log_var, float* z, const float* target, float* row_terms, void* stream);

/* VAE.decode (models.py:74-76): y [B, out] from z [B, latent]; or, z null, from the prior stream
 * (seed, ctr, P3D_VAE_PRIOR_SITE, row0 + r, c4), written to z_out when non-null.
 * One launch (k_vae_dec, csrc/p3d_vae_dec.h) that holds only the decoder's parameters in LDS and
 * runs the forward's own layer arithmetic in the forward's order: y is bit-identical to the y
 * p3d_vae_forward writes for the same z, NaN and Inf included.  Works on every filter kind (a bones
 * filter: y is [B, 64] = [mag | cos]; a wide filter: the decoder behind its core), for any
 * 1 <= B <= 2^20 whatever max_batch is: no workspace is used.  Asynchronous, capturable.
 * The prior stream: columns 4c .. 4c+3 of row r are p3d_vae_eps's construction (one Philox4x32-10
 * block through TF's Box-Muller) over the counter (g, c, P3D_VAE_PRIOR_SITE, ctr), key seed, with
 * g = row0 + r (its low 32 bits, and ctr's) and P3D_VAE_PRIOR_SITE = 0x505249 -- a site of its own
 * (eps: 0x564145, noise: 0x4E4F49 / 0x4E4F52, dropout: < 64), so a sample is never the eps a
 * training step draws at the same (seed, ctr, row).  Rows are keyed by g alone: a call over rows
 * row0 .. row0 + B - 1 gives those rows of one longer call.
 * P3D_ERR_ARG ("p3d_vae_decode: ..."), without touching the GPU: a null handle, a null y, B out of
 * range, z and z_out both given, row0 < 0, ctr == P3D_CTR_GLOBAL_STEP. */
int p3d_vae_decode(p3d_vae* v, const float* z, int64_t B, uint64_t ctr, int64_t row0,
                   float* y, float* z_out, void* stream);
/* Dynamic LDS bytes of the decoder kernels for this shape (host only; 0 for a refused shape): the
 * decoder's packed parameters and four z-and-activation tiles, with the packed rows staggered as
 * p3d_vae_create's first layout does (a filter that only fits unstaggered uses less). */
int64_t p3d_vae_dec_lds_bytes(int32_t latent, int32_t n_dec, const int32_t* dec_dims, int32_t out, int32_t bones);
/* Workgroups of p3d_vae_decode per CU: 1 .. what a CU's LDS holds, 0 the default (as many as it
 * holds, four at the most; MEASUREMENTS.md §20).  Same bits whatever the grid. */
int p3d_vae_dec_set_grid(p3d_vae* v, int32_t wgs_per_cu);

/* ELBO.compute_loss (losses.py:14-40): loss3_dev =[likef mean_B like, kcsf mean_B kcs,
 * dklf mean_B dkl] for factors = {likef, kcsf, dklf}; B <= max_batch.  kcsf must be 0 unless
 * out == 48 (P3D_ERR_ARG).
 * Bones filter: factors[4] = {mag, cos, dkl, ang}, t is [B, 64] and loss3_dev receives FOUR floats
 * [MAG, COS, DKL, ANG] (losses.py:154). */
int p3d_vae_loss(p3d_vae* v, const float* x, const float* t, int64_t B, const float* eps, uint64_t ctr,
                 const float* factors, float* loss3_dev, void* stream);
/* The same plus tape.gradient of the three terms' sum (3d_pose_vae_filter.py:191-194) into the
 * gradient buffer; no optimizer.  Sums are associated by row index alone (16-row tiles in order
 * inside a 64-row block, blocks in order), so the gradient does not depend on the launch form.
 * Bones filter: factors[4] and a four-float loss as p3d_vae_loss; the gradient is that of the four
 * terms' sum. */
int p3d_vae_grad(p3d_vae* v, const float* x, const float* t, int64_t B, const float* eps, uint64_t ctr,
                 const float* factors, float* loss3_dev, void* stream);
/* train_step_vae (3d_pose_vae_filter.py:188-196): loss, gradient and Keras Adam
 * (optimizer.apply_gradients; beta 0.9 / 0.999, epsilon 1e-7) with the device step counter as
 * the eps counter.  B <= 64 is ONE launch; larger batches add the block reduction + Adam launch.
 * Bones filter: factors[4] and a four-float loss as p3d_vae_loss; the launches are the same. */
int p3d_vae_train_step(p3d_vae* v, const float* x, const float* t, int64_t B, const float* eps,
                       const float* factors, float lr, float* loss3_dev, void* stream);
/* Keras Adam over the gradient buffer as it stands (after p3d_vae_grad): the stand-alone form
 * of the optimizer inside p3d_vae_train_step, bit-identical to it. */
int p3d_vae_adam_apply(p3d_vae* v, float lr, void* stream);
/* form = 1 runs p3d_vae_grad / p3d_vae_train_step through the per-block partials and the
 * reduction launch also at B <= 64 (0, the default: one launch there).  Same bits either way. */
int p3d_vae_set_form(p3d_vae* v, int32_t form);
/* optimizer.iterations and the beta powers (device-resident; these two calls synchronise). */
int p3d_vae_get_step(const p3d_vae* v, int64_t* step, float* beta1_power, float* beta2_power);
int p3d_vae_set_step(p3d_vae* v, int64_t step, float beta1_power, float beta2_power);

/* Rows row0 .. row0 + B - 1 of the eps stream (tf.random.normal of models.py:70) as
 * p3d_vae_forward draws them: out [B, latent], latent a multiple of 4. */
int p3d_vae_eps(uint64_t seed, uint64_t ctr, int64_t row0, int64_t B, int32_t latent, float* out, void* stream);
/* The noise the filters are trained to remove (data_handler.py:48-84 add_noise) as a counter-based
 * stream, one launch (k_vae_noise, csrc/p3d_vae_noise.h).  Output row r is the `width` contiguous
 * floats of the table src [rows, d] that begin at row starts[r] (width = k d: a window of k frames
 * read in place; the device clamps starts[r] into [0, rows - k]); with starts null, width == d and
 * output row r is row r of src.  With g = row0 + r (its low 32 bits, and ctr's):
 *
 *   element normals  columns 4c .. 4c+3: p3d_vae_eps's construction over the Philox counter
 *                    (g, c, P3D_NOISE_SITE, ctr), key seed
 *   row block A      counter (g, 0, P3D_NOISE_ROW_SITE, ctr): the row is noised iff
 *                    A.x >= 0xB103AF11 = floor(Phi(0.5) 2^32) (30.85 % of the rows); the chosen
 *                    column is jc = ((uint64_t)A.y * width) >> 32, its joint starts at jid = jc - jc % 3
 *   row block B      counter (g, 1, P3D_NOISE_ROW_SITE, ctr) through the same Box-Muller: its first
 *                    three normals j0, j1, j2
 *
 * A row that is not noised is copied bit for bit.  A noised row gets, in float32 with every
 * operation rounded once, v[c] = x[c] + (e[c] * noise + offset) on every column and then
 * v[jid + k] = v[jid + k] + j_k * joint_scale for k = 0, 1, 2.
 * width a multiple of 12 in 12 .. 240 and of d, d a multiple of 4, 1 <= B <= 2^20, src and out
 * 16-byte aligned, rows >= B without starts.  Without starts out may be src (in place); in the
 * window form out may not overlap src.  Asynchronous, capturable.
 * P3D_NOISE_SITE = 0x4E4F49 and P3D_NOISE_ROW_SITE = 0x4E4F52 (the eps stream's site is 0x564145,
 * the dropout sites are < 64). */
int p3d_vae_add_noise(const float* src, int64_t rows, int32_t d,      /* table [rows, d] float32          */
                      const int64_t* starts, int32_t width, int64_t B,/* null: row r is src row r         */
                      uint64_t seed, uint64_t ctr, int64_t row0,
                      float noise, float offset, float joint_scale,
                      float* out /* [B, width] */, void* stream);
/* The same with the threshold word given (0 .. 2^32: 0 noises every row, 2^32 none).  For
 * measurements of what the clean rows' skipped Box-Muller saves; training code calls the above. */
int p3d_vae_add_noise_thr(const float* src, int64_t rows, int32_t d, const int64_t* starts, int32_t width,
                          int64_t B, uint64_t seed, uint64_t ctr, int64_t row0, float noise, float offset,
                          float joint_scale, uint64_t threshold, float* out, void* stream);
/* Bytes of the library-owned workspace a gradient over B rows uses (per-block partials; a wide
 * filter: the partials of the layers behind layer 0, plus h0 and dz0, 2 B enc_dims[0] floats). */
int64_t p3d_vae_workspace(const p3d_vae* v, int64_t B);

/* The input as a concatenation [seg 0 | seg 1 | ...] of up to four column segments, each a
 * resident table read row by row or through an index vector -- the reference's
 * tf.concat([inputs, out_3d, effnet_out], axis=1) (models.py:532-536) with the feature rows picked
 * by the epoch's permutation, formed inside the kernels instead of by a concat and a gather per
 * step.  The struct is read at the call.  The device clamps every index into [0, rows - 1]. */
typedef struct {
  int32_t n;                 /* 1 .. 4 segments, widths multiples of 8 summing to `in`            */
  const float* p[4];         /* device, 16-byte aligned; segment s is [rows_s, w[s]] row-major    */
  int32_t w[4];
  const int64_t* idx[4];     /* device [B] or null: row r of the input reads row idx[s][r]        */
  int64_t rows[4];           /* rows of segment s's table; idx values are clamped into it         */
} p3d_vae_cat;
/* The struct's checks against a filter of `in` inputs and a call of B rows (P3D_ERR_ARG and a
 * message): n, the widths and their sum, null or misaligned pointers, rows >= 1, and rows >= B for
 * a segment without an index.  Host only. */
int p3d_vae_cat_check(const p3d_vae_cat* cat, int32_t in, int64_t B);
/* p3d_vae_forward / _loss / _grad / _train_step with the segments in place of x: the bits of the
 * plain call on the materialised concatenation.  They serve narrow filters too ([x2d | out_3d],
 * in = 80, is the reference's use_2d alone).  On a wide filter the plain calls are the
 * one-segment, no-index case of the same kernels.
 * Bones filter: factors[4], loss[4] and row_terms [B, 4] as at the plain calls. */
int p3d_vae_forward_cat(p3d_vae* v, const p3d_vae_cat* cat, int64_t B, const float* eps, uint64_t ctr, float* y,
                        float* mean, float* log_var, float* z, const float* target, float* row_terms, void* stream);
int p3d_vae_loss_cat(p3d_vae* v, const p3d_vae_cat* cat, const float* t, int64_t B, const float* eps, uint64_t ctr,
                     const float* factors, float* loss3_dev, void* stream);
int p3d_vae_grad_cat(p3d_vae* v, const p3d_vae_cat* cat, const float* t, int64_t B, const float* eps, uint64_t ctr,
                     const float* factors, float* loss3_dev, void* stream);
int p3d_vae_train_step_cat(p3d_vae* v, const p3d_vae_cat* cat, const float* t, int64_t B, const float* eps,
                           const float* factors, float lr, float* loss3_dev, void* stream);

/* The temporal filter (in == seq_len * out, 1 <= seq_len <= 5) run as the reference's recurrence
 * (3d_pose_vae_filter_kin.py evaluate()) over S whole sequences in ONE launch:
 *
 *   buffer = [p_0] * seq_len
 *   per frame f: buffer = buffer[1:] + [p_f];  r_f = VAE(concat(buffer), eps_f);  buffer[-1] = r_f
 *
 * Row r of frame f is bit-identical to p3d_vae_forward on the same input and eps row.  eps null:
 * the Philox stream p3d_vae_eps(seed, ctr, eps_row0, N, ...) gives.  err_pred / err_ref are
 * mean_out (target - p_f)^2 and mean_out (target - r_f)^2 per frame (float32) and their
 * frame-ordered sums per sequence (double).  state / started carry the buffer's first seq_len - 1
 * groups across calls so that a stream can be filtered in chunks: started[s] == 0 primes the
 * buffer from the chunk's first frame and sets started[s] = 1.  Empty sequences write nothing
 * (their seq_err is 0) and leave their state untouched.  Asynchronous, capturable; all pointers
 * are device pointers, the float arrays 16-byte aligned.  S and N in 1 .. 2^20.
 * A bones filter has no sequence form: P3D_ERR_ARG. */
int p3d_vae_seq_filter(p3d_vae* v,
        const float* pred,          /* [N, out] lifter outputs, sequences concatenated          */
        const int64_t* seq_off,     /* device, [S + 1], non-decreasing, seq_off[0] = 0, [S] = N */
        int64_t S, int64_t N,
        const float* eps, uint64_t ctr, int64_t eps_row0,
        const float* target,        /* [N, out] or null                                          */
        float* state, int32_t* started,  /* [S, (seq_len-1) * out], [S]; both null = fresh, stateless */
        float* ref,                 /* [N, out]                                                  */
        float* frame_err,           /* [N, 2] {err_pred, err_ref} or null (needs target)         */
        double* seq_err,            /* [S, 2] frame-ordered sums of the above, or null           */
        void* stream);
/* form 0: one wave per 16-sequence tile; form 1 (the default, the faster one as measured): four
 * waves per tile, a layer's column tiles dealt among them.  Same bits either way. */
int p3d_vae_seq_set_form(p3d_vae* v, int32_t form);
/* Dynamic LDS bytes of the sequence kernel for a shape; 0 for a shape it does not serve.  Host only. */
int64_t p3d_vae_seq_lds_bytes(int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent,
                              int32_t n_dec, const int32_t* dec_dims, int32_t out, int32_t form);

/* The filter averaged over K posterior samples inside ONE launch (k_vae_fwd_mc / k_vae_fwd_mc_cat /
 * k_vae_seq4_mc, csrc/p3d_vae_mc.h): the encoder runs once per row, the decoder K times on the tile
 * that is already in LDS, and the statistics are folded in registers.  For a row with encoder
 * outputs mean, log_var and K draws eps_k, sample k is
 *
 *   y_k = decoder(eps_k * exp(0.5 log_var) + mean)
 *
 * in exactly p3d_vae_forward's arithmetic: with the caller's eps [K, B, latent], y_k has the bits
 * p3d_vae_forward writes for eps_k = eps[k]; with eps null, draw k uses the library's stream at
 * counter ctr + k (same seed, same site, row r of the call) and is the y of
 * p3d_vae_forward(..., eps = null, ctr + k).  Per output element, in float32 with every operation
 * rounded once and no division on the device:
 *
 *   m = y_0;  M = 0
 *   for k = 1 .. K - 1:   d = y_k - m;   m = m + d * c_k;   M = M + d * (y_k - m)
 *   y_mean = m            y_var = M * c_{K-1}            c_j = (float)(1.0 / (double)(j + 1))
 *
 * (y_var is the population variance of the K samples.)  K = 1 gives y_mean = y_0 bit for bit and
 * y_var = 0.  mean, log_var [B, latent] and y_var [B, out] are written when non-null.  B up to 2^20;
 * a wide filter needs B <= max_batch, as at p3d_vae_forward.  Asynchronous, capturable.
 * P3D_ERR_ARG ("p3d_vae_forward_mc: ..."), without touching the GPU: a null handle, a null y_mean,
 * K outside 1 .. 64, ctr == P3D_CTR_GLOBAL_STEP, and a bones filter: its outputs are lengths and
 * direction cosines, and direction cosines do not average. */
int p3d_vae_forward_mc(p3d_vae* v, const float* x, int64_t B, int32_t K,
                       const float* eps /* [K, B, latent] or null */, uint64_t ctr,
                       float* y_mean, float* y_var /* or null */,
                       float* mean, float* log_var /* or null */, void* stream);
/* The same with the segments in place of x: the bits of the plain call on the materialised
 * concatenation. */
int p3d_vae_forward_mc_cat(p3d_vae* v, const p3d_vae_cat* cat, int64_t B, int32_t K,
                           const float* eps /* [K, B, latent] or null */, uint64_t ctr,
                           float* y_mean, float* y_var /* or null */,
                           float* mean, float* log_var /* or null */, void* stream);
/* p3d_vae_seq_filter with r_f = the mean of K samples, fed back frame by frame inside the launch:
 *
 *   per frame f: buffer = buffer[1:] + [p_f];  (r_f, v_f) = (y_mean, y_var) of the K samples of
 *                VAE(concat(buffer)) as defined above;  buffer[-1] = r_f
 *
 * eps is [K, N, latent] (draw k of frame g at eps[k][g]), or null: draw k is the stream
 * p3d_vae_eps(seed, ctr + k, eps_row0, N, ...) gives.  ref [N, out] receives r_f, ref_var [N, out]
 * (or null) v_f; err_ref / seq_err are taken of r_f.  Row r of frame f has the bits of
 * p3d_vae_forward_mc on the same input and eps rows; K = 1 has the bits of p3d_vae_seq_filter.
 * state / started chunk a stream as there: chunks give the bits of one call.  The four-wave form
 * only.  P3D_ERR_ARG as above (a null ref for y_mean) and whatever p3d_vae_seq_filter refuses. */
int p3d_vae_seq_filter_mc(p3d_vae* v, const float* pred, const int64_t* seq_off, int64_t S, int64_t N,
                          int32_t K, const float* eps /* [K, N, latent] or null */, uint64_t ctr, int64_t eps_row0,
                          const float* target, float* state, int32_t* started,
                          float* ref, float* ref_var /* [N, out] or null */,
                          float* frame_err, double* seq_err, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* P3D_H_ */
