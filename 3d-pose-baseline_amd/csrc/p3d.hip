// p3d.hip -- MI355X (gfx950) kernels and the C ABI (include/p3d.h) of the 2D->3D
// pose-lifting MLP: the hot path of EsauPR/3d-pose-baseline src/linear_model.py.
//
// Kernels (one launch each, all on the caller's stream):
//   k_fwd        Y = epi(X*W + b): fp32 MFMA GEMM on fragment-major operands + fused
//                epilogue (max-norm scale, bias, BN eval|train (+moving-average update),
//                ReLU, Philox dropout, residual add).     linear_model.py:103-124,171-199
//   k_dgrad      dX = dZ*W^T (+ residual grad) fused with the PREVIOUS layer's
//                dropout/ReLU/BN backward -> dZ_prev, dgamma, dbeta.
//   k_wgrad      dW = X^T*dZ and db = colsum(dZ) (64x64 tiles, LDS staged).
//   k_adam       TF1 ApplyAdam over the flat trainable buffer.  linear_model.py:137,145
//   k_pack       W (TF layout) -> the two fragment-major operand copies Wf / Wd.
//   k_mse        loss = mean((y-t)^2), dy = 2(y-t)/(B*D).     linear_model.py:129
//   k_mpjpe      fused un-normalize + per-joint L2 (fp64).   predict_3dpose.py:399-430
//   k_dot_*      per-tensor reductions for --max_norm (||W||^2, <G,W>).
#include <hip/hip_ext.h>
#include "p3d_kernels.h"
#include "p3d_bf16.h"
#include "p3d_eval.h"
#include "p3d_gemm.h"
#include "p3d_data.h"
#include "p3d_sample.h"
#include "p3d_clip.h"
#include "p3d_clips.h"
#include "p3d_live.h"
#include "p3d_serve.h"
#include "p3d_serve6.h"
#include "p3d_serve_plan.h"
#include "p3d_gemv.h"
#include "p3d_xchg.h"
#include "../../include/p3d.h"

#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <cstdlib>
#include <mutex>
#include <string>
#include <unordered_set>
#include <vector>

#include "p3d_layers.h"
#include "p3d_vae.h"
#include "p3d_bones.h"
#include "p3d_vae_seq.h"
#include "p3d_vae_wide.h"
#include "p3d_vae_noise.h"
#include "p3d_vae_dec.h"
#include "p3d_vae_mc.h"

// =====================================================================================
// host side
// =====================================================================================
namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) return fail(P3D_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define LAUNCH_CHECK(what)                                                          \
  do {                                                                              \
    hipError_t e_ = hipGetLastError();                                              \
    if (e_ != hipSuccess) return fail(P3D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e_)); \
  } while (0)

int64_t pad64(int64_t n) { return (n + 63) / 64 * 64; }

// Host-side segment timing of serve_impl (dev builds: -DP3D_HOSTPROF; tools/host_prof.sh): per
// segment the summed steady-clock nanoseconds and count, printed at exit.
#ifdef P3D_HOSTPROF
#include <chrono>
struct HostProf {
  double ns[16] = {}; long n[16] = {};
  ~HostProf() {
    fprintf(stderr, "P3D_HOSTPROF");
    for (int i = 0; i < 16; ++i) if (n[i]) fprintf(stderr, " s%d=%.3fus", i, ns[i] / n[i] / 1000.0);
    fprintf(stderr, "\n");
  }
};
static HostProf g_hp;
#define HP_START auto hp_t = std::chrono::steady_clock::now();
#define HP(i) do { auto t_ = std::chrono::steady_clock::now(); \
    g_hp.ns[i] += std::chrono::duration<double, std::nano>(t_ - hp_t).count(); ++g_hp.n[i]; hp_t = t_; } while (0)
#else
#define HP_START
#define HP(i) do { } while (0)
#endif

struct Tensor {
  std::string name;
  int64_t numel;
  int64_t off;   // element offset (flat trainable buffer, or moving buffer for kind 1)
  int kind;      // 0 trainable, 1 moving stat
};

struct Layer {
  int K, N;
  int64_t w, b, gamma = -1, beta = -1;  // offsets in params
  int64_t mmean = -1, mvar = -1;        // offsets in moving
  int64_t wf, wd;                       // offsets in the packed-weight buffer
  int64_t wbf = -1;                     // bf16 models: offset (bf16 units) of packed Wt
  int64_t aff = -1;                     // bf16 models: offset of [inv | shift] (2N floats)
  int widx;                             // weight index (max-norm tables)
  int site;                             // dropout site; -1 for the output layer
  bool bn, relu;
};

}  // namespace

struct p3d_comm;
struct p3d_model {
  p3d_cfg cfg;
  std::vector<Tensor> tensors;
  std::vector<Layer> layers;  // in, A0, B0, ..., out
  int64_t n_flat = 0, n_moving = 0, n_wpk = 0;
  int64_t Bpad = 0;           // max_batch rounded up to 64 (packed row padding)
  float* flat[4] = {nullptr, nullptr, nullptr, nullptr};  // params, grads, m, v
  float* moving = nullptr;
  float* wpk = nullptr;       // packed weights (Wf, Wd per layer)
  float* ws = nullptr;        // activation workspace
  float* scratch = nullptr;   // reductions (max-norm)
  float* bnpart = nullptr;    // inside scratch: split BN-train row-tile partials
  float* lossp = nullptr;     // inside scratch: fused-MSE per-workgroup loss partials
  int nlossp = 0;
  float* loss_dst = nullptr;  // set during p3d_train_fwd_bwd: the backward folds the loss here
  const AdamFuse* fuse_adam = nullptr;  // set during p3d_train_step: Adam fused into the backward
  int adam_in_wgrad = 1;      // env P3D_FUSE_ADAM (default 1): p3d_train_step applies Adam inside k_wgrad_multi
                              // (bit-identical; measured slower than k_adam_pack at cfg3)
  float* dybuf = nullptr;     // [max_batch, output_size]: dy of the fused MSE
  int out_part = 1;           // training output layer as split-K partials + dy in its dgrad (env P3D_OUT_PART)
  float* opart = nullptr;     // [16 row tiles][4 column tiles][8] 1 KB partials (k_out_part)
  bool opart_pending = false; // the last training forward left the output layer to the backward's first launch
  const float* opart_t = nullptr;   // its targets and y (row-major, the caller's)
  float* opart_y = nullptr;
  int train_split = 1;        // BN-train layers as GEMM (256 WGs) + k_bn_fwd / k_bn_bwd (env P3D_TRAIN_SPLIT)
  int in_train_wk = 2;        // waves of the BN-train input-layer launch (exchange form; env P3D_IN_TRAIN_WK: 8, 4, 2)
  int dgrad_out_wk = 4;       // waves of the output layer's dgrad launch (K = 48; env P3D_DGRAD_OUT_WK: 8, 4)
  int xchg_wk = 8;            // BN-train hidden exchange-form forward: 8 waves with an 8-deep ring (measured and
                              // pruned in round 4: 16 waves 8.6 vs 6.8 us; rings of 4 / 2 within 1 %)
  int dgrad_wk = 16;          // hidden data-gradient tiling (env P3D_DGRAD_WK: 16 waves, else 8)
  int train_xchg = 1;         // split BN-train layers as ONE launch when the grid fits (env P3D_TRAIN_XCHG, p3d_xchg.h)
  int num_cus = 0;            // compute units of the device (exchange-form residency bound)
  unsigned* xsync = nullptr;  // exchange form: per site (layer, direction) L/16 column-tile epoch words (one
                              // 128-B line each), then per site P3D_XCHG_MAXR x L 16-B slots (p3d_xchg.h)
  int64_t xslots_off = 0;     // word offset of the slot arrays in xsync
  int xchg_delay = 0;         // test hook: late row-tile siblings (env P3D_XCHG_TEST_DELAY, p3d_xchg.h)
  int xchg_remap = 1;         // exchange launches as 1-D grids with the siblings on one XCD (env P3D_XCHG_REMAP)
  // error words the kernels write and the host reads without a device round trip (pinned, mapped):
  // [0] a BN-train exchange / split-K hand-off timed out, [1] a p3d_serve launch failed (1: a spin
  // ran out, 2: an XCD group smaller than the launch was sized for)
  int* errw = nullptr;        // host view
  int* xerr = nullptr;        // device view of errw[0]
  int* serve_err = nullptr;   // device view of errw[1]
  // completion word of the *_sync calls (errw[8]; p3d_serve_mse_sync, p3d_lift_sync): the launch's
  // last output writer stores the call's sequence number there once its host-memory outputs are
  // system-visible, and the host spins on it instead of waiting for the runtime's completion signal
  unsigned* hflag_dev = nullptr;   // device view of errw[8]
  unsigned hseq = 0;               // last sequence number issued
  unsigned hwait = 0;              // the sequence number the launch being built stores (0: none)
  bool harmed = false;             // the launch just built carries it
  unsigned* hcnt = nullptr;        // device arrival counter of those launches (zero between them);
                                   // [8]: p3d_host_signal's counter; [256, 512): the batch <= 4 chain's
                                   // squared differences (p3d_serve_mse's fused loss)
  // bf16 inference models (cfg5)
  unsigned short* wbf = nullptr;    // packed bf16 weights
  float* aff = nullptr;             // BN-eval affine per BN layer
  unsigned short* abf = nullptr;    // bf16 packed activations, one slab per layer (+ x slab)
  int64_t Mpad128 = 0;
  int bf16_stages = 48;             // hidden bf16 GEMM form (launch_bf16_layer; env P3D_BF16_STAGES: 48, 0)
  std::string bf16_kname;           // the kernel the last hidden bf16 layer ran (p3d_kernel_name 5)
  float* wsq = nullptr;       // [nW] ||W||^2
  float* gw = nullptr;        // [nW] <G,W>
  PackTable pt;
  UnpackTable ut;
  // --max_norm off: every optimizer reads the weights from Wd and leaves the TF-layout master
  // unwritten (AdamFuse::wsrc); w_stale marks a master behind Wd until p3d_params_sync (env
  // P3D_W_MASTER=1: the optimizers write the master, as before round 4)
  int w_pk = 1;
  bool w_stale = false;
  bool w_sticky = false;         // an optimizer was captured into a graph: its replays leave the masters
                                 // behind without this host code seeing it, so every sync re-derives them
  AdamTable at;
  int adam_blocks = 0;
  StepState* dstate = nullptr;  // device: global_step, beta powers, arrival counter
  DotTable wtab;
  // per-layer workspace (packed, Bpad rows)
  std::vector<float*> act;    // output of layer l (layer B_i holds the block output)
  std::vector<float*> z;      // pre-BN z of layer l
  std::vector<float*> bmean, bvar;
  std::vector<float*> dz;     // gradient wrt z of layer l
  float* dout[2] = {nullptr, nullptr};
  // training cache
  bool have_cache = false;
  const float* x_cached = nullptr;
  int64_t B_cached = 0;
  float keep = 1.f;
  uint64_t seed = 0, ctr = 0;
  int64_t row_off = 0;
  const int64_t* ctr_dev = nullptr;   // cached training-forward counter source
  // waves per inference workgroup (P3D_INFER_WK = 8 | 16).  8 waves x 94 VGPRs lets two
  // workgroups co-reside per CU, so independent batches on different streams overlap
  // (tools/streams_sweep2.py: 4 streams 5.6 M poses/s vs 4.9 M with 16-wave workgroups).
  int infer_wk = 82;        // inference tiling variant (launch_fwd_k), env P3D_INFER_WK
  int in_wk = 2, out_wk = 16; // input / output layer variants (env P3D_IN_WK, P3D_OUT_WK; 0 = infer_wk)
  int out_train_wk = 8;       // training output layer (fused MSE) variant (env P3D_OUT_TRAIN_WK)
  int train_wk = 8;         // waves per whole-batch BN-train workgroup (P3D_TRAIN_SPLIT=0 forms)
  int big_m = 256;          // inference hidden layers with M >= big_m use k_gemm_f32 (0: never)
  int gemv_maxb = 4;        // inference at B <= gemv_maxb runs the k_gemv layers (env P3D_GEMV_MAXB, 0..4)
  int gemv_fold = 1;        // ... with the input / output layers folded into the first / last hidden layer's
                            // launch (k_gemv_fold; env P3D_GEMV_FOLD; the same bits either way)
  int gemv_chain = 1;       // ... as ONE persistent launch where the hidden layers' tiles fit on the device
                            // (k_gemv_chain; env P3D_GEMV_CHAIN; the same bits; cfg2 batch 1: 16.3 vs 21.4 us)
  int gemv_slots = 0;       // workspace slots (ws_row / 16) the fold's hand-off buffer covers (others unfolded)
  int64_t gemv_slot_floats = 0;     // hand-off floats per slot (the chain's H layers, or the fold's one)
  float* gemv_hand = nullptr;       // [slot][layers][4 rows][L / 2] 16-B granules (layer-output hand-offs)
  float* lift_x = nullptr;          // p3d_lift's normalised rows and outputs where it runs the three steps
  float* lift_y = nullptr;
  unsigned* gemv_epoch = nullptr;   // [slot] epoch words, P3D_XCHG_EPOCH_STRIDE apart
  // persistent XCD-local evaluation (p3d_serve): per-XCD activation slabs, output partials,
  // census/barrier words and the spin-timeout flag; allocated at the first call
  float* serve_buf = nullptr;
  float* serve6_act = nullptr;   // k_serve6's activation slabs (4 per group, P3D_SERVE6_ROWS rows in all)
  float* serve_loss = nullptr;   // p3d_serve_mse: per-output-tile partials + the arrival counter
  float* serve_ecg = nullptr;      // k_serve6 epilogue-constant table (k_serve_prep), [layer][tile][48] + divisors
  bool serve_ec_dirty = true;      // parameters or moving statistics changed since the table was formed
  unsigned* serve_sync = nullptr;  // [k_serve6 bank 0 | bank 1 | k_serve5 bank | device epoch word ...]
  int serve_delay = 0, serve_delay_xcc = 0;  // test hook (env P3D_SERVE_TEST_DELAY=n[,xcc]): on odd-numbered
                                   // p3d_serve calls every workgroup on XCD xcc starts ~n x 3.4 us late
  int64_t serve_calls = 0;
  int serve_fault = 0;             // test hook: the census waits for one workgroup more than the grid
                                   // (env P3D_SERVE_TEST_FAULT): every launch fails its census
  int serve_grid = 0;
  int serve_groups = 0;     // at most this many groups take steps, 0 = all (env P3D_SERVE_GROUPS)
  // (k_serve5: two groups per XCD, two units per contraction, a 4-deep ring where L / 64 allows; the
  // other group counts, unit pairings and ring depths measured slower and were removed in round 6,
  // DESIGN 5a; k_serve, for models without residual blocks: 4 K slices, a 2-deep ring)
  std::vector<hipEvent_t> gev;   // per-bucket gradient-ready events (p3d_grad_buckets / p3d_grad_events)
  std::vector<hipEvent_t> aev;   // per-bucket "parameters free" events: the backward's last reader of the
                                 // bucket's parameters (dgrad of its lowest layer) has been issued
  std::vector<AdamTable> bat;    // per-bucket optimizer tables (p3d_adam_apply_bucket)
  std::vector<int> bat_blocks;
  std::vector<int> bucket_lo;    // lowest layer of each bucket, buckets in backward order (layers hi..lo)
  const AdamFuse* alpha_af = nullptr;  // set during p3d_train_fwd_bwd_lr: the backward forms the step's alpha
  AdamFuse dp_af{};              // hyper-parameters of the last p3d_train_fwd_bwd_lr (p3d_adam_apply)
  bool alpha_ready = false;      // the last backward formed alpha_dev (p3d_adam_apply reads it)
  int wgrad_multi = 1;           // all layers' dW in one k_wgrad_multi launch (env P3D_WGRAD_MULTI)
                                 // (measured and rejected, round 3: two adjacent 64x64 tiles per
                                 // workgroup, 528 workgroups in one round instead of 768 + 288:
                                 // 29.7 vs 28.4 us -- the launch is bound by its 148 MB HBM stream)
  // (measured and removed, round 6: weight-gradient + Adam tiles riding the data-gradient launches,
  // 109.5 vs 102.2 us per cfg3 step; each layer's on a side stream, 197-202 vs 122 us -- DESIGN 5c)
  float* alpha_dev = nullptr;    // the step's Adam alpha, formed by the first backward launch
  bool step_advanced = false;    // set by a backward whose last launch advanced the step state
  ServeKnobs serve_knobs;   // env P3D_SERVE6* (p3d_serve_plan.h)
  // the last launch's choice, by (batch, with loss): serve_plan prices 64 candidates, redone only
  // when the key changes -- the host enqueue of a serving loop
  int64_t serve_B = -1;
  bool serve_with_loss = false;
  ServeChoice serve_choice;
  // data-parallel step with the library's own all-reduce (p3d_dp.h)
  p3d_comm* comm = nullptr;      // not owned (p3d_comm_create / p3d_comm_destroy)
  hipStream_t cst = nullptr;     // comm stream (non-blocking), forked from / joined to the caller's stream
  hipEvent_t cjoin = nullptr;    // join event of the comm-stream optimizer form (P3D_DP_ADAM=2)
  std::vector<hipEvent_t> rev;   // per-bucket "all-reduce done" events
  int dp_adam = 1;               // env P3D_DP_ADAM: 1 per-bucket optimizer on the compute stream behind its
                                 // all-reduce, 0 one optimizer pass after the last bucket, 2 per bucket on the
                                 // comm stream (round 3's form: slows the neighbouring dgrad launches)
  int dp_force_multi = 0;        // env P3D_DP_FORCE_MULTI=1 (tests, bench): a 1-rank group takes the N > 1 form
                                 // -- comm-stream fork, per-bucket ncclAvg, rev joins -- so the single-GPU box
                                 // executes and times the code every rank of an 8-GPU run executes
  // live kernel timing (p3d_profile_start/stop): one hipEvent pair per launch
  bool prof = false;
  std::vector<hipEvent_t> ev;
  std::vector<const char*> ev_tag;
  size_t ev_used = 0;
};

namespace {
struct ProfScope {  // times one kernel launch when profiling (p3d_profile_start/stop)
  p3d_model* m; hipEvent_t e0, e1; bool on;
  ProfScope(p3d_model* m_, const char* tag) : m(m_), e0(nullptr), e1(nullptr), on(false) {
    if (m && m->prof && 2 * (m->ev_used + 1) <= m->ev.size()) {
      on = true;
      m->ev_tag[m->ev_used] = tag;
      e0 = m->ev[2 * m->ev_used];
      e1 = m->ev[2 * m->ev_used + 1];
    }
  }
  ~ProfScope() {
    if (on) ++m->ev_used;
  }
};

// Launch `k`; under profiling the event pair is attached to the dispatch itself
// (hipExtLaunchKernel start/stop events = the AQL packet's begin/end timestamps, the
// same interval rocprofv3 --kernel-trace reports), not recorded as separate packets.
template <typename F, typename... A>
void go(const ProfScope& ps, F k, dim3 grid, dim3 block, hipStream_t st, A... args) {
  if (ps.on) hipExtLaunchKernelGGL(k, grid, block, 0, st, ps.e0, ps.e1, 0, args...);
  else k<<<grid, block, 0, st>>>(args...);
}

// An optimizer is issued that leaves the TF-layout masters behind Wd (AdamFuse::wsrc).
void mark_w_stale(p3d_model* m, hipStream_t st) {
  if (!m->w_pk) return;
  m->w_stale = true;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) m->w_sticky = true;
}

void free_all(p3d_model* m) {
  for (auto e : m->ev) (void)hipEventDestroy(e);
  for (auto& p : m->flat) if (p) (void)hipFree(p);
  if (m->moving) (void)hipFree(m->moving);
  if (m->wpk) (void)hipFree(m->wpk);
  if (m->ws) (void)hipFree(m->ws);
  if (m->scratch) (void)hipFree(m->scratch);
  if (m->opart) (void)hipFree(m->opart);
  if (m->dstate) (void)hipFree(m->dstate);
  if (m->wbf) (void)hipFree(m->wbf);
  if (m->aff) (void)hipFree(m->aff);
  if (m->abf) (void)hipFree(m->abf);
  if (m->serve_buf) (void)hipFree(m->serve_buf);
  if (m->serve6_act) (void)hipFree(m->serve6_act);
  if (m->serve_loss) (void)hipFree(m->serve_loss);
  if (m->serve_sync) (void)hipFree(m->serve_sync);
  if (m->serve_ecg) (void)hipFree(m->serve_ecg);
  if (m->xsync) (void)hipFree(m->xsync);
  if (m->gemv_hand) (void)hipFree(m->gemv_hand);
  if (m->lift_x) (void)hipFree(m->lift_x);
  if (m->lift_y) (void)hipFree(m->lift_y);
  if (m->gemv_epoch) (void)hipFree(m->gemv_epoch);
  if (m->errw) (void)hipHostFree(m->errw);
  if (m->alpha_dev) (void)hipFree(m->alpha_dev);
  if (m->hcnt) (void)hipFree(m->hcnt);
  for (hipEvent_t e : m->rev) (void)hipEventDestroy(e);
  m->rev.clear();
  if (m->cjoin) (void)hipEventDestroy(m->cjoin);
  m->cjoin = nullptr;
  if (m->cst) (void)hipStreamDestroy(m->cst);
  m->cst = nullptr;
}
// ---- teardown in any order -------------------------------------------------------------
// A model's device memory must go while the HIP runtime is alive and nothing still runs on
// it.  p3d_destroy synchronises the device before freeing (kernels of an aborted step may
// still be queued), and the first p3d_create registers a process-exit handler that releases
// every model still alive.  That handler runs before the HIP runtime's own teardown (exit
// handlers run in reverse order of registration, and the runtime registered its own when it
// was initialised, before any model existed); a p3d_destroy arriving after it -- a Python
// finaliser during interpreter teardown -- finds the model gone and touches nothing.
std::mutex g_live_mu;
std::unordered_set<p3d_model*>* g_live = nullptr;
bool g_exit_hooked = false;

void release_model(p3d_model* m) {
  (void)hipDeviceSynchronize();
  for (hipEvent_t e : m->gev) (void)hipEventDestroy(e);
  for (hipEvent_t e : m->aev) (void)hipEventDestroy(e);
  free_all(m);
  delete m;
}

void release_live_models_at_exit() {
  std::unordered_set<p3d_model*> live;
  {
    std::lock_guard<std::mutex> g(g_live_mu);
    if (g_live) live.swap(*g_live);
  }
  for (p3d_model* m : live) release_model(m);
}

void live_models_add(p3d_model* m) {
  std::lock_guard<std::mutex> g(g_live_mu);
  if (!g_live) g_live = new std::unordered_set<p3d_model*>();
  g_live->insert(m);
  if (!g_exit_hooked) {
    g_exit_hooked = true;
    std::atexit(release_live_models_at_exit);
  }
}

bool live_models_remove(p3d_model* m) {
  std::lock_guard<std::mutex> g(g_live_mu);
  return g_live && g_live->erase(m) > 0;
}
}  // namespace

extern "C" const char* p3d_last_error(void) { return g_err.c_str(); }

extern "C" int p3d_create(const p3d_cfg* cfg_in, p3d_model** out) {
  if (!cfg_in || !out) return fail(P3D_ERR_ARG, "p3d_create: null argument");
  const p3d_cfg c = *cfg_in;
  if (c.linear_size <= 0 || c.linear_size % 64 != 0)
    return fail(P3D_ERR_ARG, "linear_size must be a positive multiple of 64");
  if (c.num_layers < 0) return fail(P3D_ERR_ARG, "num_layers must be >= 0");
  if (c.input_size <= 0 || c.input_size % 16 != 0)
    return fail(P3D_ERR_ARG, "input_size must be a positive multiple of 16");
  if (c.output_size <= 0) return fail(P3D_ERR_ARG, "output_size must be positive");
  if (c.max_batch <= 0) return fail(P3D_ERR_ARG, "max_batch must be positive");
  if (c.dtype != P3D_DTYPE_F32 && c.dtype != P3D_DTYPE_BF16) return fail(P3D_ERR_ARG, "dtype must be F32 or BF16");
  if (c.dtype == P3D_DTYPE_BF16 && (c.linear_size % 128 != 0 || c.input_size % 32 != 0))
    return fail(P3D_ERR_ARG, "bf16 models need linear_size % 128 == 0 and input_size % 32 == 0");
  p3d_model* m = new p3d_model();
  m->cfg = c;
  const int L = c.linear_size;
  m->Bpad = pad64(c.max_batch);
  auto add = [&](const std::string& name, int64_t n) {
    Tensor t{name, n, m->n_flat, 0};
    m->n_flat += pad64(n);
    m->tensors.push_back(t);
    return t.off;
  };
  auto addm = [&](const std::string& name, int64_t n) {
    Tensor t{name, n, m->n_moving, 1};
    m->n_moving += pad64(n);
    m->tensors.push_back(t);
    return t.off;
  };
  // trainables in TF creation order (linear_model.py:103-124, 171-193)
  std::vector<std::string> bn_scope;
  Layer lin{};
  lin.K = c.input_size; lin.N = L; lin.site = 0; lin.bn = c.batch_norm; lin.relu = true;
  lin.w = add("linear_model/w1", (int64_t)c.input_size * L);
  lin.b = add("linear_model/b1", L);
  if (c.batch_norm) {
    lin.gamma = add("linear_model/batch_normalization/gamma", L);
    lin.beta = add("linear_model/batch_normalization/beta", L);
    bn_scope.push_back("linear_model/batch_normalization");
  }
  m->layers.push_back(lin);
  for (int i = 0; i < c.num_layers; ++i) {
    const std::string s = "linear_model/two_linear_" + std::to_string(i) + "/";
    for (int h = 0; h < 2; ++h) {
      Layer ly{};
      ly.K = L; ly.N = L; ly.site = 1 + 2 * i + h; ly.bn = c.batch_norm; ly.relu = true;
      const std::string wn = (h == 0 ? "w2_" : "w3_") + std::to_string(i);
      const std::string bnm = (h == 0 ? "b2_" : "b3_") + std::to_string(i);
      ly.w = add(s + wn, (int64_t)L * L);
      ly.b = add(s + bnm, L);
      if (c.batch_norm) {
        const std::string sc = s + "batch_normalization" + std::to_string(h + 1) + std::to_string(i);
        ly.gamma = add(sc + "/gamma", L);
        ly.beta = add(sc + "/beta", L);
        bn_scope.push_back(sc);
      }
      m->layers.push_back(ly);
    }
  }
  Layer lo{};
  lo.K = L; lo.N = c.output_size; lo.site = -1; lo.bn = false; lo.relu = false;
  lo.w = add("linear_model/w4", (int64_t)L * c.output_size);
  lo.b = add("linear_model/b4", c.output_size);
  m->layers.push_back(lo);
  if (c.batch_norm) {
    for (size_t l = 0; l + 1 < m->layers.size(); ++l) {
      m->layers[l].mmean = addm(bn_scope[l] + "/moving_mean", L);
      m->layers[l].mvar = addm(bn_scope[l] + "/moving_variance", L);
    }
  }
  // packed-weight buffer and tables
  m->pt.n = 0;
  m->ut.n = 0;
  m->ut.begin[0] = 0;
  m->wtab.n = 0;
  int64_t f4 = 0;
  for (size_t l = 0; l < m->layers.size(); ++l) {
    Layer& ly = m->layers[l];
    const int K = ly.K, N = ly.N, NP = (N + 15) / 16 * 16;
    const int t = m->pt.n++;
    if (t >= P3D_MAX_W) { delete m; return fail(P3D_ERR_ARG, "too many layers"); }
    ly.wf = m->n_wpk; m->n_wpk += pad64((int64_t)NP * K);
    ly.wd = m->n_wpk; m->n_wpk += pad64((int64_t)NP * K);
    m->pt.K[t] = K; m->pt.N[t] = N;
    m->pt.src[t] = ly.w; m->pt.dstf[t] = ly.wf; m->pt.dstd[t] = ly.wd;
    m->pt.begin[t] = f4;
    f4 += 2 * (int64_t)NP * K / 4;
    m->ut.N[t] = N; m->ut.src[t] = ly.w; m->ut.dstd[t] = ly.wd;
    m->ut.begin[t + 1] = m->ut.begin[t] + (int64_t)K * N;
    m->ut.n = t + 1;
    ly.widx = t;
    m->wtab.off[t] = ly.w;
    m->wtab.len[t] = (int64_t)K * N;
    m->wtab.n = t + 1;
  }
  m->pt.begin[m->pt.n] = f4;
  // optimizer table: weight matrices as 16x16 tiles, everything else as 1-D vectors
  {
    AdamTable& at = m->at;
    at.nw = 0; at.nv = 0;
    int tiles = 0, vch = 0;
    for (size_t l = 0; l < m->layers.size(); ++l) {
      const Layer& ly = m->layers[l];
      const int t = at.nw++;
      at.K[t] = ly.K; at.N[t] = ly.N; at.off[t] = ly.w; at.wf[t] = ly.wf; at.wd[t] = ly.wd;
      at.tile_begin[t] = tiles;
      tiles += ((ly.K + 63) / 64) * ((ly.N + 63) / 64);
    }
    at.tile_begin[at.nw] = tiles;
    for (const Tensor& tn : m->tensors) {
      if (tn.kind != 0) continue;
      bool is_w = false;
      for (const Layer& ly : m->layers) if (ly.w == tn.off) is_w = true;
      if (is_w) continue;
      if (at.nv >= P3D_MAX_V) { delete m; return fail(P3D_ERR_ARG, "too many parameter vectors"); }
      at.voff[at.nv] = tn.off; at.vlen[at.nv] = (int)tn.numel; at.vbegin[at.nv] = vch;
      vch += (int)((tn.numel + 1023) / 1024);
      at.nv++;
    }
    at.vbegin[at.nv] = vch;
    m->adam_blocks = tiles + vch;
  }

  auto cleanup = [&](hipError_t e) {
    g_err = std::string("p3d_create: ") + hipGetErrorString(e);
    free_all(m);
    delete m;
    return P3D_ERR_HIP;
  };
  hipError_t e;
  for (int k = 0; k < 4; ++k) {
    if ((e = hipMalloc(&m->flat[k], m->n_flat * sizeof(float))) != hipSuccess) return cleanup(e);
    if ((e = hipMemset(m->flat[k], 0, m->n_flat * sizeof(float))) != hipSuccess) return cleanup(e);
  }
  if ((e = hipMalloc(&m->moving, (m->n_moving + 64) * sizeof(float))) != hipSuccess) return cleanup(e);
  if ((e = hipMemset(m->moving, 0, (m->n_moving + 64) * sizeof(float))) != hipSuccess) return cleanup(e);
  if ((e = hipMalloc(&m->wpk, m->n_wpk * sizeof(float))) != hipSuccess) return cleanup(e);
  if ((e = hipMemset(m->wpk, 0, m->n_wpk * sizeof(float))) != hipSuccess) return cleanup(e);
  // workspace: per hidden layer act, z, dz (packed [Bpad, L]); stats; dout x2
  const int64_t Bp = m->Bpad;
  const int nl = (int)m->layers.size();
  int64_t need = 0;
  for (int l = 0; l < nl - 1; ++l) need += 3 * pad64(Bp * L) + 2 * pad64(L);
  need += 2 * pad64(Bp * L);
  if ((e = hipMalloc(&m->ws, need * sizeof(float))) != hipSuccess) return cleanup(e);
  if ((e = hipMemset(m->ws, 0, need * sizeof(float))) != hipSuccess) return cleanup(e);
  float* cur = m->ws;
  m->act.assign(nl, nullptr); m->z.assign(nl, nullptr); m->dz.assign(nl, nullptr);
  m->bmean.assign(nl, nullptr); m->bvar.assign(nl, nullptr);
  for (int l = 0; l < nl - 1; ++l) {
    m->act[l] = cur; cur += pad64(Bp * L);
    m->z[l] = cur; cur += pad64(Bp * L);
    m->dz[l] = cur; cur += pad64(Bp * L);
    m->bmean[l] = cur; cur += pad64(L);
    m->bvar[l] = cur; cur += pad64(L);
  }
  m->dout[0] = cur; cur += pad64(Bp * L);
  m->dout[1] = cur; cur += pad64(Bp * L);
  // split BN-train partials [R][L][2] and fused-MSE loss partials for R = max_batch/16 row tiles
  const int64_t R_max = (c.max_batch + 15) / 16;
  const int64_t nlossp_max = pad64(R_max * ((c.output_size + 15) / 16));
  const int64_t scratch_n = (int64_t)P3D_MAX_W * DOT_CHUNKS + 2 * 64 + R_max * 2 * (int64_t)L + nlossp_max +
                            pad64((int64_t)c.max_batch * ((c.output_size + 15) / 16 * 16));
  if ((e = hipMalloc(&m->scratch, scratch_n * sizeof(float))) != hipSuccess) return cleanup(e);
  if ((e = hipMemset(m->scratch, 0, scratch_n * sizeof(float))) != hipSuccess) return cleanup(e);
  if ((e = hipMalloc(&m->opart, (size_t)16 * 4 * 8 * 256 * sizeof(float))) != hipSuccess) return cleanup(e);
  if (const char* ev = getenv("P3D_OUT_PART")) m->out_part = atoi(ev);
  if (const char* ev = getenv("P3D_INFER_WK")) m->infer_wk = atoi(ev);
  if (const char* ev = getenv("P3D_IN_WK")) m->in_wk = atoi(ev);
  if (const char* ev = getenv("P3D_OUT_WK")) m->out_wk = atoi(ev);
  if (const char* ev = getenv("P3D_OUT_TRAIN_WK")) m->out_train_wk = atoi(ev);
  if (const char* ev = getenv("P3D_BIG_M")) m->big_m = atoi(ev);
  if (const char* ev = getenv("P3D_GEMV_MAXB")) m->gemv_maxb = std::max(0, std::min(4, atoi(ev)));
  if (const char* ev = getenv("P3D_GEMV_FOLD")) m->gemv_fold = atoi(ev);
  if (const char* ev = getenv("P3D_GEMV_CHAIN")) m->gemv_chain = atoi(ev);
  if (const char* ev = getenv("P3D_TRAIN_SPLIT")) m->train_split = atoi(ev);
  if (const char* ev = getenv("P3D_IN_TRAIN_WK")) m->in_train_wk = atoi(ev);
  if (const char* ev = getenv("P3D_DGRAD_OUT_WK")) m->dgrad_out_wk = atoi(ev);
  if (const char* ev = getenv("P3D_DGRAD_WK")) m->dgrad_wk = atoi(ev);
  if (const char* ev = getenv("P3D_TRAIN_XCHG")) m->train_xchg = atoi(ev);
  {
    int dev = 0;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return cleanup(e);
    if ((e = hipDeviceGetAttribute(&m->num_cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess)
      return cleanup(e);
    m->xslots_off = (int64_t)2 * nl * (L / 16) * P3D_XCHG_EPOCH_STRIDE;
    const int64_t nx = m->xslots_off + (int64_t)2 * 2 * nl * P3D_XCHG_MAXR * L * 4;   // sc1 + plain copies
    if ((e = hipMalloc(&m->xsync, nx * sizeof(unsigned))) != hipSuccess) return cleanup(e);
    if ((e = hipMemset(m->xsync, 0, nx * sizeof(unsigned))) != hipSuccess) return cleanup(e);
    if (m->gemv_fold && m->gemv_maxb > 0 && c.dtype == P3D_DTYPE_F32 && L <= P3D_GEMV_FOLD_MAXK) {
      // batch <= 4 fold: the first 64 workspace slots (ws_row < 1024) get a hand-off area of
      // 4 rows x L / 2 granules (32 KB at L = 1024) and an epoch word each
      m->gemv_slots = (int)std::min<int64_t>(64, (c.max_batch + 15) / 16);
      const int H = nl - 2;
      const bool chain = H >= 1 && H <= P3D_GEMV_CHAIN_MAXH && L <= P3D_GEMV_CHAIN_MAXK && H * (L / 16) <= m->num_cus;
      m->gemv_slot_floats = (int64_t)(chain ? H + 1 : 1) * 4 * (L / 2) * 4;
      const int64_t nh = (int64_t)m->gemv_slots * m->gemv_slot_floats;
      if ((e = hipMalloc(&m->gemv_hand, nh * sizeof(float))) != hipSuccess) return cleanup(e);
      if ((e = hipMemset(m->gemv_hand, 0, nh * sizeof(float))) != hipSuccess) return cleanup(e);
      const int64_t ne = (int64_t)m->gemv_slots * P3D_XCHG_EPOCH_STRIDE;
      if ((e = hipMalloc(&m->gemv_epoch, ne * sizeof(unsigned))) != hipSuccess) return cleanup(e);
      if ((e = hipMemset(m->gemv_epoch, 0, ne * sizeof(unsigned))) != hipSuccess) return cleanup(e);
    }
    if (c.dtype == P3D_DTYPE_F32) {
      // p3d_lift's three-step form (any batch; every float32 model, whether or not the batch <= 4
      // fold / chain is configured): normalised rows and network outputs
      if ((e = hipMalloc(&m->lift_x, (size_t)c.max_batch * c.input_size * sizeof(float))) != hipSuccess) return cleanup(e);
      if ((e = hipMalloc(&m->lift_y, (size_t)c.max_batch * c.output_size * sizeof(float))) != hipSuccess) return cleanup(e);
    }
    if ((e = hipHostMalloc((void**)&m->errw, 64 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess)
      return cleanup(e);
    memset(m->errw, 0, 64 * sizeof(int));
    int* dv = nullptr;
    if ((e = hipHostGetDevicePointer((void**)&dv, m->errw, 0)) != hipSuccess) return cleanup(e);
    m->xerr = dv;
    m->serve_err = dv + 1;
    m->hflag_dev = (unsigned*)(dv + 8);
  }
  if (const char* ev = getenv("P3D_XCHG_TEST_DELAY")) m->xchg_delay = atoi(ev);
  if (const char* ev = getenv("P3D_DP_ADAM")) m->dp_adam = atoi(ev);
  if (const char* ev = getenv("P3D_DP_FORCE_MULTI")) m->dp_force_multi = atoi(ev) != 0;
  if (const char* ev = getenv("P3D_W_MASTER")) m->w_pk = atoi(ev) ? 0 : 1;
  if (m->cfg.max_norm) m->w_pk = 0;   // (||W||^2 of the max-norm scale is summed over the master)
  if (const char* ev = getenv("P3D_XCHG_REMAP")) m->xchg_remap = atoi(ev);
  if (const char* ev = getenv("P3D_SERVE_TEST_FAULT")) m->serve_fault = atoi(ev);
  if (const char* ev = getenv("P3D_SERVE_TEST_DELAY")) {
    m->serve_delay = atoi(ev);
    if (const char* c = strchr(ev, ',')) m->serve_delay_xcc = atoi(c + 1) & 7;
  }
  if (const char* ev = getenv("P3D_FUSE_ADAM")) m->adam_in_wgrad = atoi(ev);
  if (const char* ev = getenv("P3D_WGRAD_MULTI")) m->wgrad_multi = atoi(ev);
  if ((e = hipMalloc(&m->alpha_dev, 64 * sizeof(float))) != hipSuccess) return cleanup(e);
  if ((e = hipMalloc(&m->hcnt, 512 * sizeof(unsigned))) != hipSuccess) return cleanup(e);
  if ((e = hipMemset(m->hcnt, 0, 512 * sizeof(unsigned))) != hipSuccess) return cleanup(e);
  if (const char* ev = getenv("P3D_SERVE_GROUPS")) m->serve_groups = atoi(ev);
  m->serve_knobs = serve_knobs_from_env();
  {
    StepState s0{};
    s0.global_step = 0; s0.beta1_power = 0.9f; s0.beta2_power = 0.999f; s0.arrivals = 0;
    if ((e = hipMalloc(&m->dstate, sizeof(StepState))) != hipSuccess) return cleanup(e);
    if ((e = hipMemcpy(m->dstate, &s0, sizeof(StepState), hipMemcpyHostToDevice)) != hipSuccess) return cleanup(e);
  }
  m->wsq = m->scratch + P3D_MAX_W * DOT_CHUNKS;
  m->gw = m->wsq + 64;
  m->bnpart = m->gw + 64;   // [R_max row tiles][L][2]: split BN-train partial moments / sums
  m->lossp = m->bnpart + R_max * 2 * (int64_t)L;
  m->dybuf = m->lossp + nlossp_max;
  // TF defaults: BN gamma = 1, moving_variance = 1 (beta/mean = 0 already)
  if (c.batch_norm) {
    std::vector<float> ones(L, 1.0f);
    for (int l = 0; l < nl - 1; ++l) {
      if ((e = hipMemcpy(m->flat[0] + m->layers[l].gamma, ones.data(), L * 4, hipMemcpyHostToDevice)) != hipSuccess)
        return cleanup(e);
      if ((e = hipMemcpy(m->moving + m->layers[l].mvar, ones.data(), L * 4, hipMemcpyHostToDevice)) != hipSuccess)
        return cleanup(e);
    }
  }
  if (c.dtype == P3D_DTYPE_BF16) {
    int64_t nbf = 0, naff = 0;
    for (auto& ly : m->layers) {
      const int NP = (ly.N + 15) / 16 * 16;
      ly.wbf = nbf; nbf += pad64((int64_t)NP * ly.K);
      if (ly.bn) { ly.aff = naff; naff += 2 * pad64(ly.N); }
    }
    m->Mpad128 = (c.max_batch + 127) / 128 * 128;
    if (const char* ev = getenv("P3D_BF16_STAGES")) m->bf16_stages = atoi(ev);
    const int64_t slab = m->Mpad128 * L;  // bf16 elements per activation slab
    if ((e = hipMalloc(&m->wbf, nbf * 2)) != hipSuccess) return cleanup(e);
    if ((e = hipMemset(m->wbf, 0, nbf * 2)) != hipSuccess) return cleanup(e);
    if ((e = hipMalloc(&m->aff, (naff + 64) * 4)) != hipSuccess) return cleanup(e);
    if ((e = hipMalloc(&m->abf, (int64_t)(nl + 1) * slab * 2)) != hipSuccess) return cleanup(e);
    if ((e = hipMemset(m->abf, 0, (int64_t)(nl + 1) * slab * 2)) != hipSuccess) return cleanup(e);
  }
  live_models_add(m);
  *out = m;
  return P3D_OK;
}

extern "C" int p3d_destroy(p3d_model* m) {
  if (!m) return P3D_OK;
  if (!live_models_remove(m)) return P3D_OK;   // released already (process exit)
  release_model(m);
  return P3D_OK;
}

extern "C" int p3d_param_count(const p3d_model* m, int32_t* count) {
  if (!m || !count) return fail(P3D_ERR_ARG, "null argument");
  *count = (int32_t)m->tensors.size();
  return P3D_OK;
}

extern "C" int p3d_param_info(const p3d_model* m, int32_t idx, const char** name, int64_t* numel,
                              int32_t* kind, int64_t* offset) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  if (idx < 0 || idx >= (int32_t)m->tensors.size()) return fail(P3D_ERR_ARG, "param index out of range");
  const Tensor& t = m->tensors[idx];
  if (name) *name = t.name.c_str();
  if (numel) *numel = t.numel;
  if (kind) *kind = t.kind;
  if (offset) *offset = t.off;
  return P3D_OK;
}

extern "C" int p3d_param_ptr(p3d_model* m, const char* name, void** dptr, int64_t* numel) {
  if (!m || !name || !dptr) return fail(P3D_ERR_ARG, "null argument");
  for (const Tensor& t : m->tensors) {
    if (t.name == name) {
      *dptr = (t.kind == 0 ? m->flat[0] : m->moving) + t.off;
      if (numel) *numel = t.numel;
      return P3D_OK;
    }
  }
  return fail(P3D_ERR_NOTFOUND, std::string("unknown parameter: ") + name);
}

extern "C" int p3d_flat_ptr(p3d_model* m, int32_t which, void** dptr, int64_t* numel) {
  if (!m || !dptr) return fail(P3D_ERR_ARG, "null argument");
  if (which >= 0 && which < 4) {
    *dptr = m->flat[which];
    if (numel) *numel = m->n_flat;
    return P3D_OK;
  }
  if (which == 4) {
    *dptr = m->moving;
    if (numel) *numel = m->n_moving;
    return P3D_OK;
  }
  return fail(P3D_ERR_ARG, "p3d_flat_ptr: which must be 0..4");
}

static int refresh_derived(p3d_model* m, hipStream_t st) {
  m->serve_ec_dirty = true;
  if (m->cfg.dtype == P3D_DTYPE_BF16) {
    for (const Layer& ly : m->layers) {
      const int NP = (ly.N + 15) / 16 * 16;
      const int64_t items = (int64_t)(NP / 16) * (ly.K / 32) * 64;
      k_pack_bf16<<<(unsigned)((items + 255) / 256), 256, 0, st>>>(m->flat[0] + ly.w, ly.K, ly.N, m->wbf + ly.wbf);
      LAUNCH_CHECK("k_pack_bf16");
      if (ly.bn) {
        k_bn_affine<<<(ly.N + 255) / 256, 256, 0, st>>>(m->flat[0] + ly.gamma, m->flat[0] + ly.beta,
                                                        m->moving + ly.mmean, m->moving + ly.mvar, m->cfg.bn_eps,
                                                        ly.N, m->aff + ly.aff, m->aff + ly.aff + ly.N);
        LAUNCH_CHECK("k_bn_affine");
      }
    }
  }
  const int64_t n4 = m->pt.begin[m->pt.n];
  {
    ProfScope ps(m, "pack");
    go(ps, k_pack, dim3((unsigned)((n4 + 255) / 256)), dim3(256), st, (const float*)m->flat[0], m->wpk, m->pt);
  }
  LAUNCH_CHECK("k_pack");
  if (m->cfg.max_norm) {
    k_dot_partial<<<dim3(DOT_CHUNKS, m->wtab.n), 256, 0, st>>>(m->flat[0], m->flat[0], m->wtab, m->scratch);
    LAUNCH_CHECK("k_dot_partial");
    k_dot_final<<<1, 64, 0, st>>>(m->scratch, m->wtab.n, m->wsq);
    LAUNCH_CHECK("k_dot_final");
  }
  return P3D_OK;
}

// The TF-layout weight masters, re-derived from Wd if an optimizer left them behind (w_stale).
// (mark_w_stale is defined next to the model: the optimizers call it when they skip the masters.)
static int ensure_w(p3d_model* m, hipStream_t st) {
  if (!m->w_stale && !m->w_sticky) return P3D_OK;
  const int64_t n = m->ut.begin[m->ut.n];
  {
    ProfScope ps(m, "unpack_w");
    go(ps, k_unpack_w, dim3((unsigned)((n + 255) / 256)), dim3(256), st, (const float*)m->wpk, m->flat[0], m->ut);
  }
  LAUNCH_CHECK("k_unpack_w");
  m->w_stale = false;
  return P3D_OK;
}

extern "C" int p3d_params_sync(p3d_model* m, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  return ensure_w(m, (hipStream_t)stream);
}

extern "C" int p3d_params_updated(p3d_model* m, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  // the host wrote the masters it holds: they must not have been behind Wd (it syncs first)
  if (m->w_stale) return fail(P3D_ERR_STATE, "p3d_params_updated: weight masters were stale (p3d_params_sync "
                                             "before writing parameters)");
  return refresh_derived(m, (hipStream_t)stream);
}

// Device-side parameter changes the host did not see issued (a replayed graph of training
// steps: the kernels ran, this library's host code did not): tables derived from the
// parameters on the host's schedule -- k_serve6's epilogue constants -- are re-formed at their
// next use.  No device work.
extern "C" int p3d_params_changed(p3d_model* m) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  m->serve_ec_dirty = true;
  return P3D_OK;
}

// ---- launch helpers ------------------------------------------------------------------
// Inference: 16x16 output tile per workgroup (grid 64 x 4 = 256 WGs for the 1024-wide
// layers at B = 64), 8 (or 16) waves split the contraction (every operand load of a wave
// issued up front).  BN-train: one workgroup owns all 64 rows of its 16 columns (batch statistics
// are workgroup-local), 8 waves split the contraction.
template <bool APK, bool YPK, int KIND>
static void launch_fwd_k(const ProfScope& ps, const FwdArgs& a, bool whole_batch, int wk, hipStream_t st) {
  const int gx = (a.N + 15) / 16;
  if (whole_batch) {
    go(ps, k_fwd<4, 8, 8, 2, APK, YPK, KIND>, dim3(gx, 1), dim3(512), st, a);
  } else {
    // tiling variants (P3D_INFER_WK): 82 = 1 row tile x 8 waves, 2-group register ring (the
    // inference default), 8 = the same with an 8-group ring (the training output layer), else 16
    // waves with a 4-group ring (the inference output layer).  (Round 6 removed the ten other
    // tilings the round-1 sweeps had measured slower.)
    const int gy = (a.M + 15) / 16;
    if (wk == 8) go(ps, k_fwd<1, 8, 8, 2, APK, YPK, KIND>, dim3(gx, gy), dim3(512), st, a);
    else if (wk == 82) go(ps, k_fwd<1, 8, 2, 2, APK, YPK, KIND>, dim3(gx, gy), dim3(512), st, a);
    else go(ps, k_fwd<1, 16, 4, 2, APK, YPK, KIND>, dim3(gx, gy), dim3(1024), st, a);
  }
}

// Large-M inference hidden layer (p3d_gemm.h): 128x128 tiles, grid = ceil(M/128) * N/128.
static bool use_big(const p3d_model* m, const FwdArgs& a, int kind, bool whole_batch) {
  return kind == 1 && !whole_batch && m->big_m > 0 && a.M >= m->big_m && a.N % 128 == 0 &&
         a.K % 32 == 0 &&
         a.bn != 2 && !a.z_save && a.ldy == 0;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static GemmF32Args big_args(const FwdArgs& a) {
  GemmF32Args g{};
  g.A = a.X; g.Wf = a.Wf; g.bias = a.bias; g.wsq = a.wsq;
  g.M = a.M; g.K = a.K; g.N = a.N;
  g.bn = a.bn; g.gamma = a.gamma; g.beta = a.beta; g.mmean = a.mmean; g.mvar = a.mvar; g.eps = a.eps;
  g.relu = a.relu; g.keep = a.keep; g.seed = a.seed; g.ctr = a.ctr; g.site = a.site; g.row_off = a.row_off;
  g.ctr_dev = a.ctr_dev; g.res = a.res; g.Y = a.Y;
  return g;
}

static void launch_big(p3d_model* m, const FwdArgs& a, hipStream_t st) {
  const GemmF32Args g = big_args(a);
  const unsigned grid = (unsigned)(((a.M + 127) / 128) * (a.N / 128));
  ProfScope ps(m, "fwd_hidden_big");
  // the LDS ring: 2 k-groups x 2 stages (64 KB); (1 k-group x 4 stages and 2 x 3 stages measured
  // slower in round 1 and were removed in round 6)
  go(ps, k_gemm_f32<2, 2>, dim3(grid), dim3(256), st, g);
}

// BN-train layer, split form: 16x16 GEMM tiles (256 workgroups at L = 1024, B = 64) write z
// and row-tile moments, then k_bn_fwd applies batch-stat BN / ReLU / dropout / residual.
// The exchange form (p3d_xchg.h: one launch, the row-tile siblings swap their BN partials)
// needs every workgroup of the grid resident at once: one per CU at most, <= 16 row tiles.
static bool use_xchg(const p3d_model* m, int N, int M) {
  const int gx = (N + 15) / 16, gy = (M + 15) / 16;
  return m->train_xchg && gy <= P3D_XCHG_MAXR && gx * gy <= m->num_cus;
}
static XchgSite xchg_site(const p3d_model* m, int slot) {
  const int nl = (int)m->layers.size();
  const int L = m->cfg.linear_size;
  XchgSite x;
  x.epoch = m->xsync + (int64_t)slot * (L / 16) * P3D_XCHG_EPOCH_STRIDE;
  x.slots = (float*)(m->xsync + m->xslots_off) + (int64_t)slot * P3D_XCHG_MAXR * L * 4;
  x.near = x.slots + (int64_t)2 * nl * P3D_XCHG_MAXR * L * 4;
  x.err = m->xerr;
  x.delay = m->xchg_delay;
  return x;
}

static int launch_fwd_split(p3d_model* m, const FwdArgs& a0, int kind, hipStream_t st) {
  FwdArgs a = a0;
  a.bn = 3; a.bnpart = m->bnpart;
  const dim3 grid((a.N + 15) / 16, (a.M + 15) / 16);
  if (use_xchg(m, a.N, a.M)) {   // BN-train layer as ONE launch
    a.bn = 4; a.xs = xchg_site(m, a.site);
    static const char* tags[2] = {"fwd_in_train_x", "fwd_hidden_train_x"};
    ProfScope ps(m, tags[kind == 0 ? 0 : 1]);
    dim3 g = grid;
    if (m->xchg_remap && grid.x % 8 == 0) { a.remap_gy = (int)grid.y; g = dim3(grid.x * grid.y); }
    if (kind == 0 && m->in_train_wk == 2 && a.K <= 32) go(ps, k_fwd<1, 2, 1, 2, false, true, 0>, g, dim3(128), st, a);
    else if (kind == 0 && m->in_train_wk == 4 && a.K <= 64) go(ps, k_fwd<1, 4, 1, 2, false, true, 0>, g, dim3(256), st, a);
    else if (kind == 0) go(ps, k_fwd<1, 8, 8, 2, false, true, 0>, g, dim3(512), st, a);
    else go(ps, k_fwd<1, 8, 8, 2, true, true, 1>, g, dim3(512), st, a);
    LAUNCH_CHECK("k_fwd");
    return P3D_OK;
  }
  {
    static const char* tags[3] = {"fwd_in_train_z", "fwd_hidden_train_z", "fwd_out_train_z"};
    ProfScope ps(m, tags[kind]);
    if (kind == 0) go(ps, k_fwd<1, 8, 8, 2, false, true, 0>, grid, dim3(512), st, a);
    else go(ps, k_fwd<1, 8, 8, 2, true, true, 1>, grid, dim3(512), st, a);
  }
  LAUNCH_CHECK("k_fwd");
  BnFwdArgs b{};
  b.z = a.z_save; b.part = m->bnpart; b.M = a.M; b.N = a.N;
  b.gamma = a.gamma; b.beta = a.beta; b.mmean = a.mmean; b.mvar = a.mvar; b.eps = a.eps; b.decay = a.decay;
  b.mean_save = a.mean_save; b.var_save = a.var_save;
  b.relu = a.relu; b.keep = a.keep; b.seed = a.seed; b.ctr = a.ctr; b.site = a.site; b.row_off = a.row_off;
  b.ctr_dev = a.ctr_dev; b.res = a.res; b.Y = a.Y;
  {
    ProfScope ps(m, "bn_fwd");
    go(ps, k_bn_fwd, grid, dim3(64), st, b);
  }
  LAUNCH_CHECK("k_bn_fwd");
  return P3D_OK;
}

static int launch_fwd(p3d_model* m, const FwdArgs& a, int kind, bool whole_batch, hipStream_t st) {
  if (use_big(m, a, kind, whole_batch)) {
    launch_big(m, a, st);
    LAUNCH_CHECK("k_gemm_f32");
    return P3D_OK;
  }
  if (kind == 0 && !whole_batch && m->big_m > 0 && a.M >= m->big_m && a.N % 128 == 0 && a.K == 32 &&
      a.bn != 2 && !a.z_save && a.ldy == 0 && aligned16(a.X)) {
    // input layer at large M: the 128x128-tile LDS-DMA GEMM, A DMA'd from the row-major input
    ProfScope ps(m, "fwd_in_big");
    GemmF32Args g = big_args(a);
    g.lda = a.ldx;
    go(ps, k_gemm_f32<2, 2, false>, dim3((unsigned)(((a.M + 127) / 128) * (a.N / 128))), dim3(256), st, g);
    LAUNCH_CHECK("k_gemm_f32");
    return P3D_OK;
  }
  if (kind == 0 && !whole_batch && m->big_m > 0 && a.M >= m->big_m) {
    // input layer (K = 32: two k-groups) at large M: 64 rows x 16 columns per wave
    ProfScope ps(m, "fwd_in_big");
    go(ps, k_fwd<4, 2, 2, 2, false, true, 0>, dim3((a.N + 15) / 16, (a.M + 63) / 64), dim3(128), st, a);
    LAUNCH_CHECK("k_fwd");
    return P3D_OK;
  }
  static const char* tags[2][3] = {{"fwd_in", "fwd_hidden", "fwd_out"},
                                   {"fwd_in_train", "fwd_hidden_train", "fwd_out_train"}};
  // (the output layer with the fused MSE -- a training step that does not take k_out_part -- is
  // told apart from the inference output layer in the profile)
  ProfScope ps(m, tags[whole_batch || (kind == 2 && a.tgt) ? 1 : 0][kind]);
  int wk = whole_batch ? m->train_wk : m->infer_wk;
  if (!whole_batch && kind == 0 && m->in_wk) wk = m->in_wk;
  // training output layer (fused MSE, 12 workgroups at B = 64): the 8-deep ring (all of a wave's
  // K slice requested at once) -- 6.85 vs 7.8 us with the inference tiling (A/B on one box);
  // env P3D_OUT_TRAIN_WK overrides
  if (!whole_batch && kind == 2 && a.tgt) wk = m->out_train_wk;
  else if (!whole_batch && kind == 2 && m->out_wk) wk = m->out_wk;
  const dim3 g16((a.N + 15) / 16, (a.M + 15) / 16);
  if (kind == 0 && wk == 2) {   // K = 32: one k-group per wave
    go(ps, k_fwd<1, 2, 1, 2, false, true, 0>, g16, dim3(128), st, a);
    LAUNCH_CHECK("k_fwd");
    return P3D_OK;
  }
  if (kind == 0) launch_fwd_k<false, true, 0>(ps, a, whole_batch, wk, st);
  else if (kind == 1) launch_fwd_k<true, true, 1>(ps, a, whole_batch, wk, st);
  else launch_fwd_k<true, false, 2>(ps, a, whole_batch, wk, st);
  LAUNCH_CHECK("k_fwd");
  return P3D_OK;
}

static int launch_bf16_layer(p3d_model* m, int l, int Mp, hipStream_t st) {
  const p3d_cfg& c = m->cfg;
  const int64_t slab = m->Mpad128 * c.linear_size;
  const int nl = (int)m->layers.size();
  const Layer& ly = m->layers[l];
  GemmBf16Args a{};
  a.A = l == 0 ? m->abf + (int64_t)nl * slab : m->abf + (int64_t)(l - 1) * slab;
  a.Bt = m->wbf + ly.wbf; a.Y = m->abf + (int64_t)l * slab;
  a.M = Mp; a.N = ly.N; a.K = ly.K;
  a.epi.bias = m->flat[0] + ly.b;
  a.epi.inv = ly.bn ? m->aff + ly.aff : nullptr;
  a.epi.shift = ly.bn ? m->aff + ly.aff + ly.N : nullptr;
  a.epi.relu = 1;
  const bool second = (l >= 1 && ((l - 1) % 2 == 1));
  a.res = (c.residual && second) ? m->abf + (int64_t)(l - 2) * slab : nullptr;
  const unsigned grid = (unsigned)((Mp / 128) * (ly.N / 128));
  // hidden layers: k_gemm_bf16p<64, 4, 8> (default), the unpipelined k_gemm_bf16<64, 4>
  // (P3D_BF16_STAGES=0, reference form)
  const bool bplain = m->bf16_stages == 0;
  if (l > 0) m->bf16_kname = bplain ? "k_gemm_bf16<64, 4>" : "k_gemm_bf16p<64, 4, 8, false>";
  {
    ProfScope ps(m, l == 0 ? "bf16_in" : "bf16_hidden");
    if (l == 0) go(ps, k_gemm_bf16<32, 2>, dim3(grid), dim3(256), st, a);
    else if (bplain) go(ps, k_gemm_bf16<64, 4>, dim3(grid), dim3(256), st, a);
    else go(ps, k_gemm_bf16p<64, 4, 8>, dim3(grid), dim3(512), st, a);
  }
  LAUNCH_CHECK("k_gemm_bf16");
  return P3D_OK;
}

// cfg5 path: x -> bf16 packed, input layer and every hidden layer through the LDS-staged
// bf16 GEMM (fused bias/BN/ReLU/residual, bf16 out), output layer register-direct (fp32 out).
static int forward_bf16(p3d_model* m, const float* x, int64_t B, float* y, hipStream_t st) {
  const p3d_cfg& c = m->cfg;
  const int L = c.linear_size;
  const int Mp = (int)((B + 127) / 128 * 128);
  const int64_t slab = m->Mpad128 * L;
  const int nl = (int)m->layers.size();
  unsigned short* xs = m->abf + (int64_t)nl * slab;
  {
    const int64_t items = (int64_t)(Mp / 16) * (c.input_size / 32) * 64;
    ProfScope ps(m, "bf16_x");
    go(ps, k_x_to_bf16, dim3((unsigned)((items + 255) / 256)), dim3(256), st, x, (int)B, c.input_size, xs, Mp);
  }
  LAUNCH_CHECK("k_x_to_bf16");
  for (int l = 0; l < nl - 1; ++l) {
    const int rc = launch_bf16_layer(m, l, Mp, st);
    if (rc) return rc;
  }
  const unsigned short* in = m->abf + (int64_t)(nl - 2) * slab;
  const Layer& lo = m->layers[nl - 1];
  SmallBf16Args o{};
  o.A = in; o.Bt = m->wbf + lo.wbf; o.M = (int)B; o.N = lo.N; o.K = lo.K;
  o.bias = m->flat[0] + lo.b; o.Y = y; o.ldy = lo.N;
  {
    ProfScope ps(m, "bf16_out");
    go(ps, k_out_bf16<16>, dim3((lo.N + 15) / 16, Mp / 16), dim3(1024), st, o);
  }
  LAUNCH_CHECK("k_out_bf16");
  return P3D_OK;
}

// Batch <= 4 inference (p3d_gemv.h): every layer as one weight-streaming k_gemv launch, the input
// and output layers folded into the first / last hidden layer's launch (k_gemv_fold) where the
// workspace slot has a hand-off area -- four launches instead of six at num_layers = 2, same bits.
// fr (p3d_lift): the chain reads the raw rows and writes the unnormalised ones; returns 1 without
// launching anything where the chain does not run (the caller then takes the three steps).
static int forward_gemv(p3d_model* m, const float* x, int64_t B, float* y, float keep_prob, uint64_t seed,
                        uint64_t ctr, int64_t row_offset, int64_t ws_row, hipStream_t st,
                        const GemvFrames* fr = nullptr) {
  const p3d_cfg& c = m->cfg;
  const int nl = (int)m->layers.size();
  const int64_t wsoff = (ws_row >> 4) * (int64_t)(c.linear_size >> 4) * 256;  // packed row-tile offset
  auto fill = [&](int l, const float* in, GemvArgs& a) {
    const Layer& ly = m->layers[l];
    const bool last = (l == nl - 1);
    a = GemvArgs{};
    a.X = in; a.ldx = c.input_size; a.xpk = l > 0;
    a.Wf = m->wpk + ly.wf;
    a.bias = m->flat[0] + ly.b;
    a.wsq = c.max_norm ? m->wsq + ly.widx : nullptr;
    a.M = (int)B; a.K = ly.K; a.N = ly.N;
    if (ly.bn) {
      a.bn = 1;
      a.gamma = m->flat[0] + ly.gamma; a.beta = m->flat[0] + ly.beta;
      a.mmean = m->moving + ly.mmean; a.mvar = m->moving + ly.mvar;
      a.eps = c.bn_eps;
    }
    a.relu = ly.relu;
    a.keep = last ? 1.0f : keep_prob;
    a.seed = seed; a.ctr = ctr; a.site = ly.site; a.row_off = row_offset;
    a.ctr_dev = (ctr == P3D_CTR_GLOBAL_STEP) ? &m->dstate->global_step : nullptr;
    const bool second = (l >= 1 && !last && ((l - 1) % 2 == 1));
    if (c.residual && second) a.res = m->act[l - 2] + wsoff;
    if (last) { a.Y = y; a.ldy = ly.N; a.ypk = 0; }
    else { a.Y = m->act[l] + wsoff; a.ldy = 0; a.ypk = 1; }
  };
  const int64_t slot = ws_row >> 4;
  const int L = c.linear_size;
  const bool fold = m->gemv_fold && m->gemv_hand && slot < m->gemv_slots && nl >= 4 && L % 16 == 0 &&
                    L <= P3D_GEMV_FOLD_MAXK && c.input_size == P3D_GEMV_FOLD_MAXIN &&
                    c.output_size <= 64;
  const int H = nl - 2, T = L / 16;
  if (fold && m->gemv_chain && H <= P3D_GEMV_CHAIN_MAXH && L <= P3D_GEMV_CHAIN_MAXK && H * T <= m->num_cus &&
      m->gemv_slot_floats >= (int64_t)(H + 1) * 4 * (L / 2) * 4) {
    GemvChain ch{};
    fill(0, x, ch.in);
    ch.in.Y = nullptr;
    for (int l = 1; l <= H; ++l) {
      fill(l, nullptr, ch.ly[l - 1]);
      ch.ly[l - 1].res = nullptr;   // (added by the chain itself)
      ch.ly[l - 1].Y = nullptr;
    }
    fill(nl - 1, nullptr, ch.out);
    ch.H = H; ch.T = T; ch.res = c.residual ? 1 : 0;
    ch.hand = m->gemv_hand + slot * m->gemv_slot_floats;
    ch.epoch = m->gemv_epoch + slot * P3D_XCHG_EPOCH_STRIDE;
    ch.err = m->xerr;
    if (fr) {
      ch.fr = *fr;
      if (ch.fr.out) ch.out.Y = nullptr;   // (p3d_lift: the unNormalizeData'd rows instead)
      if (ch.fr.hflag || ch.fr.loss) ch.fr.hcount = (ch.out.N + 15) >> 4;   // the output-tile workgroups (p3d_gemv.h)
    }
    {
      ProfScope ps(m, "gemv_chain");
      go(ps, k_gemv_chain<4, 4>, dim3((unsigned)(H * T)), dim3(1024), st, ch);
    }
    LAUNCH_CHECK("k_gemv_chain");
    return P3D_OK;
  }
  if (fr) return 1;
  const float* in = x;
  for (int l = 0; l < nl; ++l) {
    const bool last = (l == nl - 1);
    GemvArgs a;
    fill(l, in, a);
    if (fold && (l == 0 || l == nl - 1)) continue;   // run inside the first / last hidden layer's launch
    if (fold && (l == 1 || l == nl - 2)) {
      GemvFold f{};
      if (l == 1) {
        f.fin = 1;
        fill(0, x, f.in);
        // layer 0's output is read again only as layer 2's residual
        if (!(c.residual && nl - 2 >= 2)) f.in.Y = nullptr;
      }
      if (l == nl - 2) {
        f.fout = 1;
        fill(nl - 1, nullptr, f.out);
        f.hand = m->gemv_hand + slot * m->gemv_slot_floats;
        f.epoch = m->gemv_epoch + slot * P3D_XCHG_EPOCH_STRIDE;
        f.err = m->xerr;
        a.Y = nullptr;
      }
      const dim3 grid((unsigned)(L / 16 + (f.fout ? 1 : 0)));
      {
        ProfScope ps(m, f.fin ? (f.fout ? "gemv_in_hidden_out" : "gemv_in_hidden") : "gemv_hidden_out");
        go(ps, k_gemv_fold<4, 16, 4>, grid, dim3(1024), st, a, f);
      }
      LAUNCH_CHECK("k_gemv_fold");
      in = m->act[l] + wsoff;
      continue;
    }
    const Layer& ly = m->layers[l];
    const dim3 grid((unsigned)((ly.N + 15) / 16));
    {
      ProfScope ps(m, l == 0 ? "gemv_in" : (last ? "gemv_out" : "gemv_hidden"));
      if (l == 0) go(ps, k_gemv<4, 2, 4>, grid, dim3(128), st, a);
      else go(ps, k_gemv<4, 16, 4>, grid, dim3(1024), st, a);
    }
    LAUNCH_CHECK("k_gemv");
    in = a.Y;
  }
  return P3D_OK;
}

static int forward_impl(p3d_model* m, const float* x, int64_t B, float* y, int32_t training, float keep_prob,
                        uint64_t seed, uint64_t ctr, int64_t row_offset, int64_t ws_row, void* stream,
                        const float* tgt);

extern "C" int p3d_forward_ex(p3d_model* m, const float* x, int64_t B, float* y, int32_t training,
                              float keep_prob, uint64_t seed, uint64_t ctr, int64_t row_offset, int64_t ws_row,
                              void* stream) {
  return forward_impl(m, x, B, y, training, keep_prob, seed, ctr, row_offset, ws_row, stream, nullptr);
}

// tgt != null (training): the output layer also forms dy = 2(y - t)/(B*D) into m->dybuf and
// per-workgroup loss partials into m->lossp (p3d_train_fwd_bwd).
// The training output layer as split-K partials (k_out_part) with y / dy / loss formed by the
// backward's first launch: B <= 256 rows, N <= 64, the split BN-train kernels, a hidden layer
// whose data gradient folds the loss afterwards (num_layers >= 1).
static bool out_part_ok(const p3d_model* m, int64_t B) {
  return m->out_part && m->train_split && B <= 256 && m->cfg.output_size <= 64 && m->layers.size() >= 3 &&
         m->dgrad_out_wk == 4;
}

static int forward_impl(p3d_model* m, const float* x, int64_t B, float* y, int32_t training, float keep_prob,
                        uint64_t seed, uint64_t ctr, int64_t row_offset, int64_t ws_row, void* stream,
                        const float* tgt) {
  if (!m || !x || !y) return fail(P3D_ERR_ARG, "p3d_forward: null argument");
  m->opart_pending = false;
  const p3d_cfg& c = m->cfg;
  if (B <= 0) return fail(P3D_ERR_ARG, "p3d_forward: batch must be positive");
  if (ws_row < 0 || ws_row % 16 != 0) return fail(P3D_ERR_ARG, "p3d_forward_ex: ws_row must be a multiple of 16");
  if (training && ws_row != 0) return fail(P3D_ERR_ARG, "p3d_forward_ex: training uses workspace rows from 0");
  if (ws_row + B > c.max_batch)
    return fail(P3D_ERR_ARG, "p3d_forward: batch " + std::to_string(B) + " (+ workspace row " + std::to_string(ws_row) +
                                 ") exceeds max_batch " + std::to_string(c.max_batch));
  if (training && c.batch_norm && B > 64 && !m->train_split)
    return fail(P3D_ERR_ARG, "p3d_forward: the whole-batch BN-train kernels (P3D_TRAIN_SPLIT=0) need B <= 64");
  if (!(keep_prob > 0.f && keep_prob <= 1.f)) return fail(P3D_ERR_ARG, "keep_prob must be in (0, 1]");
  if (!aligned16(x)) return fail(P3D_ERR_ARG, "p3d_forward: x must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (c.dtype == P3D_DTYPE_BF16) {
    if (training) return fail(P3D_ERR_ARG, "p3d_forward: bf16 models are inference-only");
    if (keep_prob < 1.0f) return fail(P3D_ERR_ARG, "p3d_forward: bf16 models do not implement dropout");
    if (ws_row != 0) return fail(P3D_ERR_ARG, "p3d_forward_ex: bf16 models use workspace row 0");
    return forward_bf16(m, x, B, y, st);
  }
  const float decay = 1.0f - c.bn_momentum;
  const int nl = (int)m->layers.size();
  const int64_t wsoff = (ws_row >> 4) * (int64_t)(c.linear_size >> 4) * 256;  // packed row-tile offset
  if (!training && !tgt && B <= m->gemv_maxb) return forward_gemv(m, x, B, y, keep_prob, seed, ctr, row_offset, ws_row, st);
  const float* in = x;
  for (int l = 0; l < nl; ++l) {
    const Layer& ly = m->layers[l];
    FwdArgs a{};
    a.X = in; a.ldx = c.input_size;
    a.Wf = m->wpk + ly.wf;
    a.bias = m->flat[0] + ly.b;
    a.wsq = c.max_norm ? m->wsq + ly.widx : nullptr;
    a.M = (int)B; a.K = ly.K; a.N = ly.N;
    const bool last = (l == nl - 1);
    if (ly.bn) {
      a.bn = training ? 2 : 1;
      a.gamma = m->flat[0] + ly.gamma; a.beta = m->flat[0] + ly.beta;
      a.mmean = m->moving + ly.mmean; a.mvar = m->moving + ly.mvar;
      a.eps = c.bn_eps; a.decay = decay;
      if (training) { a.mean_save = m->bmean[l]; a.var_save = m->bvar[l]; }
    }
    if (training && !last) a.z_save = m->z[l];
    a.relu = ly.relu;
    a.keep = last ? 1.0f : keep_prob;
    a.seed = seed; a.ctr = ctr; a.site = ly.site; a.row_off = row_offset;
    a.ctr_dev = (ctr == P3D_CTR_GLOBAL_STEP) ? &m->dstate->global_step : nullptr;
    // residual: second layer of block i adds the block input (layer l-2's output)
    const bool second = (l >= 1 && !last && ((l - 1) % 2 == 1));
    if (c.residual && second) a.res = m->act[l - 2] + wsoff;
    if (last) { a.Y = y; a.ldy = ly.N; }
    else { a.Y = m->act[l] + wsoff; a.ldy = 0; }
    if (last && tgt) {
      a.tgt = tgt; a.dy = m->dybuf; a.lddy = (ly.N + 15) / 16 * 16;
      a.dscale = (1.0f / (float)(B * ly.N)) * 2.0f; a.lossp = m->lossp;
      m->nlossp = (int)(((ly.N + 15) / 16) * ((B + 15) / 16));
    }
    const int kind = (l == 0) ? 0 : (last ? 2 : 1);
    if (last && tgt && out_part_ok(m, B)) {
      // split-K partials; y, dy and the loss partials are formed by the backward's first launch
      OutPartArgs o{};
      o.X = in; o.Wf = a.Wf; o.M = (int)B; o.K = ly.K; o.part = m->opart;
      {
        ProfScope ps(m, "fwd_out_part");
        go(ps, k_out_part<8>, dim3((unsigned)((ly.N + 15) / 16), (unsigned)((B + 15) / 16), 8u), dim3(64), st, o);
      }
      LAUNCH_CHECK("k_out_part");
      m->opart_pending = true;
      m->opart_t = tgt;
      m->opart_y = y;
      in = a.Y;
      continue;
    }
#ifdef P3D_DIAG_SKIP_IN   // diagnostic builds only (tools/): drop the input-layer launch
    if (!training && l == 0) { in = a.Y; continue; }
#endif
    if (training && ly.bn && m->train_split) {
      const int rc = launch_fwd_split(m, a, kind, st);
      if (rc) return rc;
      in = a.Y;
      continue;
    }
    const int rc = launch_fwd(m, a, kind, training && ly.bn, st);
    if (rc) return rc;
    in = a.Y;
  }
  if (training) {
    m->serve_ec_dirty = true;   // moving statistics updated (UPDATE_OPS)
    m->have_cache = true;
    m->x_cached = x;
    m->B_cached = B;
    m->keep = keep_prob;
    m->seed = seed; m->ctr = ctr; m->row_off = row_offset;
    m->ctr_dev = (ctr == P3D_CTR_GLOBAL_STEP) ? &m->dstate->global_step : nullptr;
  }
  return P3D_OK;
}

extern "C" int p3d_forward(p3d_model* m, const float* x, int64_t B, float* y, int32_t training,
                           float keep_prob, uint64_t seed, uint64_t ctr, int64_t row_offset, void* stream) {
  return p3d_forward_ex(m, x, B, y, training, keep_prob, seed, ctr, row_offset, 0, stream);
}

// ---- persistent XCD-local evaluation (p3d_serve.h, p3d_serve6.h) ------------------------
// Which kernel a launch runs is decided in p3d_serve_plan.h (the list of built forms and the
// planner over it); here the kernels are attached to that list, row for row.
static_assert(kServe6Rows == P3D_SERVE6_ROWS, "p3d_serve_plan.h plans for the slabs p3d_serve.h sizes");
#define SERVE_KERNEL_k_serve(D, NDT, NCM, RT, PAIR) k_serve<D, NDT, 4>
#define SERVE_KERNEL_k_serve5(D, NDT, NCM, RT, PAIR) k_serve5<D, NDT, 2, 2>
#define SERVE_KERNEL_k_serve6(D, NDT, NCM, RT, PAIR) k_serve6<D, NDT, NCM, RT, PAIR>
#define SERVE_KERNEL_k_serve6_rounds(D, NDT, NCM, RT, PAIR) k_serve6_rounds<D, NDT, NCM, RT>
#define SERVE_KERNEL_k_serve6_rounds_w4(D, NDT, NCM, RT, PAIR) k_serve6_rounds_w4<D, NDT, NCM, RT>
#define SERVE_KERNEL_ROW(KIND, D, NDT, NCM, RT, PAIR) SERVE_KERNEL_##KIND(D, NDT, NCM, RT, PAIR),
static void (*const kServeKernels[])(ServeArgs) = {P3D_SERVE_FORMS(SERVE_KERNEL_ROW)};
#undef SERVE_KERNEL_ROW

#define SERVE_TRY(expr)                                                                                     \
  do {                                                                                                      \
    hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess) return fail(P3D_ERR_HIP, std::string("p3d_serve: ") + hipGetErrorString(e_)); \
  } while (0)

// Why p3d_serve does not take this model shape or batch (nullptr: it does).
static const char* serve_shape_error(const p3d_cfg& c, int64_t B) {
  if (B <= 0) return "p3d_serve: batch must be positive";
  if (c.dtype != P3D_DTYPE_F32) return "p3d_serve: fp32 models only";
  if (c.linear_size <= 0 || c.linear_size % 128 != 0 || c.input_size > 64 || c.output_size > 64 ||
      2 * c.num_layers + 2 > P3D_SERVE_MAXL)
    return "p3d_serve: needs linear_size % 128 == 0, input/output size <= 64, <= 7 blocks";
  if ((B + 63) / 64 > 0x7fffffff) return "p3d_serve: too many rows";
  return nullptr;
}

// The first call's buffers, k_serve6's with the others: a later call that takes
// k_serve6 for the first time may be inside a graph capture, where hipMalloc is not allowed.
static int serve_alloc(p3d_model* m) {
  const p3d_cfg& c = m->cfg;
  const int L = c.linear_size, U = L / 32, NDT = (c.output_size + 15) / 16;
  const int64_t slab = (int64_t)64 * L, PT = (int64_t)4 * NDT * 256;
  int dev = 0, cus = 0;
  SERVE_TRY(hipGetDevice(&dev));
  SERVE_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  m->serve_grid = cus;   // one 512-thread workgroup per CU (the LDS ring admits one)
  // output partials: k_serve5 keeps one per 32-column unit (U), k_serve6 one per 16-column tile (2U)
  const int64_t nbuf = P3D_SERVE_GROUPS * 3 * slab + P3D_SERVE_GROUPS * 2 * (int64_t)(2 * U) * PT;
  SERVE_TRY(hipMalloc(&m->serve_buf, nbuf * sizeof(float)));
  SERVE_TRY(hipMemset(m->serve_buf, 0, nbuf * sizeof(float)));
  // [bank 0 | bank 1 | k_serve5 bank | epoch word]: k_serve6 alternates banks 0 / 1 by the
  // device epoch word (p3d_serve6.h), k_serve5 uses bank 2 (zeroed before each of its launches)
  SERVE_TRY(hipMalloc(&m->serve_sync, P3D_SERVE_SYNC_ALL * sizeof(unsigned)));
  SERVE_TRY(hipMemset(m->serve_sync, 0, P3D_SERVE_SYNC_ALL * sizeof(unsigned)));
  const int64_t necg = (int64_t)(2 * c.num_layers + 2) * (L / 16) * 48 + 64;
  SERVE_TRY(hipMalloc(&m->serve_ecg, necg * sizeof(float)));
  SERVE_TRY(hipMalloc(&m->serve6_act, (int64_t)4 * P3D_SERVE6_ROWS * L * sizeof(float)));
  // the fused MSE's per-tile partials (kServeLossTiles: serve_plan refuses a loss over more) and
  // its arrival counter (the word after them), zero between launches
  SERVE_TRY(hipMalloc(&m->serve_loss, (kServeLossTiles + 64) * sizeof(float)));
  SERVE_TRY(hipMemset(m->serve_loss, 0, (kServeLossTiles + 64) * sizeof(float)));
  m->serve_ec_dirty = true;
  return P3D_OK;
}

static int serve_impl(p3d_model* m, const float* x, int64_t B, float* y, const float* t, float* loss,
                      void* stream) {
  HP_START
  if (!m || !x || !y) return fail(P3D_ERR_ARG, "p3d_serve: null argument");
  const p3d_cfg& c = m->cfg;
  if (const char* why = serve_shape_error(c, B)) return fail(P3D_ERR_ARG, why);
  if (!aligned16(x)) return fail(P3D_ERR_ARG, "p3d_serve: x must be 16-byte aligned");
  // an earlier launch failed and nobody has collected the error (p3d_serve_check): refuse, so a
  // caller never keeps receiving rows of a launch whose workgroups could not synchronise
  if (m->errw && m->errw[1])
    return fail(P3D_ERR_HIP, "p3d_serve: an earlier launch failed (not all workgroups resident); p3d_serve_check "
                             "reports and clears it");
  hipStream_t st = (hipStream_t)stream;
  // batch <= 4 with the loss: the persistent small-batch forward (k_gemv_chain, ~13 us where a 64-row
  // k_serve6 unit takes ~30) with the loss reduced by its last output workgroup -- still one launch;
  // y has p3d_forward's bits at this batch, the loss p3d_mse's on that y (stream-ordered with the
  // model's other batch <= 4 calls: they share workspace slot 0)
  if (t && loss && B <= m->gemv_maxb) {
    GemvFrames fr{};
    fr.tgt = t; fr.loss = loss;
    fr.hcnt = m->hcnt; fr.sq = reinterpret_cast<float*>(m->hcnt + 256);
    if (m->hwait) { fr.hflag = m->hflag_dev; fr.hseq = m->hwait; }
    const int r = forward_gemv(m, x, B, y, 1.0f, 0, 0, 0, 0, st, &fr);
    if (r == P3D_OK && m->hwait) m->harmed = true;
    if (r != 1) return r;   // (1: no chain form for this model -- k_serve6 below)
  }
  if (!m->serve_buf) {
    const int r = serve_alloc(m);
    if (r != P3D_OK) return r;
  }
  const int L = c.linear_size;
  ServeArgs a{};
  a.x = x; a.y = y; a.M = B;
  a.L = L; a.K0 = c.input_size; a.ND = c.output_size; a.nblk = c.num_layers;
  a.bn = c.batch_norm; a.residual = c.residual; a.eps = c.bn_eps;
  a.act = m->serve_buf; a.part = m->serve_buf + P3D_SERVE_GROUPS * 3 * (int64_t)64 * L;
  a.sync = m->serve_sync; a.err = m->serve_err;
  a.epoch = m->serve_sync + 3 * P3D_SERVE_SYNC_WORDS;
  a.census_extra = m->serve_fault ? 1 : 0;
  a.delay = (m->serve_delay > 0 && (m->serve_calls++ & 1) == 0) ? m->serve_delay : 0;
  a.delay_xcc = m->serve_delay_xcc;
  a.max_groups = m->serve_groups;
  for (size_t l = 0; l < m->layers.size(); ++l) {
    const Layer& ly = m->layers[l];
    ServeLayer& s = a.ly[l];
    s.Wf = m->wpk + ly.wf; s.bias = m->flat[0] + ly.b;
    if (ly.bn) {
      s.gamma = m->flat[0] + ly.gamma; s.beta = m->flat[0] + ly.beta;
      s.mmean = m->moving + ly.mmean; s.mvar = m->moving + ly.mvar;
    }
    s.wsq = c.max_norm ? m->wsq + ly.widx : nullptr;
  }
  if (B != m->serve_B || (t != nullptr) != m->serve_with_loss) {
    const ServeChoice ch = serve_plan(L, c.num_layers, (c.output_size + 15) / 16, m->serve_grid, m->serve_knobs, B,
                                      t != nullptr);
    if (ch.refused) return fail(P3D_ERR_ARG, ch.refused);
    m->serve_choice = ch; m->serve_B = B; m->serve_with_loss = t != nullptr;
  }
  const ServeForm& f = *m->serve_choice.form;
  const bool use6 = serve_kind_is6(f.kind);
  a.split = m->serve_choice.S;
  a.nb = m->serve_choice.nb;   // batch-64 steps, or k_serve6's units of 16 RT rows
  a.ecg = m->serve_ecg;
  // a HIP graph being captured replays this call with whatever parameters it then finds: the
  // epilogue-constant table is formed inside the graph (one small launch per replay), not
  // decided once at capture time
  HP(0);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  SERVE_TRY(hipStreamIsCapturing(st, &cap));
  const bool capturing = cap != hipStreamCaptureStatusNone;
  HP(1);

  if (use6 && (m->serve_ec_dirty || capturing)) {
    // the epilogue-constant table, formed once per parameter version (refresh_derived, a
    // training forward and every Adam step mark it stale): steady-state calls are one launch
    const int nl = 2 * c.num_layers + 1;
    k_serve_prep<<<(unsigned)((nl * L + 255) / 256), 256, 0, st>>>(a, m->serve_ecg);
    LAUNCH_CHECK("k_serve_prep");
    if (!capturing) m->serve_ec_dirty = false;
  }
  if (use6) {
    // (k_serve6 picks its bank from the device epoch word: no memset in front, graph replays
    // alternate the banks by themselves)
    a.act = m->serve6_act;                   // [group][4 slabs][16 RT rows][L]; no output partials
    a.part = nullptr;
  } else {   // k_serve5: its own bank, zeroed in front of every launch
    a.sync = m->serve_sync + 2 * P3D_SERVE_SYNC_WORDS;
    SERVE_TRY(hipMemsetAsync(a.sync, 0, P3D_SERVE_SYNC_WORDS * sizeof(unsigned), st));
  }
  if (t) {   // (serve_plan lets only k_serve6 forms carry the loss)
    a.tgt = t; a.loss = loss;
    a.lpart = m->serve_loss; a.lcnt = (unsigned*)(m->serve_loss + kServeLossTiles);
    if (m->hwait && !f.pair) { a.hflag = m->hflag_dev; a.hseq = m->hwait; m->harmed = true; }
  }
  ProfScope ps(m, "serve");
  HP(2);
  go(ps, kServeKernels[&f - kServeForms], dim3((unsigned)m->serve_grid), dim3((unsigned)serve_kind_threads(f.kind)), st, a);
  HP(3);
  LAUNCH_CHECK("k_serve");
  return P3D_OK;
}
#undef SERVE_TRY

extern "C" int p3d_serve(p3d_model* m, const float* x, int64_t B, float* y, void* stream) {
  return serve_impl(m, x, B, y, nullptr, nullptr, stream);
}

// (include/p3d.h) p3d_serve with the MSE of linear_model.py:129 fused into its output phase
extern "C" int p3d_serve_mse(p3d_model* m, const float* x, int64_t B, float* y, const float* t, float* loss,
                             void* stream) {
  if (!t || !loss) return fail(P3D_ERR_ARG, "p3d_serve_mse: null argument");
  return serve_impl(m, x, B, y, t, loss, stream);
}

// (include/p3d.h) the planner's answer for a model shape and device size, no GPU touched
extern "C" int p3d_serve_plan(const p3d_cfg* cfg, int32_t cus, int64_t B, int32_t with_loss, char* name,
                              int64_t name_len, int32_t* shape) {
  if (!cfg || !name || name_len <= 0 || cus < 1) return fail(P3D_ERR_ARG, "p3d_serve_plan: bad argument");
  if (const char* why = serve_shape_error(*cfg, B)) return fail(P3D_ERR_ARG, why);
  const ServeChoice ch = serve_plan(cfg->linear_size, cfg->num_layers, (cfg->output_size + 15) / 16, cus,
                                    serve_knobs_from_env(), B, with_loss != 0);
  if (ch.refused) return fail(P3D_ERR_ARG, ch.refused);
  strncpy(name, serve_form_name(*ch.form).c_str(), (size_t)name_len - 1);
  name[name_len - 1] = 0;
  if (shape) {
    shape[0] = ch.S; shape[1] = ch.form->rt; shape[2] = ch.form->ncm; shape[3] = ch.form->depth; shape[4] = ch.nb;
  }
  return P3D_OK;
}

static const char* serve_err_text(int v) {
  return v == 2 ? "p3d_serve: an XCD group had fewer workgroups than the launch was sized for"
                : "p3d_serve: a workgroup's synchronisation timed out (not all workgroups resident); the "
                  "launch's rows hold NaN where its census failed";
}

// Reported once: the word and the sync words are cleared, so later launches are judged on their own.
static int serve_report(p3d_model* m, int v) {
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess && m->serve_sync) e = hipMemset(m->serve_sync, 0, P3D_SERVE_SYNC_ALL * sizeof(unsigned));
  // (a failed launch may have left the fused MSE's arrival counter short)
  if (e == hipSuccess && m->serve_loss) e = hipMemset(m->serve_loss, 0, (kServeLossTiles + 64) * sizeof(float));
  if (e != hipSuccess) return fail(P3D_ERR_HIP, std::string("p3d_serve_check: ") + hipGetErrorString(e));
  __atomic_store_n(&m->errw[1], 0, __ATOMIC_SEQ_CST);
  return fail(P3D_ERR_HIP, serve_err_text(v));
}

extern "C" int p3d_serve_check(p3d_model* m) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return fail(P3D_ERR_HIP, std::string("p3d_serve_check: ") + hipGetErrorString(e));
  const int v = __atomic_load_n(&m->errw[1], __ATOMIC_SEQ_CST);
  return v ? serve_report(m, v) : P3D_OK;
}

extern "C" int p3d_sync_check(p3d_model* m) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return fail(P3D_ERR_HIP, std::string("p3d_sync_check: ") + hipGetErrorString(e));
  if (__atomic_load_n(&m->errw[0], __ATOMIC_SEQ_CST)) {
    __atomic_store_n(&m->errw[0], 0, __ATOMIC_SEQ_CST);
    return fail(P3D_ERR_HIP, "p3d_sync_check: a BN-train exchange timed out (row-tile workgroups not all resident)");
  }
  return P3D_OK;
}

// The error words as the kernels left them, read from pinned host memory: no device round trip,
// no synchronisation (a caller checks after a synchronisation it makes anyway: a loss read, an
// output copy).  flags: bit 0 an exchange timed out, bit 1 a serve spin ran out, bit 2 a serve
// placement the launch was not sized for.  With clear != 0 the reported words are reset (a
// reported serve error also clears the serve sync words: that part synchronises).
extern "C" int p3d_error_flags(p3d_model* m, int32_t* flags, int32_t clear) {
  if (!m || !flags) return fail(P3D_ERR_ARG, "p3d_error_flags: null argument");
  const int x = __atomic_load_n(&m->errw[0], __ATOMIC_SEQ_CST), v = __atomic_load_n(&m->errw[1], __ATOMIC_SEQ_CST);
  *flags = (x ? 1 : 0) | (v == 1 ? 2 : 0) | (v == 2 ? 4 : 0);
  if (clear) {
    if (x) __atomic_store_n(&m->errw[0], 0, __ATOMIC_SEQ_CST);
    if (v) {
      (void)serve_report(m, v);
      g_err.clear();
    }
  }
  return P3D_OK;
}

// Timing hook: `reps` back-to-back launches of hidden layer `layer` (1 .. 2N) of the
// inference forward on workspace rows [0, B) (act[layer-1] -> act[layer]).  Idempotent.
extern "C" int p3d_time_layer(p3d_model* m, int32_t layer, int64_t B, int32_t reps, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  const p3d_cfg& c = m->cfg;
  const int nl = (int)m->layers.size();
  if (layer < 1 || layer > nl - 2) return fail(P3D_ERR_ARG, "p3d_time_layer: layer must be a hidden layer");
  if (B <= 0 || B > c.max_batch) return fail(P3D_ERR_ARG, "p3d_time_layer: bad batch");
  if (c.dtype == P3D_DTYPE_BF16) {
    const int Mp = (int)((B + 127) / 128 * 128);
    for (int r = 0; r < reps; ++r) {
      const int rc = launch_bf16_layer(m, layer, Mp, (hipStream_t)stream);
      if (rc) return rc;
    }
    return P3D_OK;
  }
  const Layer& ly = m->layers[layer];
  FwdArgs a{};
  a.X = m->act[layer - 1]; a.Wf = m->wpk + ly.wf; a.bias = m->flat[0] + ly.b;
  a.wsq = c.max_norm ? m->wsq + ly.widx : nullptr;
  a.M = (int)B; a.K = ly.K; a.N = ly.N;
  if (ly.bn) {
    a.bn = 1; a.gamma = m->flat[0] + ly.gamma; a.beta = m->flat[0] + ly.beta;
    a.mmean = m->moving + ly.mmean; a.mvar = m->moving + ly.mvar; a.eps = c.bn_eps;
  }
  a.relu = 1; a.keep = 1.0f; a.site = ly.site;
  if (c.residual && ((layer - 1) % 2 == 1)) a.res = m->act[layer - 2];
  a.Y = m->act[layer];
  for (int r = 0; r < reps; ++r) {
    const int rc = launch_fwd(m, a, 1, false, (hipStream_t)stream);
    if (rc) return rc;
  }
  return P3D_OK;
}

extern "C" int p3d_mse(const float* y, const float* t, int64_t B, int32_t D, float* loss_dev, float* dy,
                       void* stream) {
  if (!y || !t) return fail(P3D_ERR_ARG, "p3d_mse: null argument");
  if (B <= 0 || D <= 0) return fail(P3D_ERR_ARG, "p3d_mse: bad shape");
  k_mse<<<1, 256, 0, (hipStream_t)stream>>>(y, t, B * D, loss_dev, dy);
  LAUNCH_CHECK("k_mse");
  return P3D_OK;
}

static int launch_wgrad(p3d_model* m, const WgradArgs& a, hipStream_t st) {
  ProfScope ps(m, "wgrad");
  go(ps, k_wgrad, dim3((a.N + 63) / 64, (a.K + 63) / 64), dim3(256), st, a);
  LAUNCH_CHECK("k_wgrad");
  return P3D_OK;
}

extern "C" int p3d_backward(p3d_model* m, const float* dy, int64_t B, void* stream) {
  if (!m || !dy) return fail(P3D_ERR_ARG, "p3d_backward: null argument");
  if (!m->have_cache) return fail(P3D_ERR_STATE, "p3d_backward: no training forward to differentiate");
  if (B != m->B_cached) return fail(P3D_ERR_ARG, "p3d_backward: batch differs from the training forward");
  if (B > 64 && !m->train_split)
    return fail(P3D_ERR_ARG, "p3d_backward: the whole-batch kernels (P3D_TRAIN_SPLIT=0) need B <= 64");
  const p3d_cfg& c = m->cfg;
  hipStream_t st = (hipStream_t)stream;
  // dy enters the output layer's GEMMs as a row-major operand read in 16-column groups:
  // use it in place when its rows are 16-float aligned, else through the zero-padded dybuf
  const int np_out = (c.output_size + 15) / 16 * 16;
  int64_t ld_dy = c.output_size;
  if (dy == m->dybuf) {
    ld_dy = np_out;
  } else if (c.output_size % 16 != 0 || !aligned16(dy)) {
    HIP_TRY(hipMemcpy2DAsync(m->dybuf, (size_t)np_out * 4, dy, (size_t)c.output_size * 4,
                             (size_t)c.output_size * 4, (size_t)B, hipMemcpyDeviceToDevice, st));
    dy = m->dybuf;
    ld_dy = np_out;
  }
  const int nl = (int)m->layers.size();
  float* grads = m->flat[1];
  const float* params = m->flat[0];
  // the training forward left the output layer as split-K partials (k_out_part): the first data-
  // gradient launch forms y, dy (into dybuf, where the output layer's weight gradient reads it)
  // and the loss partials
  const bool opart = m->opart_pending && dy == m->dybuf;
  if (m->opart_pending && !opart)
    return fail(P3D_ERR_STATE, "p3d_backward: the last training forward deferred its output layer to "
                               "p3d_train_fwd_bwd's backward");
  m->opart_pending = false;
  const float* dz_cur = dy;   // gradient wrt z of the current layer l
  bool dz_pk = false;         // dy is row-major; every later dz is packed
  int dsel = 0;
  const float* dres_next = nullptr;  // block-output gradient to add when differentiating an A-layer
  // weight gradients batched into one launch after the loop -- or, with gradient-ready buckets
  // (data-parallel all-reduce overlapping the backward), one launch per bucket as soon as its
  // layers' dZ and BN-parameter gradients exist, followed by the bucket's event
  const bool multi = m->wgrad_multi && nl <= P3D_WG_MULTI;
  const bool bucketed = !m->gev.empty() && !c.max_norm && multi && m->bucket_lo.size() == m->gev.size();
  size_t kb = 0;                     // next bucket
  WgradMulti mw{};
  if (m->fuse_adam) {
    mw.adam = 1; mw.af = *m->fuse_adam; mw.w = m->flat[0]; mw.m = m->flat[2]; mw.v = m->flat[3]; mw.gflat = grads;
  }
  // fused single-GPU step: Adam's alpha formed once by the first backward launch, so the last
  // launch (which reads no step state) advances it -- no k_step_advance launch
  const bool fused_tail = multi && m->fuse_adam && m->train_split && !bucketed;
  if (fused_tail) mw.alpha_dev = m->alpha_dev;
  m->step_advanced = false;
  m->alpha_ready = false;
  // bucket kb's parameters are free for its optimizer once dgrad of its lowest layer (the last
  // reader of W / Wd of the bucket) is issued: its event at the top of the next iteration
  int aev_pending = -1;
  auto flush_bucket = [&](int l) -> int {   // bucket kb ends at layer l: its tiles, then its event
    if (!bucketed || kb >= m->bucket_lo.size() || l != m->bucket_lo[kb]) return P3D_OK;
    aev_pending = (int)kb;
    if (mw.n > 0) {
      ProfScope ps(m, "wgrad_bucket");
      if (mw.adam) go(ps, k_wgrad_multi, dim3(mw.begin[mw.n]), dim3(256), st, mw);
      else go(ps, k_wgrad_grad, dim3(mw.begin[mw.n]), dim3(256), st, mw);
      LAUNCH_CHECK("k_wgrad_multi (bucket)");
      mw.n = 0;
      mw.begin[0] = 0;
    }
    HIP_TRY(hipEventRecord(m->gev[kb], st));
    ++kb;
    return P3D_OK;
  };
  auto emit = [&](const WgradArgs& wa) -> int {
    if (!multi) return launch_wgrad(m, wa, st);
    WgradLayer& w = mw.ly[mw.n];
    w.X = wa.X; w.dZ = wa.dZ; w.dW = wa.dW; w.db = wa.db; w.ldx = wa.ldx; w.ldz = wa.ldz;
    w.xpk = wa.xpk; w.zpk = wa.zpk; w.M = wa.M; w.K = wa.K; w.N = wa.N;
    w.bn_adam = wa.bn_adam; w.woff = wa.woff; w.boff = wa.boff; w.goff = wa.goff; w.btoff = wa.btoff;
    w.wd = wa.wd; w.wf = wa.wf;
    mw.gx[mw.n] = (wa.N + 63) / 64;
    mw.begin[mw.n + 1] = mw.begin[mw.n] + mw.gx[mw.n] * ((wa.K + 63) / 64);
    ++mw.n;
    return P3D_OK;
  };
  for (int l = nl - 1; l >= 0; --l) {
    if (aev_pending >= 0) { HIP_TRY(hipEventRecord(m->aev[aev_pending], st)); aev_pending = -1; }
    const Layer& ly = m->layers[l];
    WgradArgs wa{};
    wa.X = (l == 0) ? m->x_cached : m->act[l - 1]; wa.ldx = c.input_size; wa.xpk = (l != 0);
    wa.dZ = dz_cur; wa.ldz = dz_pk ? ly.N : ld_dy; wa.zpk = dz_pk;
    wa.M = (int)B; wa.K = ly.K; wa.N = ly.N;
    wa.dW = grads + ly.w; wa.db = grads + ly.b;
    const bool fuse = m->fuse_adam != nullptr;
    // the per-layer k_wgrad of the output layer reads dy: where this layer's data-gradient launch
    // forms it (from k_out_part's partials) the weight gradient follows that launch.  (The
    // one-launch forms run after the loop, the fused step's after each data gradient anyway.)
    const bool defer_out = !fuse && !multi && opart && l == nl - 1;
    if (fuse) {
      // single-GPU train step: Adam where the gradient is formed.  W(l) is read by dgrad(l),
      // so dW + Adam(l) runs after it; the previous layer's gamma/beta (read by dgrad(l) and
      // k_bn_bwd) are updated here too, from the gradients k_bn_bwd stored.
      wa.adam = 1; wa.af = *m->fuse_adam;
      wa.w = m->flat[0]; wa.m = m->flat[2]; wa.v = m->flat[3]; wa.woff = ly.w; wa.boff = ly.b;
      wa.wd = m->wpk + ly.wd; wa.wf = m->wpk + ly.wf;
      if (l >= 1 && m->layers[l - 1].bn) {
        wa.bn_adam = 1; wa.gflat = grads; wa.goff = m->layers[l - 1].gamma; wa.btoff = m->layers[l - 1].beta;
      }
    } else if (!defer_out) {
      int rc = emit(wa);
      if (!rc) rc = flush_bucket(l);
      if (rc) return rc;
    }
    if (l == 0) {
      if (fuse) {
        int rc = emit(wa);
        if (rc) return rc;
      }
      break;
    }
    const Layer& pv = m->layers[l - 1];
    BwdArgs a{};
    a.dZ = dz_cur; a.ldz = dz_pk ? ly.N : ld_dy;
    a.Wd = m->wpk + ly.wd; a.ngB = (ly.N + 15) / 16;
    a.wsq = c.max_norm ? m->wsq + ly.widx : nullptr;
    a.M = (int)B; a.K = ly.K; a.N = ly.N;
    const bool is_out = (l == nl - 1);
    const bool is_A = !is_out && ((l - 1) % 2 == 0);   // first layer of a block
    if (c.residual) {
      if (is_out) {
        a.draw = m->dout[dsel];              // d(last block output): kept for its residual
      } else if (is_A) {
        a.dres = dres_next;                  // dX of a block input = dZ*W^T + d(block output)
        if (l - 1 >= 1) a.draw = m->dout[dsel];
      }
    }
    // the forward's loss partials are folded by the first backward launch -- or, when that launch
    // forms them itself (output layer from split-K partials), by the next one
    if (m->loss_dst && (opart ? l == nl - 2 : is_out)) {
      a.lossp = m->lossp; a.nlossp = m->nlossp; a.loss = m->loss_dst;
      a.loss_scale = 1.0f / (float)(B * m->layers[nl - 1].N);
    }
    if (is_out && opart) {
      a.opart = m->opart; a.ont = (ly.N + 15) / 16;
      a.obias = params + ly.b; a.otgt = m->opart_t; a.oldt = ly.N;
      a.oy = m->opart_y; a.oldy = ly.N;
      a.ody = m->dybuf; a.oldd = np_out;
      a.odscale = (1.0f / (float)(B * ly.N)) * 2.0f; a.olossp = m->lossp;
    }
    a.prev = 1;
    a.bn = pv.bn;
    a.z = m->z[l - 1]; a.mean = m->bmean[l - 1]; a.var = m->bvar[l - 1];
    if (pv.bn) { a.gamma = params + pv.gamma; a.beta = params + pv.beta; }
    a.eps = c.bn_eps;
    a.relu = pv.relu;
    a.keep = m->keep; a.seed = m->seed; a.ctr = m->ctr; a.site = pv.site; a.row_off = m->row_off;
    a.ctr_dev = m->ctr_dev;
    a.dz = m->dz[l - 1];
    if (pv.bn) { a.dgamma = grads + pv.gamma; a.dbeta = grads + pv.beta; }
    if (m->train_split) {
      if (pv.bn) a.bnpart = m->bnpart;
      // (also beside a concurrent bucket all-reduce: its kernels share CUs with the siblings,
      // which delays a sibling's start but never blocks it -- the spins are bounded regardless)
      const bool xchg = pv.bn && use_xchg(m, a.K, a.M);
      if (xchg) { a.xchg = 1; a.xs = xchg_site(m, nl + l - 1); }   // dz, dgamma, dbeta here
      const dim3 grid((a.K + 15) / 16, (a.M + 15) / 16);
      if (fused_tail && is_out) { a.alpha_out = m->alpha_dev; a.af = *m->fuse_adam; }
      if (m->alpha_af && is_out) {   // data-parallel step: alpha for p3d_adam_apply after the all-reduce
        a.alpha_out = m->alpha_dev; a.af = *m->alpha_af; m->alpha_ready = true;
      }
      {
        ProfScope ps(m, is_out ? "dgrad_out" : "dgrad_hidden");
        if (dz_pk) {
          dim3 g = grid;
          if (xchg && m->xchg_remap && grid.x % 8 == 0) { a.remap_gy = (int)grid.y; g = dim3(grid.x * grid.y); }
          // 16 waves (both BN forms, so they keep giving the same bits): 6.8 vs 7.0-7.1 us per
          // hidden dgrad (A/B, one box)
          if (m->dgrad_wk == 16) go(ps, k_dgrad<1, 16, 4, 2, true, 1>, g, dim3(1024), st, a);
          else go(ps, k_dgrad<1, 8, 8, 2, true, 1>, g, dim3(512), st, a);
        } else {
          dim3 g = grid;
          if (xchg && m->xchg_remap && grid.x % 8 == 0) { a.remap_gy = (int)grid.y; g = dim3(grid.x * grid.y); }
          if (m->dgrad_out_wk == 4) go(ps, k_dgrad<1, 4, 4, 2, false, 2>, g, dim3(256), st, a);
          else go(ps, k_dgrad<1, 8, 8, 2, false, 2>, g, dim3(512), st, a);
        }
      }
      LAUNCH_CHECK("k_dgrad");
      if (pv.bn && !xchg) {
        BnBwdArgs b{};
        b.dz = a.dz; b.z = a.z; b.part = m->bnpart; b.M = a.M; b.K = a.K;
        b.mean = a.mean; b.var = a.var; b.gamma = a.gamma; b.eps = a.eps;
        b.dgamma = a.dgamma; b.dbeta = a.dbeta;
        ProfScope ps(m, "bn_bwd");
        go(ps, k_bn_bwd, grid, dim3(64), st, b);
        LAUNCH_CHECK("k_bn_bwd");
      }
    } else {
      {
        ProfScope ps(m, is_out ? "dgrad_out" : "dgrad_hidden");
        const dim3 grid((a.K + 15) / 16, 1);
        if (dz_pk) go(ps, k_dgrad<4, 8, 8, 2, true, 1>, grid, dim3(512), st, a);
        else go(ps, k_dgrad<4, 8, 8, 2, false, 2>, grid, dim3(512), st, a);
      }
      LAUNCH_CHECK("k_dgrad");
    }
    if (a.draw) { dres_next = a.draw; dsel ^= 1; }
    if (fuse || defer_out) {
      int rc = emit(wa);
      if (rc) return rc;
    }
    dz_cur = m->dz[l - 1];
    dz_pk = true;
  }
  if (multi && mw.n > 0) {
    if (fused_tail) { mw.advance = m->dstate; m->step_advanced = true; }   // the step's last launch
    ProfScope ps(m, "wgrad_multi");
    if (mw.adam) go(ps, k_wgrad_multi, dim3(mw.begin[mw.n]), dim3(256), st, mw);
    else go(ps, k_wgrad_grad, dim3(mw.begin[mw.n]), dim3(256), st, mw);
    LAUNCH_CHECK("k_wgrad_multi");
  }
  if (!m->gev.empty() && !bucketed && !c.max_norm)   // (per-layer k_wgrad form: every bucket at the end)
    for (hipEvent_t e : m->gev) HIP_TRY(hipEventRecord(e, st));
  if (aev_pending >= 0) { HIP_TRY(hipEventRecord(m->aev[aev_pending], st)); aev_pending = -1; }
  if (!bucketed)
    for (hipEvent_t e : m->aev) HIP_TRY(hipEventRecord(e, st));
  if (c.max_norm) {
    // G (dL/dW_eff) -> dL/dW through clip_by_norm
    k_dot_partial<<<dim3(DOT_CHUNKS, m->wtab.n), 256, 0, st>>>(grads, params, m->wtab, m->scratch);
    LAUNCH_CHECK("k_dot_partial");
    k_dot_final<<<1, 64, 0, st>>>(m->scratch, m->wtab.n, m->gw);
    LAUNCH_CHECK("k_dot_final");
    k_maxnorm_grad<<<dim3(64, m->wtab.n), 256, 0, st>>>(grads, params, m->wtab, m->wsq, m->gw);
    LAUNCH_CHECK("k_maxnorm_grad");
    for (hipEvent_t e : m->gev) HIP_TRY(hipEventRecord(e, st));
  }
  return P3D_OK;
}

extern "C" int p3d_grad_buckets(p3d_model* m, int32_t n, const int32_t* lowest) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_grad_buckets: null model");
  const int nl = (int)m->layers.size();
  if (n > P3D_MAX_W) return fail(P3D_ERR_ARG, "p3d_grad_buckets: bad bucket count");
  if (n < 0 || n > nl || (n > 0 && !lowest)) return fail(P3D_ERR_ARG, "p3d_grad_buckets: bad bucket count");
  for (int k = 0; k < n; ++k)   // contiguous, backward order, the last one ending at layer 0
    if (lowest[k] < 0 || lowest[k] >= nl || (k > 0 && lowest[k] >= lowest[k - 1]) || (k == n - 1 && lowest[k] != 0))
      return fail(P3D_ERR_ARG, "p3d_grad_buckets: lowest layers must decrease and end at layer 0");
  for (hipEvent_t e : m->gev) HIP_TRY(hipEventDestroy(e));
  for (hipEvent_t e : m->aev) HIP_TRY(hipEventDestroy(e));
  m->gev.clear();
  m->aev.clear();
  m->bat.clear();
  m->bat_blocks.clear();
  m->bucket_lo.assign(lowest, lowest + n);
  m->gev.resize((size_t)n, nullptr);
  m->aev.resize((size_t)n, nullptr);
  for (hipEvent_t& e : m->gev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (hipEvent_t& e : m->aev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  // per-bucket optimizer tables: the weight tiles of the bucket's layers and the 1-D tensors
  // (biases, gamma, beta) inside their flat ranges -- the whole-model table split by bucket
  for (int k = 0; k < n; ++k) {
    const int hi = k == 0 ? nl - 1 : lowest[k - 1] - 1, lo = lowest[k];
    const int64_t fb = m->layers[lo].w, fe = hi + 1 < nl ? m->layers[hi + 1].w : m->n_flat;
    AdamTable t{};
    int tiles = 0, vch = 0;
    for (int wi = 0; wi < m->at.nw; ++wi) {
      if (m->at.off[wi] < fb || m->at.off[wi] >= fe) continue;
      const int j = t.nw++;
      t.K[j] = m->at.K[wi]; t.N[j] = m->at.N[wi]; t.off[j] = m->at.off[wi]; t.wf[j] = m->at.wf[wi]; t.wd[j] = m->at.wd[wi];
      t.tile_begin[j] = tiles;
      tiles += m->at.tile_begin[wi + 1] - m->at.tile_begin[wi];
    }
    t.tile_begin[t.nw] = tiles;
    for (int vi = 0; vi < m->at.nv; ++vi) {
      if (m->at.voff[vi] < fb || m->at.voff[vi] >= fe) continue;
      const int j = t.nv++;
      t.voff[j] = m->at.voff[vi]; t.vlen[j] = m->at.vlen[vi]; t.vbegin[j] = vch;
      vch += m->at.vbegin[vi + 1] - m->at.vbegin[vi];
    }
    t.vbegin[t.nv] = vch;
    m->bat.push_back(t);
    m->bat_blocks.push_back(tiles + vch);
  }
  return P3D_OK;
}

extern "C" int p3d_grad_events(p3d_model* m, int32_t enable) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_grad_events: null model");
  std::vector<int32_t> lo;
  if (enable)
    for (int l = (int)m->layers.size() - 1; l >= 0; --l) lo.push_back(l);   // one bucket per layer
  return p3d_grad_buckets(m, (int32_t)lo.size(), lo.data());
}

// flat range of layer l's trainables (TF creation order: W, b[, gamma, beta]), padding included
extern "C" int p3d_layer_grad_range(const p3d_model* m, int32_t layer, int64_t* begin, int64_t* end) {
  if (!m || !begin || !end) return fail(P3D_ERR_ARG, "p3d_layer_grad_range: null argument");
  if (layer < 0 || layer >= (int32_t)m->layers.size()) return fail(P3D_ERR_ARG, "p3d_layer_grad_range: bad layer");
  *begin = m->layers[layer].w;
  *end = layer + 1 < (int32_t)m->layers.size() ? m->layers[layer + 1].w : m->n_flat;
  return P3D_OK;
}

extern "C" int p3d_stream_wait_grad(p3d_model* m, int32_t bucket, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_stream_wait_grad: null model");
  if (m->gev.empty()) return fail(P3D_ERR_STATE, "p3d_stream_wait_grad: no gradient buckets (p3d_grad_buckets)");
  if (bucket < 0 || bucket >= (int32_t)m->gev.size()) return fail(P3D_ERR_ARG, "p3d_stream_wait_grad: bad bucket");
  HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, m->gev[bucket], 0));
  return P3D_OK;
}

// Forward (training, dropout counter from the device step state) + fused MSE + backward,
// one call: the loss lands in loss_dev, the gradients in the flat grads buffer.  The
// output layer forms dy and the loss partials in its epilogue; the first backward kernel
// folds the partials (no k_mse launch).
extern "C" int p3d_train_fwd_bwd(p3d_model* m, const float* x, const float* t, int64_t B, float* y,
                                 float keep_prob, uint64_t seed, int64_t row_offset, float* loss_dev,
                                 void* stream) {
  if (!m || !x || !t || !y || !loss_dev) return fail(P3D_ERR_ARG, "p3d_train_fwd_bwd: null argument");
  if (m->cfg.dtype != P3D_DTYPE_F32) return fail(P3D_ERR_ARG, "p3d_train_fwd_bwd: bf16 models are inference-only");
  if (B <= 0 || B > m->cfg.max_batch) return fail(P3D_ERR_ARG, "p3d_train_fwd_bwd: B must be in 1..max_batch");
  if (!aligned16(t)) return fail(P3D_ERR_ARG, "p3d_train_fwd_bwd: t must be 16-byte aligned");
  int rc = forward_impl(m, x, B, y, 1, keep_prob, seed, P3D_CTR_GLOBAL_STEP, row_offset, 0, stream, t);
  if (rc) return rc;
  m->loss_dst = loss_dev;
  rc = p3d_backward(m, m->dybuf, B, stream);
  m->loss_dst = nullptr;
  return rc;
}

// The data-parallel step's first half: p3d_train_fwd_bwd, with the step's Adam alpha (lr =
// lr0 * decay_rate^(global_step / decay_steps), bias corrections from the device step state)
// formed by the backward's first launch, so that p3d_adam_apply -- after the caller's gradient
// all-reduce -- is one launch that also advances the step state.
extern "C" int p3d_train_fwd_bwd_lr(p3d_model* m, const float* x, const float* t, int64_t B, float* y,
                                    float keep_prob, uint64_t seed, int64_t row_offset, float lr0,
                                    float decay_steps, float decay_rate, float* loss_dev, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_train_fwd_bwd_lr: null model");
  if (!(decay_steps > 0.f)) return fail(P3D_ERR_ARG, "p3d_train_fwd_bwd_lr: decay_steps must be > 0");
  AdamFuse af{};
  af.st = m->dstate; af.lr_host = -1.0f; af.lr0 = lr0; af.decay_steps = decay_steps; af.decay_rate = decay_rate;
  af.b1 = 0.9f; af.b2 = 0.999f; af.eps = 1e-8f;
  m->dp_af = af;
  m->alpha_af = &m->dp_af;
  const int rc = p3d_train_fwd_bwd(m, x, t, B, y, keep_prob, seed, row_offset, loss_dev, stream);
  m->alpha_af = nullptr;
  return rc;
}

static int adam_launch(p3d_model* m, float lr_host, float lr0, float steps, float rate, hipStream_t st);

// The data-parallel step's second half (after the all-reduce of the flat gradient): TF1 Adam +
// re-pack of every weight with the alpha the backward formed, the step state advanced in the
// same launch.  Falls back to p3d_adam_step_decay's two launches when the backward formed no
// alpha (the whole-batch BN kernels, P3D_TRAIN_SPLIT=0).
extern "C" int p3d_adam_apply(p3d_model* m, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_adam_apply: null model");
  if (m->dp_af.decay_steps <= 0.f) return fail(P3D_ERR_STATE, "p3d_adam_apply: no p3d_train_fwd_bwd_lr before it");
  if (!m->alpha_ready)
    return adam_launch(m, -1.0f, m->dp_af.lr0, m->dp_af.decay_steps, m->dp_af.decay_rate, (hipStream_t)stream);
  m->alpha_ready = false;
  return adam_launch(m, -2.0f, m->dp_af.lr0, m->dp_af.decay_steps, m->dp_af.decay_rate, (hipStream_t)stream);
}

// The optimizer of ONE gradient bucket (p3d_grad_buckets), for the caller's stream right after
// that bucket's all-reduce: the stream first waits until the backward has issued the last
// reader of the bucket's parameters (dgrad of its lowest layer), then TF1 Adam + re-pack of
// the bucket's tensors with the alpha the backward formed; the last bucket's launch advances
// the step state.  Per element the arithmetic of p3d_adam_apply (bit-identical results); the
// buckets' optimizers overlap the rest of the backward instead of following it.  Without a
// backward-formed alpha (P3D_TRAIN_SPLIT=0) the last bucket runs p3d_adam_apply's fallback and
// the others nothing.
extern "C" int p3d_adam_apply_bucket(p3d_model* m, int32_t bucket, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_adam_apply_bucket: null model");
  if (m->bat.empty()) return fail(P3D_ERR_STATE, "p3d_adam_apply_bucket: no gradient buckets (p3d_grad_buckets)");
  if (bucket < 0 || bucket >= (int32_t)m->bat.size()) return fail(P3D_ERR_ARG, "p3d_adam_apply_bucket: bad bucket");
  if (m->dp_af.decay_steps <= 0.f) return fail(P3D_ERR_STATE, "p3d_adam_apply_bucket: no p3d_train_fwd_bwd_lr before it");
  if (m->cfg.max_norm) return fail(P3D_ERR_STATE, "p3d_adam_apply_bucket: max_norm models take p3d_adam_apply");
  hipStream_t st = (hipStream_t)stream;
  const bool last = bucket == (int32_t)m->bat.size() - 1;
  HIP_TRY(hipStreamWaitEvent(st, m->aev[bucket], 0));
  if (!m->alpha_ready) {
    if (!last) return P3D_OK;
    return adam_launch(m, -1.0f, m->dp_af.lr0, m->dp_af.decay_steps, m->dp_af.decay_rate, st);
  }
  m->serve_ec_dirty = true;
  AdamArgs a{};
  a.w = m->flat[0]; a.g = m->flat[1]; a.m = m->flat[2]; a.v = m->flat[3];
  a.wpk = m->wpk; a.st = m->dstate;
  a.lr_host = -2.0f; a.lr0 = m->dp_af.lr0; a.decay_steps = m->dp_af.decay_steps; a.decay_rate = m->dp_af.decay_rate;
  a.b1 = 0.9f; a.b2 = 0.999f; a.eps = 1e-8f;
  a.wsrc = m->w_pk;
  mark_w_stale(m, st);
  a.wblocks = m->bat[bucket].tile_begin[m->bat[bucket].nw];
  a.alpha_dev = m->alpha_dev;
  a.advance = last ? m->dstate : nullptr;
  if (m->bat_blocks[bucket] > 0) {
    ProfScope ps(m, "adam_bucket");
    go(ps, k_adam_pack, dim3(m->bat_blocks[bucket]), dim3(256), st, a, m->bat[bucket]);
    LAUNCH_CHECK("k_adam_pack (bucket)");
  }
  if (last) m->alpha_ready = false;
  return P3D_OK;
}

// One whole single-GPU TF1 training step (session.run([updates, loss, ...]),
// linear_model.py:225-237): forward + fused MSE + backward with the Adam update applied
// inside the weight-gradient kernels (no separate optimizer pass, no gradient round trip
// through HBM), then the step state advances.  --max_norm models (the clip's gradient needs
// every G first) take the unfused sequence.  lr = lr0 * decay_rate^(global_step/decay_steps).
extern "C" int p3d_train_step(p3d_model* m, const float* x, const float* t, int64_t B, float* y,
                              float keep_prob, uint64_t seed, float lr0, float decay_steps, float decay_rate,
                              float* loss_dev, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_train_step: null model");
  hipStream_t st = (hipStream_t)stream;
  if (m->cfg.max_norm || !m->train_split || !m->adam_in_wgrad) {
    int rc = p3d_train_fwd_bwd(m, x, t, B, y, keep_prob, seed, 0, loss_dev, stream);
    if (rc) return rc;
    return adam_launch(m, -1.0f, lr0, decay_steps, decay_rate, st);
  }
  AdamFuse af{};
  af.st = m->dstate; af.lr_host = -1.0f; af.lr0 = lr0; af.decay_steps = decay_steps; af.decay_rate = decay_rate;
  af.b1 = 0.9f; af.b2 = 0.999f; af.eps = 1e-8f;
  af.wsrc = m->w_pk;
  mark_w_stale(m, st);
  m->fuse_adam = &af;
  const int rc = p3d_train_fwd_bwd(m, x, t, B, y, keep_prob, seed, 0, loss_dev, stream);
  m->fuse_adam = nullptr;
  if (rc) return rc;
  if (!m->step_advanced) {   // (the attached form advanced it in its last launch)
    k_step_advance<<<1, 1, 0, st>>>(m->dstate, af.b1, af.b2);
    LAUNCH_CHECK("k_step_advance");
  }
  m->step_advanced = false;
  return P3D_OK;
}

static int adam_launch(p3d_model* m, float lr_host, float lr0, float steps, float rate, hipStream_t st) {
  m->serve_ec_dirty = true;
  AdamArgs a{};
  a.w = m->flat[0]; a.g = m->flat[1]; a.m = m->flat[2]; a.v = m->flat[3];
  a.wpk = m->wpk; a.st = m->dstate;
  a.lr_host = lr_host; a.lr0 = lr0; a.decay_steps = steps; a.decay_rate = rate;
  a.b1 = 0.9f; a.b2 = 0.999f; a.eps = 1e-8f;
  a.wsrc = m->w_pk;
  mark_w_stale(m, st);
  a.wblocks = m->at.tile_begin[m->at.nw];
  const bool pre = lr_host == -2.0f;   // alpha formed by the backward (p3d_adam_apply): advance in-launch
  if (pre) { a.alpha_dev = m->alpha_dev; a.advance = m->dstate; }
  {
    ProfScope ps(m, "adam_pack");
    go(ps, k_adam_pack, dim3(m->adam_blocks), dim3(256), st, a, m->at);
  }
  LAUNCH_CHECK("k_adam_pack");
  if (!pre) {
    k_step_advance<<<1, 1, 0, st>>>(m->dstate, a.b1, a.b2);
    LAUNCH_CHECK("k_step_advance");
  }
  if (m->cfg.max_norm) {
    k_dot_partial<<<dim3(DOT_CHUNKS, m->wtab.n), 256, 0, st>>>(m->flat[0], m->flat[0], m->wtab, m->scratch);
    LAUNCH_CHECK("k_dot_partial");
    k_dot_final<<<1, 64, 0, st>>>(m->scratch, m->wtab.n, m->wsq);
    LAUNCH_CHECK("k_dot_final");
  }
  return P3D_OK;
}

extern "C" int p3d_adam_step(p3d_model* m, float lr, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  if (!(lr >= 0.f)) return fail(P3D_ERR_ARG, "p3d_adam_step: lr must be >= 0");
  return adam_launch(m, lr, 0.f, 1.f, 1.f, (hipStream_t)stream);
}

extern "C" int p3d_adam_step_decay(p3d_model* m, float lr0, float decay_steps, float decay_rate, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  if (!(decay_steps > 0.f)) return fail(P3D_ERR_ARG, "p3d_adam_step_decay: decay_steps must be > 0");
  return adam_launch(m, -1.f, lr0, decay_steps, decay_rate, (hipStream_t)stream);
}

extern "C" int p3d_get_step(const p3d_model* m, int64_t* gs, float* b1p, float* b2p) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  StepState s{};
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&s, m->dstate, sizeof(StepState), hipMemcpyDeviceToHost));
  if (gs) *gs = s.global_step;
  if (b1p) *b1p = s.beta1_power;
  if (b2p) *b2p = s.beta2_power;
  return P3D_OK;
}

extern "C" int p3d_set_step(p3d_model* m, int64_t gs, float b1p, float b2p) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  StepState s{};
  s.global_step = gs; s.beta1_power = b1p; s.beta2_power = b2p; s.arrivals = 0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(m->dstate, &s, sizeof(StepState), hipMemcpyHostToDevice));
  return P3D_OK;
}

extern "C" int p3d_mpjpe_accum_ex(const float* pred_n, const float* gt_n, int32_t D, const double* mean96,
                                  const double* std96, const int32_t* dims, int64_t B, int32_t n_joints,
                                  int32_t procrustes, double* joint_sum, double* sq_sum, void* stream) {
  if (!pred_n || !gt_n || !mean96 || !std96 || !dims || !joint_sum)
    return fail(P3D_ERR_ARG, "p3d_mpjpe_accum: null argument");
  if (B <= 0) return fail(P3D_ERR_ARG, "p3d_mpjpe_accum: batch must be positive");
  if (n_joints < 1 || n_joints > P3D_MAX_JOINTS || D <= 0 || D % 3 != 0 ||
      (3 * n_joints - D != 0 && 3 * n_joints - D != 3))
    return fail(P3D_ERR_ARG, "p3d_mpjpe_accum: need D == 3*n_joints (predict_14) or 3*(n_joints-1) (root prepended)");
  MpjpeArgs a{};
  a.pred = pred_n; a.gt = gt_n; a.D = D; a.J = n_joints; a.root = (3 * n_joints - D) / 3;
  a.mean = mean96; a.stdv = std96; a.dims = dims; a.B = B; a.joint_sum = joint_sum; a.sq_sum = sq_sum;
  const unsigned grid = (unsigned)((B + 63) / 64);
  if (procrustes) k_mpjpe<true><<<grid, 64, 0, (hipStream_t)stream>>>(a);
  else k_mpjpe<false><<<grid, 64, 0, (hipStream_t)stream>>>(a);
  LAUNCH_CHECK("k_mpjpe");
  return P3D_OK;
}

extern "C" int p3d_mpjpe_accum(const float* pred_n, const float* gt_n, const double* mean96,
                               const double* std96, const int32_t* dims48, int64_t B, double* joint_sum17,
                               void* stream) {
  return p3d_mpjpe_accum_ex(pred_n, gt_n, 48, mean96, std96, dims48, B, 17, 0, joint_sum17, nullptr, stream);
}

// rocprofv3 name of the kernel a launch of `what` uses under the current tiling variants:
// 0 = inference hidden layer at B <= 64 (bench.py's roofline kernel), 1 = inference hidden
// layer at large M, 2 = BN-train hidden GEMM, 3 = the last p3d_serve kernel, 4 = inference hidden
// layer at batch <= 4 (k_gemv).
extern "C" int p3d_kernel_name(const p3d_model* m, int32_t what, char* out, int64_t out_len) {
  if (!m || !out || out_len <= 0) return fail(P3D_ERR_ARG, "p3d_kernel_name: bad argument");
  std::string n;
  if (what == 0) {
    switch (m->infer_wk) {
      case 8: n = "k_fwd<1, 8, 8, 2, true, true, 1>"; break;
      case 82: n = "k_fwd<1, 8, 2, 2, true, true, 1>"; break;
      default: n = "k_fwd<1, 16, 4, 2, true, true, 1>"; break;
    }
  } else if (what == 1) {
    n = "k_gemm_f32<2, 2>";
  } else if (what == 6) {
    // the optimizers' weight source (bench.py's byte count): "packed" = W read from its Wd copy, the
    // TF-layout master not written (28 B per weight element per fused step); "master" = 32 B
    n = m->w_pk ? "packed" : "master";
  } else if (what == 3 && m->serve_choice.form) {
    n = serve_form_name(*m->serve_choice.form);   // the kernel the last p3d_serve launched
  } else if (what == 3) {   // before any launch: the form launches no k_serve6 form takes run
    const int nl = m->cfg.num_layers;
    n = serve_kernel_name(serve_fallback_kind(nl), serve_fallback_depth(m->cfg.linear_size, nl),
                          (m->cfg.output_size + 15) / 16, 0, 4, false);
  } else if (what == 2) {
    n = m->train_split ? "k_fwd<1, 8, 8, 2, true, true, 1>" : "k_fwd<4, 8, 8, 2, true, true, 1>";
  } else if (what == 4) {
    n = "k_gemv<4, 16, 4>";   // inference hidden layer at B <= gemv_maxb
  } else if (what == 5) {
    n = m->bf16_kname;        // the kernel the last hidden bf16 layer ran
  } else {
    return fail(P3D_ERR_ARG, "p3d_kernel_name: unknown kernel selector");
  }
  strncpy(out, n.c_str(), (size_t)out_len - 1);
  out[out_len - 1] = 0;
  return P3D_OK;
}

// DLPack (v0.8 ABI) alias of device memory for the host binding (torch.from_dlpack):
// the managed-tensor record and its deleter live here, so freeing the view never calls
// back into Python (a ctypes-callback deleter crashed interpreter teardown).
namespace {
struct DlDevice { int32_t device_type; int32_t device_id; };
struct DlDType { uint8_t code; uint8_t bits; uint16_t lanes; };
struct DlTensor {
  void* data; DlDevice device; int32_t ndim; DlDType dtype; int64_t* shape; int64_t* strides;
  uint64_t byte_offset;
};
struct DlManaged { DlTensor dl_tensor; void* manager_ctx; void (*deleter)(DlManaged*); };
void dl_free(DlManaged* t) {
  if (!t) return;
  free(t->dl_tensor.shape);
  free(t);
}
}  // namespace

extern "C" void* p3d_dlpack_alias(void* data, int32_t ndim, const int64_t* shape, int32_t device_id,
                                  int32_t dtype_code, int32_t bits) {
  if (ndim <= 0 || !shape) return nullptr;
  DlManaged* t = (DlManaged*)calloc(1, sizeof(DlManaged));
  if (!t) return nullptr;
  t->dl_tensor.shape = (int64_t*)malloc(sizeof(int64_t) * (size_t)ndim);
  if (!t->dl_tensor.shape) { free(t); return nullptr; }
  for (int i = 0; i < ndim; ++i) t->dl_tensor.shape[i] = shape[i];
  t->dl_tensor.data = data;
  t->dl_tensor.device.device_type = 10;   // kDLROCM
  t->dl_tensor.device.device_id = device_id;
  t->dl_tensor.ndim = ndim;
  t->dl_tensor.dtype.code = (uint8_t)dtype_code;
  t->dl_tensor.dtype.bits = (uint8_t)bits;
  t->dl_tensor.dtype.lanes = 1;
  t->deleter = dl_free;
  return t;
}

__global__ void k_empty() {}

// (include/p3d.h) an empty launch through the model's launch path: the fixed cost of a launch +
// synchronise round trip that the headline's timed region pays beside its kernel (bench.py)
extern "C" int p3d_empty_launch(p3d_model* m, int32_t grid, void* stream) {
  if (!m || grid <= 0) return fail(P3D_ERR_ARG, "p3d_empty_launch: bad argument");
  ProfScope ps(m, "empty");
  HP_START
  go(ps, k_empty, dim3((unsigned)grid), dim3(256), (hipStream_t)stream);
  HP(8);
  LAUNCH_CHECK("k_empty");
  return P3D_OK;
}

extern "C" int p3d_profile_start(p3d_model* m, int32_t max_launches) {
  if (!m || max_launches <= 0) return fail(P3D_ERR_ARG, "p3d_profile_start: bad argument");
  for (auto e : m->ev) (void)hipEventDestroy(e);
  m->ev.assign(2 * (size_t)max_launches, nullptr);
  m->ev_tag.assign((size_t)max_launches, nullptr);
  for (auto& e : m->ev) HIP_TRY(hipEventCreate(&e));
  m->ev_used = 0;
  m->prof = true;
  return P3D_OK;
}

// Synchronises, then writes "tag<TAB>count<TAB>total_us<TAB>min_us<TAB>max_us\n" per tag.
extern "C" int p3d_profile_stop(p3d_model* m, char* out, int64_t out_len) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  m->prof = false;
  std::vector<std::string> tags;
  std::vector<double> tot, mn, mx;
  std::vector<int64_t> cnt;
  for (size_t k = 0; k < m->ev_used; ++k) {
    HIP_TRY(hipEventSynchronize(m->ev[2 * k + 1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, m->ev[2 * k], m->ev[2 * k + 1]));
    const double us = 1000.0 * ms;
    size_t t = 0;
    while (t < tags.size() && tags[t] != m->ev_tag[k]) ++t;
    if (t == tags.size()) { tags.push_back(m->ev_tag[k]); tot.push_back(0); mn.push_back(1e30); mx.push_back(0); cnt.push_back(0); }
    tot[t] += us; cnt[t] += 1;
    if (us < mn[t]) mn[t] = us;
    if (us > mx[t]) mx[t] = us;
  }
  std::string rep;
  char line[256];
  for (size_t t = 0; t < tags.size(); ++t) {
    snprintf(line, sizeof line, "%s\t%lld\t%.3f\t%.3f\t%.3f\n", tags[t].c_str(), (long long)cnt[t], tot[t], mn[t], mx[t]);
    rep += line;
  }
  if (out && out_len > 0) {
    strncpy(out, rep.c_str(), (size_t)out_len - 1);
    out[out_len - 1] = 0;
  }
  for (auto e : m->ev) (void)hipEventDestroy(e);
  m->ev.clear();
  m->ev_tag.clear();
  m->ev_used = 0;
  return P3D_OK;
}

// =====================================================================================
// H3.6M data pipeline (p3d_data.h)
// =====================================================================================
static int64_t p3d_moments_blocks(int64_t F) {
  int64_t g = (F + 255) / 256;
  return g < 1 ? 1 : (g > 4096 ? 4096 : g);
}

extern "C" int p3d_cam_transform(const double* P, int64_t n, int64_t in_cam_stride, const double* cams,
                                 int32_t C, int32_t inverse, double* out, void* stream) {
  if (n < 0 || C < 0) return fail(P3D_ERR_ARG, "p3d_cam_transform: negative size");
  if (n == 0 || C == 0) return 0;
  if (!P || !cams || !out) return fail(P3D_ERR_ARG, "p3d_cam_transform: null argument");
  if (in_cam_stride != 0 && in_cam_stride < 3 * n) return fail(P3D_ERR_ARG, "p3d_cam_transform: in_cam_stride < 3n");
  if (in_cam_stride == 0 && inverse == 0 && (const double*)out == P) return fail(P3D_ERR_ARG, "p3d_cam_transform: out aliases P");
  CamArgs a{P, in_cam_stride, n, cams, C, out, nullptr, nullptr, nullptr, nullptr};
  const dim3 grid((unsigned)((n + 255) / 256));
  if (inverse) k_cam_points<1><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  else k_cam_points<0><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  LAUNCH_CHECK("k_cam_points");
  return 0;
}

extern "C" int p3d_cam_project(const double* P, int64_t n, const double* cams, int32_t C, double* proj,
                               double* depth, double* radial, double* tan, double* r2, void* stream) {
  if (n < 0 || C < 0) return fail(P3D_ERR_ARG, "p3d_cam_project: negative size");
  if (n == 0 || C == 0) return 0;
  if (!P || !cams || !proj) return fail(P3D_ERR_ARG, "p3d_cam_project: null argument");
  CamArgs a{P, 0, n, cams, C, proj, depth, radial, tan, r2};
  k_cam_points<2><<<dim3((unsigned)((n + 255) / 256)), 256, 0, (hipStream_t)stream>>>(a);
  LAUNCH_CHECK("k_cam_points");
  return 0;
}

extern "C" int p3d_root_center(const double* poses, int64_t F, int32_t width, double* out, double* root,
                               void* stream) {
  if (F < 0 || width < 3 || width % 3) return fail(P3D_ERR_ARG, "p3d_root_center: width must be 3 * joints");
  if (F == 0) return 0;
  if (!poses || !out) return fail(P3D_ERR_ARG, "p3d_root_center: null argument");
  if ((const double*)out == poses) return fail(P3D_ERR_ARG, "p3d_root_center: out must not alias poses");
  const int64_t total = F * width;
  k_root_center<<<dim3((unsigned)((total + 255) / 256)), 256, 0, (hipStream_t)stream>>>(poses, F, width, out, root);
  LAUNCH_CHECK("k_root_center");
  return 0;
}

extern "C" int p3d_normalize(const double* x, int64_t F, int32_t D, const double* mean, const double* stdv,
                             const int32_t* dims_to_use, int32_t U, void* out, int32_t out_dtype, void* stream) {
  if (F < 0 || D <= 0 || U < 0) return fail(P3D_ERR_ARG, "p3d_normalize: bad size");
  if (out_dtype != P3D_DTYPE_F32 && out_dtype != P3D_DTYPE_F64) return fail(P3D_ERR_ARG, "p3d_normalize: out_dtype F32 or F64");
  if (F == 0 || U == 0) return 0;
  if (!x || !mean || !stdv || !dims_to_use || !out) return fail(P3D_ERR_ARG, "p3d_normalize: null argument");
  const int64_t total = F * U;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (out_dtype == P3D_DTYPE_F32) k_normalize<true><<<grid, 256, 0, (hipStream_t)stream>>>(x, F, D, mean, stdv, dims_to_use, U, out);
  else k_normalize<false><<<grid, 256, 0, (hipStream_t)stream>>>(x, F, D, mean, stdv, dims_to_use, U, out);
  LAUNCH_CHECK("k_normalize");
  return 0;
}

extern "C" int p3d_unnormalize(const void* xn, int32_t in_dtype, int64_t F, int32_t U, const double* mean,
                               const double* stdv, const int32_t* dims_to_use, int32_t D, double* out, void* stream) {
  if (F < 0 || U < 0 || D <= 0 || D > 256 || U > D) return fail(P3D_ERR_ARG, "p3d_unnormalize: need 0 <= U <= D <= 256");
  if (in_dtype != P3D_DTYPE_F32 && in_dtype != P3D_DTYPE_F64) return fail(P3D_ERR_ARG, "p3d_unnormalize: in_dtype F32 or F64");
  if (F == 0) return 0;
  if (!mean || !stdv || !out || (U > 0 && (!xn || !dims_to_use))) return fail(P3D_ERR_ARG, "p3d_unnormalize: null argument");
  const int64_t total = F * D;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (in_dtype == P3D_DTYPE_F32) k_unnormalize<true><<<grid, 256, 0, (hipStream_t)stream>>>(xn, F, U, mean, stdv, dims_to_use, D, out);
  else k_unnormalize<false><<<grid, 256, 0, (hipStream_t)stream>>>(xn, F, U, mean, stdv, dims_to_use, D, out);
  LAUNCH_CHECK("k_unnormalize");
  return 0;
}

// sample()'s numbers (src/predict_3dpose.py:512-546) for N rows in one launch: p3d_unnormalize,
// + root, p3d_cam_transform(inverse = 1) with each row's camera, p3d_root_center -- the same bits.
extern "C" int p3d_sample_world(const void* yn, int32_t in_dtype, int64_t N, int32_t U, const double* mean96,
                                const double* std96, const int32_t* dims_to_use, const double* root,
                                const double* cams, int32_t C, const int32_t* cam_of_row, double* out,
                                void* stream) {
  if (!yn || !mean96 || !std96 || !dims_to_use || !cams || !out)
    return fail(P3D_ERR_ARG, "p3d_sample_world: null argument");
  if (N < 1 || N > (1 << 20)) return fail(P3D_ERR_ARG, "p3d_sample_world: N must be in 1 .. 2^20");
  if (U < 1 || U > P3D_SAMPLE_W) return fail(P3D_ERR_ARG, "p3d_sample_world: U must be in 1 .. 96");
  if (C < 1 || C > P3D_SAMPLE_MAX_CAMS) return fail(P3D_ERR_ARG, "p3d_sample_world: C must be in 1 .. 64");
  if (in_dtype != P3D_DTYPE_F32 && in_dtype != P3D_DTYPE_F64)
    return fail(P3D_ERR_ARG, "p3d_sample_world: in_dtype F32 or F64");
  if (!aligned16(out)) return fail(P3D_ERR_ARG, "p3d_sample_world: out must be 16-byte aligned");
  if (((uintptr_t)root & 7) != 0) return fail(P3D_ERR_ARG, "p3d_sample_world: root must be 8-byte aligned");
  SampleArgs a{yn, N, U, mean96, std96, dims_to_use, root, cams, C, cam_of_row, out};
  const int64_t tiles = (N + P3D_SAMPLE_ROWS - 1) / P3D_SAMPLE_ROWS;
  const dim3 grid((unsigned)(tiles < P3D_SAMPLE_MAX_BLOCKS ? tiles : P3D_SAMPLE_MAX_BLOCKS));
  hipStream_t s = (hipStream_t)stream;
  if (in_dtype == P3D_DTYPE_F64) k_sample_world<false, false><<<grid, 256, 0, s>>>(a);
  else if (aligned16(yn)) k_sample_world<true, true><<<grid, 256, 0, s>>>(a);
  else k_sample_world<true, false><<<grid, 256, 0, s>>>(a);
  LAUNCH_CHECK("k_sample_world");
  return 0;
}

// src/openpose_3dpose_sandbox.py:347-356 per call: normalise the mapped 2D rows (float32, the
// placeholder cast), the eval forward, unNormalizeData -- as ONE launch where the batch-1 chain
// runs (B <= 4, the model's hidden layers on the device at once), else as p3d_normalize +
// p3d_forward_ex + p3d_unnormalize; the same bits either way.
extern "C" int p3d_lift(p3d_model* m, const double* raw, int64_t B, int32_t D2, const double* mean2,
                        const double* std2, const int32_t* use2, int32_t U2, const double* mean3, const double* std3,
                        const int32_t* use3, int32_t U3, int32_t D3, double* out, void* stream) {
  if (!m || !raw || !mean2 || !std2 || !use2 || !mean3 || !std3 || !use3 || !out)
    return fail(P3D_ERR_ARG, "p3d_lift: null argument");
  const p3d_cfg& c = m->cfg;
  if (B <= 0 || B > c.max_batch) return fail(P3D_ERR_ARG, "p3d_lift: batch must be in 1..max_batch");
  if (U2 != c.input_size || U3 != c.output_size || D2 < U2 || D3 < U3 || D3 > 256)
    return fail(P3D_ERR_ARG, "p3d_lift: dimension sets do not match the model");
  if (c.dtype != P3D_DTYPE_F32 || !m->lift_x) return fail(P3D_ERR_ARG, "p3d_lift: float32 models only");
  hipStream_t st = (hipStream_t)stream;
  if (B <= m->gemv_maxb) {
    GemvFrames fr{};
    fr.raw = raw; fr.ldraw = D2; fr.mean2 = mean2; fr.std2 = std2; fr.use2 = use2;
    fr.out = out; fr.D3 = D3; fr.mean3 = mean3; fr.std3 = std3; fr.use3 = use3;
    if (m->hwait) { fr.hflag = m->hflag_dev; fr.hcnt = m->hcnt; fr.hseq = m->hwait; }
    const int r = forward_gemv(m, nullptr, B, nullptr, 1.0f, 0, 0, 0, 0, st, &fr);   // (keep 1: no dropout, seed unused)
    if (r == P3D_OK && m->hwait) m->harmed = true;
    if (r != 1) return r;
  }
  int r = p3d_normalize(raw, B, D2, mean2, std2, use2, U2, m->lift_x, P3D_DTYPE_F32, stream);
  if (r) return r;
  r = forward_impl(m, m->lift_x, B, m->lift_y, 0, 1.0f, 0, 0, 0, 0, stream, nullptr);
  if (r) return r;
  return p3d_unnormalize(m->lift_y, P3D_DTYPE_F32, B, U3, mean3, std3, use3, D3, out, stream);
}

// ---- the *_sync calls: launch, then wait for the results in host memory --------------------------
// The launch's last output writer stores the call's sequence number into the completion word (errw[8],
// pinned and coherent) once its host-memory outputs are system-visible; the host spins on that word
// instead of the runtime's completion signal (tools/flag_probe.hip on MI355X: 8.5 vs 13.6 us for a
// one-workgroup kernel, 32.1 vs 37.8 us for 256 workgroups writing 256 KB of rows).  Every 4096 polls
// the stream is queried, so a launch that ends without storing the word (a fault, a launch whose
// workgroups could not synchronise) is reported instead of waited for.  The stream's own completion
// is not waited for: later work on it is ordered behind the launch as usual.
// the kernels' pinned error words, read after a host wait so that the caller's separate check is
// needed only when the call fails (p3d_error_flags reports and clears them)
static int host_errors(p3d_model* m, const char* what) {
  if (__atomic_load_n(&m->errw[0], __ATOMIC_ACQUIRE) || __atomic_load_n(&m->errw[1], __ATOMIC_ACQUIRE))
    return fail(P3D_ERR_HIP, std::string(what) + ": a kernel reported a failed in-launch synchronisation "
                                                 "(p3d_error_flags)");
  return P3D_OK;
}

// idx 8 (the *_sync calls): the word must equal the launch's own sequence number.  idx 9
// (p3d_host_signal's counter, which only advances): a count already passed has been reached too,
// compared as a wrapping difference.
static int host_wait(p3d_model* m, unsigned seq, hipStream_t st, const char* what, int idx = 8) {
  unsigned* word = reinterpret_cast<unsigned*>(m->errw) + idx;
  const auto reached = [&]() {
    const unsigned w = __atomic_load_n(word, __ATOMIC_ACQUIRE);
    return idx == 9 ? (int32_t)(w - seq) >= 0 : w == seq;
  };
  for (uint64_t n = 1;; ++n) {
    if (reached()) return P3D_OK;
    if ((n & 4095) == 0) {
      const hipError_t e = hipStreamQuery(st);
      if (e == hipSuccess) {
        if (reached()) return P3D_OK;
        return fail(P3D_ERR_HIP, std::string(what) + ": the launch completed without storing its completion word");
      }
      if (e != hipErrorNotReady) return fail(P3D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
}

// arm the next launch with a fresh sequence number; refuses a capturing stream (a replayed graph
// would store a stale number)
static int host_arm(p3d_model* m, hipStream_t st, const char* what, unsigned& seq) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const hipError_t e = hipStreamIsCapturing(st, &cap);
  if (e != hipSuccess) return fail(P3D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  if (cap != hipStreamCaptureStatusNone) return fail(P3D_ERR_STATE, std::string(what) + ": not capturable (waits on the host)");
  if (++m->hseq == 0) ++m->hseq;
  seq = m->hseq;
  m->hwait = seq;
  m->harmed = false;
  return P3D_OK;
}

static int host_finish(p3d_model* m, int rc, unsigned seq, hipStream_t st, const char* what) {
  const bool armed = m->harmed;
  m->hwait = 0;
  m->harmed = false;
  if (rc) return rc;
  if (!armed) {   // a form without the completion word: the runtime's completion
    const hipError_t e = hipStreamSynchronize(st);
    return e == hipSuccess ? P3D_OK : fail(P3D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  }
  if (int rc2 = host_wait(m, seq, st, what)) return rc2;
  return host_errors(m, what);
}

// (include/p3d.h) p3d_serve_mse, returning once y and *loss hold the results
extern "C" int p3d_serve_mse_sync(p3d_model* m, const float* x, int64_t B, float* y, const float* t, float* loss,
                                  void* stream) {
  if (!m || !t || !loss) return fail(P3D_ERR_ARG, "p3d_serve_mse_sync: null argument");
  hipStream_t st = (hipStream_t)stream;
  unsigned seq = 0;
  if (int rc = host_arm(m, st, "p3d_serve_mse_sync", seq)) return rc;
  return host_finish(m, serve_impl(m, x, B, y, t, loss, stream), seq, st, "p3d_serve_mse_sync");
}

// (include/p3d.h) p3d_lift, returning once out holds the results
extern "C" int p3d_lift_sync(p3d_model* m, const double* raw, int64_t B, int32_t D2, const double* mean2,
                             const double* std2, const int32_t* use2, int32_t U2, const double* mean3,
                             const double* std3, const int32_t* use3, int32_t U3, int32_t D3, double* out,
                             void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_lift_sync: null model");
  hipStream_t st = (hipStream_t)stream;
  unsigned seq = 0;
  if (int rc = host_arm(m, st, "p3d_lift_sync", seq)) return rc;
  return host_finish(m, p3d_lift(m, raw, B, D2, mean2, std2, use2, U2, mean3, std3, use3, U3, D3, out, stream), seq, st,
                     "p3d_lift_sync");
}

// ---- a whole OpenPose clip (p3d_clip.h; src/openpose_3dpose_sandbox.py:140-227, 317-417) ---------
static int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }

static ClipWork clip_work(void* work, int64_t N) {
  const int64_t nch = p3d_clip_chunks(N);
  char* p = (char*)work;
  ClipWork w;
  w.mask = (unsigned long long*)p;
  w.last = (double*)(p + nch * 8);
  w.first = (int32_t*)(p + nch * 8 + nch * P3D_CLIP_COLS * 8);
  return w;
}

extern "C" int32_t p3d_clip_chunk(void) { return P3D_CLIP_CHUNK; }

extern "C" int64_t p3d_clip_workspace(int64_t N) {
  if (N <= 0) return 0;
  return align256(p3d_clip_chunks(N) * (8 + P3D_CLIP_COLS * (8 + 4)));
}

static int clip_check_n(const char* what, int64_t N, int32_t smooth, void* work, int64_t work_bytes) {
  if (N < 1 || N > P3D_CLIP_MAX_N)
    return fail(P3D_ERR_ARG, std::string(what) + ": N must be in 1.." + std::to_string(P3D_CLIP_MAX_N) + " frames");
  if (smooth && N >= 2 && N <= 8)
    return fail(P3D_ERR_ARG, std::string(what) + ": need more frames, min 9 frames for smoothing");
  if (!work || ((uintptr_t)work & 7)) return fail(P3D_ERR_ARG, std::string(what) + ": null or misaligned workspace");
  if (work_bytes < p3d_clip_workspace(N)) return fail(P3D_ERR_ARG, std::string(what) + ": workspace too small");
  return P3D_OK;
}

extern "C" int p3d_clip_prepare(const double* xy, int64_t N, int32_t smooth, const double* mean2, const double* std2,
                                const int32_t* use2, int32_t U2, float* x, double* xy_s, void* work,
                                int64_t work_bytes, void* stream) {
  if (!xy || !mean2 || !std2 || !use2 || !x || !xy_s) return fail(P3D_ERR_ARG, "p3d_clip_prepare: null argument");
  if (int rc = clip_check_n("p3d_clip_prepare", N, smooth, work, work_bytes)) return rc;
  if (U2 < 1 || U2 > 64) return fail(P3D_ERR_ARG, "p3d_clip_prepare: U2 must be in 1..64");
  if ((const double*)xy_s == xy) return fail(P3D_ERR_ARG, "p3d_clip_prepare: xy_s must not alias xy");
  ClipInArgs a{};
  a.xy = xy; a.N = N; a.smooth = (smooth && N > 1) ? 1 : 0;   // (a single frame passes through, :140-143)
  a.mean2 = mean2; a.std2 = std2; a.use2 = use2; a.U2 = U2; a.x = x; a.xy_s = xy_s;
  a.w = clip_work(work, N);
  const unsigned nch = (unsigned)p3d_clip_chunks(N);
  hipStream_t st = (hipStream_t)stream;
  k_clip_in<<<dim3(nch), P3D_CLIP_THREADS, 0, st>>>(a);
  LAUNCH_CHECK("k_clip_in");
  if (a.smooth && nch > 1) {   // the hold across chunk boundaries
    k_clip_in_carry<<<dim3(nch - 1), P3D_CLIP_THREADS, 0, st>>>(a);
    LAUNCH_CHECK("k_clip_in_carry");
  }
  return P3D_OK;
}

extern "C" int p3d_clip_finish(const float* y, int64_t N, const double* xy_s, const double* mean3, const double* std3,
                               const int32_t* use3, int32_t U3, int32_t D3, int32_t cache_on_fail, double* poses,
                               int32_t* src, void* work, int64_t work_bytes, void* stream) {
  if (!y || !xy_s || !mean3 || !std3 || !use3 || !poses) return fail(P3D_ERR_ARG, "p3d_clip_finish: null argument");
  if (int rc = clip_check_n("p3d_clip_finish", N, 0, work, work_bytes)) return rc;
  if (D3 != P3D_CLIP_D3) return fail(P3D_ERR_ARG, "p3d_clip_finish: D3 must be 96 (32 joints)");
  if (U3 < 1 || U3 > D3) return fail(P3D_ERR_ARG, "p3d_clip_finish: U3 must be in 1..96");
  ClipOutArgs a{};
  a.y = y; a.N = N; a.xy_s = xy_s; a.mean3 = mean3; a.std3 = std3; a.use3 = use3; a.U3 = U3;
  a.cache_on_fail = cache_on_fail ? 1 : 0; a.poses = poses; a.src = src;
  a.w = clip_work(work, N);
  const unsigned nch = (unsigned)p3d_clip_chunks(N);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)P3D_CLIP_CHUNK * U3 * sizeof(float);
  k_clip_out<<<dim3(nch), P3D_CLIP_THREADS, lds, st>>>(a);
  LAUNCH_CHECK("k_clip_out");
  if (a.cache_on_fail && nch > 1) {   // the held pose across chunk boundaries
    k_clip_out_carry<<<dim3(nch - 1), P3D_CLIP_THREADS, 0, st>>>(a);
    LAUNCH_CHECK("k_clip_out_carry");
  }
  return P3D_OK;
}

extern "C" int64_t p3d_clip_lift_workspace(int64_t N, int32_t U2, int32_t U3) {
  if (N <= 0 || U2 <= 0 || U3 <= 0) return 0;
  return p3d_clip_workspace(N) + align256(N * U2 * (int64_t)sizeof(float)) + align256(N * U3 * (int64_t)sizeof(float));
}

// prepare, the eval forward in tiles of max_batch rows (the forward_impl of p3d_lift's three-step
// form: every tile's rows carry p3d_lift's bits at that batch), finish -- all on `stream`
extern "C" int p3d_clip_lift(p3d_model* m, const double* xy, int64_t N, int32_t smooth, const double* mean2,
                             const double* std2, const int32_t* use2, int32_t U2, const double* mean3,
                             const double* std3, const int32_t* use3, int32_t U3, int32_t D3, int32_t cache_on_fail,
                             double* xy_s, double* poses, int32_t* src, void* work, int64_t work_bytes, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_clip_lift: null model");
  const p3d_cfg& c = m->cfg;
  if (c.dtype != P3D_DTYPE_F32) return fail(P3D_ERR_ARG, "p3d_clip_lift: float32 models only");
  if (U2 != c.input_size || U3 != c.output_size) return fail(P3D_ERR_ARG, "p3d_clip_lift: dimension sets do not match the model");
  if (int rc = clip_check_n("p3d_clip_lift", N, smooth, work, work_bytes)) return rc;
  if (work_bytes < p3d_clip_lift_workspace(N, U2, U3)) return fail(P3D_ERR_ARG, "p3d_clip_lift: workspace too small");
  if ((uintptr_t)work & 255) return fail(P3D_ERR_ARG, "p3d_clip_lift: workspace must be 256-byte aligned");
  const int64_t wb = p3d_clip_workspace(N);
  float* x = (float*)((char*)work + wb);
  float* y = (float*)((char*)x + align256(N * U2 * (int64_t)sizeof(float)));
  int rc = p3d_clip_prepare(xy, N, smooth, mean2, std2, use2, U2, x, xy_s, work, wb, stream);
  if (rc) return rc;
  for (int64_t r = 0; r < N; r += c.max_batch) {
    const int64_t B = N - r < c.max_batch ? N - r : (int64_t)c.max_batch;
    rc = forward_impl(m, x + r * U2, B, y + r * U3, 0, 1.0f, 0, 0, 0, 0, stream, nullptr);
    if (rc) return rc;
  }
  return p3d_clip_finish(y, N, xy_s, mean3, std3, use3, U3, D3, cache_on_fail, poses, src, work, wb, stream);
}

// One workgroup, stream-ordered behind everything before it (a captured step's last node): the
// model's signal counter advanced and its new value stored into the pinned word errw[9] with a
// system-scope release.  The earlier kernels' host-memory outputs must be in coherent host memory
// (p3d_host_alloc: uncached on the device, complete when their kernels complete).
__global__ void k_host_signal(unsigned* cnt, unsigned* word) {
  if (threadIdx.x == 0) {
    const unsigned v = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
    __hip_atomic_store(cnt, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(word, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// (include/p3d.h) enqueue the signal; capturable (each replay of a graph holding it signals once)
extern "C" int p3d_host_signal(p3d_model* m, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_host_signal: null model");
  k_host_signal<<<1, 64, 0, (hipStream_t)stream>>>(m->hcnt + 8, reinterpret_cast<unsigned*>(m->hflag_dev) + 1);
  LAUNCH_CHECK("k_host_signal");
  return P3D_OK;
}

// (include/p3d.h) wait on the host until the model's signal count reaches `count`, then read the
// kernels' error words (the stream is queried every 4096 polls, as the *_sync calls do)
extern "C" int p3d_host_wait(p3d_model* m, uint32_t count, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_host_wait: null model");
  if (int rc = host_wait(m, count, (hipStream_t)stream, "p3d_host_wait", 9)) return rc;
  return host_errors(m, "p3d_host_wait");
}

// (include/p3d.h) coherent pinned host memory the kernels write without caching it on the device
extern "C" void* p3d_host_alloc(int64_t bytes) {
  void* p = nullptr;
  if (bytes <= 0) { fail(P3D_ERR_ARG, "p3d_host_alloc: bytes must be positive"); return nullptr; }
  const hipError_t e = hipHostMalloc(&p, (size_t)bytes, hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) { fail(P3D_ERR_HIP, std::string("p3d_host_alloc: ") + hipGetErrorString(e)); return nullptr; }
  memset(p, 0, (size_t)bytes);
  return p;
}

extern "C" int p3d_host_free(void* p) {
  if (!p) return P3D_OK;
  const hipError_t e = hipHostFree(p);
  return e == hipSuccess ? P3D_OK : fail(P3D_ERR_HIP, std::string("p3d_host_free: ") + hipGetErrorString(e));
}

extern "C" int64_t p3d_moments_workspace(int64_t F, int32_t D) {
  if (F <= 0 || D <= 0) return 0;
  return p3d_moments_blocks(F) * (int64_t)D * (int64_t)sizeof(double);
}

extern "C" int p3d_moments(const double* x, int64_t F, int32_t D, double* mean, double* stdv, void* work,
                           int64_t work_bytes, void* stream) {
  if (F <= 0 || D <= 0 || D > 256) return fail(P3D_ERR_ARG, "p3d_moments: need F >= 1 and 1 <= D <= 256");
  if (!x || !mean || !stdv || !work) return fail(P3D_ERR_ARG, "p3d_moments: null argument");
  if (work_bytes < p3d_moments_workspace(F, D)) return fail(P3D_ERR_ARG, "p3d_moments: workspace too small");
  const int64_t G = p3d_moments_blocks(F), chunk = (F + G - 1) / G;
  const hipStream_t st = (hipStream_t)stream;
  double* part = (double*)work;
  const dim3 gf((unsigned)D);
  k_col_partial<1><<<dim3((unsigned)G), 256, 0, st>>>(x, F, D, chunk, nullptr, part);
  k_col_final<1><<<gf, 256, 0, st>>>(part, (int)G, D, F, mean);
  k_col_partial<2><<<dim3((unsigned)G), 256, 0, st>>>(x, F, D, chunk, mean, part);
  k_col_final<2><<<gf, 256, 0, st>>>(part, (int)G, D, F, stdv);
  LAUNCH_CHECK("k_col_partial");
  return 0;
}

// ---------------------------------------------------------------------------------------
// CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) of host memory, slicing-by-8: the
// checksum of TF's tensor bundles (every tensor's bytes and every index-table block,
// checkpoint_io.py / tf_bundle.py), far too slow byte by byte in Python for 51 MB of state.
// crc = p3d_crc32c(data, n, 0) for a whole buffer; pass the previous result to continue.
// ---------------------------------------------------------------------------------------
namespace {
struct Crc32cTables {
  uint32_t t[8][256];
  Crc32cTables() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xFFu];
  }
};
const Crc32cTables& crc32c_tables() {
  static const Crc32cTables tb;
  return tb;
}
}  // namespace

extern "C" uint32_t p3d_crc32c(const void* data, int64_t n, uint32_t crc) {
  const Crc32cTables& tb = crc32c_tables();
  const unsigned char* p = (const unsigned char*)data;
  uint32_t c = ~crc;
  while (n > 0 && ((uintptr_t)p & 7)) { c = (c >> 8) ^ tb.t[0][(c ^ *p++) & 0xFFu]; --n; }
  while (n >= 8) {
    uint64_t v;
    memcpy(&v, p, 8);
    const uint32_t lo = (uint32_t)v ^ c, hi = (uint32_t)(v >> 32);
    c = tb.t[7][lo & 0xFF] ^ tb.t[6][(lo >> 8) & 0xFF] ^ tb.t[5][(lo >> 16) & 0xFF] ^ tb.t[4][lo >> 24] ^
        tb.t[3][hi & 0xFF] ^ tb.t[2][(hi >> 8) & 0xFF] ^ tb.t[1][(hi >> 16) & 0xFF] ^ tb.t[0][hi >> 24];
    p += 8;
    n -= 8;
  }
  while (n-- > 0) c = (c >> 8) ^ tb.t[0][(c ^ *p++) & 0xFFu];
  return ~c;
}

// The VAE pose filter, its noise and its bones (include/p3d.h; kernels in p3d_vae*.h, p3d_bones.h)
#include "p3d_vae_host.h"
#include "p3d_clips_host.h"
#include "p3d_live_host.h"

#include "p3d_dp.h"
