// p3d_model.h -- the lifter's model (include/p3d.h: p3d_model): its tensors and layers, the owner
// of its device memory, events and comm stream (DevMem), the environment knobs (Knobs and their one
// table), the state of each concern as a sub-struct, create / destroy / teardown at exit, the
// parameter access and re-derivation calls, the step state, p3d_kernel_name, the profiler's entry
// points and the caller-owned pinned memory (p3d_host_alloc / p3d_host_free).  Host code; included
// by p3d.hip behind p3d_host.h, the kernel headers (their argument structs and tables) and
// p3d_serve_plan.h.
#pragma once

struct p3d_comm;

namespace {

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

// ---- the one owner of device memory, pinned host memory, events and the comm stream ------------
// Every slot is a member of the model (its address holds as long as the model does).  A slot is
// recorded when the owner fills it (alloc) or is told of it (adopt: the event groups and the comm
// stream that p3d_grad_buckets, p3d_profile_start and p3d_dp.h create where they need them);
// release() destroys whatever the recorded slots hold and nulls them, so it is safe on a partly
// filled owner and on slots never filled.
enum MemFill { kMemAsIs, kMemZero, kMemCopy, kMemPinned };

// one block: n elements at *slot.  kMemCopy: filled from n host elements at src; kMemPinned: mapped,
// coherent, zeroed host memory, its device view stored at *dview
struct MemRow { void** slot; int64_t n; size_t elem; MemFill fill; const void* src; void** dview; };
template <typename T>
MemRow mem_row(T** slot, int64_t n, MemFill fill, const void* src = nullptr, T** dview = nullptr) {
  return {(void**)slot, n, sizeof(T), fill, src, (void**)dview};
}

struct DevMem {
  enum Kind { kDev, kPinned, kEvent, kEvents, kStream };
  struct Rec { Kind kind; void* slot; };
  std::vector<Rec> recs;

  // the rows in order, each allocated, recorded and filled; rows of no elements are skipped
  hipError_t alloc(std::initializer_list<MemRow> rows) {
    for (const MemRow& r : rows) {
      if (r.n <= 0) continue;
      const size_t bytes = (size_t)r.n * r.elem;
      const bool pin = r.fill == kMemPinned;
      hipError_t e = pin ? hipHostMalloc(r.slot, bytes, hipHostMallocMapped | hipHostMallocCoherent) : hipMalloc(r.slot, bytes);
      if (e != hipSuccess) return e;
      recs.push_back({pin ? kPinned : kDev, r.slot});
      if (pin) memset(*r.slot, 0, bytes);
      if (pin && (e = hipHostGetDevicePointer(r.dview, *r.slot, 0)) != hipSuccess) return e;
      if (r.fill == kMemZero && (e = hipMemset(*r.slot, 0, bytes)) != hipSuccess) return e;
      if (r.fill == kMemCopy && (e = hipMemcpy(*r.slot, r.src, bytes, hipMemcpyHostToDevice)) != hipSuccess) return e;
    }
    return hipSuccess;
  }
  void adopt(hipEvent_t* e) { recs.push_back({kEvent, e}); }
  void adopt(std::vector<hipEvent_t>* v) { recs.push_back({kEvents, v}); }
  void adopt(hipStream_t* s) { recs.push_back({kStream, s}); }
  // an adopted event group, destroyed and emptied ahead of its re-creation
  static void drop(std::vector<hipEvent_t>& v) {
    for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e);
    v.clear();
  }
  // everything recorded from record `from` on (serve_alloc undoes its own rows with it)
  void release(size_t from = 0) {
    for (size_t i = recs.size(); i-- > from;) {
      void** s = (void**)recs[i].slot;   // (events and streams are pointers too)
      if (recs[i].kind == kEvents) { drop(*(std::vector<hipEvent_t>*)recs[i].slot); continue; }
      if (!*s) continue;
      switch (recs[i].kind) {
        case kDev: (void)hipFree(*s); break;
        case kPinned: (void)hipHostFree(*s); break;
        case kEvent: (void)hipEventDestroy((hipEvent_t)*s); break;
        case kStream: (void)hipStreamDestroy((hipStream_t)*s); break;
        case kEvents: break;
      }
      *s = nullptr;
    }
    recs.resize(from);
  }
};

// ---- the environment knobs ------------------------------------------------------------------
// Read once, at the top of p3d_create (knobs_from_env below: one row per variable).
struct Knobs {
  int adam_in_wgrad = 1;      // env P3D_FUSE_ADAM (default 1): p3d_train_step applies Adam inside k_wgrad_multi
                              // (bit-identical; measured slower than k_adam_pack at cfg3)
  int out_part = 1;           // training output layer as split-K partials + dy in its dgrad (env P3D_OUT_PART)
  int train_split = 1;        // BN-train layers as GEMM (256 WGs) + k_bn_fwd / k_bn_bwd (env P3D_TRAIN_SPLIT)
  int in_train_wk = 2;        // waves of the BN-train input-layer launch (exchange form; env P3D_IN_TRAIN_WK: 8, 4, 2)
  int dgrad_out_wk = 4;       // waves of the output layer's dgrad launch (K = 48; env P3D_DGRAD_OUT_WK: 8, 4)
  int xchg_wk = 8;            // BN-train hidden exchange-form forward: 8 waves with an 8-deep ring (measured and
                              // pruned in round 4: 16 waves 8.6 vs 6.8 us; rings of 4 / 2 within 1 %)
  int dgrad_wk = 16;          // hidden data-gradient tiling (env P3D_DGRAD_WK: 16 waves, else 8)
  int train_xchg = 1;         // split BN-train layers as ONE launch when the grid fits (env P3D_TRAIN_XCHG, p3d_xchg.h)
  int xchg_delay = 0;         // test hook: late row-tile siblings (env P3D_XCHG_TEST_DELAY, p3d_xchg.h)
  int xchg_remap = 1;         // exchange launches as 1-D grids with the siblings on one XCD (env P3D_XCHG_REMAP)
  int bf16_stages = 48;             // hidden bf16 GEMM form (launch_bf16_layer; env P3D_BF16_STAGES: 48, 0)
  // --max_norm off: every optimizer reads the weights from Wd and leaves the TF-layout master
  // unwritten (AdamFuse::wsrc); w_stale marks a master behind Wd until p3d_params_sync (env
  // P3D_W_MASTER=1: the optimizers write the master, as before round 4)
  int w_pk = 1;
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
  int serve_delay = 0, serve_delay_xcc = 0;  // test hook (env P3D_SERVE_TEST_DELAY=n[,xcc]): on odd-numbered
                                   // p3d_serve calls every workgroup on XCD xcc starts ~n x 3.4 us late
  int serve_fault = 0;             // test hook: the census waits for one workgroup more than the grid
                                   // (env P3D_SERVE_TEST_FAULT): every launch fails its census
  int serve_groups = 0;     // at most this many groups take steps, 0 = all (env P3D_SERVE_GROUPS)
  // (k_serve5: two groups per XCD, two units per contraction, a 4-deep ring where L / 64 allows; the
  // other group counts, unit pairings and ring depths measured slower and were removed in round 6,
  // DESIGN 5a; k_serve, for models without residual blocks: 4 K slices, a 2-deep ring)
  int wgrad_multi = 1;           // all layers' dW in one k_wgrad_multi launch (env P3D_WGRAD_MULTI)
                                 // (measured and rejected, round 3: two adjacent 64x64 tiles per
                                 // workgroup, 528 workgroups in one round instead of 768 + 288:
                                 // 29.7 vs 28.4 us -- the launch is bound by its 148 MB HBM stream)
  // (measured and removed, round 6: weight-gradient + Adam tiles riding the data-gradient launches,
  // 109.5 vs 102.2 us per cfg3 step; each layer's on a side stream, 197-202 vs 122 us -- DESIGN 5c)
  int dp_adam = 1;               // env P3D_DP_ADAM: 1 per-bucket optimizer on the compute stream behind its
                                 // all-reduce, 0 one optimizer pass after the last bucket, 2 per bucket on the
                                 // comm stream (round 3's form: slows the neighbouring dgrad launches)
  int dp_force_multi = 0;        // env P3D_DP_FORCE_MULTI=1 (tests, bench): a 1-rank group takes the N > 1 form
                                 // -- comm-stream fork, per-bucket ncclAvg, rev joins -- so the single-GPU box
                                 // executes and times the code every rank of an 8-GPU run executes
  ServeKnobs serve_knobs;   // env P3D_SERVE6* (p3d_serve_plan.h)
};

// how a variable's text becomes the member's value: atoi | atoi clamped to 0..4 | 0 where atoi is
// non-zero, else 1 | 1 where atoi is non-zero, else 0 | "n[,xcc]": atoi, and xcc & 7 into serve_delay_xcc
enum KnobRule { kKnobInt, kKnobClamp04, kKnobInverted, kKnobNonZero, kKnobDelayXcc };
struct KnobRow { const char* env; int Knobs::*member; KnobRule rule; };
const KnobRow kKnobRows[] = {
    {"P3D_OUT_PART", &Knobs::out_part, kKnobInt},            // training output layer as split-K partials
    {"P3D_INFER_WK", &Knobs::infer_wk, kKnobInt},            // inference tiling variant: 82, 8, else 16 waves
    {"P3D_IN_WK", &Knobs::in_wk, kKnobInt},                  // input layer variant, 0 = infer_wk
    {"P3D_OUT_WK", &Knobs::out_wk, kKnobInt},                // output layer variant, 0 = infer_wk
    {"P3D_OUT_TRAIN_WK", &Knobs::out_train_wk, kKnobInt},    // training output layer (fused MSE) variant
    {"P3D_BIG_M", &Knobs::big_m, kKnobInt},                  // M from which inference takes k_gemm_f32, 0 never
    {"P3D_GEMV_MAXB", &Knobs::gemv_maxb, kKnobClamp04},      // inference at B <= this runs the k_gemv layers
    {"P3D_GEMV_FOLD", &Knobs::gemv_fold, kKnobInt},          // ... input / output layers folded into their neighbours
    {"P3D_GEMV_CHAIN", &Knobs::gemv_chain, kKnobInt},        // ... as one persistent launch
    {"P3D_TRAIN_SPLIT", &Knobs::train_split, kKnobInt},      // BN-train layers as GEMM + k_bn_fwd / k_bn_bwd
    {"P3D_IN_TRAIN_WK", &Knobs::in_train_wk, kKnobInt},      // waves of the BN-train input layer: 8, 4, 2
    {"P3D_DGRAD_OUT_WK", &Knobs::dgrad_out_wk, kKnobInt},    // waves of the output layer's dgrad: 8, 4
    {"P3D_DGRAD_WK", &Knobs::dgrad_wk, kKnobInt},            // hidden data-gradient tiling: 16 waves, else 8
    {"P3D_TRAIN_XCHG", &Knobs::train_xchg, kKnobInt},        // split BN-train layers as one launch when the grid fits
    {"P3D_XCHG_TEST_DELAY", &Knobs::xchg_delay, kKnobInt},   // test hook: late row-tile siblings
    {"P3D_DP_ADAM", &Knobs::dp_adam, kKnobInt},              // data-parallel optimizer placement: 1, 0, 2
    {"P3D_DP_FORCE_MULTI", &Knobs::dp_force_multi, kKnobNonZero},   // a 1-rank group takes the N > 1 form
    {"P3D_W_MASTER", &Knobs::w_pk, kKnobInverted},           // 1: the optimizers write the TF-layout master
    {"P3D_XCHG_REMAP", &Knobs::xchg_remap, kKnobInt},        // exchange launches as 1-D grids, siblings on one XCD
    {"P3D_SERVE_TEST_FAULT", &Knobs::serve_fault, kKnobInt}, // test hook: every serve launch fails its census
    {"P3D_SERVE_TEST_DELAY", &Knobs::serve_delay, kKnobDelayXcc},   // test hook: XCD xcc starts ~n x 3.4 us late
    {"P3D_FUSE_ADAM", &Knobs::adam_in_wgrad, kKnobInt},      // p3d_train_step applies Adam inside k_wgrad_multi
    {"P3D_WGRAD_MULTI", &Knobs::wgrad_multi, kKnobInt},      // all layers' dW in one k_wgrad_multi launch
    {"P3D_SERVE_GROUPS", &Knobs::serve_groups, kKnobInt},    // at most this many serve groups take steps, 0 = all
    {"P3D_BF16_STAGES", &Knobs::bf16_stages, kKnobInt},      // hidden bf16 GEMM form: 48, 0
};

Knobs knobs_from_env() {
  Knobs k;
  for (const KnobRow& r : kKnobRows) {
    const char* ev = getenv(r.env);
    if (!ev) continue;
    const int v = atoi(ev);
    switch (r.rule) {
      case kKnobInt: k.*r.member = v; break;
      case kKnobClamp04: k.*r.member = std::max(0, std::min(4, v)); break;
      case kKnobInverted: k.*r.member = v ? 0 : 1; break;
      case kKnobNonZero: k.*r.member = v != 0; break;
      case kKnobDelayXcc:
        k.*r.member = v;
        if (const char* c = strchr(ev, ',')) k.serve_delay_xcc = atoi(c + 1) & 7;
        break;
    }
  }
  k.serve_knobs = serve_knobs_from_env();
  return k;
}

// ---- the model's state by concern (the files named use it) ------------------------------------
// p3d_train_host.h: what a training forward leaves for its backward, the fused step's hand-overs,
// the gradient buckets
struct TrainCache {
  float* loss_dst = nullptr;  // set during p3d_train_fwd_bwd: the backward folds the loss here
  const AdamFuse* fuse_adam = nullptr;  // set during p3d_train_step: Adam fused into the backward
  float* opart = nullptr;     // [16 row tiles][4 column tiles][8] 1 KB partials (k_out_part)
  bool opart_pending = false; // the last training forward left the output layer to the backward's first launch
  const float* opart_t = nullptr;   // its targets and y (row-major, the caller's)
  float* opart_y = nullptr;
  // training cache
  bool have_cache = false;
  const float* x_cached = nullptr;
  int64_t B_cached = 0;
  float keep = 1.f;
  uint64_t seed = 0, ctr = 0;
  int64_t row_off = 0;
  const int64_t* ctr_dev = nullptr;   // cached training-forward counter source
  std::vector<hipEvent_t> gev;   // per-bucket gradient-ready events (p3d_grad_buckets / p3d_grad_events)
  std::vector<hipEvent_t> aev;   // per-bucket "parameters free" events: the backward's last reader of the
                                 // bucket's parameters (dgrad of its lowest layer) has been issued
  std::vector<AdamTable> bat;    // per-bucket optimizer tables (p3d_adam_apply_bucket)
  std::vector<int> bat_blocks;
  std::vector<int> bucket_lo;    // lowest layer of each bucket, buckets in backward order (layers hi..lo)
  const AdamFuse* alpha_af = nullptr;  // set during p3d_train_fwd_bwd_lr: the backward forms the step's alpha
  AdamFuse dp_af{};              // hyper-parameters of the last p3d_train_fwd_bwd_lr (p3d_adam_apply)
  bool alpha_ready = false;      // the last backward formed alpha_dev (p3d_adam_apply reads it)
  float* alpha_dev = nullptr;    // the step's Adam alpha, formed by the first backward launch
  bool step_advanced = false;    // set by a backward whose last launch advanced the step state
};

// p3d_forward_host.h (use_xchg / xchg_site), p3d_train_host.h: the BN-train exchange form
struct XchgState {
  unsigned* xsync = nullptr;  // exchange form: per site (layer, direction) L/16 column-tile epoch words (one
                              // 128-B line each), then per site P3D_XCHG_MAXR x L 16-B slots (p3d_xchg.h)
  int64_t xslots_off = 0;     // word offset of the slot arrays in xsync
};

// p3d_serve_host.h (host_wait / host_arm / host_finish, the error checks): what host and kernels
// exchange through pinned memory
struct HostSync {
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
};

// p3d_forward_host.h (launch_bf16_layer, forward_bf16)
struct Bf16State {
  // bf16 inference models (cfg5)
  unsigned short* wbf = nullptr;    // packed bf16 weights
  float* aff = nullptr;             // BN-eval affine per BN layer
  unsigned short* abf = nullptr;    // bf16 packed activations, one slab per layer (+ x slab)
  int64_t Mpad128 = 0;
  std::string kname;                // the kernel the last hidden bf16 layer ran (p3d_kernel_name 5)
};

// p3d_forward_host.h (forward_gemv), p3d_data_host.h (p3d_lift): batch <= 4 inference
struct GemvState {
  int slots = 0;            // workspace slots (ws_row / 16) the fold's hand-off buffer covers (others unfolded)
  int64_t slot_floats = 0;          // hand-off floats per slot (the chain's H layers, or the fold's one)
  float* hand = nullptr;            // [slot][layers][4 rows][L / 2] 16-B granules (layer-output hand-offs)
  float* lift_x = nullptr;          // p3d_lift's normalised rows and outputs where it runs the three steps
  float* lift_y = nullptr;
  unsigned* epoch = nullptr;        // [slot] epoch words, P3D_XCHG_EPOCH_STRIDE apart
};

// p3d_serve_host.h
struct ServeState {
  // persistent XCD-local evaluation (p3d_serve): per-XCD activation slabs, output partials,
  // census/barrier words and the spin-timeout flag; allocated at the first call
  float* buf = nullptr;
  float* act6 = nullptr;         // k_serve6's activation slabs (4 per group, P3D_SERVE6_ROWS rows in all)
  float* loss = nullptr;         // p3d_serve_mse: per-output-tile partials + the arrival counter
  float* ecg = nullptr;            // k_serve6 epilogue-constant table (k_serve_prep), [layer][tile][48] + divisors
  bool ec_dirty = true;            // parameters or moving statistics changed since the table was formed
  unsigned* sync = nullptr;        // [k_serve6 bank 0 | bank 1 | k_serve5 bank | device epoch word ...]
  int64_t calls = 0;
  int grid = 0;
  // the last launch's choice, by (batch, with loss): serve_plan prices 64 candidates, redone only
  // when the key changes -- the host enqueue of a serving loop
  int64_t B = -1;
  bool with_loss = false;
  ServeChoice choice;
};

// p3d_dp.h
struct DpState {
  // data-parallel step with the library's own all-reduce (p3d_dp.h)
  p3d_comm* comm = nullptr;      // not owned (p3d_comm_create / p3d_comm_destroy)
  hipStream_t cst = nullptr;     // comm stream (non-blocking), forked from / joined to the caller's stream
  hipEvent_t cjoin = nullptr;    // join event of the comm-stream optimizer form (P3D_DP_ADAM=2)
  std::vector<hipEvent_t> rev;   // per-bucket "all-reduce done" events
};

}  // namespace

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
  float* dybuf = nullptr;     // [max_batch, output_size]: dy of the fused MSE
  int num_cus = 0;            // compute units of the device (exchange-form residency bound)
  float* wsq = nullptr;       // [nW] ||W||^2
  float* gw = nullptr;        // [nW] <G,W>
  PackTable pt;
  UnpackTable ut;
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
  Knobs knobs;
  TrainCache train;
  XchgState xchg;
  HostSync host;
  Bf16State bf16;
  GemvState gemv;
  ServeState serve;
  DpState dp;
  ProfState prof;
  DevMem mem;                 // owns every device / pinned block, event and stream above
};

inline ProfScope::ProfScope(p3d_model* m, const char* tag) : ProfScope(m ? &m->prof : nullptr, tag) {}

namespace {

// The pointers the kernels of layer l take from the model: the packed forward weights, bias, the
// BN parameters and moving statistics (null without BN), the max-norm ||W||^2 (null without
// max_norm), and for bf16 models the packed bf16 weights and the BN-eval affine.
struct LayerPtrs {
  const float *Wf, *bias, *gamma, *beta, *wsq;
  float *mmean, *mvar;   // (a BN-train forward updates them)
  const unsigned short* Bt;
  const float *inv, *shift;
};
LayerPtrs layer_ptrs(const p3d_model* m, int l) {
  const Layer& ly = m->layers[l];
  const bool bf = m->cfg.dtype == P3D_DTYPE_BF16;
  LayerPtrs p{};
  p.Wf = m->wpk + ly.wf; p.bias = m->flat[0] + ly.b;
  p.wsq = m->cfg.max_norm ? m->wsq + ly.widx : nullptr;
  if (ly.bn) {
    p.gamma = m->flat[0] + ly.gamma; p.beta = m->flat[0] + ly.beta;
    p.mmean = m->moving + ly.mmean; p.mvar = m->moving + ly.mvar;
  }
  if (bf) p.Bt = m->bf16.wbf + ly.wbf;
  if (bf && ly.bn) { p.inv = m->bf16.aff + ly.aff; p.shift = m->bf16.aff + ly.aff + ly.N; }
  return p;
}

// An optimizer is issued that leaves the TF-layout masters behind Wd (AdamFuse::wsrc).
void mark_w_stale(p3d_model* m, hipStream_t st) {
  if (!m->knobs.w_pk) return;
  m->w_stale = true;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) m->w_sticky = true;
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
  m->mem.release();
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
  m->knobs = knobs_from_env();
  if (m->cfg.max_norm) m->knobs.w_pk = 0;   // (||W||^2 of the max-norm scale is summed over the master)
  // the one way out of a failed create: whatever the owner holds so far is released
  auto bail = [&](int code, const std::string& msg) {
    m->mem.release();
    delete m;
    return fail(code, msg);
  };
  // the events and the stream created later, where they are needed, are the owner's to destroy
  m->mem.adopt(&m->train.gev);
  m->mem.adopt(&m->train.aev);
  m->mem.adopt(&m->prof.ev);
  m->mem.adopt(&m->dp.rev);
  m->mem.adopt(&m->dp.cjoin);
  m->mem.adopt(&m->dp.cst);
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
    if (t >= P3D_MAX_W) return bail(P3D_ERR_ARG, "too many layers");
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
      if (at.nv >= P3D_MAX_V) return bail(P3D_ERR_ARG, "too many parameter vectors");
      at.voff[at.nv] = tn.off; at.vlen[at.nv] = (int)tn.numel; at.vbegin[at.nv] = vch;
      vch += (int)((tn.numel + 1023) / 1024);
      at.nv++;
    }
    at.vbegin[at.nv] = vch;
    m->adam_blocks = tiles + vch;
  }


  const auto hip_bail = [&](hipError_t e) { return bail(P3D_ERR_HIP, std::string("p3d_create: ") + hipGetErrorString(e)); };
  hipError_t e;
  // workspace: per hidden layer act, z, dz (packed [Bpad, L]); stats; dout x2
  const int64_t Bp = m->Bpad;
  const int nl = (int)m->layers.size();
  int64_t need = 0;
  for (int l = 0; l < nl - 1; ++l) need += 3 * pad64(Bp * L) + 2 * pad64(L);
  need += 2 * pad64(Bp * L);
  // split BN-train partials [R][L][2] and fused-MSE loss partials for R = max_batch/16 row tiles
  const int64_t R_max = (c.max_batch + 15) / 16;
  const int64_t nlossp_max = pad64(R_max * ((c.output_size + 15) / 16));
  const int64_t scratch_n = (int64_t)P3D_MAX_W * DOT_CHUNKS + 2 * 64 + R_max * 2 * (int64_t)L + nlossp_max +
                            pad64((int64_t)c.max_batch * ((c.output_size + 15) / 16 * 16));
  if ((e = m->mem.alloc({
           mem_row(&m->flat[0], m->n_flat, kMemZero),
           mem_row(&m->flat[1], m->n_flat, kMemZero),
           mem_row(&m->flat[2], m->n_flat, kMemZero),
           mem_row(&m->flat[3], m->n_flat, kMemZero),
           mem_row(&m->moving, m->n_moving + 64, kMemZero),
           mem_row(&m->wpk, m->n_wpk, kMemZero),
           mem_row(&m->ws, need, kMemZero),
           mem_row(&m->scratch, scratch_n, kMemZero),
           mem_row(&m->train.opart, (int64_t)16 * 4 * 8 * 256, kMemAsIs),
       })) != hipSuccess)
    return hip_bail(e);
  int dev = 0;
  if ((e = hipGetDevice(&dev)) != hipSuccess) return hip_bail(e);
  if ((e = hipDeviceGetAttribute(&m->num_cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess)
    return hip_bail(e);
  m->xchg.xslots_off = (int64_t)2 * nl * (L / 16) * P3D_XCHG_EPOCH_STRIDE;
  const int64_t nx = m->xchg.xslots_off + (int64_t)2 * 2 * nl * P3D_XCHG_MAXR * L * 4;   // sc1 + plain copies
  int64_t nh = 0, ne = 0;
  if (m->knobs.gemv_fold && m->knobs.gemv_maxb > 0 && c.dtype == P3D_DTYPE_F32 && L <= P3D_GEMV_FOLD_MAXK) {
    // batch <= 4 fold: the first 64 workspace slots (ws_row < 1024) get a hand-off area of
    // 4 rows x L / 2 granules (32 KB at L = 1024) and an epoch word each
    m->gemv.slots = (int)std::min<int64_t>(64, (c.max_batch + 15) / 16);
    const int H = nl - 2;
    const bool chain = H >= 1 && H <= P3D_GEMV_CHAIN_MAXH && L <= P3D_GEMV_CHAIN_MAXK && H * (L / 16) <= m->num_cus;
    m->gemv.slot_floats = (int64_t)(chain ? H + 1 : 1) * 4 * (L / 2) * 4;
    nh = (int64_t)m->gemv.slots * m->gemv.slot_floats;
    ne = (int64_t)m->gemv.slots * P3D_XCHG_EPOCH_STRIDE;
  }
  // p3d_lift's three-step form (any batch; every float32 model, whether or not the batch <= 4
  // fold / chain is configured): normalised rows and network outputs
  const bool f32 = c.dtype == P3D_DTYPE_F32;
  int* dv = nullptr;
  StepState s0{};
  s0.global_step = 0; s0.beta1_power = 0.9f; s0.beta2_power = 0.999f; s0.arrivals = 0;
  if ((e = m->mem.alloc({
           mem_row(&m->xchg.xsync, nx, kMemZero),
           mem_row(&m->gemv.hand, nh, kMemZero),
           mem_row(&m->gemv.epoch, ne, kMemZero),
           mem_row(&m->gemv.lift_x, f32 ? (int64_t)c.max_batch * c.input_size : 0, kMemAsIs),
           mem_row(&m->gemv.lift_y, f32 ? (int64_t)c.max_batch * c.output_size : 0, kMemAsIs),
           mem_row(&m->host.errw, 64, kMemPinned, nullptr, &dv),
           mem_row(&m->train.alpha_dev, 64, kMemAsIs),
           mem_row(&m->host.hcnt, 512, kMemZero),
           mem_row(&m->dstate, 1, kMemCopy, &s0),
       })) != hipSuccess)
    return hip_bail(e);
  m->host.xerr = dv;
  m->host.serve_err = dv + 1;
  m->host.hflag_dev = (unsigned*)(dv + 8);
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
        return hip_bail(e);
      if ((e = hipMemcpy(m->moving + m->layers[l].mvar, ones.data(), L * 4, hipMemcpyHostToDevice)) != hipSuccess)
        return hip_bail(e);
    }
  }
  if (c.dtype == P3D_DTYPE_BF16) {
    int64_t nbf = 0, naff = 0;
    for (auto& ly : m->layers) {
      const int NP = (ly.N + 15) / 16 * 16;
      ly.wbf = nbf; nbf += pad64((int64_t)NP * ly.K);
      if (ly.bn) { ly.aff = naff; naff += 2 * pad64(ly.N); }
    }
    m->bf16.Mpad128 = (c.max_batch + 127) / 128 * 128;
    const int64_t slab = m->bf16.Mpad128 * L;  // bf16 elements per activation slab
    if ((e = m->mem.alloc({
             mem_row(&m->bf16.wbf, nbf, kMemZero),
             mem_row(&m->bf16.aff, naff + 64, kMemAsIs),
             mem_row(&m->bf16.abf, (int64_t)(nl + 1) * slab, kMemZero),
         })) != hipSuccess)
      return hip_bail(e);
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
  m->serve.ec_dirty = true;
  if (m->cfg.dtype == P3D_DTYPE_BF16) {
    for (const Layer& ly : m->layers) {
      const int NP = (ly.N + 15) / 16 * 16;
      const int64_t items = (int64_t)(NP / 16) * (ly.K / 32) * 64;
      k_pack_bf16<<<(unsigned)((items + 255) / 256), 256, 0, st>>>(m->flat[0] + ly.w, ly.K, ly.N, m->bf16.wbf + ly.wbf);
      LAUNCH_CHECK("k_pack_bf16");
      if (ly.bn) {
        k_bn_affine<<<(ly.N + 255) / 256, 256, 0, st>>>(m->flat[0] + ly.gamma, m->flat[0] + ly.beta,
                                                        m->moving + ly.mmean, m->moving + ly.mvar, m->cfg.bn_eps,
                                                        ly.N, m->bf16.aff + ly.aff, m->bf16.aff + ly.aff + ly.N);
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
  m->serve.ec_dirty = true;
  return P3D_OK;
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

// rocprofv3 name of the kernel a launch of `what` uses under the current tiling variants:
// 0 = inference hidden layer at B <= 64 (bench.py's roofline kernel), 1 = inference hidden
// layer at large M, 2 = BN-train hidden GEMM, 3 = the last p3d_serve kernel, 4 = inference hidden
// layer at batch <= 4 (k_gemv).
extern "C" int p3d_kernel_name(const p3d_model* m, int32_t what, char* out, int64_t out_len) {
  if (!m || !out || out_len <= 0) return fail(P3D_ERR_ARG, "p3d_kernel_name: bad argument");
  std::string n;
  if (what == 0) {
    switch (m->knobs.infer_wk) {
      case 8: n = "k_fwd<1, 8, 8, 2, true, true, 1>"; break;
      case 82: n = "k_fwd<1, 8, 2, 2, true, true, 1>"; break;
      default: n = "k_fwd<1, 16, 4, 2, true, true, 1>"; break;
    }
  } else if (what == 1) {
    n = "k_gemm_f32<2, 2>";
  } else if (what == 6) {
    // the optimizers' weight source (bench.py's byte count): "packed" = W read from its Wd copy, the
    // TF-layout master not written (28 B per weight element per fused step); "master" = 32 B
    n = m->knobs.w_pk ? "packed" : "master";
  } else if (what == 3 && m->serve.choice.form) {
    n = serve_form_name(*m->serve.choice.form);   // the kernel the last p3d_serve launched
  } else if (what == 3) {   // before any launch: the form launches no k_serve6 form takes run
    const int nl = m->cfg.num_layers;
    n = serve_kernel_name(serve_fallback_kind(nl), serve_fallback_depth(m->cfg.linear_size, nl),
                          (m->cfg.output_size + 15) / 16, 0, 4, false);
  } else if (what == 2) {
    n = m->knobs.train_split ? "k_fwd<1, 8, 8, 2, true, true, 1>" : "k_fwd<4, 8, 8, 2, true, true, 1>";
  } else if (what == 4) {
    n = "k_gemv<4, 16, 4>";   // inference hidden layer at B <= gemv_maxb
  } else if (what == 5) {
    n = m->bf16.kname;        // the kernel the last hidden bf16 layer ran
  } else {
    return fail(P3D_ERR_ARG, "p3d_kernel_name: unknown kernel selector");
  }
  strncpy(out, n.c_str(), (size_t)out_len - 1);
  out[out_len - 1] = 0;
  return P3D_OK;
}

extern "C" int p3d_profile_start(p3d_model* m, int32_t max_launches) {
  if (!m || max_launches <= 0) return fail(P3D_ERR_ARG, "p3d_profile_start: bad argument");
  DevMem::drop(m->prof.ev);
  m->prof.ev.assign(2 * (size_t)max_launches, nullptr);
  m->prof.ev_tag.assign((size_t)max_launches, nullptr);
  for (auto& e : m->prof.ev) HIP_TRY(hipEventCreate(&e));
  m->prof.ev_used = 0;
  m->prof.on = true;
  return P3D_OK;
}

// Synchronises, then writes "tag<TAB>count<TAB>total_us<TAB>min_us<TAB>max_us\n" per tag.
extern "C" int p3d_profile_stop(p3d_model* m, char* out, int64_t out_len) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  m->prof.on = false;
  std::vector<std::string> tags;
  std::vector<double> tot, mn, mx;
  std::vector<int64_t> cnt;
  for (size_t k = 0; k < m->prof.ev_used; ++k) {
    HIP_TRY(hipEventSynchronize(m->prof.ev[2 * k + 1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, m->prof.ev[2 * k], m->prof.ev[2 * k + 1]));
    const double us = 1000.0 * ms;
    size_t t = 0;
    while (t < tags.size() && tags[t] != m->prof.ev_tag[k]) ++t;
    if (t == tags.size()) { tags.push_back(m->prof.ev_tag[k]); tot.push_back(0); mn.push_back(1e30); mx.push_back(0); cnt.push_back(0); }
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
  DevMem::drop(m->prof.ev);
  m->prof.ev_tag.clear();
  m->prof.ev_used = 0;
  return P3D_OK;
}

// (include/p3d.h) coherent pinned host memory the kernels write without caching it on the device
// (the caller's to free with p3d_host_free: no model owns it, so it stands beside DevMem, not in it)
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
