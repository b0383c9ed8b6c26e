// p3d_serve_host.h -- the lifter's serve path (include/p3d.h: p3d_serve*): the kernel table over
// P3D_SERVE_FORMS, the first call's buffers, serve_impl, the planner's export, the error words'
// checks (p3d_serve_check, p3d_sync_check, p3d_error_flags), the host waits on the pinned
// completion word (host_arm / host_wait / host_finish) with the *_sync calls built on them, and
// p3d_host_signal / p3d_host_wait (with the one-workgroup k_host_signal).  Host code; included by
// p3d.hip behind p3d_forward_host.h (forward_gemv) and p3d_model.h (ServeState, HostSync, DevMem);
// the kernels are in p3d_serve.h and p3d_serve6.h, the planner in p3d_serve_plan.h.
#pragma once

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
  m->serve.grid = cus;   // one 512-thread workgroup per CU (the LDS ring admits one)
  // output partials: k_serve5 keeps one per 32-column unit (U), k_serve6 one per 16-column tile (2U)
  const int64_t nbuf = P3D_SERVE_GROUPS * 3 * slab + P3D_SERVE_GROUPS * 2 * (int64_t)(2 * U) * PT;
  const int64_t necg = (int64_t)(2 * c.num_layers + 2) * (L / 16) * 48 + 64;
  // all or nothing: a failure leaves none of the rows in the model, and the next call starts over
  const size_t mark = m->mem.recs.size();
  const hipError_t e = m->mem.alloc({
      mem_row(&m->serve.buf, nbuf, kMemZero),
      // [bank 0 | bank 1 | k_serve5 bank | epoch word]: k_serve6 alternates banks 0 / 1 by the
      // device epoch word (p3d_serve6.h), k_serve5 uses bank 2 (zeroed before each of its launches)
      mem_row(&m->serve.sync, P3D_SERVE_SYNC_ALL, kMemZero),
      mem_row(&m->serve.ecg, necg, kMemAsIs),
      mem_row(&m->serve.act6, (int64_t)4 * P3D_SERVE6_ROWS * L, kMemAsIs),
      // the fused MSE's per-tile partials (kServeLossTiles: serve_plan refuses a loss over more) and
      // its arrival counter (the word after them), zero between launches
      mem_row(&m->serve.loss, kServeLossTiles + 64, kMemZero),
  });
  if (e != hipSuccess) m->mem.release(mark);
  SERVE_TRY(e);
  m->serve.ec_dirty = true;
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
  if (m->host.errw && m->host.errw[1])
    return fail(P3D_ERR_HIP, "p3d_serve: an earlier launch failed (not all workgroups resident); p3d_serve_check "
                             "reports and clears it");
  hipStream_t st = (hipStream_t)stream;
  // batch <= 4 with the loss: the persistent small-batch forward (k_gemv_chain, ~13 us where a 64-row
  // k_serve6 unit takes ~30) with the loss reduced by its last output workgroup -- still one launch;
  // y has p3d_forward's bits at this batch, the loss p3d_mse's on that y (stream-ordered with the
  // model's other batch <= 4 calls: they share workspace slot 0)
  if (t && loss && B <= m->knobs.gemv_maxb) {
    GemvFrames fr{};
    fr.tgt = t; fr.loss = loss;
    fr.hcnt = m->host.hcnt; fr.sq = reinterpret_cast<float*>(m->host.hcnt + 256);
    if (m->host.hwait) { fr.hflag = m->host.hflag_dev; fr.hseq = m->host.hwait; }
    const int r = forward_gemv(m, x, B, y, 1.0f, 0, 0, 0, 0, st, &fr);
    if (r == P3D_OK && m->host.hwait) m->host.harmed = true;
    if (r != 1) return r;   // (1: no chain form for this model -- k_serve6 below)
  }
  if (!m->serve.buf) {
    const int r = serve_alloc(m);
    if (r != P3D_OK) return r;
  }
  const int L = c.linear_size;
  ServeArgs a{};
  a.x = x; a.y = y; a.M = B;
  a.L = L; a.K0 = c.input_size; a.ND = c.output_size; a.nblk = c.num_layers;
  a.bn = c.batch_norm; a.residual = c.residual; a.eps = c.bn_eps;
  a.act = m->serve.buf; a.part = m->serve.buf + P3D_SERVE_GROUPS * 3 * (int64_t)64 * L;
  a.sync = m->serve.sync; a.err = m->host.serve_err;
  a.epoch = m->serve.sync + 3 * P3D_SERVE_SYNC_WORDS;
  a.census_extra = m->knobs.serve_fault ? 1 : 0;
  a.delay = (m->knobs.serve_delay > 0 && (m->serve.calls++ & 1) == 0) ? m->knobs.serve_delay : 0;
  a.delay_xcc = m->knobs.serve_delay_xcc;
  a.max_groups = m->knobs.serve_groups;
  for (size_t l = 0; l < m->layers.size(); ++l) {
    const LayerPtrs p = layer_ptrs(m, (int)l);
    ServeLayer& s = a.ly[l];
    s.Wf = p.Wf; s.bias = p.bias; s.wsq = p.wsq;
    s.gamma = p.gamma; s.beta = p.beta; s.mmean = p.mmean; s.mvar = p.mvar;
  }
  if (B != m->serve.B || (t != nullptr) != m->serve.with_loss) {
    const ServeChoice ch = serve_plan(L, c.num_layers, (c.output_size + 15) / 16, m->serve.grid, m->knobs.serve_knobs, B,
                                      t != nullptr);
    if (ch.refused) return fail(P3D_ERR_ARG, ch.refused);
    m->serve.choice = ch; m->serve.B = B; m->serve.with_loss = t != nullptr;
  }
  const ServeForm& f = *m->serve.choice.form;
  const bool use6 = serve_kind_is6(f.kind);
  a.split = m->serve.choice.S;
  a.nb = m->serve.choice.nb;   // batch-64 steps, or k_serve6's units of 16 RT rows
  a.ecg = m->serve.ecg;
  // a HIP graph being captured replays this call with whatever parameters it then finds: the
  // epilogue-constant table is formed inside the graph (one small launch per replay), not
  // decided once at capture time
  HP(0);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  SERVE_TRY(hipStreamIsCapturing(st, &cap));
  const bool capturing = cap != hipStreamCaptureStatusNone;
  HP(1);

  if (use6 && (m->serve.ec_dirty || capturing)) {
    // the epilogue-constant table, formed once per parameter version (refresh_derived, a
    // training forward and every Adam step mark it stale): steady-state calls are one launch
    const int nl = 2 * c.num_layers + 1;
    k_serve_prep<<<(unsigned)((nl * L + 255) / 256), 256, 0, st>>>(a, m->serve.ecg);
    LAUNCH_CHECK("k_serve_prep");
    if (!capturing) m->serve.ec_dirty = false;
  }
  if (use6) {
    // (k_serve6 picks its bank from the device epoch word: no memset in front, graph replays
    // alternate the banks by themselves)
    a.act = m->serve.act6;                   // [group][4 slabs][16 RT rows][L]; no output partials
    a.part = nullptr;
  } else {   // k_serve5: its own bank, zeroed in front of every launch
    a.sync = m->serve.sync + 2 * P3D_SERVE_SYNC_WORDS;
    SERVE_TRY(hipMemsetAsync(a.sync, 0, P3D_SERVE_SYNC_WORDS * sizeof(unsigned), st));
  }
  if (t) {   // (serve_plan lets only k_serve6 forms carry the loss)
    a.tgt = t; a.loss = loss;
    a.lpart = m->serve.loss; a.lcnt = (unsigned*)(m->serve.loss + kServeLossTiles);
    if (m->host.hwait && !f.pair) { a.hflag = m->host.hflag_dev; a.hseq = m->host.hwait; m->host.harmed = true; }
  }
  ProfScope ps(m, "serve");
  HP(2);
  go(ps, kServeKernels[&f - kServeForms], dim3((unsigned)m->serve.grid), dim3((unsigned)serve_kind_threads(f.kind)), st, a);
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
  if (e == hipSuccess && m->serve.sync) e = hipMemset(m->serve.sync, 0, P3D_SERVE_SYNC_ALL * sizeof(unsigned));
  // (a failed launch may have left the fused MSE's arrival counter short)
  if (e == hipSuccess && m->serve.loss) e = hipMemset(m->serve.loss, 0, (kServeLossTiles + 64) * sizeof(float));
  if (e != hipSuccess) return fail(P3D_ERR_HIP, std::string("p3d_serve_check: ") + hipGetErrorString(e));
  __atomic_store_n(&m->host.errw[1], 0, __ATOMIC_SEQ_CST);
  return fail(P3D_ERR_HIP, serve_err_text(v));
}

extern "C" int p3d_serve_check(p3d_model* m) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return fail(P3D_ERR_HIP, std::string("p3d_serve_check: ") + hipGetErrorString(e));
  const int v = __atomic_load_n(&m->host.errw[1], __ATOMIC_SEQ_CST);
  return v ? serve_report(m, v) : P3D_OK;
}

extern "C" int p3d_sync_check(p3d_model* m) {
  if (!m) return fail(P3D_ERR_ARG, "null model");
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return fail(P3D_ERR_HIP, std::string("p3d_sync_check: ") + hipGetErrorString(e));
  if (__atomic_load_n(&m->host.errw[0], __ATOMIC_SEQ_CST)) {
    __atomic_store_n(&m->host.errw[0], 0, __ATOMIC_SEQ_CST);
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
  const int x = __atomic_load_n(&m->host.errw[0], __ATOMIC_SEQ_CST), v = __atomic_load_n(&m->host.errw[1], __ATOMIC_SEQ_CST);
  *flags = (x ? 1 : 0) | (v == 1 ? 2 : 0) | (v == 2 ? 4 : 0);
  if (clear) {
    if (x) __atomic_store_n(&m->host.errw[0], 0, __ATOMIC_SEQ_CST);
    if (v) {
      (void)serve_report(m, v);
      g_err.clear();
    }
  }
  return P3D_OK;
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
  if (__atomic_load_n(&m->host.errw[0], __ATOMIC_ACQUIRE) || __atomic_load_n(&m->host.errw[1], __ATOMIC_ACQUIRE))
    return fail(P3D_ERR_HIP, std::string(what) + ": a kernel reported a failed in-launch synchronisation "
                                                 "(p3d_error_flags)");
  return P3D_OK;
}

// idx 8 (the *_sync calls): the word must equal the launch's own sequence number.  idx 9
// (p3d_host_signal's counter, which only advances): a count already passed has been reached too,
// compared as a wrapping difference.
static int host_wait(p3d_model* m, unsigned seq, hipStream_t st, const char* what, int idx = 8) {
  unsigned* word = reinterpret_cast<unsigned*>(m->host.errw) + idx;
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
  if (++m->host.hseq == 0) ++m->host.hseq;
  seq = m->host.hseq;
  m->host.hwait = seq;
  m->host.harmed = false;
  return P3D_OK;
}

static int host_finish(p3d_model* m, int rc, unsigned seq, hipStream_t st, const char* what) {
  const bool armed = m->host.harmed;
  m->host.hwait = 0;
  m->host.harmed = false;
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
  k_host_signal<<<1, 64, 0, (hipStream_t)stream>>>(m->host.hcnt + 8, reinterpret_cast<unsigned*>(m->host.hflag_dev) + 1);
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
