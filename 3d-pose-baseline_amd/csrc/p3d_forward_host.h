// p3d_forward_host.h -- the lifter's forward dispatch (include/p3d.h: p3d_forward*): the launch
// helpers of the fp32 layers in their tilings, the BN-train split and exchange forms, the bf16
// path, the batch <= 4 k_gemv forms, forward_impl over them, and the p3d_time_layer timing hook.
// Host code; included by p3d.hip behind p3d_model.h (the model, layer_ptrs, ProfScope / go); the
// kernels are in p3d_kernels.h, p3d_gemm.h, p3d_bf16.h, p3d_gemv.h and p3d_xchg.h.
#pragma once

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
  return kind == 1 && !whole_batch && m->knobs.big_m > 0 && a.M >= m->knobs.big_m && a.N % 128 == 0 &&
         a.K % 32 == 0 &&
         a.bn != 2 && !a.z_save && a.ldy == 0;
}


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
  return m->knobs.train_xchg && gy <= P3D_XCHG_MAXR && gx * gy <= m->num_cus;
}
static XchgSite xchg_site(const p3d_model* m, int slot) {
  const int nl = (int)m->layers.size();
  const int L = m->cfg.linear_size;
  XchgSite x;
  x.epoch = m->xchg.xsync + (int64_t)slot * (L / 16) * P3D_XCHG_EPOCH_STRIDE;
  x.slots = (float*)(m->xchg.xsync + m->xchg.xslots_off) + (int64_t)slot * P3D_XCHG_MAXR * L * 4;
  x.near = x.slots + (int64_t)2 * nl * P3D_XCHG_MAXR * L * 4;
  x.err = m->host.xerr;
  x.delay = m->knobs.xchg_delay;
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
    if (m->knobs.xchg_remap && grid.x % 8 == 0) { a.remap_gy = (int)grid.y; g = dim3(grid.x * grid.y); }
    if (kind == 0 && m->knobs.in_train_wk == 2 && a.K <= 32) go(ps, k_fwd<1, 2, 1, 2, false, true, 0>, g, dim3(128), st, a);
    else if (kind == 0 && m->knobs.in_train_wk == 4 && a.K <= 64) go(ps, k_fwd<1, 4, 1, 2, false, true, 0>, g, dim3(256), st, a);
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
  if (kind == 0 && !whole_batch && m->knobs.big_m > 0 && a.M >= m->knobs.big_m && a.N % 128 == 0 && a.K == 32 &&
      a.bn != 2 && !a.z_save && a.ldy == 0 && aligned16(a.X)) {
    // input layer at large M: the 128x128-tile LDS-DMA GEMM, A DMA'd from the row-major input
    ProfScope ps(m, "fwd_in_big");
    GemmF32Args g = big_args(a);
    g.lda = a.ldx;
    go(ps, k_gemm_f32<2, 2, false>, dim3((unsigned)(((a.M + 127) / 128) * (a.N / 128))), dim3(256), st, g);
    LAUNCH_CHECK("k_gemm_f32");
    return P3D_OK;
  }
  if (kind == 0 && !whole_batch && m->knobs.big_m > 0 && a.M >= m->knobs.big_m) {
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
  int wk = whole_batch ? m->knobs.train_wk : m->knobs.infer_wk;
  if (!whole_batch && kind == 0 && m->knobs.in_wk) wk = m->knobs.in_wk;
  // training output layer (fused MSE, 12 workgroups at B = 64): the 8-deep ring (all of a wave's
  // K slice requested at once) -- 6.85 vs 7.8 us with the inference tiling (A/B on one box);
  // env P3D_OUT_TRAIN_WK overrides
  if (!whole_batch && kind == 2 && a.tgt) wk = m->knobs.out_train_wk;
  else if (!whole_batch && kind == 2 && m->knobs.out_wk) wk = m->knobs.out_wk;
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
  const int64_t slab = m->bf16.Mpad128 * c.linear_size;
  const int nl = (int)m->layers.size();
  const Layer& ly = m->layers[l];
  const LayerPtrs p = layer_ptrs(m, l);
  GemmBf16Args a{};
  a.A = l == 0 ? m->bf16.abf + (int64_t)nl * slab : m->bf16.abf + (int64_t)(l - 1) * slab;
  a.Bt = p.Bt; a.Y = m->bf16.abf + (int64_t)l * slab;
  a.M = Mp; a.N = ly.N; a.K = ly.K;
  a.epi.bias = p.bias; a.epi.inv = p.inv; a.epi.shift = p.shift;
  a.epi.relu = 1;
  const bool second = (l >= 1 && ((l - 1) % 2 == 1));
  a.res = (c.residual && second) ? m->bf16.abf + (int64_t)(l - 2) * slab : nullptr;
  const unsigned grid = (unsigned)((Mp / 128) * (ly.N / 128));
  // hidden layers: k_gemm_bf16p<64, 4, 8> (default), the unpipelined k_gemm_bf16<64, 4>
  // (P3D_BF16_STAGES=0, reference form)
  const bool bplain = m->knobs.bf16_stages == 0;
  if (l > 0) m->bf16.kname = bplain ? "k_gemm_bf16<64, 4>" : "k_gemm_bf16p<64, 4, 8, false>";
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
  const int64_t slab = m->bf16.Mpad128 * L;
  const int nl = (int)m->layers.size();
  unsigned short* xs = m->bf16.abf + (int64_t)nl * slab;
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
  const unsigned short* in = m->bf16.abf + (int64_t)(nl - 2) * slab;
  const Layer& lo = m->layers[nl - 1];
  SmallBf16Args o{};
  const LayerPtrs po = layer_ptrs(m, nl - 1);
  o.A = in; o.Bt = po.Bt; o.M = (int)B; o.N = lo.N; o.K = lo.K;
  o.bias = po.bias; o.Y = y; o.ldy = lo.N;
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
    const LayerPtrs p = layer_ptrs(m, l);
    const bool last = (l == nl - 1);
    a = GemvArgs{};
    a.X = in; a.ldx = c.input_size; a.xpk = l > 0;
    a.Wf = p.Wf; a.bias = p.bias; a.wsq = p.wsq;
    a.M = (int)B; a.K = ly.K; a.N = ly.N;
    a.gamma = p.gamma; a.beta = p.beta; a.mmean = p.mmean; a.mvar = p.mvar;
    if (ly.bn) { a.bn = 1; a.eps = c.bn_eps; }
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
  const bool fold = m->knobs.gemv_fold && m->gemv.hand && slot < m->gemv.slots && nl >= 4 && L % 16 == 0 &&
                    L <= P3D_GEMV_FOLD_MAXK && c.input_size == P3D_GEMV_FOLD_MAXIN &&
                    c.output_size <= 64;
  const int H = nl - 2, T = L / 16;
  if (fold && m->knobs.gemv_chain && H <= P3D_GEMV_CHAIN_MAXH && L <= P3D_GEMV_CHAIN_MAXK && H * T <= m->num_cus &&
      m->gemv.slot_floats >= (int64_t)(H + 1) * 4 * (L / 2) * 4) {
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
    ch.hand = m->gemv.hand + slot * m->gemv.slot_floats;
    ch.epoch = m->gemv.epoch + slot * P3D_XCHG_EPOCH_STRIDE;
    ch.err = m->host.xerr;
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
        f.hand = m->gemv.hand + slot * m->gemv.slot_floats;
        f.epoch = m->gemv.epoch + slot * P3D_XCHG_EPOCH_STRIDE;
        f.err = m->host.xerr;
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
  return m->knobs.out_part && m->knobs.train_split && B <= 256 && m->cfg.output_size <= 64 && m->layers.size() >= 3 &&
         m->knobs.dgrad_out_wk == 4;
}

static int forward_impl(p3d_model* m, const float* x, int64_t B, float* y, int32_t training, float keep_prob,
                        uint64_t seed, uint64_t ctr, int64_t row_offset, int64_t ws_row, void* stream,
                        const float* tgt) {
  if (!m || !x || !y) return fail(P3D_ERR_ARG, "p3d_forward: null argument");
  m->train.opart_pending = false;
  const p3d_cfg& c = m->cfg;
  if (B <= 0) return fail(P3D_ERR_ARG, "p3d_forward: batch must be positive");
  if (ws_row < 0 || ws_row % 16 != 0) return fail(P3D_ERR_ARG, "p3d_forward_ex: ws_row must be a multiple of 16");
  if (training && ws_row != 0) return fail(P3D_ERR_ARG, "p3d_forward_ex: training uses workspace rows from 0");
  if (ws_row + B > c.max_batch)
    return fail(P3D_ERR_ARG, "p3d_forward: batch " + std::to_string(B) + " (+ workspace row " + std::to_string(ws_row) +
                                 ") exceeds max_batch " + std::to_string(c.max_batch));
  if (training && c.batch_norm && B > 64 && !m->knobs.train_split)
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
  if (!training && !tgt && B <= m->knobs.gemv_maxb) return forward_gemv(m, x, B, y, keep_prob, seed, ctr, row_offset, ws_row, st);
  const float* in = x;
  for (int l = 0; l < nl; ++l) {
    const Layer& ly = m->layers[l];
    const LayerPtrs p = layer_ptrs(m, l);
    FwdArgs a{};
    a.X = in; a.ldx = c.input_size;
    a.Wf = p.Wf; a.bias = p.bias; a.wsq = p.wsq;
    a.M = (int)B; a.K = ly.K; a.N = ly.N;
    const bool last = (l == nl - 1);
    a.gamma = p.gamma; a.beta = p.beta; a.mmean = p.mmean; a.mvar = p.mvar;
    if (ly.bn) {
      a.bn = training ? 2 : 1;
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
      o.X = in; o.Wf = a.Wf; o.M = (int)B; o.K = ly.K; o.part = m->train.opart;
      {
        ProfScope ps(m, "fwd_out_part");
        go(ps, k_out_part<8>, dim3((unsigned)((ly.N + 15) / 16), (unsigned)((B + 15) / 16), 8u), dim3(64), st, o);
      }
      LAUNCH_CHECK("k_out_part");
      m->train.opart_pending = true;
      m->train.opart_t = tgt;
      m->train.opart_y = y;
      in = a.Y;
      continue;
    }
#ifdef P3D_DIAG_SKIP_IN   // diagnostic builds only (tools/): drop the input-layer launch
    if (!training && l == 0) { in = a.Y; continue; }
#endif
    if (training && ly.bn && m->knobs.train_split) {
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
    m->serve.ec_dirty = true;   // moving statistics updated (UPDATE_OPS)
    m->train.have_cache = true;
    m->train.x_cached = x;
    m->train.B_cached = B;
    m->train.keep = keep_prob;
    m->train.seed = seed; m->train.ctr = ctr; m->train.row_off = row_offset;
    m->train.ctr_dev = (ctr == P3D_CTR_GLOBAL_STEP) ? &m->dstate->global_step : nullptr;
  }
  return P3D_OK;
}

extern "C" int p3d_forward(p3d_model* m, const float* x, int64_t B, float* y, int32_t training,
                           float keep_prob, uint64_t seed, uint64_t ctr, int64_t row_offset, void* stream) {
  return p3d_forward_ex(m, x, B, y, training, keep_prob, seed, ctr, row_offset, 0, stream);
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
  const LayerPtrs p = layer_ptrs(m, layer);
  FwdArgs a{};
  a.X = m->act[layer - 1]; a.Wf = p.Wf; a.bias = p.bias; a.wsq = p.wsq;
  a.M = (int)B; a.K = ly.K; a.N = ly.N;
  a.gamma = p.gamma; a.beta = p.beta; a.mmean = p.mmean; a.mvar = p.mvar;
  if (ly.bn) { a.bn = 1; a.eps = c.bn_eps; }
  a.relu = 1; a.keep = 1.0f; a.site = ly.site;
  if (c.residual && ((layer - 1) % 2 == 1)) a.res = m->act[layer - 2];
  a.Y = m->act[layer];
  for (int r = 0; r < reps; ++r) {
    const int rc = launch_fwd(m, a, 1, false, (hipStream_t)stream);
    if (rc) return rc;
  }
  return P3D_OK;
}
