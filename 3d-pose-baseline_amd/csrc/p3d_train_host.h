// p3d_train_host.h -- the lifter's training step (include/p3d.h): p3d_mse, the backward with its
// weight-gradient forms (per layer, one launch, per gradient bucket), the gradient buckets and
// their events, p3d_train_fwd_bwd*, and the optimizers (adam_launch, p3d_adam_*, p3d_train_step).
// Host code; included by p3d.hip behind p3d_forward_host.h (forward_impl, use_xchg, xchg_site) and
// p3d_model.h (TrainCache, mark_w_stale).
#pragma once

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
  if (!m->train.have_cache) return fail(P3D_ERR_STATE, "p3d_backward: no training forward to differentiate");
  if (B != m->train.B_cached) return fail(P3D_ERR_ARG, "p3d_backward: batch differs from the training forward");
  if (B > 64 && !m->knobs.train_split)
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
  const bool opart = m->train.opart_pending && dy == m->dybuf;
  if (m->train.opart_pending && !opart)
    return fail(P3D_ERR_STATE, "p3d_backward: the last training forward deferred its output layer to "
                               "p3d_train_fwd_bwd's backward");
  m->train.opart_pending = false;
  const float* dz_cur = dy;   // gradient wrt z of the current layer l
  bool dz_pk = false;         // dy is row-major; every later dz is packed
  int dsel = 0;
  const float* dres_next = nullptr;  // block-output gradient to add when differentiating an A-layer
  // weight gradients batched into one launch after the loop -- or, with gradient-ready buckets
  // (data-parallel all-reduce overlapping the backward), one launch per bucket as soon as its
  // layers' dZ and BN-parameter gradients exist, followed by the bucket's event
  const bool multi = m->knobs.wgrad_multi && nl <= P3D_WG_MULTI;
  const bool bucketed = !m->train.gev.empty() && !c.max_norm && multi && m->train.bucket_lo.size() == m->train.gev.size();
  size_t kb = 0;                     // next bucket
  WgradMulti mw{};
  if (m->train.fuse_adam) {
    mw.adam = 1; mw.af = *m->train.fuse_adam; mw.w = m->flat[0]; mw.m = m->flat[2]; mw.v = m->flat[3]; mw.gflat = grads;
  }
  // fused single-GPU step: Adam's alpha formed once by the first backward launch, so the last
  // launch (which reads no step state) advances it -- no k_step_advance launch
  const bool fused_tail = multi && m->train.fuse_adam && m->knobs.train_split && !bucketed;
  if (fused_tail) mw.alpha_dev = m->train.alpha_dev;
  m->train.step_advanced = false;
  m->train.alpha_ready = false;
  // bucket kb's parameters are free for its optimizer once dgrad of its lowest layer (the last
  // reader of W / Wd of the bucket) is issued: its event at the top of the next iteration
  int aev_pending = -1;
  auto flush_bucket = [&](int l) -> int {   // bucket kb ends at layer l: its tiles, then its event
    if (!bucketed || kb >= m->train.bucket_lo.size() || l != m->train.bucket_lo[kb]) return P3D_OK;
    aev_pending = (int)kb;
    if (mw.n > 0) {
      ProfScope ps(m, "wgrad_bucket");
      if (mw.adam) go(ps, k_wgrad_multi, dim3(mw.begin[mw.n]), dim3(256), st, mw);
      else go(ps, k_wgrad_grad, dim3(mw.begin[mw.n]), dim3(256), st, mw);
      LAUNCH_CHECK("k_wgrad_multi (bucket)");
      mw.n = 0;
      mw.begin[0] = 0;
    }
    HIP_TRY(hipEventRecord(m->train.gev[kb], st));
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
    if (aev_pending >= 0) { HIP_TRY(hipEventRecord(m->train.aev[aev_pending], st)); aev_pending = -1; }
    const Layer& ly = m->layers[l];
    WgradArgs wa{};
    wa.X = (l == 0) ? m->train.x_cached : m->act[l - 1]; wa.ldx = c.input_size; wa.xpk = (l != 0);
    wa.dZ = dz_cur; wa.ldz = dz_pk ? ly.N : ld_dy; wa.zpk = dz_pk;
    wa.M = (int)B; wa.K = ly.K; wa.N = ly.N;
    wa.dW = grads + ly.w; wa.db = grads + ly.b;
    const bool fuse = m->train.fuse_adam != nullptr;
    // the per-layer k_wgrad of the output layer reads dy: where this layer's data-gradient launch
    // forms it (from k_out_part's partials) the weight gradient follows that launch.  (The
    // one-launch forms run after the loop, the fused step's after each data gradient anyway.)
    const bool defer_out = !fuse && !multi && opart && l == nl - 1;
    if (fuse) {
      // single-GPU train step: Adam where the gradient is formed.  W(l) is read by dgrad(l),
      // so dW + Adam(l) runs after it; the previous layer's gamma/beta (read by dgrad(l) and
      // k_bn_bwd) are updated here too, from the gradients k_bn_bwd stored.
      wa.adam = 1; wa.af = *m->train.fuse_adam;
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
    if (m->train.loss_dst && (opart ? l == nl - 2 : is_out)) {
      a.lossp = m->lossp; a.nlossp = m->nlossp; a.loss = m->train.loss_dst;
      a.loss_scale = 1.0f / (float)(B * m->layers[nl - 1].N);
    }
    if (is_out && opart) {
      a.opart = m->train.opart; a.ont = (ly.N + 15) / 16;
      a.obias = params + ly.b; a.otgt = m->train.opart_t; a.oldt = ly.N;
      a.oy = m->train.opart_y; a.oldy = ly.N;
      a.ody = m->dybuf; a.oldd = np_out;
      a.odscale = (1.0f / (float)(B * ly.N)) * 2.0f; a.olossp = m->lossp;
    }
    a.prev = 1;
    a.bn = pv.bn;
    a.z = m->z[l - 1]; a.mean = m->bmean[l - 1]; a.var = m->bvar[l - 1];
    if (pv.bn) { a.gamma = params + pv.gamma; a.beta = params + pv.beta; }
    a.eps = c.bn_eps;
    a.relu = pv.relu;
    a.keep = m->train.keep; a.seed = m->train.seed; a.ctr = m->train.ctr; a.site = pv.site; a.row_off = m->train.row_off;
    a.ctr_dev = m->train.ctr_dev;
    a.dz = m->dz[l - 1];
    if (pv.bn) { a.dgamma = grads + pv.gamma; a.dbeta = grads + pv.beta; }
    if (m->knobs.train_split) {
      if (pv.bn) a.bnpart = m->bnpart;
      // (also beside a concurrent bucket all-reduce: its kernels share CUs with the siblings,
      // which delays a sibling's start but never blocks it -- the spins are bounded regardless)
      const bool xchg = pv.bn && use_xchg(m, a.K, a.M);
      if (xchg) { a.xchg = 1; a.xs = xchg_site(m, nl + l - 1); }   // dz, dgamma, dbeta here
      const dim3 grid((a.K + 15) / 16, (a.M + 15) / 16);
      if (fused_tail && is_out) { a.alpha_out = m->train.alpha_dev; a.af = *m->train.fuse_adam; }
      if (m->train.alpha_af && is_out) {   // data-parallel step: alpha for p3d_adam_apply after the all-reduce
        a.alpha_out = m->train.alpha_dev; a.af = *m->train.alpha_af; m->train.alpha_ready = true;
      }
      {
        ProfScope ps(m, is_out ? "dgrad_out" : "dgrad_hidden");
        if (dz_pk) {
          dim3 g = grid;
          if (xchg && m->knobs.xchg_remap && grid.x % 8 == 0) { a.remap_gy = (int)grid.y; g = dim3(grid.x * grid.y); }
          // 16 waves (both BN forms, so they keep giving the same bits): 6.8 vs 7.0-7.1 us per
          // hidden dgrad (A/B, one box)
          if (m->knobs.dgrad_wk == 16) go(ps, k_dgrad<1, 16, 4, 2, true, 1>, g, dim3(1024), st, a);
          else go(ps, k_dgrad<1, 8, 8, 2, true, 1>, g, dim3(512), st, a);
        } else {
          dim3 g = grid;
          if (xchg && m->knobs.xchg_remap && grid.x % 8 == 0) { a.remap_gy = (int)grid.y; g = dim3(grid.x * grid.y); }
          if (m->knobs.dgrad_out_wk == 4) go(ps, k_dgrad<1, 4, 4, 2, false, 2>, g, dim3(256), st, a);
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
    if (fused_tail) { mw.advance = m->dstate; m->train.step_advanced = true; }   // the step's last launch
    ProfScope ps(m, "wgrad_multi");
    if (mw.adam) go(ps, k_wgrad_multi, dim3(mw.begin[mw.n]), dim3(256), st, mw);
    else go(ps, k_wgrad_grad, dim3(mw.begin[mw.n]), dim3(256), st, mw);
    LAUNCH_CHECK("k_wgrad_multi");
  }
  if (!m->train.gev.empty() && !bucketed && !c.max_norm)   // (per-layer k_wgrad form: every bucket at the end)
    for (hipEvent_t e : m->train.gev) HIP_TRY(hipEventRecord(e, st));
  if (aev_pending >= 0) { HIP_TRY(hipEventRecord(m->train.aev[aev_pending], st)); aev_pending = -1; }
  if (!bucketed)
    for (hipEvent_t e : m->train.aev) HIP_TRY(hipEventRecord(e, st));
  if (c.max_norm) {
    // G (dL/dW_eff) -> dL/dW through clip_by_norm
    k_dot_partial<<<dim3(DOT_CHUNKS, m->wtab.n), 256, 0, st>>>(grads, params, m->wtab, m->scratch);
    LAUNCH_CHECK("k_dot_partial");
    k_dot_final<<<1, 64, 0, st>>>(m->scratch, m->wtab.n, m->gw);
    LAUNCH_CHECK("k_dot_final");
    k_maxnorm_grad<<<dim3(64, m->wtab.n), 256, 0, st>>>(grads, params, m->wtab, m->wsq, m->gw);
    LAUNCH_CHECK("k_maxnorm_grad");
    for (hipEvent_t e : m->train.gev) HIP_TRY(hipEventRecord(e, st));
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
  DevMem::drop(m->train.gev);
  DevMem::drop(m->train.aev);
  m->train.bat.clear();
  m->train.bat_blocks.clear();
  m->train.bucket_lo.assign(lowest, lowest + n);
  m->train.gev.resize((size_t)n, nullptr);
  m->train.aev.resize((size_t)n, nullptr);
  for (hipEvent_t& e : m->train.gev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (hipEvent_t& e : m->train.aev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
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
    m->train.bat.push_back(t);
    m->train.bat_blocks.push_back(tiles + vch);
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
  if (m->train.gev.empty()) return fail(P3D_ERR_STATE, "p3d_stream_wait_grad: no gradient buckets (p3d_grad_buckets)");
  if (bucket < 0 || bucket >= (int32_t)m->train.gev.size()) return fail(P3D_ERR_ARG, "p3d_stream_wait_grad: bad bucket");
  HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, m->train.gev[bucket], 0));
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
  m->train.loss_dst = loss_dev;
  rc = p3d_backward(m, m->dybuf, B, stream);
  m->train.loss_dst = nullptr;
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
  m->train.dp_af = af;
  m->train.alpha_af = &m->train.dp_af;
  const int rc = p3d_train_fwd_bwd(m, x, t, B, y, keep_prob, seed, row_offset, loss_dev, stream);
  m->train.alpha_af = nullptr;
  return rc;
}

static int adam_launch(p3d_model* m, float lr_host, float lr0, float steps, float rate, hipStream_t st);

// The data-parallel step's second half (after the all-reduce of the flat gradient): TF1 Adam +
// re-pack of every weight with the alpha the backward formed, the step state advanced in the
// same launch.  Falls back to p3d_adam_step_decay's two launches when the backward formed no
// alpha (the whole-batch BN kernels, P3D_TRAIN_SPLIT=0).
extern "C" int p3d_adam_apply(p3d_model* m, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_adam_apply: null model");
  if (m->train.dp_af.decay_steps <= 0.f) return fail(P3D_ERR_STATE, "p3d_adam_apply: no p3d_train_fwd_bwd_lr before it");
  if (!m->train.alpha_ready)
    return adam_launch(m, -1.0f, m->train.dp_af.lr0, m->train.dp_af.decay_steps, m->train.dp_af.decay_rate, (hipStream_t)stream);
  m->train.alpha_ready = false;
  return adam_launch(m, -2.0f, m->train.dp_af.lr0, m->train.dp_af.decay_steps, m->train.dp_af.decay_rate, (hipStream_t)stream);
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
  if (m->train.bat.empty()) return fail(P3D_ERR_STATE, "p3d_adam_apply_bucket: no gradient buckets (p3d_grad_buckets)");
  if (bucket < 0 || bucket >= (int32_t)m->train.bat.size()) return fail(P3D_ERR_ARG, "p3d_adam_apply_bucket: bad bucket");
  if (m->train.dp_af.decay_steps <= 0.f) return fail(P3D_ERR_STATE, "p3d_adam_apply_bucket: no p3d_train_fwd_bwd_lr before it");
  if (m->cfg.max_norm) return fail(P3D_ERR_STATE, "p3d_adam_apply_bucket: max_norm models take p3d_adam_apply");
  hipStream_t st = (hipStream_t)stream;
  const bool last = bucket == (int32_t)m->train.bat.size() - 1;
  HIP_TRY(hipStreamWaitEvent(st, m->train.aev[bucket], 0));
  if (!m->train.alpha_ready) {
    if (!last) return P3D_OK;
    return adam_launch(m, -1.0f, m->train.dp_af.lr0, m->train.dp_af.decay_steps, m->train.dp_af.decay_rate, st);
  }
  m->serve.ec_dirty = true;
  AdamArgs a{};
  a.w = m->flat[0]; a.g = m->flat[1]; a.m = m->flat[2]; a.v = m->flat[3];
  a.wpk = m->wpk; a.st = m->dstate;
  a.lr_host = -2.0f; a.lr0 = m->train.dp_af.lr0; a.decay_steps = m->train.dp_af.decay_steps; a.decay_rate = m->train.dp_af.decay_rate;
  a.b1 = 0.9f; a.b2 = 0.999f; a.eps = 1e-8f;
  a.wsrc = m->knobs.w_pk;
  mark_w_stale(m, st);
  a.wblocks = m->train.bat[bucket].tile_begin[m->train.bat[bucket].nw];
  a.alpha_dev = m->train.alpha_dev;
  a.advance = last ? m->dstate : nullptr;
  if (m->train.bat_blocks[bucket] > 0) {
    ProfScope ps(m, "adam_bucket");
    go(ps, k_adam_pack, dim3(m->train.bat_blocks[bucket]), dim3(256), st, a, m->train.bat[bucket]);
    LAUNCH_CHECK("k_adam_pack (bucket)");
  }
  if (last) m->train.alpha_ready = false;
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
  if (m->cfg.max_norm || !m->knobs.train_split || !m->knobs.adam_in_wgrad) {
    int rc = p3d_train_fwd_bwd(m, x, t, B, y, keep_prob, seed, 0, loss_dev, stream);
    if (rc) return rc;
    return adam_launch(m, -1.0f, lr0, decay_steps, decay_rate, st);
  }
  AdamFuse af{};
  af.st = m->dstate; af.lr_host = -1.0f; af.lr0 = lr0; af.decay_steps = decay_steps; af.decay_rate = decay_rate;
  af.b1 = 0.9f; af.b2 = 0.999f; af.eps = 1e-8f;
  af.wsrc = m->knobs.w_pk;
  mark_w_stale(m, st);
  m->train.fuse_adam = &af;
  const int rc = p3d_train_fwd_bwd(m, x, t, B, y, keep_prob, seed, 0, loss_dev, stream);
  m->train.fuse_adam = nullptr;
  if (rc) return rc;
  if (!m->train.step_advanced) {   // (the attached form advanced it in its last launch)
    k_step_advance<<<1, 1, 0, st>>>(m->dstate, af.b1, af.b2);
    LAUNCH_CHECK("k_step_advance");
  }
  m->train.step_advanced = false;
  return P3D_OK;
}

static int adam_launch(p3d_model* m, float lr_host, float lr0, float steps, float rate, hipStream_t st) {
  m->serve.ec_dirty = true;
  AdamArgs a{};
  a.w = m->flat[0]; a.g = m->flat[1]; a.m = m->flat[2]; a.v = m->flat[3];
  a.wpk = m->wpk; a.st = m->dstate;
  a.lr_host = lr_host; a.lr0 = lr0; a.decay_steps = steps; a.decay_rate = rate;
  a.b1 = 0.9f; a.b2 = 0.999f; a.eps = 1e-8f;
  a.wsrc = m->knobs.w_pk;
  mark_w_stale(m, st);
  a.wblocks = m->at.tile_begin[m->at.nw];
  const bool pre = lr_host == -2.0f;   // alpha formed by the backward (p3d_adam_apply): advance in-launch
  if (pre) { a.alpha_dev = m->train.alpha_dev; a.advance = m->dstate; }
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
