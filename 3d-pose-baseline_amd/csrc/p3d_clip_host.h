// p3d_clip_host.h -- the host side of a whole OpenPose clip (include/p3d.h: p3d_clip_*; kernels in
// p3d_clip.h; src/openpose_3dpose_sandbox.py:140-227, 317-417) and the stage that the three lift
// calls share (p3d_clip_lift here, p3d_clips_lift in p3d_clips_host.h, p3d_live_push in
// p3d_live_host.h): the statistics' way into the kernel arguments, the workspace layout, the model
// check, the forward tiles and the filter stage; and the checked arguments of the two batched calls
// (p3d_clips_lift, p3d_clips_lift_resampled in p3d_spline_host.h).  Included by p3d.hip behind
// p3d_vae_host.h (the filter calls) and p3d_forward_host.h (forward_impl).
#pragma once

namespace {

int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }

// ---- what the three lift calls share ---------------------------------------------------------------
// the statistics of either side as the entry points take them, built once per call
struct Stat2 { const double* mean; const double* stdv; const int32_t* use; int32_t U; };
struct Stat3 { const double* mean; const double* stdv; const int32_t* use; int32_t U; int32_t cache_on_fail; };

// the 2D / 3D half of the kernel arguments; the caller adds its own input, flags and workspace
ClipInArgs lift_in_args(const Stat2& s, int64_t N, float* x, double* xy_s) {
  ClipInArgs a{};
  a.N = N; a.mean2 = s.mean; a.std2 = s.stdv; a.use2 = s.use; a.U2 = s.U; a.x = x; a.xy_s = xy_s;
  return a;
}

ClipOutArgs lift_out_args(const Stat3& s, const float* y, int64_t N, const double* xy_s, double* poses, int32_t* src) {
  ClipOutArgs a{};
  a.y = y; a.N = N; a.xy_s = xy_s; a.mean3 = s.mean; a.std3 = s.stdv; a.use3 = s.use; a.U3 = s.U;
  a.cache_on_fail = s.cache_on_fail ? 1 : 0; a.poses = poses; a.src = src;
  return a;
}

// A lift call's workspace: the path's own `head` bytes | x [rows, U2] | y [rows, U3] | with a filter
// ref [rows, U3]; float32, each 256-aligned; `total` bytes in all (work may be null where only the
// size is asked for).  openpose_frontend.lift_layout mirrors it.
struct LiftLayout {
  float *x, *y, *ref;
  int64_t total;
  LiftLayout(void* work, int64_t head, int64_t rows, int32_t U2, int32_t U3, bool with_filter) {
    const int64_t xb = align256(rows * U2 * (int64_t)sizeof(float)), yb = align256(rows * U3 * (int64_t)sizeof(float));
    const uintptr_t p = (uintptr_t)work + head;
    x = (float*)p; y = (float*)(p + xb); ref = (float*)(p + xb + yb);
    total = head + xb + yb + (with_filter ? yb : 0);
  }
};

int lift_check_model(const char* what, const p3d_model* m, int32_t U2, int32_t U3) {
  if (m->cfg.dtype != P3D_DTYPE_F32) return fail(P3D_ERR_ARG, std::string(what) + ": float32 models only");
  if (U2 != m->cfg.input_size || U3 != m->cfg.output_size)
    return fail(P3D_ERR_ARG, std::string(what) + ": dimension sets do not match the model");
  return P3D_OK;
}

// the filter of a lift call: a sequence filter for U3 values per frame
int lift_check_filter(const char* what, const p3d_vae* v, int32_t U3) {
  const VaeSeqFault f = vae_seq_fault(v->plan, U3);
  if (f == VAE_SEQ_BONES) return fail(P3D_ERR_ARG, std::string(what) + ": a bones filter has no sequence form");
  if (f != VAE_SEQ_OK)
    return fail(P3D_ERR_ARG, std::string(what) + ": the filter must be a sequence filter with out == U3 and in == seq_len * U3");
  return P3D_OK;
}

// the two batched lift calls (p3d_clips_lift, p3d_clips_lift_resampled): the filter's arguments and the
// outputs that need one, as the entry points take them
struct LiftFilter {
  p3d_vae* v; int32_t K; const float* eps; uint64_t ctr; int64_t eps_row0;
  double* poses_unfiltered; int32_t* src_unfiltered; float* ref_var;
};

// the checked arguments: the model, the statistics, U2 / U3 / D3, the alias, the filter block.
// null_arg: one of the call's own pointers is null; alias: the call's own alias fault, null: none
int lift_batch_check(const char* what, const p3d_model* m, const LiftFilter& f, bool null_arg, int32_t U2, int32_t U3,
                     int32_t D3, const char* alias) {
  const std::string w(what);
  if (!m) return fail(P3D_ERR_ARG, w + ": null model");
  if (null_arg) return fail(P3D_ERR_ARG, w + ": null argument");
  if (int rc = lift_check_model(what, m, U2, U3)) return rc;
  if (U2 < 1 || U2 > 64 || U3 < 1 || U3 > P3D_CLIP_D3) return fail(P3D_ERR_ARG, w + ": U2 must be in 1..64, U3 in 1..96");
  if (D3 != P3D_CLIP_D3) return fail(P3D_ERR_ARG, w + ": D3 must be 96 (32 joints)");
  if (alias) return fail(P3D_ERR_ARG, w + ": " + alias);
  if (!f.v) {
    if (f.ref_var || f.poses_unfiltered || f.src_unfiltered)
      return fail(P3D_ERR_ARG, w + ": ref_var and the unfiltered outputs need a filter");
    return P3D_OK;
  }
  if (int rc = lift_check_filter(what, f.v, U3)) return rc;
  if (f.K < 0 || f.K > P3D_VAE_MC_MAX_K)
    return fail(P3D_ERR_ARG, w + ": K must be in 1 .. " + std::to_string(P3D_VAE_MC_MAX_K) + " (0: one draw)");
  if (f.K >= 1 && f.ctr == P3D_CTR_GLOBAL_STEP)
    return fail(P3D_ERR_ARG, w + ": draw k uses the counter ctr + k (ctr may not be P3D_CTR_GLOBAL_STEP)");
  if (f.ref_var && f.K < 1) return fail(P3D_ERR_ARG, w + ": ref_var needs K >= 1");
  if (f.src_unfiltered && !f.poses_unfiltered) return fail(P3D_ERR_ARG, w + ": src_unfiltered needs poses_unfiltered");
  if (f.eps_row0 < 0) return fail(P3D_ERR_ARG, w + ": eps_row0 must be >= 0");
  if ((uintptr_t)f.eps % 16 != 0 || (uintptr_t)f.ref_var % 16 != 0)
    return fail(P3D_ERR_ARG, w + ": eps and ref_var must be 16-byte aligned");
  return P3D_OK;
}

// the eval forward of rows [r0, r1) in tiles of max_batch rows (the forward_impl of p3d_lift's
// three-step form: every tile's rows carry p3d_lift's bits at that batch)
int lift_forward(p3d_model* m, const float* x, float* y, int64_t r0, int64_t r1, void* stream) {
  const p3d_cfg& c = m->cfg;
  for (int64_t r = r0; r < r1; r += c.max_batch) {
    const int64_t B = r1 - r < c.max_batch ? r1 - r : (int64_t)c.max_batch;
    if (int rc = forward_impl(m, x + r * c.input_size, B, y + r * c.output_size, 0, 1.0f, 0, 0, 0, 0, stream, nullptr))
      return rc;
  }
  return P3D_OK;
}

// the temporal filter over S sequences of y into ref: the mean of K draws, K = 0: one draw
int lift_filter_run(p3d_vae* v, int32_t K, const float* y, const int64_t* seq_off, int64_t S, int64_t N, const float* eps,
                    uint64_t ctr, int64_t eps_row0, float* state, int32_t* started, float* ref, float* ref_var,
                    void* stream) {
  return K >= 1 ? p3d_vae_seq_filter_mc(v, y, seq_off, S, N, K, eps, ctr, eps_row0, nullptr, state, started, ref, ref_var,
                                        nullptr, nullptr, stream)
                : p3d_vae_seq_filter(v, y, seq_off, S, N, eps, ctr, eps_row0, nullptr, state, started, ref, nullptr,
                                     nullptr, stream);
}

// ---- the single clip -------------------------------------------------------------------------------
ClipWork clip_work(void* work, int64_t N) {
  const int64_t nch = p3d_clip_chunks(N);
  char* p = (char*)work;
  ClipWork w;
  w.mask = (unsigned long long*)p;
  w.last = (double*)(p + nch * 8);
  w.first = (int32_t*)(p + nch * 8 + nch * P3D_CLIP_COLS * 8);
  return w;
}

int clip_check_n(const char* what, int64_t N, int32_t smooth, void* work, int64_t work_bytes) {
  if (N < 1 || N > P3D_CLIP_MAX_N)
    return fail(P3D_ERR_ARG, std::string(what) + ": N must be in 1.." + std::to_string(P3D_CLIP_MAX_N) + " frames");
  if (smooth && N >= 2 && N <= 8)
    return fail(P3D_ERR_ARG, std::string(what) + ": need more frames, min 9 frames for smoothing");
  if (!work || ((uintptr_t)work & 7)) return fail(P3D_ERR_ARG, std::string(what) + ": null or misaligned workspace");
  if (work_bytes < p3d_clip_workspace(N)) return fail(P3D_ERR_ARG, std::string(what) + ": workspace too small");
  return P3D_OK;
}

}  // namespace

extern "C" int32_t p3d_clip_chunk(void) { return P3D_CLIP_CHUNK; }

extern "C" int64_t p3d_clip_workspace(int64_t N) {
  if (N <= 0) return 0;
  return align256(p3d_clip_chunks(N) * (8 + P3D_CLIP_COLS * (8 + 4)));
}

extern "C" int p3d_clip_prepare(const double* xy, int64_t N, int32_t smooth, const double* mean2, const double* std2,
                                const int32_t* use2, int32_t U2, float* x, double* xy_s, void* work,
                                int64_t work_bytes, void* stream) {
  if (!xy || !mean2 || !std2 || !use2 || !x || !xy_s) return fail(P3D_ERR_ARG, "p3d_clip_prepare: null argument");
  if (int rc = clip_check_n("p3d_clip_prepare", N, smooth, work, work_bytes)) return rc;
  if (U2 < 1 || U2 > 64) return fail(P3D_ERR_ARG, "p3d_clip_prepare: U2 must be in 1..64");
  if ((const double*)xy_s == xy) return fail(P3D_ERR_ARG, "p3d_clip_prepare: xy_s must not alias xy");
  ClipInArgs a = lift_in_args({mean2, std2, use2, U2}, N, x, xy_s);
  a.xy = xy; a.smooth = (smooth && N > 1) ? 1 : 0;   // (a single frame passes through, :140-143)
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
  ClipOutArgs a = lift_out_args({mean3, std3, use3, U3, cache_on_fail}, y, N, xy_s, poses, src);
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
  return LiftLayout(nullptr, p3d_clip_workspace(N), N, U2, U3, false).total;
}

// prepare, the forward tiles, finish -- all on `stream`
extern "C" int p3d_clip_lift(p3d_model* m, const double* xy, int64_t N, int32_t smooth, const double* mean2,
                             const double* std2, const int32_t* use2, int32_t U2, const double* mean3,
                             const double* std3, const int32_t* use3, int32_t U3, int32_t D3, int32_t cache_on_fail,
                             double* xy_s, double* poses, int32_t* src, void* work, int64_t work_bytes, void* stream) {
  if (!m) return fail(P3D_ERR_ARG, "p3d_clip_lift: null model");
  if (int rc = lift_check_model("p3d_clip_lift", m, U2, U3)) return rc;
  if (int rc = clip_check_n("p3d_clip_lift", N, smooth, work, work_bytes)) return rc;
  const int64_t wb = p3d_clip_workspace(N);
  const LiftLayout l(work, wb, N, U2, U3, false);
  if (work_bytes < l.total) return fail(P3D_ERR_ARG, "p3d_clip_lift: workspace too small");
  if ((uintptr_t)work & 255) return fail(P3D_ERR_ARG, "p3d_clip_lift: workspace must be 256-byte aligned");
  if (int rc = p3d_clip_prepare(xy, N, smooth, mean2, std2, use2, U2, l.x, xy_s, work, wb, stream)) return rc;
  if (int rc = lift_forward(m, l.x, l.y, 0, N, stream)) return rc;
  return p3d_clip_finish(l.y, N, xy_s, mean3, std3, use3, U3, D3, cache_on_fail, poses, src, work, wb, stream);
}
