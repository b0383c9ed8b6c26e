// p3d_spline_host.h -- the host side of the spline resampling (include/p3d.h: p3d_clips_resample*,
// p3d_clips_lift_resampled*; kernels in p3d_spline.h): the spline's own checks (R, the
// rows, the frames per clip, the LDS plan), the two launches, and the clips lift with the resampling
// between prepare and the forward.  Included by p3d.hip behind p3d_clips_host.h (the check of the
// offsets, the clips' launches, and the checked arguments and the run tail the two batched lift calls
// share) and p3d_clip_host.h (LiftLayout, the statistics).
//
// p3d_clips_resample's workspace (bytes, every area 256-aligned):
//   t f64 [36 (N + 4 S)] | c f64 [36 (N + 4 S)] | info i32 [S, 36, 5] | state f64 [36 (N + 4 S) * 24]
// curve (clip s at rows lo .., column col, m frames) keeps its m + 4 knots and coefficients at
// 36 (lo + 4 s) + col (m + 4) of t and c, and, where it is too long for LDS, its state at 24 times that.
// p3d_clips_lift_resampled's: p3d_clips_workspace(N, S) | the above | p3d_clips_workspace(R N, S) |
// LiftLayout's rows over R N.
#pragma once

namespace {

int64_t spline_coef_doubles(int64_t N, int64_t S) { return 36 * (N + 4 * S); }

struct SplineLayout {
  double *t, *c, *state;
  int32_t* info;
  int64_t total;
  SplineLayout(void* work, int64_t N, int64_t S) {
    const int64_t cb = align256(spline_coef_doubles(N, S) * 8), ib = align256(S * P3D_CLIP_COLS * P3D_SPL_INFO * 4);
    const uintptr_t p = (uintptr_t)work;
    t = (double*)p; c = (double*)(p + cb); info = (int32_t*)(p + 2 * cb); state = (double*)(p + 2 * cb + ib);
    total = 2 * cb + ib + align256(spline_coef_doubles(N, S) * 24 * 8);
  }
};

struct SplinePlan {
  size_t lds;          // the fit's dynamic LDS: the longest clip's state that fits
  int64_t max_m;
};

// what R and the clips' lengths can be refused for, beyond clips_check_offsets (which has walked the offsets)
int spline_check(const std::string& w, const int64_t* off_host, int64_t S, int64_t N, int32_t R, SplinePlan& sp) {
  if (R < 1 || R > P3D_SPL_MAX_R) return fail(P3D_ERR_ARG, w + ": R must be in 1.." + std::to_string(P3D_SPL_MAX_R));
  if ((int64_t)R * N > P3D_CLIP_MAX_N)
    return fail(P3D_ERR_ARG, w + ": R * N must be at most " + std::to_string(P3D_CLIP_MAX_N) + " rows");
  sp.lds = 0; sp.max_m = 0;
  for (int64_t s = 0; s < S; ++s) {
    const int64_t n = off_host[s + 1] - off_host[s];
    if (n < P3D_SPL_MIN_M)
      return fail(P3D_ERR_ARG, w + ": clip " + std::to_string(s) + ": need more frames, min 4 frames for a cubic spline");
    if (n > P3D_SPL_MAX_M)
      return fail(P3D_ERR_ARG, w + ": clip " + std::to_string(s) + ": at most " + std::to_string(P3D_SPL_MAX_M) +
                                   " frames per resampled clip");
    const size_t b = (size_t)SPL_STATE(n) * 8;
    if (b <= P3D_SPL_LDS_BYTES && b > sp.lds) sp.lds = b;
    if (n > sp.max_m) sp.max_m = n;
  }
  return P3D_OK;
}

int spline_run(const SplineLayout& l, const SplinePlan& sp, const double* xy_s, const int64_t* off_dev, int64_t S,
               int64_t N, int32_t R, const Stat2& s2, float* x, double* xy_r, int64_t* off_out, int32_t* info,
               hipStream_t st) {
  SplArgs a;
  a.xy_s = xy_s; a.N = N; a.R = R; a.tcoef = l.t; a.ccoef = l.c; a.state = l.state;
  a.info = info ? info : l.info;
  a.lds_doubles = (int64_t)(sp.lds / 8);
  a.xy_r = xy_r; a.off_out = off_out;
  ClipSeg g;
  g.off = off_dev; g.chunk_base = nullptr; g.S = S;
  const int64_t curves = S * P3D_CLIP_COLS;
  k_spline_fit<<<dim3((unsigned)(curves < (1 << 20) ? curves : (1 << 20))), 64, sp.lds, st>>>(a, g);
  LAUNCH_CHECK("k_spline_fit");
  const ClipInArgs in = lift_in_args(s2, (int64_t)R * N, x, nullptr);
  const int64_t chunks = ((int64_t)R * sp.max_m + P3D_SPL_ROWS - 1) / P3D_SPL_ROWS;
  k_spline_rows<<<dim3((unsigned)S, (unsigned)(chunks < 65535 ? chunks : 65535)), P3D_CLIP_THREADS, 0, st>>>(a, in, g);
  LAUNCH_CHECK("k_spline_rows");
  return P3D_OK;
}

}  // namespace

extern "C" int64_t p3d_clips_resample_workspace(int64_t N, int64_t S, int32_t R) {
  if (N <= 0 || S <= 0 || S > N || R < 1 || R > P3D_SPL_MAX_R) return 0;
  return SplineLayout(nullptr, N, S).total;
}

extern "C" int p3d_clips_resample(const double* xy_s, const int64_t* clip_off_host, const int64_t* clip_off_dev,
                                  int64_t S, int64_t N, int32_t R, const double* mean2, const double* std2,
                                  const int32_t* use2, int32_t U2, float* x, double* xy_r, int64_t* off_out_dev,
                                  int32_t* info, void* work, int64_t work_bytes, void* stream) {
  const std::string w("p3d_clips_resample");
  if (!xy_s || !mean2 || !std2 || !use2 || !x || !xy_r || !off_out_dev) return fail(P3D_ERR_ARG, w + ": null argument");
  ClipsPlan pl;
  if (int rc = clips_check_offsets(w, clip_off_host, clip_off_dev, S, N, 0, pl)) return rc;
  SplinePlan sp;
  if (int rc = spline_check(w, clip_off_host, S, N, R, sp)) return rc;
  if (U2 < 1 || U2 > 64) return fail(P3D_ERR_ARG, w + ": U2 must be in 1..64");
  if (xy_r == xy_s) return fail(P3D_ERR_ARG, w + ": xy_r must not alias xy_s");
  if (!work || ((uintptr_t)work & 7)) return fail(P3D_ERR_ARG, w + ": null or misaligned workspace");
  if (work_bytes < p3d_clips_resample_workspace(N, S, R)) return fail(P3D_ERR_ARG, w + ": workspace too small");
  return spline_run(SplineLayout(work, N, S), sp, xy_s, clip_off_dev, S, N, R, {mean2, std2, use2, U2}, x, xy_r,
                    off_out_dev, info, (hipStream_t)stream);
}

extern "C" int64_t p3d_clips_lift_resampled_workspace(int64_t N, int64_t S, int32_t R, int32_t U2, int32_t U3,
                                                      int32_t with_filter) {
  if (N <= 0 || S <= 0 || S > N || U2 <= 0 || U3 <= 0 || R < 1 || R > P3D_SPL_MAX_R) return 0;
  const int64_t head = p3d_clips_workspace(N, S) + SplineLayout(nullptr, N, S).total + p3d_clips_workspace(R * N, S);
  return LiftLayout(nullptr, head, R * N, U2, U3, with_filter != 0).total;
}

// index, prepare (xy_s, the N smoothed rows), resample (xy_r, the model's R N input rows, off_out_dev), index
// over the R N rows, then lift_batch_tail on the resampled offsets and xy_r -- p3d_clips_lift on the resampled
// clips with smooth = 0, bit for bit
extern "C" int p3d_clips_lift_resampled(p3d_model* m, p3d_vae* v, int32_t K, const float* eps, uint64_t ctr,
                                        int64_t eps_row0, const double* xy, const int64_t* clip_off_host,
                                        const int64_t* clip_off_dev, int64_t S, int64_t N, int32_t smooth,
                                        const double* mean2, const double* std2, const int32_t* use2, int32_t U2,
                                        const double* mean3, const double* std3, const int32_t* use3, int32_t U3,
                                        int32_t D3, int32_t cache_on_fail, double* xy_s, double* poses, int32_t* src,
                                        double* poses_unfiltered, int32_t* src_unfiltered, float* ref_var, int32_t R,
                                        double* xy_r, int64_t* off_out_dev, int32_t* info, void* work,
                                        int64_t work_bytes, void* stream) {
  const char* what = "p3d_clips_lift_resampled";
  const std::string w(what);
  const LiftFilter f{v, K, eps, ctr, eps_row0, poses_unfiltered, src_unfiltered, ref_var};
  if (int rc = lift_batch_check(what, m, f, !xy || !mean2 || !std2 || !use2 || !mean3 || !std3 || !use3 || !xy_s || !poses ||
                                                !xy_r || !off_out_dev,
                                U2, U3, D3, (const double*)xy_s == xy || xy_r == xy_s || (const double*)xy_r == xy
                                                ? "xy, xy_s and xy_r must not alias" : nullptr))
    return rc;
  ClipsPlan pl;
  if (int rc = clips_check(what, clip_off_host, clip_off_dev, S, N, smooth, work, work_bytes, pl)) return rc;
  SplinePlan sp;
  if (int rc = spline_check(w, clip_off_host, S, N, R, sp)) return rc;
  if ((uintptr_t)work & 255) return fail(P3D_ERR_ARG, w + ": workspace must be 256-byte aligned");
  if (work_bytes < p3d_clips_lift_resampled_workspace(N, S, R, U2, U3, v != nullptr))
    return fail(P3D_ERR_ARG, w + ": workspace too small");
  const int64_t RN = (int64_t)R * N, wb1 = p3d_clips_workspace(N, S), wb2 = p3d_clips_workspace(RN, S);
  const SplineLayout sl((char*)work + wb1, N, S);
  std::vector<int64_t> off_r((size_t)S + 1);           // the resampled clips' offsets: read at this call only
  for (int64_t s = 0; s <= S; ++s) off_r[s] = R * clip_off_host[s];
  ClipsPlan pr;
  if (int rc = clips_check(what, off_r.data(), off_out_dev, S, RN, 0, (char*)work + wb1 + sl.total, wb2, pr)) return rc;
  const LiftLayout l(work, wb1 + sl.total + wb2, RN, U2, U3, v != nullptr);
  const Stat2 s2{mean2, std2, use2, U2};
  hipStream_t st = (hipStream_t)stream;
  if (int rc = clips_index(pl.g, N, st)) return rc;
  if (int rc = clips_prepare(pl, xy, N, smooth, s2, l.x, xy_s, st)) return rc;   // (x: rewritten by the resampling)
  if (int rc = spline_run(sl, sp, xy_s, clip_off_dev, S, N, R, s2, l.x, xy_r, off_out_dev, info, st)) return rc;
  if (int rc = clips_index(pr.g, RN, st)) return rc;
  return lift_batch_tail(m, f, pr, l, off_r.data(), RN, xy_r, {mean3, std3, use3, U3, cache_on_fail}, poses, src, stream);
}
