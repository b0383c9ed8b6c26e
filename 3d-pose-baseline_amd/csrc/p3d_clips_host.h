// p3d_clips_host.h -- the host side of a batch of OpenPose clips (include/p3d.h: p3d_clips_*):
// S clips stored one after another through the segmented clip kernels (p3d_clips.h), the
// eval forward tiled clip by clip, and between the forward and the post-processing the temporal
// VAE filter over the clips as its sequences.  Included by p3d.hip behind p3d_clip_host.h (the single
// clip's helpers and the stage the lift calls share).
//
// workspace (bytes): chunk_base i32 [S + 1] (256-aligned) | the scan's summaries of p3d_clip_workspace
// over the largest chunk total S clips of N frames can have.  p3d_clips_lift adds LiftLayout's rows.
#pragma once

namespace {

// sum ceil(n_s / CHUNK) over S clips of n_s >= 1 frames, sum n_s = N, is at most this
int64_t clips_max_chunks(int64_t N, int64_t S) { return (N - S) / P3D_CLIP_CHUNK + S; }
int64_t clips_index_bytes(int64_t S) { return align256((S + 1) * (int64_t)sizeof(int32_t)); }

struct ClipsPlan {
  ClipSeg g;
  ClipWork w;
  unsigned nch;     // the chunk total of the host offsets: the grids
  bool multi;       // some clip has more than one chunk: the carry launches have work
};

// everything the offsets and the workspace can be refused for, without touching the GPU
int clips_check(const char* what, const int64_t* off_host, const int64_t* off_dev, int64_t S, int64_t N, int32_t smooth,
                void* work, int64_t work_bytes, ClipsPlan& pl) {
  const std::string w(what);
  if (!off_host || !off_dev) return fail(P3D_ERR_ARG, w + ": null clip offsets");
  if (N < 1 || N > P3D_CLIP_MAX_N)
    return fail(P3D_ERR_ARG, w + ": N must be in 1.." + std::to_string(P3D_CLIP_MAX_N) + " frames");
  if (S < 1 || S > N) return fail(P3D_ERR_ARG, w + ": S must be in 1..N clips");
  if (off_host[0] != 0 || off_host[S] != N)
    return fail(P3D_ERR_ARG, w + ": clip offsets must start at 0 and end at N");
  int64_t nch = 0;
  bool multi = false;
  for (int64_t s = 0; s < S; ++s) {
    const int64_t n = off_host[s + 1] - off_host[s];
    if (n < 0) return fail(P3D_ERR_ARG, w + ": clip offsets must not decrease (clip " + std::to_string(s) + ")");
    if (n == 0) return fail(P3D_ERR_ARG, w + ": clip " + std::to_string(s) + " is empty");
    if (off_host[s + 1] > N) return fail(P3D_ERR_ARG, w + ": clip offsets must end at N");
    if (smooth && n >= 2 && n <= 8)
      return fail(P3D_ERR_ARG, w + ": clip " + std::to_string(s) + ": need more frames, min 9 frames for smoothing");
    nch += p3d_clip_chunks(n);
    multi = multi || n > P3D_CLIP_CHUNK;
  }
  if (!work || ((uintptr_t)work & 7)) return fail(P3D_ERR_ARG, w + ": null or misaligned workspace");
  if (work_bytes < p3d_clips_workspace(N, S)) return fail(P3D_ERR_ARG, w + ": workspace too small");
  char* p = (char*)work;
  pl.g.off = off_dev; pl.g.chunk_base = (int32_t*)p; pl.g.S = S;
  const int64_t cap = clips_max_chunks(N, S);
  p += clips_index_bytes(S);
  pl.w.mask = (unsigned long long*)p;
  pl.w.last = (double*)(p + cap * 8);
  pl.w.first = (int32_t*)(p + cap * 8 + cap * P3D_CLIP_COLS * 8);
  pl.nch = (unsigned)nch;
  pl.multi = multi;
  return P3D_OK;
}

int clips_index(const ClipsPlan& pl, int64_t N, hipStream_t st) {
  k_clips_index<<<1, P3D_CLIP_THREADS, 0, st>>>(pl.g, N);
  LAUNCH_CHECK("k_clips_index");
  return P3D_OK;
}

int clips_prepare(const ClipsPlan& pl, const double* xy, int64_t N, int32_t smooth, const Stat2& s2, float* x,
                  double* xy_s, hipStream_t st) {
  ClipInArgs a = lift_in_args(s2, N, x, xy_s);
  a.xy = xy; a.smooth = smooth ? 1 : 0;
  a.w = pl.w;
  k_clips_in<<<dim3(pl.nch), P3D_CLIP_THREADS, 0, st>>>(a, pl.g);
  LAUNCH_CHECK("k_clips_in");
  if (a.smooth && pl.multi) {   // the hold across chunk boundaries inside a clip
    k_clips_in_carry<<<dim3(pl.nch), P3D_CLIP_THREADS, 0, st>>>(a, pl.g);
    LAUNCH_CHECK("k_clips_in_carry");
  }
  return P3D_OK;
}

int clips_finish(const ClipsPlan& pl, const float* y, int64_t N, const double* xy_s, const Stat3& s3, double* poses,
                 int32_t* src, hipStream_t st) {
  ClipOutArgs a = lift_out_args(s3, y, N, xy_s, poses, src);
  a.w = pl.w;
  const size_t lds = (size_t)P3D_CLIP_CHUNK * s3.U * sizeof(float);
  k_clips_out<<<dim3(pl.nch), P3D_CLIP_THREADS, lds, st>>>(a, pl.g);
  LAUNCH_CHECK("k_clips_out");
  if (a.cache_on_fail && pl.multi) {   // the held pose across chunk boundaries inside a clip
    k_clips_out_carry<<<dim3(pl.nch), P3D_CLIP_THREADS, 0, st>>>(a, pl.g);
    LAUNCH_CHECK("k_clips_out_carry");
  }
  return P3D_OK;
}

}  // namespace

extern "C" int64_t p3d_clips_workspace(int64_t N, int64_t S) {
  if (N <= 0 || S <= 0 || S > N) return 0;
  return clips_index_bytes(S) + align256(clips_max_chunks(N, S) * (8 + P3D_CLIP_COLS * (8 + 4)));
}

extern "C" int p3d_clips_prepare(const double* xy, const int64_t* clip_off_host, const int64_t* clip_off_dev, int64_t S,
                                 int64_t N, int32_t smooth, const double* mean2, const double* std2,
                                 const int32_t* use2, int32_t U2, float* x, double* xy_s, void* work,
                                 int64_t work_bytes, void* stream) {
  if (!xy || !mean2 || !std2 || !use2 || !x || !xy_s) return fail(P3D_ERR_ARG, "p3d_clips_prepare: null argument");
  ClipsPlan pl;
  if (int rc = clips_check("p3d_clips_prepare", clip_off_host, clip_off_dev, S, N, smooth, work, work_bytes, pl)) return rc;
  if (U2 < 1 || U2 > 64) return fail(P3D_ERR_ARG, "p3d_clips_prepare: U2 must be in 1..64");
  if ((const double*)xy_s == xy) return fail(P3D_ERR_ARG, "p3d_clips_prepare: xy_s must not alias xy");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = clips_index(pl, N, st)) return rc;
  return clips_prepare(pl, xy, N, smooth, {mean2, std2, use2, U2}, x, xy_s, st);
}

extern "C" int p3d_clips_finish(const float* y, const int64_t* clip_off_host, const int64_t* clip_off_dev, int64_t S,
                                int64_t N, const double* xy_s, const double* mean3, const double* std3,
                                const int32_t* use3, int32_t U3, int32_t D3, int32_t cache_on_fail, double* poses,
                                int32_t* src, void* work, int64_t work_bytes, void* stream) {
  if (!y || !xy_s || !mean3 || !std3 || !use3 || !poses) return fail(P3D_ERR_ARG, "p3d_clips_finish: null argument");
  ClipsPlan pl;
  if (int rc = clips_check("p3d_clips_finish", clip_off_host, clip_off_dev, S, N, 0, work, work_bytes, pl)) return rc;
  if (D3 != P3D_CLIP_D3) return fail(P3D_ERR_ARG, "p3d_clips_finish: D3 must be 96 (32 joints)");
  if (U3 < 1 || U3 > D3) return fail(P3D_ERR_ARG, "p3d_clips_finish: U3 must be in 1..96");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = clips_index(pl, N, st)) return rc;
  return clips_finish(pl, y, N, xy_s, {mean3, std3, use3, U3, cache_on_fail}, poses, src, st);
}

extern "C" int64_t p3d_clips_lift_workspace(int64_t N, int64_t S, int32_t U2, int32_t U3, int32_t with_filter) {
  if (N <= 0 || S <= 0 || S > N || U2 <= 0 || U3 <= 0) return 0;
  return LiftLayout(nullptr, p3d_clips_workspace(N, S), N, U2, U3, with_filter != 0).total;
}

// index, prepare, the forward tiles starting again at every clip's first frame (clip s carries
// p3d_clip_lift's bits on clip s alone), the temporal filter over the
// clips as its sequences (fresh state), finish on the refined rows and, where asked for, a second
// finish on the network's own rows -- all on `stream`
extern "C" int p3d_clips_lift(p3d_model* m, p3d_vae* v, int32_t K, const float* eps, uint64_t ctr, int64_t eps_row0,
                              const double* xy, const int64_t* clip_off_host, const int64_t* clip_off_dev, int64_t S,
                              int64_t N, int32_t smooth, const double* mean2, const double* std2, const int32_t* use2,
                              int32_t U2, const double* mean3, const double* std3, const int32_t* use3, int32_t U3,
                              int32_t D3, int32_t cache_on_fail, double* xy_s, double* poses, int32_t* src,
                              double* poses_unfiltered, int32_t* src_unfiltered, float* ref_var, void* work,
                              int64_t work_bytes, void* stream) {
  const char* what = "p3d_clips_lift";
  if (!m) return fail(P3D_ERR_ARG, "p3d_clips_lift: null model");
  if (!xy || !mean2 || !std2 || !use2 || !mean3 || !std3 || !use3 || !xy_s || !poses)
    return fail(P3D_ERR_ARG, "p3d_clips_lift: null argument");
  if (int rc = lift_check_model(what, m, U2, U3)) return rc;
  if (U2 < 1 || U2 > 64 || U3 < 1 || U3 > P3D_CLIP_D3) return fail(P3D_ERR_ARG, "p3d_clips_lift: U2 must be in 1..64, U3 in 1..96");
  if (D3 != P3D_CLIP_D3) return fail(P3D_ERR_ARG, "p3d_clips_lift: D3 must be 96 (32 joints)");
  if ((const double*)xy_s == xy) return fail(P3D_ERR_ARG, "p3d_clips_lift: xy_s must not alias xy");
  if (!v) {
    if (ref_var || poses_unfiltered || src_unfiltered)
      return fail(P3D_ERR_ARG, "p3d_clips_lift: ref_var and the unfiltered outputs need a filter");
  } else {
    if (int rc = lift_check_filter(what, v, U3)) return rc;
    if (K < 0 || K > P3D_VAE_MC_MAX_K)
      return fail(P3D_ERR_ARG, "p3d_clips_lift: K must be in 1 .. " + std::to_string(P3D_VAE_MC_MAX_K) + " (0: one draw)");
    if (K >= 1 && ctr == P3D_CTR_GLOBAL_STEP)
      return fail(P3D_ERR_ARG, "p3d_clips_lift: draw k uses the counter ctr + k (ctr may not be P3D_CTR_GLOBAL_STEP)");
    if (ref_var && K < 1) return fail(P3D_ERR_ARG, "p3d_clips_lift: ref_var needs K >= 1");
    if (src_unfiltered && !poses_unfiltered) return fail(P3D_ERR_ARG, "p3d_clips_lift: src_unfiltered needs poses_unfiltered");
    if (eps_row0 < 0) return fail(P3D_ERR_ARG, "p3d_clips_lift: eps_row0 must be >= 0");
    if ((uintptr_t)eps % 16 != 0 || (uintptr_t)ref_var % 16 != 0)
      return fail(P3D_ERR_ARG, "p3d_clips_lift: eps and ref_var must be 16-byte aligned");
  }
  ClipsPlan pl;
  if (int rc = clips_check(what, clip_off_host, clip_off_dev, S, N, smooth, work, work_bytes, pl)) return rc;
  const LiftLayout l(work, p3d_clips_workspace(N, S), N, U2, U3, v != nullptr);
  if (work_bytes < l.total) return fail(P3D_ERR_ARG, "p3d_clips_lift: workspace too small");
  if ((uintptr_t)work & 255) return fail(P3D_ERR_ARG, "p3d_clips_lift: workspace must be 256-byte aligned");
  const Stat3 s3{mean3, std3, use3, U3, cache_on_fail};
  hipStream_t st = (hipStream_t)stream;
  if (int rc = clips_index(pl, N, st)) return rc;
  if (int rc = clips_prepare(pl, xy, N, smooth, {mean2, std2, use2, U2}, l.x, xy_s, st)) return rc;
  for (int64_t s = 0; s < S; ++s)
    if (int rc = lift_forward(m, l.x, l.y, clip_off_host[s], clip_off_host[s + 1], stream)) return rc;
  if (!v) return clips_finish(pl, l.y, N, xy_s, s3, poses, src, st);
  if (int rc = lift_filter_run(v, K, l.y, clip_off_dev, S, N, eps, ctr, eps_row0, nullptr, nullptr, l.ref, ref_var, stream))
    return rc;
  const int rc = clips_finish(pl, l.ref, N, xy_s, s3, poses, src, st);
  if (rc || !poses_unfiltered) return rc;
  return clips_finish(pl, l.y, N, xy_s, s3, poses_unfiltered, src_unfiltered, st);
}
