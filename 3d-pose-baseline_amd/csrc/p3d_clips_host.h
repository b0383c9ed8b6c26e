// p3d_clips_host.h -- the host side of a batch of OpenPose clips (include/p3d.h: p3d_clips_*):
// S clips stored one after another through the segmented clip kernels (p3d_clips.h), the
// eval forward tiled clip by clip, and between the forward and the post-processing the temporal
// VAE filter over the clips as its sequences.  Also what every call over clip offsets shares: the one
// check of the host offsets and the carve of the chunk index (the skeleton, p3d_skel_host.h, and the
// resampling, p3d_spline_host.h, stand on them), and the run tail of the two batched lift calls
// (p3d_clips_lift here, p3d_clips_lift_resampled in p3d_spline_host.h).  Included by p3d.hip behind
// p3d_clip_host.h (the single clip's helpers and the stage the lift calls share, the batched calls'
// checked arguments among it).
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

// everything the host offsets can be refused for (the only walk of them for validity; smooth: and
// for a clip of 2..8 frames) -> the chunk total, and whether some clip has more than one chunk
int clips_check_offsets(const std::string& w, const int64_t* off_host, const int64_t* off_dev, int64_t S, int64_t N,
                        int32_t smooth, ClipsPlan& pl) {
  if (!off_host || !off_dev) return fail(P3D_ERR_ARG, w + ": null clip offsets");
  if (N < 1 || N > P3D_CLIP_MAX_N)
    return fail(P3D_ERR_ARG, w + ": N must be in 1.." + std::to_string(P3D_CLIP_MAX_N) + " frames");
  if (S < 1 || S > N) return fail(P3D_ERR_ARG, w + ": S must be in 1..N clips");
  if (off_host[0] != 0 || off_host[S] != N)
    return fail(P3D_ERR_ARG, w + ": clip offsets must start at 0 and end at N");
  int64_t nch = 0;
  pl.multi = false;
  for (int64_t s = 0; s < S; ++s) {
    const int64_t n = off_host[s + 1] - off_host[s];
    if (n < 0) return fail(P3D_ERR_ARG, w + ": clip offsets must not decrease (clip " + std::to_string(s) + ")");
    if (n == 0) return fail(P3D_ERR_ARG, w + ": clip " + std::to_string(s) + " is empty");
    if (off_host[s + 1] > N) return fail(P3D_ERR_ARG, w + ": clip offsets must end at N");
    if (smooth && n >= 2 && n <= 8)
      return fail(P3D_ERR_ARG, w + ": clip " + std::to_string(s) + ": need more frames, min 9 frames for smoothing");
    nch += p3d_clip_chunks(n);
    pl.multi = pl.multi || n > P3D_CLIP_CHUNK;
  }
  pl.nch = (unsigned)nch;
  return P3D_OK;
}

// chunk_base at the head of a workspace -> the area behind it
char* clips_carve(void* work, const int64_t* off_dev, int64_t S, ClipSeg& g) {
  g.off = off_dev; g.chunk_base = (int32_t*)work; g.S = S;
  return (char*)work + clips_index_bytes(S);
}

// everything the offsets and the workspace can be refused for, without touching the GPU
int clips_check(const char* what, const int64_t* off_host, const int64_t* off_dev, int64_t S, int64_t N, int32_t smooth,
                void* work, int64_t work_bytes, ClipsPlan& pl) {
  const std::string w(what);
  if (int rc = clips_check_offsets(w, off_host, off_dev, S, N, smooth, pl)) return rc;
  if (!work || ((uintptr_t)work & 7)) return fail(P3D_ERR_ARG, w + ": null or misaligned workspace");
  if (work_bytes < p3d_clips_workspace(N, S)) return fail(P3D_ERR_ARG, w + ": workspace too small");
  char* p = clips_carve(work, off_dev, S, pl.g);
  const int64_t cap = clips_max_chunks(N, S);
  pl.w.mask = (unsigned long long*)p;
  pl.w.last = (double*)(p + cap * 8);
  pl.w.first = (int32_t*)(p + cap * 8 + cap * P3D_CLIP_COLS * 8);
  return P3D_OK;
}

int clips_index(const ClipSeg& g, int64_t N, hipStream_t st) {
  k_clips_index<<<1, P3D_CLIP_THREADS, 0, st>>>(g, N);
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

// ---- what the two batched lift calls share, behind lift_batch_check (p3d_clip_host.h) -----------------
// the run tail over the N rows l.x under the offsets of pl: the forward tiles starting again at every
// clip's first row, the temporal filter over the clips as its sequences (fresh state), finish on the
// refined rows and, where asked for, a second finish on the network's own rows
int lift_batch_tail(p3d_model* m, const LiftFilter& f, const ClipsPlan& pl, const LiftLayout& l, const int64_t* off_host,
                    int64_t N, const double* xy_s, const Stat3& s3, double* poses, int32_t* src, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  for (int64_t s = 0; s < pl.g.S; ++s)
    if (int rc = lift_forward(m, l.x, l.y, off_host[s], off_host[s + 1], stream)) return rc;
  if (!f.v) return clips_finish(pl, l.y, N, xy_s, s3, poses, src, st);
  if (int rc = lift_filter_run(f.v, f.K, l.y, pl.g.off, pl.g.S, N, f.eps, f.ctr, f.eps_row0, nullptr, nullptr, l.ref,
                               f.ref_var, stream))
    return rc;
  const int rc = clips_finish(pl, l.ref, N, xy_s, s3, poses, src, st);
  if (rc || !f.poses_unfiltered) return rc;
  return clips_finish(pl, l.y, N, xy_s, s3, f.poses_unfiltered, f.src_unfiltered, st);
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
  if (int rc = clips_index(pl.g, N, st)) return rc;
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
  if (int rc = clips_index(pl.g, N, st)) return rc;
  return clips_finish(pl, y, N, xy_s, {mean3, std3, use3, U3, cache_on_fail}, poses, src, st);
}

extern "C" int64_t p3d_clips_lift_workspace(int64_t N, int64_t S, int32_t U2, int32_t U3, int32_t with_filter) {
  if (N <= 0 || S <= 0 || S > N || U2 <= 0 || U3 <= 0) return 0;
  return LiftLayout(nullptr, p3d_clips_workspace(N, S), N, U2, U3, with_filter != 0).total;
}

// index, prepare, then lift_batch_tail (clip s carries p3d_clip_lift's bits on clip s alone) -- all on `stream`
extern "C" int p3d_clips_lift(p3d_model* m, p3d_vae* v, int32_t K, const float* eps, uint64_t ctr, int64_t eps_row0,
                              const double* xy, const int64_t* clip_off_host, const int64_t* clip_off_dev, int64_t S,
                              int64_t N, int32_t smooth, const double* mean2, const double* std2, const int32_t* use2,
                              int32_t U2, const double* mean3, const double* std3, const int32_t* use3, int32_t U3,
                              int32_t D3, int32_t cache_on_fail, double* xy_s, double* poses, int32_t* src,
                              double* poses_unfiltered, int32_t* src_unfiltered, float* ref_var, void* work,
                              int64_t work_bytes, void* stream) {
  const char* what = "p3d_clips_lift";
  const LiftFilter f{v, K, eps, ctr, eps_row0, poses_unfiltered, src_unfiltered, ref_var};
  if (int rc = lift_batch_check(what, m, f, !xy || !mean2 || !std2 || !use2 || !mean3 || !std3 || !use3 || !xy_s || !poses,
                                U2, U3, D3, (const double*)xy_s == xy ? "xy_s must not alias xy" : nullptr))
    return rc;
  ClipsPlan pl;
  if (int rc = clips_check(what, clip_off_host, clip_off_dev, S, N, smooth, work, work_bytes, pl)) return rc;
  const LiftLayout l(work, p3d_clips_workspace(N, S), N, U2, U3, v != nullptr);
  if (work_bytes < l.total) return fail(P3D_ERR_ARG, "p3d_clips_lift: workspace too small");
  if ((uintptr_t)work & 255) return fail(P3D_ERR_ARG, "p3d_clips_lift: workspace must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = clips_index(pl.g, N, st)) return rc;
  if (int rc = clips_prepare(pl, xy, N, smooth, {mean2, std2, use2, U2}, l.x, xy_s, st)) return rc;
  return lift_batch_tail(m, f, pl, l, clip_off_host, N, xy_s, {mean3, std3, use3, U3, cache_on_fail}, poses, src, stream);
}
