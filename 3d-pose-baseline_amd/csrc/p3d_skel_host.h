// p3d_skel_host.h -- the host side of the rigid skeleton (include/p3d.h: p3d_skel_*; kernels in
// p3d_skel.h): the checks that answer before the GPU is touched, the lengths' two launches behind
// the clips' index kernel, and the per-frame launch.  Needs no model handle.  Included by p3d.hip
// behind p3d_clips_host.h (clips_max_chunks, clips_index_bytes: the chunks are the clip kernels').
//
// workspace (bytes): chunk_base i32 [S + 1] (256-aligned) | psum f64 [chunks, 16] | pcnt i64 [chunks],
// chunks the largest chunk total S clips of N frames can have.
#pragma once

namespace {

// what the offsets can be refused for -> the chunk total of the host offsets
int skel_check_offsets(const std::string& w, const int64_t* off_host, const int64_t* off_dev, int64_t S, int64_t N,
                       int64_t& nch) {
  if (!off_host || !off_dev) return fail(P3D_ERR_ARG, w + ": null clip offsets");
  if (N < 1 || N > P3D_CLIP_MAX_N)
    return fail(P3D_ERR_ARG, w + ": N must be in 1.." + std::to_string(P3D_CLIP_MAX_N) + " frames");
  if (S < 1 || S > N) return fail(P3D_ERR_ARG, w + ": S must be in 1..N clips");
  if (off_host[0] != 0 || off_host[S] != N) return fail(P3D_ERR_ARG, w + ": clip offsets must start at 0 and end at N");
  nch = 0;
  for (int64_t s = 0; s < S; ++s) {
    const int64_t n = off_host[s + 1] - off_host[s];
    if (n < 0) return fail(P3D_ERR_ARG, w + ": clip offsets must not decrease (clip " + std::to_string(s) + ")");
    if (n == 0) return fail(P3D_ERR_ARG, w + ": clip " + std::to_string(s) + " is empty");
    if (off_host[s + 1] > N) return fail(P3D_ERR_ARG, w + ": clip offsets must end at N");
    nch += p3d_clip_chunks(n);
  }
  return P3D_OK;
}

}  // namespace

extern "C" int32_t p3d_skel_chunk(void) { return P3D_CLIP_CHUNK; }

extern "C" int64_t p3d_skel_workspace(int64_t N, int64_t S) {
  if (N <= 0 || S <= 0 || S > N) return 0;
  return clips_index_bytes(S) + align256(clips_max_chunks(N, S) * (16 * 8 + 8));
}

extern "C" int p3d_skel_lengths(const double* poses, const int32_t* src, const int64_t* clip_off_host,
                                const int64_t* clip_off_dev, int64_t S, int64_t N, double* lengths, int64_t* n_used,
                                void* work, int64_t work_bytes, void* stream) {
  const std::string w("p3d_skel_lengths");
  if (!poses || !lengths || !n_used) return fail(P3D_ERR_ARG, w + ": null argument");
  int64_t nch = 0;
  if (int rc = skel_check_offsets(w, clip_off_host, clip_off_dev, S, N, nch)) return rc;
  if (!work || ((uintptr_t)work & 7)) return fail(P3D_ERR_ARG, w + ": null or misaligned workspace");
  if (work_bytes < p3d_skel_workspace(N, S)) return fail(P3D_ERR_ARG, w + ": workspace too small");
  char* p = (char*)work;
  const int64_t cap = clips_max_chunks(N, S);
  ClipSeg g;
  g.off = clip_off_dev; g.chunk_base = (int32_t*)p; g.S = S;
  p += clips_index_bytes(S);
  SkelLenArgs a;
  a.poses = poses; a.src = src; a.N = N;
  a.psum = (double*)p; a.pcnt = (int64_t*)(p + cap * 16 * 8);
  a.lengths = lengths; a.n_used = n_used; a.nch = (int32_t)nch;
  hipStream_t st = (hipStream_t)stream;
  k_clips_index<<<1, P3D_CLIP_THREADS, 0, st>>>(g, N);
  LAUNCH_CHECK("k_clips_index");
  k_skel_len_part<<<dim3((unsigned)nch), P3D_SKEL_THREADS, 0, st>>>(a, g);
  LAUNCH_CHECK("k_skel_len_part");
  k_skel_len_fold<<<dim3((unsigned)S), P3D_SKEL_THREADS, 0, st>>>(a, g);
  LAUNCH_CHECK("k_skel_len_fold");
  return P3D_OK;
}

extern "C" int p3d_skel_pose(const double* poses, const int32_t* src, const int64_t* clip_off_host,
                             const int64_t* clip_off_dev, int64_t S, int64_t N, const double* lengths, double* quat,
                             double* euler, double* rigid, double* root, void* stream) {
  const std::string w("p3d_skel_pose");
  if (!poses || !lengths) return fail(P3D_ERR_ARG, w + ": null argument");
  if (!quat && !euler && !rigid && !root) return fail(P3D_ERR_ARG, w + ": null outputs: ask for at least one");
  int64_t nch = 0;
  if (int rc = skel_check_offsets(w, clip_off_host, clip_off_dev, S, N, nch)) return rc;
  SkelPoseArgs a;
  a.poses = poses; a.src = src; a.off = clip_off_dev; a.lengths = lengths; a.S = S; a.N = N;
  a.quat = quat; a.euler = euler; a.rigid = rigid; a.root = root;
  const unsigned grid = (unsigned)((N + P3D_SKEL_ROWS - 1) / P3D_SKEL_ROWS);
  k_skel_pose<<<dim3(grid), P3D_SKEL_THREADS, 0, (hipStream_t)stream>>>(a);
  LAUNCH_CHECK("k_skel_pose");
  return P3D_OK;
}
