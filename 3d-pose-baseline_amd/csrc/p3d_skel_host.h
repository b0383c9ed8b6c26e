// p3d_skel_host.h -- the host side of the rigid skeleton (include/p3d.h: p3d_skel_*; kernels in
// p3d_skel.h): the checks that answer before the GPU is touched, the lengths' two launches behind
// the clips' index kernel, and the per-frame launch.  Needs no model handle.  Included by p3d.hip
// behind p3d_clips_host.h (the chunks are the clip kernels': clips_check_offsets, clips_carve, clips_index,
// clips_max_chunks, clips_index_bytes).
//
// workspace (bytes): chunk_base i32 [S + 1] (256-aligned) | psum f64 [chunks, 16] | pcnt i64 [chunks],
// chunks the largest chunk total S clips of N frames can have.
#pragma once

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
  ClipsPlan pl;
  if (int rc = clips_check_offsets(w, clip_off_host, clip_off_dev, S, N, 0, pl)) return rc;
  if (!work || ((uintptr_t)work & 7)) return fail(P3D_ERR_ARG, w + ": null or misaligned workspace");
  if (work_bytes < p3d_skel_workspace(N, S)) return fail(P3D_ERR_ARG, w + ": workspace too small");
  char* p = clips_carve(work, clip_off_dev, S, pl.g);
  SkelLenArgs a;
  a.poses = poses; a.src = src; a.N = N;
  a.psum = (double*)p; a.pcnt = (int64_t*)(p + clips_max_chunks(N, S) * 16 * 8);
  a.lengths = lengths; a.n_used = n_used; a.nch = (int32_t)pl.nch;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = clips_index(pl.g, N, st)) return rc;
  k_skel_len_part<<<dim3(pl.nch), P3D_SKEL_THREADS, 0, st>>>(a, pl.g);
  LAUNCH_CHECK("k_skel_len_part");
  k_skel_len_fold<<<dim3((unsigned)S), P3D_SKEL_THREADS, 0, st>>>(a, pl.g);
  LAUNCH_CHECK("k_skel_len_fold");
  return P3D_OK;
}

extern "C" int p3d_skel_pose(const double* poses, const int32_t* src, const int64_t* clip_off_host,
                             const int64_t* clip_off_dev, int64_t S, int64_t N, const double* lengths, double* quat,
                             double* euler, double* rigid, double* root, void* stream) {
  const std::string w("p3d_skel_pose");
  if (!poses || !lengths) return fail(P3D_ERR_ARG, w + ": null argument");
  if (!quat && !euler && !rigid && !root) return fail(P3D_ERR_ARG, w + ": null outputs: ask for at least one");
  ClipsPlan pl;
  if (int rc = clips_check_offsets(w, clip_off_host, clip_off_dev, S, N, 0, pl)) return rc;
  SkelPoseArgs a;
  a.poses = poses; a.src = src; a.off = clip_off_dev; a.lengths = lengths; a.S = S; a.N = N;
  a.quat = quat; a.euler = euler; a.rigid = rigid; a.root = root;
  const unsigned grid = (unsigned)((N + P3D_SKEL_ROWS - 1) / P3D_SKEL_ROWS);
  k_skel_pose<<<dim3(grid), P3D_SKEL_THREADS, 0, (hipStream_t)stream>>>(a);
  LAUNCH_CHECK("k_skel_pose");
  return P3D_OK;
}
