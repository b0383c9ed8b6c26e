// p3d_traj_host.h -- the host side of the root trajectory (include/p3d.h: p3d_root_trajectory; kernels
// in p3d_traj.h): the checks that answer before the GPU is touched, the solve's launch and, with a
// window, the smoothing's behind it.  Needs no model handle.  Included by p3d.hip behind
// p3d_clips_host.h (the offsets' one check: clips_check_offsets).
//
// workspace (bytes, smooth_half > 0 only): raw f64 [N, 3] (256-aligned) | valid i32 [N] -- where the
// smoothing reads the raw rows and the flags of a caller who did not ask for them.
#pragma once

extern "C" int32_t p3d_root_trajectory_rows(void) { return P3D_TRAJ_ROWS; }

extern "C" int64_t p3d_root_trajectory_workspace(int64_t N, int32_t smooth_half) {
  if (N <= 0 || N > P3D_CLIP_MAX_N || smooth_half <= 0 || smooth_half > P3D_TRAJ_MAX_HALF) return 0;
  return align256(N * 3 * (int64_t)sizeof(double)) + align256(N * (int64_t)sizeof(int32_t));
}

extern "C" int p3d_root_trajectory(const double* poses, const double* xy_s, const int32_t* src,
                                   const int64_t* clip_off_host, const int64_t* clip_off_dev, int64_t S, int64_t N,
                                   double focal, double cx, double cy, int32_t smooth_half, double* traj,
                                   double* traj_raw, double* resid, int32_t* valid, void* work, int64_t work_bytes,
                                   void* stream) {
  const std::string w("p3d_root_trajectory");
  if (!poses || !xy_s) return fail(P3D_ERR_ARG, w + ": null argument");
  if (!traj && !traj_raw && !resid && !valid) return fail(P3D_ERR_ARG, w + ": null outputs: ask for at least one");
  ClipsPlan pl;
  if (int rc = clips_check_offsets(w, clip_off_host, clip_off_dev, S, N, 0, pl)) return rc;
  if (!std::isfinite(focal) || !(focal > 0)) return fail(P3D_ERR_ARG, w + ": focal must be finite and > 0");
  if (!std::isfinite(cx) || !std::isfinite(cy)) return fail(P3D_ERR_ARG, w + ": the principal point must be finite");
  if (smooth_half < 0 || smooth_half > P3D_TRAJ_MAX_HALF)
    return fail(P3D_ERR_ARG, w + ": smooth_half must be in 0.." + std::to_string(P3D_TRAJ_MAX_HALF));
  if (smooth_half > 0) {
    if (!work || ((uintptr_t)work & 7)) return fail(P3D_ERR_ARG, w + ": null or misaligned workspace");
    if (work_bytes < p3d_root_trajectory_workspace(N, smooth_half)) return fail(P3D_ERR_ARG, w + ": workspace too small");
  }
  TrajArgs a;
  a.poses = poses; a.xy_s = xy_s; a.src = src; a.off = clip_off_dev; a.S = S; a.N = N;
  a.focal = focal; a.cx = cx; a.cy = cy; a.half = smooth_half;
  a.raw = traj_raw; a.resid = resid; a.valid = valid;
  const bool smooth = smooth_half > 0 && traj;
  a.traj = smooth ? nullptr : traj;   // no window: traj is the raw rows, written by the solve itself
  if (smooth) {
    if (!a.raw) a.raw = (double*)work;
    if (!a.valid) a.valid = (int32_t*)((char*)work + align256(N * 3 * (int64_t)sizeof(double)));
  }
  hipStream_t st = (hipStream_t)stream;
  k_traj_solve<<<dim3((unsigned)((N + P3D_TRAJ_ROWS - 1) / P3D_TRAJ_ROWS)), P3D_TRAJ_THREADS, 0, st>>>(a);
  LAUNCH_CHECK("k_traj_solve");
  if (smooth) {
    a.traj = traj;
    k_traj_smooth<<<dim3((unsigned)((N + P3D_TRAJ_THREADS - 1) / P3D_TRAJ_THREADS)), P3D_TRAJ_THREADS, 0, st>>>(a);
    LAUNCH_CHECK("k_traj_smooth");
  }
  return P3D_OK;
}
