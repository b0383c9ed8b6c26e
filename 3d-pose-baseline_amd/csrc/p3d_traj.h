// p3d_traj.h -- the root trajectory of lifted rows (gfx950; include/p3d.h:
// p3d_root_trajectory): per frame the camera-frame translation T that puts the root-relative 3D
// joints of a `poses` row onto the 2D joints of its `xy_s` row under a pinhole camera, in closed
// form (26 equations, 3 unknowns), its reprojection residual in pixels, and a windowed mean of T
// inside the clip.  Device code only; the host side is in p3d_traj_host.h.
//
//   k_traj_solve    per frame: traj_raw [N, 3], resid [N], valid [N] (and traj where nothing is smoothed)
//   k_traj_smooth   per frame: traj [N, 3], the mean of the valid raw rows at most h frames away
//                   inside the frame's clip
//
// The 13 joints are hip, legs and arms (traj_joint); their 2D comes through the clip kernels' own
// OpenPose table (clip_openpose_of, p3d_clip.h), the hip as (RHip + LHip) / 2.  Sums over the joints
// are one fixed pairwise tree over 16 slots (traj_fold16: an xor-butterfly over a row's 16 lanes),
// the window's sum runs in ascending frame order: every order depends on positions inside the clip
// alone.  No atomics, no waiting between workgroups.  All arithmetic float64, every operation
// rounded on its own (tests/traj_oracle.py states the same operations).
#pragma once
#include "p3d_clip.h"

#define P3D_TRAJ_THREADS 256
#define P3D_TRAJ_ROWS (P3D_TRAJ_THREADS / 16)     // rows of one solve workgroup: 16 lanes per row, one per joint slot
#define P3D_TRAJ_LDS_POSE 97                      // doubles per staged poses row (96 and one of padding)
#define P3D_TRAJ_LDS_XY 37                        // doubles per staged xy_s row (36 and one of padding)
#define P3D_TRAJ_JOINTS 13
#define P3D_TRAJ_MAX_HALF 32                      // the widest window: 2 * 32 + 1 frames
#define P3D_TRAJ_DEGENERATE 1e-12                 // D below this: the 2D joints coincide

struct TrajArgs {
  const double* poses;    // [N, 96]
  const double* xy_s;     // [N, 36]
  const int32_t* src;     // [N] or null (every row its own); src[n] < 0: the row is zeros
  const int64_t* off;     // device [S + 1], read clamped into [0, N]
  int64_t S, N;
  double focal, cx, cy;
  int32_t half;           // k_traj_smooth: the window's half width (1 .. 32)
  double* traj;           // k_traj_solve: a second copy of the raw rows, or null; k_traj_smooth: the output
  double* raw;            // [N, 3]  k_traj_solve: may be null; k_traj_smooth: its input
  double* resid;          // [N] or null
  int32_t* valid;         // [N]     k_traj_solve: may be null; k_traj_smooth: its input
};

// the H3.6M joint of slot l: {0, 1, 2, 3, 6, 7, 8, 17, 18, 19, 25, 26, 27}; slots 13 .. 15: the hip (never summed)
__device__ __forceinline__ int traj_joint(int l) {
  return l < 4 ? l : l < 7 ? l + 2 : l < 10 ? l + 10 : l < P3D_TRAJ_JOINTS ? l + 15 : 0;
}

// the pairwise tree over a row's 16 slots: (((s0 + s1) + (s2 + s3)) + ...) -- every lane of the 16 gets the sum
__device__ __forceinline__ double traj_fold16(double v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) v = v + __shfl_xor(v, d, 16);
  return v;
}

// 16 rows per workgroup, staged through LDS with whole-row loads: the poses rows, and the xy_s rows
// of the same frames -- a frame that shows an earlier frame's pose (src[n] != n) fetches that
// frame's xy_s row in a second round, which a batch without held frames never enters.  Lane l of a
// row forms joint slot l's equations; the sums are traj_fold16's.  Rows past N and lanes past the
// 13 joints run the same instructions on clamped addresses and store nothing.
__global__ __launch_bounds__(P3D_TRAJ_THREADS) void k_traj_solve(TrajArgs a) {
#pragma clang fp contract(off)
  constexpr int R = P3D_TRAJ_ROWS, D = P3D_CLIP_D3, NC = P3D_CLIP_COLS, WP = P3D_TRAJ_LDS_POSE, WX = P3D_TRAJ_LDS_XY;
  constexpr int PER = R * D / P3D_TRAJ_THREADS, PERX = (R * NC + P3D_TRAJ_THREADS - 1) / P3D_TRAJ_THREADS;
  static_assert(R * D % P3D_TRAJ_THREADS == 0, "whole values per thread");
  __shared__ double spose[R * WP];
  __shared__ double sxy[R * WX];
  const int t = threadIdx.x, l = t & 15, g = t >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * R, N = a.N;
  if (r0 >= N) return;   // (uniform)
  const int64_t n = r0 + g, nc = min(n, N - 1);
  int32_t sv;
  {   // every load issued before the first is waited for (addresses clamped)
    const int64_t last = N * D - 1, lastx = N * NC - 1;
    double v[PER], w[PERX];
    sv = a.src ? a.src[nc] : (int32_t)nc;
#pragma unroll
    for (int q = 0; q < PER; ++q) v[q] = a.poses[min(r0 * D + t + q * P3D_TRAJ_THREADS, last)];
#pragma unroll
    for (int q = 0; q < PERX; ++q) w[q] = a.xy_s[min(r0 * NC + t + q * P3D_TRAJ_THREADS, lastx)];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int idx = t + q * P3D_TRAJ_THREADS;
      spose[(idx / D) * WP + idx % D] = v[q];
    }
#pragma unroll
    for (int q = 0; q < PERX; ++q) {
      const int idx = t + q * P3D_TRAJ_THREADS;
      if (idx < R * NC) sxy[(idx / NC) * WX + idx % NC] = w[q];
    }
  }
  const bool zero = sv < 0;
  const bool held = !zero && (int64_t)sv != nc;
  if (__syncthreads_or(held)) {   // (uniform) the held rows take the 2D of the frame whose pose they show
    if (held) {
      const double* from = a.xy_s + min((int64_t)sv, N - 1) * NC;
      double w[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) w[q] = from[min(l + 16 * q, NC - 1)];
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (l + 16 * q < NC) sxy[g * WX + l + 16 * q] = w[q];
    }
    __syncthreads();
  }
  const double* P = spose + g * WP;
  const double* X = sxy + g * WX;

  const bool in = l < P3D_TRAJ_JOINTS;
  const int j = traj_joint(l);
  const int oa = clip_openpose_of(j ? j : 1), ob = clip_openpose_of(j ? j : 6);   // the hip: RHip and LHip
  const double ua = X[2 * oa], va = X[2 * oa + 1], ub = X[2 * ob], vb = X[2 * ob + 1];
  const double u = j ? ua : (ua + ub) / 2, v = j ? va : (va + vb) / 2;
  const double uc = u - a.cx, vc = v - a.cy;
  const double ea = uc / a.focal, eb = vc / a.focal;
  const double x = P[3 * j] - P[0], z = P[3 * j + 1] - P[1], y = P[2] - P[3 * j + 2];
  const double p = ea * z - x, q = eb * z - y;
  const double am = traj_fold16(in ? ea : 0.0) / P3D_TRAJ_JOINTS, bm = traj_fold16(in ? eb : 0.0) / P3D_TRAJ_JOINTS;
  const double pm = traj_fold16(in ? p : 0.0) / P3D_TRAJ_JOINTS, qm = traj_fold16(in ? q : 0.0) / P3D_TRAJ_JOINTS;
  const double da = ea - am, db = eb - bm;
  const double Dn = traj_fold16(in ? da * da + db * db : 0.0);
  const double Nn = traj_fold16(in ? da * p + db * q : 0.0);
  const bool ok = !zero && !(Dn < P3D_TRAJ_DEGENERATE);   // (a NaN is not below the bound: it goes on)
  const double Tz = -Nn / Dn;
  const double Tx = pm + am * Tz, Ty = qm + bm * Tz;
  const double Zj = z + Tz;
  const double eu = a.focal * ((x + Tx) / Zj) - uc, ev = a.focal * ((y + Ty) / Zj) - vc;
  const double rs = sqrt(traj_fold16(in ? eu * eu + ev * ev : 0.0) / P3D_TRAJ_JOINTS);
  if (n >= N) return;
  if (l < 3) {
    const double T = ok ? (l == 0 ? Tx : l == 1 ? Ty : Tz) : 0.0;
    if (a.raw) a.raw[n * 3 + l] = T;
    if (a.traj) a.traj[n * 3 + l] = T;
  }
  if (l == 3 && a.resid) a.resid[n] = ok ? rs : 0.0;
  if (l == 4 && a.valid) a.valid[n] = ok ? 1 : 0;
}

// One frame per thread, 256 frames per workgroup, their raw rows and flags and `half` frames each
// side staged through LDS (addresses clamped; a staged frame outside the clip is never read).  The
// frame's clip [c0, c1): off[s] <= n < off[s + 1] over the clamped offsets (S = 1: no loads).
__global__ __launch_bounds__(P3D_TRAJ_THREADS) void k_traj_smooth(TrajArgs a) {
#pragma clang fp contract(off)
  constexpr int T = P3D_TRAJ_THREADS, SPAN = T + 2 * P3D_TRAJ_MAX_HALF, PER = (3 * SPAN + T - 1) / T, PERV = (SPAN + T - 1) / T;
  __shared__ double sraw[3 * SPAN];
  __shared__ int32_t sval[SPAN];
  const int t = threadIdx.x, h = min(max(a.half, 0), P3D_TRAJ_MAX_HALF);
  const int64_t r0 = (int64_t)blockIdx.x * T, N = a.N;
  if (r0 >= N) return;   // (uniform)
  const int64_t f0 = r0 - h;   // the first staged frame
  const int span = T + 2 * h;
  {
    double v[PER];
    int32_t w[PERV];
#pragma unroll
    for (int q = 0; q < PER; ++q) v[q] = a.raw[min(max(f0 * 3 + t + q * T, (int64_t)0), N * 3 - 1)];
#pragma unroll
    for (int q = 0; q < PERV; ++q) w[q] = a.valid[min(max(f0 + t + q * T, (int64_t)0), N - 1)];
#pragma unroll
    for (int q = 0; q < PER; ++q)
      if (t + q * T < 3 * span) sraw[t + q * T] = v[q];
#pragma unroll
    for (int q = 0; q < PERV; ++q)
      if (t + q * T < span) sval[t + q * T] = w[q];
  }
  __syncthreads();
  const int64_t n = r0 + t;
  if (n >= N) return;
  int64_t c0 = 0, c1 = N;
  if (a.S > 1) {
    int64_t s = 0;
    for (int64_t hi = a.S; hi - s > 1;) {
      const int64_t mid = (s + hi) >> 1;
      if (min(max(a.off[mid], (int64_t)0), N) <= n) s = mid; else hi = mid;
    }
    c0 = min(max(a.off[s], (int64_t)0), N);
    c1 = min(max(a.off[s + 1], (int64_t)0), N);
  }
  const int lo = (int)(max(c0, n - h) - f0), hi = (int)(min(c1 - 1, n + h) - f0);   // inside [0, span)
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int cnt = 0;
  for (int m = lo; m <= hi; ++m)
    if (sval[m]) {
      sx = sx + sraw[3 * m];
      sy = sy + sraw[3 * m + 1];
      sz = sz + sraw[3 * m + 2];
      ++cnt;
    }
  const bool ok = sval[t + h] != 0;
  const double c = (double)cnt;
  a.traj[n * 3] = ok ? sx / c : 0.0;
  a.traj[n * 3 + 1] = ok ? sy / c : 0.0;
  a.traj[n * 3 + 2] = ok ? sz / c : 0.0;
}
