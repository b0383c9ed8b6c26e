// p3d_clip.h -- a whole OpenPose clip on the GPU (src/openpose_3dpose_sandbox.py), float64 like the
// reference's Python.  Byte-moving kernels around the model's forward:
//
//   k_clip_in        xy [N, 36] -> xy_s [N, 36] (median windows + hold of dropped joints, :140-227)
//                    and x [N, U2] float32 (joint mapping :332-342, normalize_data :348-351, the
//                    float32 placeholder cast); the [N, 64] mapped rows are never stored
//   k_clip_in_carry  the hold across chunk boundaries (second launch)
//   k_clip_out       y [N, U3] float32 + xy_s -> poses [N, 96] (unNormalizeData :359, axis swap /
//                    flip / spine offset :366-383, --cache_on_fail :389-417) and src [N]
//   k_clip_out_carry the held pose across chunk boundaries (second launch)
//
// Both holds are one scan, "take the left neighbour's result where flagged": every position's
// result is that of the nearest kept (unflagged) position at or before it.  A workgroup owns
// P3D_CLIP_CHUNK consecutive frames (k_clip_in: plus a 3-frame halo each side, staged through
// LDS) and resolves the scan inside the chunk with a wave-level inclusive max-scan over "index if
// kept, else -1" (clip_last_kept).  Per chunk and column it leaves in the workspace whether the
// chunk holds a kept position (one bit of a 64-bit mask), the carried value of its last kept
// position and the length of its unresolved prefix.  The second launch -- stream-ordered behind
// the first, so every summary is complete -- walks the masks backwards to the nearest chunk with
// the bit set (clip_lookback) and fills the unresolved prefix.  No workgroup ever waits for
// another inside a launch, and nothing depends on the order in which workgroups run: the results
// are deterministic.
//
// Rounding: every product and sum is rounded separately (no FMA contraction), in the reference's
// order, so xy_s and poses carry the reference's float64 bits and x the bits of k_normalize<true>
// on the mapped rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define P3D_CLIP_CHUNK 128        // frames per workgroup (2 per lane of the scanning wave)
#define P3D_CLIP_THREADS 256
#define P3D_CLIP_HALO 3           // the median window reaches 3 frames each way
#define P3D_CLIP_COLS 36          // 18 OpenPose joints, x / y interleaved
#define P3D_CLIP_D2 64            // the mapped H3.6M 2D row (32 joints)
#define P3D_CLIP_D3 96            // the unnormalised 3D row (32 joints)
#define P3D_CLIP_MAX_N (1 << 20)

// workspace layout (bytes, nch chunks): mask u64 [nch] | last f64 [nch, 36] | first i32 [nch, 36]
// (k_clip_out uses column 0 only, `last` holding an int32 position per chunk)
__host__ __device__ inline int64_t p3d_clip_chunks(int64_t N) { return (N + P3D_CLIP_CHUNK - 1) / P3D_CLIP_CHUNK; }

struct ClipWork {
  unsigned long long* mask;
  int32_t* first;
  double* last;
};

// ---- the scan, written once ---------------------------------------------------------------
// One wave scans one column of a chunk: lane l owns positions 2l and 2l + 1, kept0 / kept1 say
// whether they are kept.  Returns in src0 / src1 the nearest kept position at or before each (-1:
// none in this chunk), in first the number of leading positions without one (CHUNK: all) and in
// last the chunk's last kept position (-1: none).  All 64 lanes must call it.
__device__ __forceinline__ void clip_last_kept(bool kept0, bool kept1, int& src0, int& src1, int& first, int& last) {
  const int lane = threadIdx.x & 63;
  const int v0 = kept0 ? 2 * lane : -1;
  const int v1 = kept1 ? 2 * lane + 1 : v0;
  int incl = v1;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl = max(incl, o);
  }
  int excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = -1;
  src0 = max(excl, v0);
  src1 = max(excl, v1);
  last = __shfl(incl, 63, 64);
  const unsigned long long b0 = __ballot(kept0), b1 = __ballot(kept1);
  const int f0 = b0 ? 2 * (__ffsll((long long)b0) - 1) : P3D_CLIP_CHUNK;
  const int f1 = b1 ? 2 * (__ffsll((long long)b1) - 1) + 1 : P3D_CLIP_CHUNK;
  first = min(f0, f1);
}

// The carry: for every column c < ncols with need[c] != 0, the nearest chunk j in lo .. k - 1
// whose mask has bit c, into found[c] (-1: none).  (lo: 0 for the single clip; a clip's first
// chunk in a batch, p3d_clips.h.)  Whole workgroup; smask: 256 words of LDS; need / found in LDS.
// The masks were written by an earlier launch.
__device__ __forceinline__ void clip_lookback(const unsigned long long* __restrict__ mask, int k, int lo, int ncols,
                                              const int* need, int* found, unsigned long long* smask) {
  const int t = threadIdx.x;
  if (t < ncols) found[t] = need[t] ? -2 : -1;
  for (int base = k - 1; base >= lo; base -= P3D_CLIP_THREADS) {
    const int j = base - t;
    smask[t] = j >= lo ? mask[j] : 0ull;
    __syncthreads();
    int pending = 0;
    if (t < ncols && found[t] == -2) {
      for (int q = 0; q < P3D_CLIP_THREADS; ++q)
        if ((smask[q] >> t) & 1ull) { found[t] = base - q; break; }
      pending = found[t] == -2;
    }
    if (!__syncthreads_or(pending)) break;
  }
  if (t < ncols && found[t] == -2) found[t] = -1;
  __syncthreads();
}

// ---- k_clip_in ------------------------------------------------------------------------------
// np.median of the reference's sorted four-frame window (the first and last four positions), as
// the elements of middle rank under a stable order (ties by window position, -0.0 == 0.0):
// Python's sorted() is stable, and which of two zeros of different sign lands in the middle
// decides the sign of (a + b) / 2 -- which position 0 keeps.  Any NaN: NaN.
__device__ __forceinline__ double clip_median4(const double (&v)[4]) {
#pragma clang fp contract(off)
  double a = 0.0, b = 0.0;
  bool nan = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j != k) rank += (v[j] < v[k] || (v[j] == v[k] && j < k)) ? 1 : 0;
    nan = nan || (v[k] != v[k]);
    if (rank == 1) a = v[k];
    if (rank == 2) b = v[k];
  }
  if (nan) return __builtin_nan("");
  return (a + b) / 2;
}

// np.median of a seven-frame window: its fourth smallest value, by a 13-exchange selection
// network of min / max (the kernel is bound by instruction issue, not bytes, and ranking seven
// values pairwise costs ten times this).  Any NaN: NaN.  Which of several equal values comes out
// does not matter: equal non-zero values have equal bits, and a zero of either sign at a position
// past the first four is held, i.e. replaced.
__device__ __forceinline__ double clip_median7(const double (&w)[7]) {
  double v[7];
  bool nan = false;
#pragma unroll
  for (int k = 0; k < 7; ++k) { v[k] = w[k]; nan = nan || (w[k] != w[k]); }
#define P3D_CLIP_CX(i, j) { const double lo_ = fmin(v[i], v[j]), hi_ = fmax(v[i], v[j]); v[i] = lo_; v[j] = hi_; }
  P3D_CLIP_CX(0, 5) P3D_CLIP_CX(0, 3) P3D_CLIP_CX(1, 6) P3D_CLIP_CX(2, 4) P3D_CLIP_CX(0, 1) P3D_CLIP_CX(3, 5)
  P3D_CLIP_CX(2, 6) P3D_CLIP_CX(2, 3) P3D_CLIP_CX(3, 6) P3D_CLIP_CX(4, 5) P3D_CLIP_CX(1, 4) P3D_CLIP_CX(1, 3)
  P3D_CLIP_CX(3, 4)
#undef P3D_CLIP_CX
  return nan ? __builtin_nan("") : v[3];
}

struct ClipInArgs {
  const double* xy;     // [N, 36]
  int64_t N;
  int smooth;
  const double* mean2;  // [64]
  const double* std2;   // [64]
  const int32_t* use2;  // [U2]
  int U2;               // <= 64
  float* x;             // [N, U2]
  double* xy_s;         // [N, 36]
  ClipWork w;
};

// How one used dimension of the mapped H3.6M 2D row (src/openpose_3dpose_sandbox.py:332-342) is
// formed from a frame's 36 OpenPose values, per workgroup in LDS: kind 0 the copied joint (`order`
// of :25 inverted; a joint OpenPose does not give: 0), 1 the mean of two (Hip = (RHip + LHip) / 2,
// Neck/Nose = (Head + Spine) / 2), 2 Thorax = 2 Spine - Neck/Nose; -1 a dimension outside the row.
struct ClipMap {
  int kind[64], ca[64], cb[64];   // columns of the 36 (-1: the value 0)
  double mean[64], stdv[64];
};

// H3.6M joint -> OpenPose joint (order = [15, 12, 25, 26, 27, 17, 18, 19, 1, 2, 3, 6, 7, 8]; -1: none).
// The one statement of the table on the device (p3d_traj.h reads its 2D joints through it too).
__device__ __forceinline__ signed char clip_openpose_of(int h) {
  static constexpr signed char inv[32] = {-1, 8, 9, 10, -1, -1, 11, 12, 13, -1, -1, -1, 1, -1, -1, 0,
                                          -1, 5, 6, 7, -1, -1, -1, -1, -1, 2, 3, 4, -1, -1, -1, -1};
  return inv[h];
}

__device__ __forceinline__ void clip_load_map(const ClipInArgs& a, ClipMap& mp) {
  for (int u = threadIdx.x; u < a.U2; u += P3D_CLIP_THREADS) {
    const int d = a.use2[u];
    const bool ok = d >= 0 && d < P3D_CLIP_D2;
    const int h = ok ? d >> 1 : 0, k = d & 1;
    int kind = 0, ja = h, jb = -1;
    if (h == 0) { kind = 1; ja = 1; jb = 6; }                       // Hip
    else if (h == 14) { kind = 1; ja = 15; jb = 12; }               // Neck/Nose
    else if (h == 13) { kind = 2; ja = 15; jb = 12; }               // Thorax
    const int ia = clip_openpose_of(ja), ib = jb >= 0 ? clip_openpose_of(jb) : -1;
    mp.kind[u] = ok ? kind : -1;
    mp.ca[u] = ia >= 0 ? 2 * ia + k : -1;
    mp.cb[u] = ib >= 0 ? 2 * ib + k : -1;
    mp.mean[u] = ok ? a.mean2[d] : 0.0;
    mp.stdv[u] = ok ? a.std2[d] : 1.0;
  }
}

// Used dimension u of the model's input row from one smoothed row (36 values): the mapped H3.6M
// value, normalize_data, rounded to float32 (k_normalize<true>); a dimension outside the row: NaN
__device__ __forceinline__ float clip_x_value(const double* row, const ClipMap& mp, int u) {
#pragma clang fp contract(off)
  const int kind = mp.kind[u], ca = mp.ca[u], cb = mp.cb[u];
  const double va = ca >= 0 ? row[ca] : 0.0, vb = cb >= 0 ? row[cb] : 0.0;
  double e = va;
  if (kind >= 1) e = (va + vb) / 2;
  if (kind == 2) e = 2 * vb - e;
  float out = __builtin_nanf("");
  if (kind >= 0) out = (float)((e - mp.mean[u]) / mp.stdv[u]);
  return out;
}

// x rows [0, r1) of the chunk (below row `end`: the clip's) from its smoothed rows in LDS (s:
// row-major [*, 36], row 0 = the chunk's first frame): normalize_data on the mapped row, rounded
// to float32 (k_normalize<true>)
__device__ __forceinline__ void clip_write_x(const ClipInArgs& a, const double* s, int64_t c0, int r1,
                                             const ClipMap& mp, int64_t end) {
#pragma clang fp contract(off)
  const int total = r1 * a.U2;
  for (int idx = threadIdx.x; idx < total; idx += P3D_CLIP_THREADS) {
    const int i = idx / a.U2, u = idx - i * a.U2;
    if (c0 + i >= end) break;
    a.x[(c0 + i) * a.U2 + u] = clip_x_value(s + i * P3D_CLIP_COLS, mp, u);
  }
}

__global__ __launch_bounds__(P3D_CLIP_THREADS) void k_clip_in(ClipInArgs a) {
#pragma clang fp contract(off)
  constexpr int C = P3D_CLIP_CHUNK, H = P3D_CLIP_HALO, NC = P3D_CLIP_COLS, PER = C * NC / P3D_CLIP_THREADS;
  static_assert(C * NC % P3D_CLIP_THREADS == 0, "whole items per thread");
  __shared__ double s[(C + 2 * H) * NC];   // frames c0 - 3 .. c0 + C + 2; then the medians in rows 3 ..
  __shared__ ClipMap mp;
  __shared__ int shas[NC];
  const int t = threadIdx.x;
  const int64_t k = blockIdx.x, c0 = k * C, N = a.N;

  // stage the chunk and its halo (rows outside the clip: zero, never read by a window).  Every
  // load is issued before the first is waited for (addresses clamped into the clip, so the loads
  // are unconditional): a rolled loop here is one HBM round trip per trip.
  {
    constexpr int TOT = (C + 2 * H) * NC, TRIPS = (TOT + P3D_CLIP_THREADS - 1) / P3D_CLIP_THREADS;
    const int64_t g0 = (c0 - H) * NC, gmax = N * NC - 1;
    double v[TRIPS];
#pragma unroll
    for (int q = 0; q < TRIPS; ++q) {
      const int64_t g = g0 + t + q * P3D_CLIP_THREADS;
      v[q] = a.xy[min(max(g, (int64_t)0), gmax)];
    }
#pragma unroll
    for (int q = 0; q < TRIPS; ++q) {
      const int idx = t + q * P3D_CLIP_THREADS;
      const int64_t g = g0 + idx;
      if (idx < TOT) s[idx] = (g >= 0 && g <= gmax) ? v[q] : 0.0;
    }
  }
  clip_load_map(a, mp);
  __syncthreads();

  // the median of every (frame, coordinate) of the chunk, kept in registers until all windows are read
  double med[PER];
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const int idx = t + r * P3D_CLIP_THREADS;
    const int i = idx / NC, col = idx - i * NC;
    const int64_t p = c0 + i;
    const double* c = s + (i + H) * NC + col;   // this frame; c[+-q * NC]: frame p +- q
    double m = c[0];
    if (a.smooth && p < N) {
      if (p < 4) {                                // the first four positions: p .. p + 3
        const double v[4] = {c[0], c[NC], c[2 * NC], c[3 * NC]};
        m = clip_median4(v);
      } else if (p >= N - 4) {                    // the last four: p - 3 .. p
        const double v[4] = {c[0], c[-NC], c[-2 * NC], c[-3 * NC]};
        m = clip_median4(v);
      } else {
        const double v[7] = {c[0], c[NC], c[2 * NC], c[3 * NC], c[-NC], c[-2 * NC], c[-3 * NC]};
        m = clip_median7(v);
      }
    }
    med[r] = m;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < PER; ++r) s[H * NC + t + r * P3D_CLIP_THREADS] = med[r];
  __syncthreads();

  // the hold: a zero median (either sign) takes the result of the position before it; position 0
  // of the clip is never flagged.  Wave w scans columns w, w + 4, ...
  double* sm = s + H * NC;                        // [C, 36] medians, then the held values
  const int lane = t & 63, wave = t >> 6;
  for (int col = wave; col < NC; col += P3D_CLIP_THREADS / 64) {
    const int i0 = 2 * lane, i1 = i0 + 1;
    const double m0 = sm[i0 * NC + col], m1 = sm[i1 * NC + col];
    const bool in0 = c0 + i0 < N, in1 = c0 + i1 < N;
    const bool kept0 = in0 && !(a.smooth && m0 == 0.0 && c0 + i0 > 0);
    const bool kept1 = in1 && !(a.smooth && m1 == 0.0 && c0 + i1 > 0);
    int src0, src1, first, last;
    clip_last_kept(kept0, kept1, src0, src1, first, last);
    // kept positions are never written, so reading them here races with nothing
    if (in0 && !kept0 && src0 >= 0) sm[i0 * NC + col] = sm[src0 * NC + col];
    if (in1 && !kept1 && src1 >= 0) sm[i1 * NC + col] = sm[src1 * NC + col];
    if (lane == 0) {
      shas[col] = last >= 0;
      a.w.first[k * NC + col] = first;
      a.w.last[k * NC + col] = last >= 0 ? sm[last * NC + col] : 0.0;
    }
  }
  __syncthreads();
  if (t == 0) {
    unsigned long long mk = 0;
    for (int col = 0; col < NC; ++col) mk |= (unsigned long long)(shas[col] != 0) << col;
    a.w.mask[k] = mk;
  }

  // xy_s and the model's input rows (rows with an unresolved prefix are rewritten by k_clip_in_carry)
  for (int idx = t; idx < C * NC; idx += P3D_CLIP_THREADS) {
    const int64_t g = c0 * NC + idx;
    if (g < N * NC) a.xy_s[g] = sm[idx];
  }
  clip_write_x(a, sm, c0, C, mp, N);
}

// second launch, one workgroup per chunk k >= 1: the positions of the chunk's columns before
// their first kept position take the value carried from the nearest earlier chunk that has one
// (chunk 0 always has: position 0 is kept), and their x rows are formed again.
__global__ __launch_bounds__(P3D_CLIP_THREADS) void k_clip_in_carry(ClipInArgs a) {
  constexpr int C = P3D_CLIP_CHUNK, NC = P3D_CLIP_COLS;
  __shared__ double s[C * NC];
  __shared__ unsigned long long smask[P3D_CLIP_THREADS];
  __shared__ int sfirst[NC], sfound[NC];
  __shared__ ClipMap mp;
  const int t = threadIdx.x;
  const int64_t k = (int64_t)blockIdx.x + 1, c0 = k * C, N = a.N;
  int f = 0;
  if (t < NC) {
    f = a.w.first[k * NC + t];
    f = (int)min((int64_t)f, N - c0);             // (the last chunk: only frames of the clip)
    sfirst[t] = f;
  }
  __syncthreads();
  int mx = 0;
  for (int col = 0; col < NC; ++col) mx = max(mx, sfirst[col]);
  if (mx == 0) return;                             // (uniform: every column resolved in its chunk)
  clip_lookback(a.w.mask, (int)k, 0, NC, sfirst, sfound, smask);
  clip_load_map(a, mp);
  for (int idx = t; idx < mx * NC; idx += P3D_CLIP_THREADS) {
    const int i = idx / NC, col = idx - i * NC;
    double v = a.xy_s[c0 * NC + idx];
    if (i < sfirst[col] && sfound[col] >= 0) {
      v = a.w.last[(int64_t)sfound[col] * NC + col];
      a.xy_s[c0 * NC + idx] = v;
    }
    s[idx] = v;
  }
  __syncthreads();
  clip_write_x(a, s, c0, mx, mp, N);
}

// ---- k_clip_out -----------------------------------------------------------------------------
struct ClipOutArgs {
  const float* y;        // [N, U3]
  int64_t N;
  const double* xy_s;    // [N, 36]
  const double* mean3;   // [96]
  const double* std3;    // [96]
  const int32_t* use3;   // [U3]
  int U3;                // <= 96
  int cache_on_fail;
  double* poses;         // [N, 96]
  int32_t* src;          // [N] or null
  ClipWork w;
};

// unNormalizeData of dimension d of the chunk's frame i (k_unnormalize's arithmetic)
__device__ __forceinline__ double clip_unnorm(const float* sy, int U3, const int* pos, const double* smean,
                                              const double* sstd, int i, int d) {
#pragma clang fp contract(off)
  const int u = pos[d];
  const float v = u >= 0 ? sy[i * U3 + u] : 0.0f;
  return (double)v * sstd[d] + smean[d];
}

// One frame judged by 8 lanes x 4 joints (q = the lane's number among the 8; every lane of the
// wave must call it: shuffles): _max / _min over the swapped z (strict compares: a NaN never
// wins), then the frame's minimum over its 96 exported values (np.min: NaN if any is NaN).
// Frame i of the rows sy [*, U3] with the spine offsets sox[i] / soz[i]; in: the frame exists.
// good: the frame shows its own pose (--cache_on_fail: its minimum is not below -1000).
__device__ __forceinline__ void clip_frame_judge(const float* sy, int U3, const int* pos, const double* smean,
                                                 const double* sstd, int i, bool in, int q, const double* sox,
                                                 const double* soz, int cache_on_fail, double& mx_out,
                                                 double& mn_out, int& good) {
#pragma clang fp contract(off)
  double zs[4], mx = 0.0, mn = 10000.0;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int j = q * 4 + jj;
    zs[jj] = in ? clip_unnorm(sy, U3, pos, smean, sstd, i, 3 * j + 1) : 0.0;   // z' = the reference's y
    if (zs[jj] > mx) mx = zs[jj];
    if (zs[jj] < mn) mn = zs[jj];
  }
#pragma unroll
  for (int d = 1; d < 8; d <<= 1) {
    const double omx = __shfl_xor(mx, d, 64), omn = __shfl_xor(mn, d, 64);
    if (omx > mx) mx = omx;
    if (omn < mn) mn = omn;
  }
  double lo = __builtin_inf();
  int nan = 0;
  if (in) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int j = q * 4 + jj;
      const double ex = clip_unnorm(sy, U3, pos, smean, sstd, i, 3 * j) + sox[i];
      const double ey = clip_unnorm(sy, U3, pos, smean, sstd, i, 3 * j + 2);
      const double ez = ((mx - zs[jj]) + mn) + soz[i];
      nan |= (ex != ex) || (ey != ey) || (ez != ez);
      if (ex < lo) lo = ex;
      if (ey < lo) lo = ey;
      if (ez < lo) lo = ez;
    }
  }
#pragma unroll
  for (int d = 1; d < 8; d <<= 1) {
    const double olo = __shfl_xor(lo, d, 64);
    nan |= __shfl_xor(nan, d, 64);
    if (olo < lo) lo = olo;
  }
  mx_out = mx; mn_out = mn;
  good = !(cache_on_fail && !nan && lo < -1000.0);
}

// exported value d (0 .. 95) of frame sl: x + the spine offset, the swapped y, the flipped z
// (smx / smn: the frame's _max / _min)
__device__ __forceinline__ double clip_export_value(const float* sy, int U3, const int* pos, const double* smean,
                                                    const double* sstd, int sl, int d, const double* smx,
                                                    const double* smn, const double* sox, const double* soz) {
#pragma clang fp contract(off)
  const int j = d / 3, c = d - 3 * j;
  if (c == 0) return clip_unnorm(sy, U3, pos, smean, sstd, sl, d) + sox[sl];
  if (c == 1) return clip_unnorm(sy, U3, pos, smean, sstd, sl, d + 1);
  return ((smx[sl] - clip_unnorm(sy, U3, pos, smean, sstd, sl, d - 1)) + smn[sl]) + soz[sl];
}

__global__ __launch_bounds__(P3D_CLIP_THREADS) void k_clip_out(ClipOutArgs a) {
#pragma clang fp contract(off)
  constexpr int C = P3D_CLIP_CHUNK, D = P3D_CLIP_D3, NC = P3D_CLIP_COLS;
  extern __shared__ float sy[];                    // [C, U3] the network's rows of the chunk
  __shared__ double smean[D], sstd[D];
  __shared__ int pos[D];
  __shared__ double sox[C], soz[C], smx[C], smn[C]; // per frame: spine offsets, _max, _min
  __shared__ int sgood[C], ssrc[C];
  const int t = threadIdx.x, U3 = a.U3;
  const int64_t k = blockIdx.x, c0 = k * C, N = a.N;
  const int nf = (int)min((int64_t)C, N - c0);     // frames of the clip in this chunk

  const int du = t < U3 ? a.use3[t] : -1;          // (U3 <= 96: one per thread; with the other loads)
  for (int d = t; d < D; d += P3D_CLIP_THREADS) { pos[d] = -1; smean[d] = a.mean3[d]; sstd[d] = a.std3[d]; }
  {   // the chunk's rows, eight loads in flight per thread (addresses clamped: unconditional loads)
    const int total = nf * U3;
    const float* yc = a.y + c0 * U3;
    for (int base = 0; base < total; base += 8 * P3D_CLIP_THREADS) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = yc[min(base + q * P3D_CLIP_THREADS + t, total - 1)];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int idx = base + q * P3D_CLIP_THREADS + t;
        if (idx < total) sy[idx] = v[q];
      }
    }
  }
  for (int i = t; i < nf; i += P3D_CLIP_THREADS) {
    sox[i] = a.xy_s[(c0 + i) * NC + 2] - 630;      // spine_x - 630   (:382)
    soz[i] = 500 - a.xy_s[(c0 + i) * NC + 3];      // 500 - spine_y   (:383)
  }
  __syncthreads();
  if (du >= 0 && du < D) pos[du] = t;
  __syncthreads();

  // per frame, 8 lanes x 4 joints: _max / _min over the swapped z (strict compares: a NaN never
  // wins), then the frame's minimum over its 96 exported values (np.min: NaN if any is NaN)
  for (int i = t >> 3; i < C; i += P3D_CLIP_THREADS / 8) {   // (every lane runs every trip: shuffles)
    const int q = t & 7;
    const bool in = i < nf;
    double mx, mn;
    int good;
    clip_frame_judge(sy, U3, pos, smean, sstd, i, in, q, sox, soz, a.cache_on_fail, mx, mn, good);
    if (q == 0 && in) {
      smx[i] = mx; smn[i] = mn;
      sgood[i] = good;
    }
  }
  __syncthreads();

  // the hold of the last good pose: the same scan, one column, on wave 0
  if (t < 64) {
    const int i0 = 2 * t, i1 = i0 + 1;
    const bool kept0 = i0 < nf && sgood[i0], kept1 = i1 < nf && sgood[i1];
    int src0, src1, first, last;
    clip_last_kept(kept0, kept1, src0, src1, first, last);
    ssrc[i0] = src0; ssrc[i1] = src1;
    if (t == 0) {
      a.w.mask[k] = last >= 0 ? 1ull : 0ull;
      a.w.first[k * NC] = first;
      reinterpret_cast<int32_t*>(a.w.last + k * NC)[0] = (int32_t)(c0 + max(last, 0));
    }
  }
  __syncthreads();

  // the exported rows: frame i shows the pose of frame ssrc[i] of this chunk; a frame with no good
  // pose before it in the chunk is zeros in chunk 0 and k_clip_out_carry's otherwise
  for (int idx = t; idx < nf * D; idx += P3D_CLIP_THREADS) {
    const int i = idx / D, d = idx - i * D;
    const int sl = ssrc[i];
    if (sl < 0 && k > 0) continue;
    double v = 0.0;
    if (sl >= 0) {
      v = clip_export_value(sy, U3, pos, smean, sstd, sl, d, smx, smn, sox, soz);
    }
    a.poses[c0 * D + idx] = v;
  }
  if (a.src)
    for (int i = t; i < nf; i += P3D_CLIP_THREADS) {
      const int sl = ssrc[i];
      if (sl >= 0 || k == 0) a.src[c0 + i] = sl >= 0 ? (int32_t)(c0 + sl) : -1;
    }
}

// second launch, one workgroup per chunk k >= 1: the frames before the chunk's first good one
// show the last good pose of the nearest earlier chunk that has one (a good frame's row, final
// since the first launch), or zeros where there is none.
__global__ __launch_bounds__(P3D_CLIP_THREADS) void k_clip_out_carry(ClipOutArgs a) {
  constexpr int C = P3D_CLIP_CHUNK, D = P3D_CLIP_D3, NC = P3D_CLIP_COLS;
  __shared__ unsigned long long smask[P3D_CLIP_THREADS];
  __shared__ int sneed[1], sfound[1];
  const int t = threadIdx.x;
  const int64_t k = (int64_t)blockIdx.x + 1, c0 = k * C, N = a.N;
  const int first = (int)min((int64_t)a.w.first[k * NC], N - c0);
  if (first <= 0) return;                          // (uniform)
  if (t == 0) sneed[0] = 1;
  __syncthreads();
  clip_lookback(a.w.mask, (int)k, 0, 1, sneed, sfound, smask);
  const int j = sfound[0];
  const int64_t from = j >= 0 ? (int64_t)reinterpret_cast<const int32_t*>(a.w.last + (int64_t)j * NC)[0] : -1;
  for (int idx = t; idx < first * D; idx += P3D_CLIP_THREADS) {
    const int d = idx % D;
    a.poses[c0 * D + idx] = from >= 0 ? a.poses[from * D + d] : 0.0;
  }
  if (a.src)
    for (int i = t; i < first; i += P3D_CLIP_THREADS) a.src[c0 + i] = (int32_t)from;
}
