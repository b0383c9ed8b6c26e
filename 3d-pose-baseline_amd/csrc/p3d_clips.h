// p3d_clips.h -- S OpenPose clips stored one after another (rows [N, 36], offsets [S + 1]): the
// kernels of p3d_clip.h with every position taken INSIDE ITS CLIP, on the same
// helpers (clip_median4 / clip_median7 / clip_last_kept / clip_lookback / clip_load_map /
// clip_write_x / clip_unnorm) and the same arithmetic, so every clip's rows carry the bits the
// single-clip kernels give for that clip alone.
//
//   k_clips_index      the device offsets -> chunk_base [S + 1], the prefix sum of ceil(n_s / CHUNK)
//   k_clips_in         k_clip_in per clip: windows, halo and hold bounded by the clip
//   k_clips_in_carry   the hold across chunk boundaries inside a clip
//   k_clips_out        k_clip_out per clip: the held pose never comes from another clip
//   k_clips_out_carry  the held pose across chunk boundaries inside a clip
//
// A chunk never straddles two clips: clip s owns the chunks chunk_base[s] .. chunk_base[s + 1] - 1,
// a workgroup finds its clip by binary search there (clip_where), the summaries are indexed by
// this global chunk number and the carry's look-back stops at the clip's first chunk.  As in
// p3d_clip.h no workgroup waits for another inside a launch and nothing depends on the order in
// which workgroups run.  The single-clip kernels stay their own text: routed through these
// bodies, lift_clip at 9 frames measured slower than the parent's (MEASUREMENTS.md 25).
#pragma once
#include "p3d_clip.h"

// S clips in one buffer: clip s is rows off[s] .. off[s + 1] - 1.  The device reads off clamped
// into [0, N] (and every end up to its start), so whatever it holds no access leaves the buffers.
struct ClipSeg {
  const int64_t* off;      // device [S + 1]
  int32_t* chunk_base;     // workspace [S + 1]: the clip's first chunk; [S]: the chunk total
  int64_t S;
};

__device__ __forceinline__ void clip_bounds(const ClipSeg& g, int64_t N, int64_t s, int64_t& lo, int64_t& hi) {
  lo = min(max(g.off[s], (int64_t)0), N);
  hi = min(max(g.off[s + 1], lo), N);
}

// chunk_base from the device offsets; one workgroup, thread t sums a contiguous span of clips
__global__ __launch_bounds__(P3D_CLIP_THREADS) void k_clips_index(ClipSeg g, int64_t N) {
  __shared__ int part[P3D_CLIP_THREADS];
  const int t = threadIdx.x;
  const int64_t per = (g.S + P3D_CLIP_THREADS - 1) / P3D_CLIP_THREADS;
  const int64_t s0 = min(t * per, g.S), s1 = min(s0 + per, g.S);
  int sum = 0;
  for (int64_t s = s0; s < s1; ++s) {
    int64_t lo, hi;
    clip_bounds(g, N, s, lo, hi);
    sum += (int)p3d_clip_chunks(hi - lo);
  }
  part[t] = sum;
  __syncthreads();
  if (t == 0) {   // (256 values: a serial exclusive scan)
    int run = 0;
    for (int q = 0; q < P3D_CLIP_THREADS; ++q) { const int v = part[q]; part[q] = run; run += v; }
    g.chunk_base[g.S] = run;
  }
  __syncthreads();
  int run = part[t];
  for (int64_t s = s0; s < s1; ++s) {
    int64_t lo, hi;
    clip_bounds(g, N, s, lo, hi);
    g.chunk_base[s] = run;
    run += (int)p3d_clip_chunks(hi - lo);
  }
}

// Where workgroup k works: rows [lo, hi) of its clip, its chunk's first row c0, the chunk's number
// inside the clip kc and the clip's first chunk kbase.  false (uniform): no chunk k (the device
// offsets give fewer chunks than the grid has).
struct ClipWhere {
  int64_t lo, hi, c0;
  int kc, kbase;
};

__device__ __forceinline__ bool clip_where(const ClipSeg& g, int64_t N, int64_t k, ClipWhere& w) {
  const int32_t* __restrict__ cb = g.chunk_base;
  if (k >= cb[g.S]) return false;
  int64_t l = 0, r = g.S;   // cb[l] <= k < cb[r]
  while (r - l > 1) {
    const int64_t mid = (l + r) >> 1;
    if (cb[mid] <= k) l = mid; else r = mid;
  }
  clip_bounds(g, N, l, w.lo, w.hi);
  w.kbase = cb[l];
  w.kc = (int)k - w.kbase;
  w.c0 = w.lo + (int64_t)w.kc * P3D_CLIP_CHUNK;
  return true;
}

__global__ __launch_bounds__(P3D_CLIP_THREADS) void k_clips_in(ClipInArgs a, ClipSeg sg) {
#pragma clang fp contract(off)
  constexpr int C = P3D_CLIP_CHUNK, H = P3D_CLIP_HALO, NC = P3D_CLIP_COLS, PER = C * NC / P3D_CLIP_THREADS;
  static_assert(C * NC % P3D_CLIP_THREADS == 0, "whole items per thread");
  __shared__ double s[(C + 2 * H) * NC];   // frames c0 - 3 .. c0 + C + 2; then the medians in rows 3 ..
  __shared__ ClipMap mp;
  __shared__ int shas[NC];
  const int t = threadIdx.x;
  const int64_t k = blockIdx.x;
  ClipWhere cw;
  if (!clip_where(sg, a.N, k, cw)) return;
  const int64_t c0 = cw.c0, lo = cw.lo, N = cw.hi;          // the clip: rows lo .. N - 1
  const int smooth = a.smooth && N - lo > 1;                // (a single frame passes through, :140-143)

  // stage the chunk and its halo (rows outside the clip: zero, never read by a window).  Every
  // load is issued before the first is waited for (addresses clamped into the clip, so the loads
  // are unconditional): a rolled loop here is one HBM round trip per trip.
  {
    constexpr int TOT = (C + 2 * H) * NC, TRIPS = (TOT + P3D_CLIP_THREADS - 1) / P3D_CLIP_THREADS;
    const int64_t g0 = (c0 - H) * NC, gmin = lo * NC, gmax = N * NC - 1;
    double v[TRIPS];
#pragma unroll
    for (int q = 0; q < TRIPS; ++q) {
      const int64_t g = g0 + t + q * P3D_CLIP_THREADS;
      v[q] = a.xy[min(max(g, gmin), gmax)];
    }
#pragma unroll
    for (int q = 0; q < TRIPS; ++q) {
      const int idx = t + q * P3D_CLIP_THREADS;
      const int64_t g = g0 + idx;
      if (idx < TOT) s[idx] = (g >= gmin && g <= gmax) ? v[q] : 0.0;
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
    if (smooth && p < N) {
      if (p - lo < 4) {                                // the first four positions: p .. p + 3
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
    const bool kept0 = in0 && !(smooth && m0 == 0.0 && c0 + i0 > lo);
    const bool kept1 = in1 && !(smooth && m1 == 0.0 && c0 + i1 > lo);
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

  // xy_s and the model's input rows (rows with an unresolved prefix are rewritten by k_clips_in_carry)
  for (int idx = t; idx < C * NC; idx += P3D_CLIP_THREADS) {
    const int64_t g = c0 * NC + idx;
    if (g < N * NC) a.xy_s[g] = sm[idx];
  }
  clip_write_x(a, sm, c0, C, mp, N);
}

// second launch, one workgroup per chunk (a clip's first returns at once): the positions of the chunk's columns before
// their first kept position take the value carried from the nearest earlier chunk of the clip that
// has one (its first always has: position 0 is kept), and their x rows are formed again.
__global__ __launch_bounds__(P3D_CLIP_THREADS) void k_clips_in_carry(ClipInArgs a, ClipSeg sg) {
  constexpr int C = P3D_CLIP_CHUNK, NC = P3D_CLIP_COLS;
  __shared__ double s[C * NC];
  __shared__ unsigned long long smask[P3D_CLIP_THREADS];
  __shared__ int sfirst[NC], sfound[NC];
  __shared__ ClipMap mp;
  const int t = threadIdx.x;
  const int64_t k = blockIdx.x;
  ClipWhere cw;
  if (!clip_where(sg, a.N, k, cw) || cw.kc == 0) return;   // (uniform)
  const int64_t c0 = cw.c0, N = cw.hi;
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
  clip_lookback(a.w.mask, (int)k, cw.kbase, NC, sfirst, sfound, smask);
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

// ---- k_clips_out ----------------------------------------------------------------------------
__global__ __launch_bounds__(P3D_CLIP_THREADS) void k_clips_out(ClipOutArgs a, ClipSeg sg) {
#pragma clang fp contract(off)
  constexpr int C = P3D_CLIP_CHUNK, D = P3D_CLIP_D3, NC = P3D_CLIP_COLS;
  extern __shared__ float sy[];                    // [C, U3] the network's rows of the chunk
  __shared__ double smean[D], sstd[D];
  __shared__ int pos[D];
  __shared__ double sox[C], soz[C], smx[C], smn[C]; // per frame: spine offsets, _max, _min
  __shared__ int sgood[C], ssrc[C];
  const int t = threadIdx.x, U3 = a.U3;
  const int64_t k = blockIdx.x;
  ClipWhere cw;
  if (!clip_where(sg, a.N, k, cw)) return;   // (uniform)
  const int64_t c0 = cw.c0, N = cw.hi;
  const bool head = cw.kc == 0;                    // the clip's first chunk
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
  // pose before it in the chunk is zeros in the clip's first chunk and k_clips_out_carry's otherwise
  for (int idx = t; idx < nf * D; idx += P3D_CLIP_THREADS) {
    const int i = idx / D, d = idx - i * D;
    const int sl = ssrc[i];
    if (sl < 0 && !head) continue;
    double v = 0.0;
    if (sl >= 0) {
      v = clip_export_value(sy, U3, pos, smean, sstd, sl, d, smx, smn, sox, soz);
    }
    a.poses[c0 * D + idx] = v;
  }
  if (a.src)
    for (int i = t; i < nf; i += P3D_CLIP_THREADS) {
      const int sl = ssrc[i];
      if (sl >= 0 || head) a.src[c0 + i] = sl >= 0 ? (int32_t)(c0 + sl) : -1;
    }
}

// second launch, one workgroup per chunk (as k_clips_in_carry): the frames
// before the chunk's first good one show the last good pose of the nearest earlier chunk of the
// clip that has one (a good frame's row, final since the first launch), or zeros where there is none.
__global__ __launch_bounds__(P3D_CLIP_THREADS) void k_clips_out_carry(ClipOutArgs a, ClipSeg sg) {
  constexpr int C = P3D_CLIP_CHUNK, D = P3D_CLIP_D3, NC = P3D_CLIP_COLS;
  __shared__ unsigned long long smask[P3D_CLIP_THREADS];
  __shared__ int sneed[1], sfound[1];
  const int t = threadIdx.x;
  const int64_t k = blockIdx.x;
  ClipWhere cw;
  if (!clip_where(sg, a.N, k, cw) || cw.kc == 0) return;   // (uniform)
  const int64_t c0 = cw.c0, N = cw.hi;
  const int first = (int)min((int64_t)a.w.first[k * NC], N - c0);
  if (first <= 0) return;                          // (uniform)
  if (t == 0) sneed[0] = 1;
  __syncthreads();
  clip_lookback(a.w.mask, (int)k, cw.kbase, 1, sneed, sfound, smask);
  const int j = sfound[0];
  const int64_t from = j >= 0 ? (int64_t)reinterpret_cast<const int32_t*>(a.w.last + (int64_t)j * NC)[0] : -1;
  for (int idx = t; idx < first * D; idx += P3D_CLIP_THREADS) {
    const int d = idx % D;
    a.poses[c0 * D + idx] = from >= 0 ? a.poses[from * D + d] : 0.0;
  }
  if (a.src)
    for (int i = t; i < first; i += P3D_CLIP_THREADS) a.src[c0 + i] = (int32_t)from;
}
