// p3d_live.h -- S live OpenPose streams lifted frame by frame with carried state:
// the clip pipeline of p3d_clip.h as recurrences.  float64 with p3d_clip.h's rounding (every
// product and sum rounded on its own, no FMA contraction) and ITS device helpers -- clip_median4 /
// clip_median7, ClipMap / clip_load_map / clip_x_value, clip_unnorm / clip_frame_judge /
// clip_export_value -- so that a stream's rows, concatenated over its ticks, carry the bits of the
// clip kernels on the stream's whole frame list.
//
//   k_live_in    appends the tick's pushed frames to the slots' rings of raw frames; per row of the
//                tick (p3d_live_plan.h) the window median from the ring, the hold of dropped joints
//                from the slot's last smoothed row, xy_s and the model's float32 row x
//   k_live_out   per row: un-normalise, swap, flip, spine offset from that row's xy_s; a failing row
//                (--cache_on_fail) shows the slot's last good pose and its position, a good one
//                becomes it
//
// One wave owns one slot and walks the slot's rows of the tick in order: the slot's state is read
// and written by that wave alone, a lane reading back only what it wrote itself.  No workgroup
// waits for another and nothing depends on the dispatch order; ticks are ordered by
// the HIP stream.  The tick's table is read from the caller's pinned host memory, every offset
// clamped where it is read and every ring index masked, so whatever the table holds no access
// leaves the buffers.
#pragma once
#include "p3d_clip.h"
#include "p3d_live_plan.h"

#define P3D_LIVE_RING 16         // raw frames kept per slot (a middle row at n frames reads n-8 .. n-2,
                                 // the head rows at n = 9 read 0 .. 7): a power of two >= 9
#define P3D_LIVE_WAVES 4         // slots per workgroup
#define P3D_LIVE_MAX_S (1 << 16)

// per-slot state in device memory: ring f64 [S, RING, 36] | last f64 [S, 36] (the last smoothed
// row) | good f64 [S, 96] (the last good pose) | good_pos i32 [S] (its frame, -1: none)
struct LiveState {
  double* ring;
  double* last;
  double* good;
  int32_t* good_pos;
};

__host__ __device__ inline LiveState live_state(void* state, int64_t S) {
  LiveState st;
  st.ring = (double*)state;
  st.last = st.ring + S * P3D_LIVE_RING * P3D_CLIP_COLS;
  st.good = st.last + S * P3D_CLIP_COLS;
  st.good_pos = (int32_t*)(st.good + S * P3D_CLIP_D3);
  return st;
}

// the tick's table (pinned host memory the device reads)
struct LiveTick {
  const int64_t* off;          // [S + 1] slot s owns rows off[s] .. off[s + 1] - 1
  const int32_t* frame;        // [N] the row's stream-local frame
  const int32_t* kind;         // [N] P3D_LIVE_KIND_*
  int64_t S, N;
};

__device__ __forceinline__ void live_rows(const LiveTick& t, int64_t s, int64_t& lo, int64_t& hi) {
  lo = min(max(t.off[s], (int64_t)0), t.N);
  hi = min(max(t.off[s + 1], lo), t.N);
}

// what one lane stored to LDS, visible to the other lanes of its wave
__device__ __forceinline__ void live_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct LiveInArgs {
  ClipInArgs c;                // mean2, std2, use2, U2; x [N, U2]; xy_s [N, 36]
  const double* xy;            // [S, 36] row s: the frame pushed to slot s in this tick
  const int32_t* push_frame;   // [S] its stream-local number, -1: none
  LiveTick t;
  LiveState st;
};

__global__ __launch_bounds__(P3D_LIVE_WAVES * 64) void k_live_in(LiveInArgs a) {
#pragma clang fp contract(off)
  constexpr int NC = P3D_CLIP_COLS, R = P3D_LIVE_RING;
  static_assert(P3D_LIVE_WAVES * 64 == P3D_CLIP_THREADS, "clip_load_map strides by P3D_CLIP_THREADS");
  static_assert((R & (R - 1)) == 0 && R >= P3D_LIVE_MIN_FRAMES, "ring indices are masked");
  __shared__ ClipMap mp;
  __shared__ double srow[P3D_LIVE_WAVES][NC];    // the wave's smoothed row, for the mapping
  clip_load_map(a.c, mp);
  __syncthreads();                                // (the only workgroup barrier: before any wave leaves)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * P3D_LIVE_WAVES + wave;
  if (s >= a.t.S) return;
  const bool col = lane < NC;
  double* ring = a.st.ring + s * R * NC + (col ? lane : 0);   // this lane's column of the slot's ring
  const int pf = a.push_frame[s];
  if (pf >= 0 && col) ring[(pf & (R - 1)) * NC] = a.xy[s * NC + lane];
  double prev = col ? a.st.last[s * NC + lane] : 0.0;
  int64_t lo, hi;
  live_rows(a.t, s, lo, hi);
  for (int64_t r = lo; r < hi; ++r) {
    const int f = a.t.frame[r], kind = a.t.kind[r];
    if (col) {
      const auto at = [&](int g) { return ring[(g & (R - 1)) * NC]; };
      double m = at(f);
      if (kind == P3D_LIVE_KIND_HEAD) {
        const double v[4] = {at(f), at(f + 1), at(f + 2), at(f + 3)};
        m = clip_median4(v);
      } else if (kind == P3D_LIVE_KIND_TAIL) {
        const double v[4] = {at(f), at(f - 1), at(f - 2), at(f - 3)};
        m = clip_median4(v);
      } else if (kind == P3D_LIVE_KIND_MIDDLE) {
        const double v[7] = {at(f), at(f + 1), at(f + 2), at(f + 3), at(f - 1), at(f - 2), at(f - 3)};
        m = clip_median7(v);
      }
      // the hold: a zero median (either sign) takes the stream's previous smoothed value; frame 0 never
      if (kind != P3D_LIVE_KIND_NONE && m == 0.0 && f > 0) m = prev;
      prev = m;
      a.c.xy_s[r * NC + lane] = m;
      srow[wave][lane] = m;
    }
    live_wave_sync();
    for (int u = lane; u < a.c.U2; u += 64) a.c.x[r * a.c.U2 + u] = clip_x_value(srow[wave], mp, u);
    live_wave_sync();                             // (the next row overwrites srow)
  }
  if (col && hi > lo) a.st.last[s * NC + lane] = prev;
}

struct LiveOutArgs {
  ClipOutArgs c;               // y [N, U3]; xy_s [N, 36]; mean3, std3, use3, U3; cache_on_fail; poses; src
  LiveTick t;
  LiveState st;
};

__global__ __launch_bounds__(P3D_LIVE_WAVES * 64) void k_live_out(LiveOutArgs a) {
#pragma clang fp contract(off)
  constexpr int D = P3D_CLIP_D3, NC = P3D_CLIP_COLS, W = P3D_LIVE_WAVES;
  __shared__ double smean[D], sstd[D];
  __shared__ int pos[D];
  __shared__ float sy[W][D];                      // the wave's row of the network
  __shared__ double sox[W], soz[W], smx[W], smn[W];
  const int t = threadIdx.x, U3 = a.c.U3;
  const int du = t < U3 ? a.c.use3[t] : -1;
  for (int d = t; d < D; d += W * 64) { pos[d] = -1; smean[d] = a.c.mean3[d]; sstd[d] = a.c.std3[d]; }
  __syncthreads();
  if (du >= 0 && du < D) pos[du] = t;
  __syncthreads();                                // (the last workgroup barrier: before any wave leaves)
  const int lane = t & 63, wave = t >> 6;
  const int64_t s = (int64_t)blockIdx.x * W + wave;
  if (s >= a.t.S) return;
  double* good = a.st.good + s * D;
  int gp = a.st.good_pos[s];
  int64_t lo, hi;
  live_rows(a.t, s, lo, hi);
  for (int64_t r = lo; r < hi; ++r) {
    const int f = a.t.frame[r];
    for (int u = lane; u < U3; u += 64) sy[wave][u] = a.c.y[r * U3 + u];
    if (lane == 0) {
      sox[wave] = a.c.xy_s[r * NC + 2] - 630;     // spine_x - 630
      soz[wave] = 500 - a.c.xy_s[r * NC + 3];     // 500 - spine_y
    }
    live_wave_sync();
    double mx, mn;
    int ok;                                       // (every group of 8 lanes judges the same frame: uniform)
    clip_frame_judge(sy[wave], U3, pos, smean, sstd, 0, true, lane & 7, sox + wave, soz + wave, a.c.cache_on_fail, mx,
                     mn, ok);
    if (lane == 0) { smx[wave] = mx; smn[wave] = mn; }
    live_wave_sync();
    for (int d = lane; d < D; d += 64) {
      double v = 0.0;
      if (ok) {
        v = clip_export_value(sy[wave], U3, pos, smean, sstd, 0, d, smx + wave, smn + wave, sox + wave, soz + wave);
        good[d] = v;
      } else if (gp >= 0) {
        v = good[d];                              // (stored by this lane)
      }
      a.c.poses[r * D + d] = v;
    }
    if (ok) gp = f;
    if (lane == 0 && a.c.src) a.c.src[r] = gp;
    live_wave_sync();                             // (the next row overwrites sy)
  }
  if (lane == 0 && hi > lo) a.st.good_pos[s] = gp;
}
