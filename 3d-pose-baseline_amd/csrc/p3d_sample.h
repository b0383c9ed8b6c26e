// p3d_sample.h -- the numbers behind sample() (src/predict_3dpose.py:447-577): normalised 3D rows
// to root-centred world coordinates in one launch.  Per row, in float64 and with every product
// and sum rounded on its own (no FMA contraction), the composition of the kernels of p3d_data.h:
//
//   k_unnormalize      float32 scatter into 96 zeros, * std + mean      src/predict_3dpose.py:512-514
//   + root             the row's root added to all 32 joints (optional)                   :526
//   k_cam_points<1>    R^T X + T with the row's camera: ((R0r x + R1r y) + R2r z) + Tr    :539
//   k_root_center      minus the transformed joint 0                                      :542
//
// bit for bit, without the three [N, 96] float64 intermediates.
//
// Thread-to-element map.  A tile is 16 rows; a block of 256 threads walks tiles with a grid
// stride.  Per tile:
//   1. the tile's 16 U input values are one contiguous run: read coalesced (16 B per lane where
//      the input is float32 and 16-byte aligned) into LDS as float32; its 16 roots and 16 camera
//      indices go to LDS in the same step, so no global read sits between the barriers;
//   2. thread (row t / 32 and t / 32 + 8, joint t % 32) un-normalises its joint's three values,
//      adds the root, applies the row's camera and writes the three world coordinates to the
//      LDS row image [16][96].  mean / std / scatter positions of the joint are in registers for
//      the whole walk; R and T of all C cameras are in LDS (12 doubles each), read as a broadcast;
//   3. the 12 KiB row image leaves as 768 16-byte chunks, lane i of a wave at base + 16 i (1 KiB
//      contiguous per store instruction).  The chunk's two elements subtract the row's
//      transformed joint 0, which step 2 formed once: it is read back from the row image.
// Two barriers per tile; no atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p3d_data.h"

#define P3D_SAMPLE_ROWS 16       // rows per tile
#define P3D_SAMPLE_W 96          // doubles per output row (32 joints x 3)
#define P3D_SAMPLE_MAX_CAMS 64
#define P3D_SAMPLE_MAX_BLOCKS 2048

struct SampleArgs {
  const void* yn;            // [N, U] float32 or float64
  int64_t N;
  int U;
  const double* mean;        // [96]
  const double* stdv;        // [96]
  const int32_t* use;        // [U] entries in 0..95
  const double* root;        // [N, 3] or null
  const double* cams;        // [C, 21]
  int C;
  const int32_t* cam_of_row; // [N] or null (camera 0)
  double* out;               // [N, 96], 16-byte aligned
};

// (six waves per SIMD: what the 25,408 bytes of LDS allow; the bound keeps the registers to that)
// INF32: the input's dtype; VEC: float32 input that is 16-byte aligned (16-byte loads of whole tiles)
template <bool INF32, bool VEC>
__global__ __launch_bounds__(256, 6) void k_sample_world(SampleArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double s_out[P3D_SAMPLE_ROWS * P3D_SAMPLE_W];
  __shared__ __attribute__((aligned(16))) float s_in[P3D_SAMPLE_ROWS * P3D_SAMPLE_W];
  __shared__ double s_cam[P3D_SAMPLE_MAX_CAMS * 12];
  __shared__ int s_pos[P3D_SAMPLE_W];
  __shared__ double s_root[P3D_SAMPLE_ROWS * 3];
  __shared__ int s_camrow[P3D_SAMPLE_ROWS];
  const int t = threadIdx.x;
  const int U = a.U;

  // once per block: scatter positions (as k_unnormalize), R and T of every camera
  if (t < P3D_SAMPLE_W) s_pos[t] = -1;
  __syncthreads();
  if (t < U) {
    const int d = a.use[t];
    if ((unsigned)d < (unsigned)P3D_SAMPLE_W) s_pos[d] = t;
  }
  for (int i = t; i < a.C * 12; i += 256) s_cam[i] = a.cams[(i / 12) * P3D_CAM_DOUBLES + i % 12];
  __syncthreads();

  // this thread's joint: positions, std and mean of its three dimensions
  const int j = t & 31, lr = t >> 5;
  int pos[3];
  double sd[3], mu[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    pos[r] = s_pos[3 * j + r];
    sd[r] = a.stdv[3 * j + r];
    mu[r] = a.mean[3 * j + r];
  }

  const int64_t tiles = (a.N + P3D_SAMPLE_ROWS - 1) / P3D_SAMPLE_ROWS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * P3D_SAMPLE_ROWS;
    const int rows = (int)min((int64_t)P3D_SAMPLE_ROWS, a.N - row0);
    const int nin = rows * U;
    // 1. the tile's inputs, rounded to float32 as unNormalizeData's float32 matrix does
    if (VEC && rows == P3D_SAMPLE_ROWS) {
      const float4* src = (const float4*)((const float*)a.yn + row0 * U);
      for (int i = t; i < nin / 4; i += 256) ((float4*)s_in)[i] = src[i];
    } else if (INF32) {
      const float* src = (const float*)a.yn + row0 * U;
      for (int i = t; i < nin; i += 256) s_in[i] = src[i];
    } else {
      const double* src = (const double*)a.yn + row0 * U;
      for (int i = t; i < nin; i += 256) s_in[i] = (float)src[i];
    }
    // ... and its roots and camera indices (waves 2 and 3: their input loads are the fewest)
    if (a.root && t >= 128 && t < 128 + rows * 3) s_root[t - 128] = a.root[row0 * 3 + (t - 128)];
    if (t >= 192 && t < 192 + rows) s_camrow[t - 192] = a.cam_of_row ? a.cam_of_row[row0 + (t - 192)] : 0;
    __syncthreads();
    // 2. un-normalise, add the root, camera -> world; rows lr and lr + 8 of the tile
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r_l = lr + 8 * h;
      if (r_l < rows) {
        double p[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          float v = 0.0f;
          if (pos[r] >= 0) v = s_in[r_l * U + pos[r]];
          p[r] = (double)v * sd[r] + mu[r];
        }
        if (a.root) {
#pragma unroll
          for (int r = 0; r < 3; ++r) p[r] = p[r] + s_root[r_l * 3 + r];
        }
        const double* cm = s_cam + s_camrow[r_l] * 12;
        double* o = s_out + r_l * P3D_SAMPLE_W + 3 * j;
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = ((cm[r] * p[0] + cm[3 + r] * p[1]) + cm[6 + r] * p[2]) + cm[9 + r];
      }
    }
    __syncthreads();
    // 3. minus the row's joint 0 (as k_root_center: v - r), out in 16-byte chunks
    double2* dst = (double2*)(a.out + row0 * P3D_SAMPLE_W);
    for (int c = t; c < rows * (P3D_SAMPLE_W / 2); c += 256) {
      const int r_l = c / (P3D_SAMPLE_W / 2);
      const int e = 2 * (c - r_l * (P3D_SAMPLE_W / 2));
      const double* rowp = s_out + r_l * P3D_SAMPLE_W;
      double2 v = *(const double2*)(rowp + e);
      v.x = v.x - rowp[e % 3];
      v.y = v.y - rowp[(e + 1) % 3];
      dst[c] = v;
    }
    // (the next tile's first barrier orders these reads of s_out before its writes)
  }
}
