// p3d_vae_wide.h -- the wide form of the VAE pose filter (in > 256, e.g. the reference's
// [x2d | out_3d | effnet_out] = 1360 inputs of src/3d_pose_effnet_2d_vae_filter.py): layer 0's
// kernel [in, enc0] does not fit a workgroup's LDS beside the rest, so it stays in its master
// buffer (HBM / L2) and the step is three launches ordered by the stream alone:
//
//   k_vae_wide_fwd         h0 = relu(x W0 + b0) -> [B, enc0]
//   k_vae_fwd / k_vae_step_dx   the filter of p3d_vae.h on the input h0 (every other layer packed in
//                          LDS); the backward also leaves d loss / d h0 as [B, enc0]
//   k_vae_wide_wgrad_adam  dW0 = x^T dz0, db0 = sum_row dz0, and Keras Adam on W0 / b0 and their
//                          slots when the call is a training step
//
// x is the concatenated, optionally row-indexed input (VaeCat); a plain [B, in] matrix is its
// one-segment case.  One wave owns an output tile; the weight gradient is ONE accumulator chain
// over all B rows in row order (16 rows a round, the four k-steps of a round in order), so its
// association depends on the row index only: not on the grid, the launch form or the wave that
// ran the tile.  No per-block partial of the [in, enc0] tensor exists.  No float atomics, no
// kernel waits on another workgroup.
#pragma once
#include "p3d_vae.h"

struct VaeWideArgs {
  VaeCat cat;
  int64_t B;
  int in, n0;                 // layer 0 is [in, n0]
  const float* w0;            // master kernel [in, n0] and bias [n0] behind it
  float* h0;                  // [B, n0]
  const float* dz0;           // [B, n0]: d loss / d h0 as the core left it (the ReLU mask h0 > 0 is applied here)
  float* g; float* w; float* m; float* v;   // flat gradient / master / Adam slots of layer 0: kernel, then bias
  const VaeState* st;
  int adam;
};

// h0 = relu(x W0 + b0).  A wave owns (16 rows, 16 columns).  Lane (i, q) takes x[row i][16 c + 4 q
// .. + 3] in one 16-byte load and feeds element j to MFMA step j of chunk c, whose B operand is
// W0[16 c + 4 q + j][column]: a fixed assignment of k to steps, the same for every input form.
__global__ __launch_bounds__(256) void k_vae_wide_fwd(VaeWideArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const int in = a.in, n0 = a.n0, NT = (n0 + 15) >> 4;
  const int64_t units = ((a.B + 15) >> 4) * NT;
  for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < units; u += (int64_t)gridDim.x * 4) {
    const int64_t rt = u / NT;
    const int ct = (int)(u - rt * NT);
    int64_t row = rt * 16 + i;
    row = row < a.B ? row : a.B - 1;   // (rows past B repeat the last; their results are dropped)
    const float* base[4];              // this lane's row of every segment, minus the segment's first column
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      base[s] = nullptr;
      if (s < a.cat.n) {
        int64_t r = row;
        if (a.cat.idx[s]) {
          r = a.cat.idx[s][row];
          r = r < 0 ? 0 : (r > a.cat.rows[s] - 1 ? a.cat.rows[s] - 1 : r);
        }
        base[s] = a.cat.p[s] + r * a.cat.w[s] - a.cat.off[s];
      }
    }
    const int n = 16 * ct + i;
    const float* wp = a.w0 + (n < n0 ? n : n0 - 1);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < in; k0 += 16) {
      const int kc = k0 + 4 * q;
      const bool ink = kc < in;          // (in is a multiple of 8: the last chunk may be half)
      const int kk = ink ? kc : in - 4;
      const float* bp = base[0];
#pragma unroll
      for (int s = 1; s < 4; ++s)
        if (s < a.cat.n && kk >= a.cat.off[s]) bp = base[s];
      const f32x4 xv = *(const f32x4*)(bp + kk);
      float b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = wp[(int64_t)(kk + j) * n0];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ink ? xv[j] : 0.0f, ink ? b[j] : 0.0f, acc, 0, 0, 0);
    }
    if (n < n0) {
      const float bias = a.w0[(int64_t)in * n0 + n];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t orow = rt * 16 + 4 * q + r;
        if (orow < a.B) a.h0[orow * n0 + n] = p3d_relu(acc[r] + bias);
      }
    }
  }
}

// With dz0 = (d loss / d h0) masked by h0 > 0:
// dW0[k][n] = sum_row x[row][k] dz0[row][n] and db0[n] = sum_row dz0[row][n] (the same chain with
// A = 1), one wave per 16 x 16 output tile, then -- in a training step -- Adam on the tile's
// elements with the alpha the core pass left in the state.  A lane's column of x is fixed, so its
// segment is chosen once.
__global__ __launch_bounds__(256) void k_vae_wide_wgrad_adam(VaeWideArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const int in = a.in, n0 = a.n0, NT = (n0 + 15) >> 4, KT = (in + 15) >> 4;
  const int u = blockIdx.x * 4 + wave;
  if (u >= KT * NT + NT) return;
  const bool bias = u >= KT * NT;        // (wave-uniform)
  const int kt = bias ? 0 : u / NT, nt = bias ? u - KT * NT : u - kt * NT;
  const int kc = 16 * kt + i;
  const bool ink = kc < in;
  const int col = ink ? kc : in - 1;
  const float* xp = a.cat.p[0];          // this lane's column in row 0 of its segment's table
  const int64_t* ix = a.cat.idx[0];
  int64_t rows = a.cat.rows[0];
  int w = a.cat.w[0], off = 0;
#pragma unroll
  for (int s = 1; s < 4; ++s)
    if (s < a.cat.n && col >= a.cat.off[s]) {
      xp = a.cat.p[s]; ix = a.cat.idx[s]; rows = a.cat.rows[s]; w = a.cat.w[s]; off = a.cat.off[s];
    }
  xp += col - off;
  const int n = 16 * nt + i;
  const bool inn = n < n0;
  const float* zp = a.dz0 + (inn ? n : n0 - 1);
  const float* hp = a.h0 + (inn ? n : n0 - 1);
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t r0 = 0; r0 < a.B; r0 += 16) {
    float av[4], bv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int64_t row = r0 + 4 * s + q;
      const bool valid = row < a.B;
      const int64_t rr = valid ? row : a.B - 1;
      float x = 1.0f;
      if (!bias) {
        int64_t xr = rr;
        if (ix) {
          xr = ix[rr];
          xr = xr < 0 ? 0 : (xr > rows - 1 ? rows - 1 : xr);
        }
        x = xp[xr * w];
      }
      const float z = zp[rr * n0] * (hp[rr * n0] > 0.0f ? 1.0f : 0.0f);   // a product (ReluGrad): a NaN gradient stays NaN
      av[s] = valid && (ink || bias) ? x : 0.0f;
      bv[s] = valid && inn ? z : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
  }
  const float alpha = a.adam ? a.st->alpha : 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = 16 * kt + 4 * q + r;
    if (!inn || (bias ? (4 * q + r) != 0 : k >= in)) continue;
    const int64_t e = bias ? (int64_t)in * n0 + n : (int64_t)k * n0 + n;
    const float g = acc[r];
    a.g[e] = g;
    if (a.adam) {
      float w1 = a.w[e], m1 = a.m[e], v1 = a.v[e];
      p3d_adam1(w1, m1, v1, g, alpha, 1.0f - 0.9f, 1.0f - 0.999f, 1.0e-7f);
      a.w[e] = w1; a.m[e] = m1; a.v[e] = v1;
    }
  }
}

// The stand-alone optimizer over layer 0's stored gradient (p3d_vae_adam_apply), behind
// k_vae_alpha: the same p3d_adam1 on the same operands as k_vae_wide_wgrad_adam's.
__global__ __launch_bounds__(256) void k_vae_wide_adam(int n, const float* __restrict__ g, float* __restrict__ w,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       const VaeState* __restrict__ st) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float w1 = w[e], m1 = m[e], v1 = v[e];
  p3d_adam1(w1, m1, v1, g[e], st->alpha, 1.0f - 0.9f, 1.0f - 0.999f, 1.0e-7f);
  w[e] = w1; m[e] = m1; v[e] = v1;
}
