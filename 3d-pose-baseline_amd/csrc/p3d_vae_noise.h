// p3d_vae_noise.h -- the noise the VAE filters are trained to remove (gfx950), drawn on the device:
// src/top_vae_3d_pose/data_handler.py:48-84 (add_noise) as a counter-based stream.  Device code
// only; the host side (p3d_vae_add_noise) is in p3d_vae_host.h.
//
// Output row r is `width` contiguous floats of the table `src` [rows, d]: its row r, or -- the
// window form -- the k = width / d rows from row starts[r] (clamped into [0, rows - k]).  With
// g = row0 + r (low 32 bits, like ctr):
//
//   element normals  columns 4 c .. 4 c + 3: vae_eps4_site over the counter (g, c, P3D_NOISE_SITE, ctr)
//   row block A      Philox (g, 0, P3D_NOISE_ROW_SITE, ctr): the row is noised iff A.x >= thr
//                    (P3D_NOISE_THRESHOLD = floor(Phi(0.5) 2^32): the reference's randn() >= 0.5);
//                    the chosen column is jc = (A.y * width) >> 32 and its joint starts at
//                    jid = jc - jc % 3
//   row block B      vae_eps4_site over (g, 1, P3D_NOISE_ROW_SITE, ctr): j0, j1, j2 of the joint
//
//   clean row        copied bit for bit
//   noised row       v[c] = x[c] + (e[c] * noise + offset); then v[jid + k] += j_k * joint_scale
//                    (float32, no contraction, every operation rounded once)
//
// The Box-Muller (one logf, one sqrtf, a sinf and a cosf per two normals) makes a noised element
// cost hundreds of VALU instructions against 8 bytes moved, so the kernel is bound by instruction
// issue, and 69 % of the rows are clean.  A wave therefore owns 64 consecutive rows and works in
// three steps: (1) lane l decides row l -- one Philox block, and for a noised row its joint's
// three normals -- and the noised rows are compacted through a ballot into a list in LDS; (2) the
// clean rows are copied, 16 bytes per lane, consecutive lanes on consecutive addresses (nothing to
// do in place); (3) the (noised row, four-column) units are dealt densely over the lanes, so every
// lane that evaluates a Box-Muller has one to evaluate: no lane idles next to a noised neighbour.
// The stream is keyed by position, so the order of the work changes no bit.
#pragma once
#include "p3d_vae.h"

#define P3D_NOISE_SITE 0x4E4F49          // element normals ("NOI"); P3D_VAE_SITE is 0x564145, dropout sites < 64
#define P3D_NOISE_ROW_SITE 0x4E4F52      // the two per-row blocks ("NOR")
#define P3D_NOISE_THRESHOLD 0xB103AF11u  // floor(Phi(0.5) * 2^32), Phi(0.5) = 0.6914624612740131
#define P3D_NOISE_MAX_WIDTH 240

struct NoiseArgs {
  const float* src;        // [rows, d]
  int64_t rows;
  const int64_t* starts;   // [B] or null
  int64_t B, row0;
  uint64_t seed, ctr;
  uint64_t thr;            // noised iff A.x >= thr (64-bit so that 2^32 noises no row: the probe's knob)
  float noise, offset, joint_scale;
  int d, width;
  uint32_t magic;          // ceil(2^32 / (width / 4)): unit -> (row, four-column group) by one multiply
  float* out;              // [B, width]; may be src in the plain form
};

__global__ __launch_bounds__(256) void k_vae_noise(NoiseArgs a) {
#pragma clang fp contract(off)
  __shared__ int64_t s_row[4][64];     // source row of the wave's row l
  __shared__ int s_lst[4][64];         // k-th noised row of the wave -> l
  __shared__ int s_jid[4][64];         // its joint's first column
  __shared__ float s_j[4][3][64];      // its joint's three normals
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t base = ((int64_t)blockIdx.x * 4 + w) * 64;
  if (base >= a.B) return;             // (a whole wave; the waves of a block share nothing)
  const int nrows = a.B - base < 64 ? (int)(a.B - base) : 64;
  const int c4n = a.width >> 2;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);

  // (1) the rows' decisions
  bool noised = false;
  uint4 A = make_uint4(0u, 0u, 0u, 0u);
  int64_t sr = base + lane;
  if (lane < nrows) {
    if (a.starts) {
      const int64_t hi = a.rows - a.width / a.d;
      sr = a.starts[base + lane];
      sr = sr < 0 ? 0 : (sr > hi ? hi : sr);
    }
    A = p3d_philox(make_uint4((uint32_t)(a.row0 + base + lane), 0u, (uint32_t)P3D_NOISE_ROW_SITE, (uint32_t)a.ctr), k0, k1);
    noised = (uint64_t)A.x >= a.thr;
  }
  s_row[w][lane] = sr;
  const uint64_t mask = __ballot(noised);
  if (noised) {
    const int k = __popcll(mask & ((1ull << lane) - 1ull));
    const int jc = (int)__umulhi(A.y, (uint32_t)a.width);
    float j[4];
    vae_eps4_site(a.seed, a.ctr, (uint32_t)P3D_NOISE_ROW_SITE, a.row0 + base + lane, 1, j);
    s_lst[w][k] = lane;
    s_jid[w][k] = jc - jc % 3;
    s_j[w][0][k] = j[0]; s_j[w][1][k] = j[1]; s_j[w][2][k] = j[2];
  }
  vae_wsync();

  // (2) the clean rows
  if (a.src != a.out) {
    const int units = nrows * c4n;
    for (int it = lane; it < units; it += 64) {
      const int l = (int)__umulhi((uint32_t)it, a.magic), c = it - l * c4n;
      if ((mask >> l) & 1ull) continue;
      *(f32x4*)(a.out + (base + l) * a.width + 4 * c) = *(const f32x4*)(a.src + s_row[w][l] * a.d + 4 * c);
    }
  }

  // (3) the noised rows, their units dense over the lanes
  const int nunits = __popcll(mask) * c4n;
  for (int it = lane; it < nunits; it += 64) {
    const int k = (int)__umulhi((uint32_t)it, a.magic), c = it - k * c4n;
    const int l = s_lst[w][k], t0 = 4 * c - s_jid[w][k];
    float e[4];
    vae_eps4_site(a.seed, a.ctr, (uint32_t)P3D_NOISE_SITE, a.row0 + base + l, c, e);
    const f32x4 x = *(const f32x4*)(a.src + s_row[w][l] * a.d + 4 * c);
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = x[i] + (e[i] * a.noise + a.offset);
      const int t = t0 + i;
      if (t >= 0 && t < 3) v[i] = v[i] + s_j[w][t][k] * a.joint_scale;
    }
    *(f32x4*)(a.out + (base + l) * a.width + 4 * c) = v;
  }
}
