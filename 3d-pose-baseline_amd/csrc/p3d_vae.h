// p3d_vae.h -- the VAE pose filter on top of the frozen lifter (gfx950): forward, ELBO loss,
// backward and Keras Adam of src/top_vae_3d_pose/models.py:12-91 (VAE), losses.py:12-109 (ELBO)
// and src/3d_pose_vae_filter.py:188-196 (train_step_vae).  Device code only: the plain structs are
// in p3d_vae_desc.h, the layout planner in p3d_vae_layout.h, the host side in p3d_vae_host.h.
//
// The filter is a small dense net (default 48 -> 40 -> 32 -> {24, 24} -> 32 -> 40 -> 48, 8.9 K
// parameters), so every kernel keeps the WHOLE parameter set in LDS for the launch -- a packed
// copy, layer l as W [K, ld] row-major with its N columns zero-padded to the 16-wide MFMA tile
// (Np) and the bias [Np] behind it; the mean and log_varianze heads are one layer of 2 * latent
// columns -- and a wave owns 16-row tiles: it runs a tile through every layer on
// v_mfma_f32_16x16x4_f32 with the activations in its own LDS area.
//
//   forward     D[row][n] = sum_k act[row][k] W[k][n]: lane (i, q) feeds A = act[i][k + q] and
//               B = W[k + q][16 ct + i] and receives column 16 ct + i, rows 4 q + r.
//   weight grad D[k][n] = sum_row act[row][k] dz[row][n]: A = act[4 s + q][16 kt + i],
//               B = dz[4 s + q][16 nt + i].  One wave owns an output tile and runs ONE accumulator
//               chain over the 64 rows of the block (row tiles 0..3 in order, the four k-steps of
//               a tile in order): the MFMA is a k-ordered fmaf chain, so the association of every
//               sum is a function of the row index only -- not of the grid, the wave that ran a
//               tile or the launch form.  64-row blocks are summed in block order (in
//               k_vae_reduce_adam).  No float atomics anywhere.
//   data grad   D[row][k] = sum_n dz[row][n] W[k][n]: A = dz[i][n + q], B = W[16 kt + i][n + q];
//               the result, masked by the ReLU, overwrites the activation it differentiates.
//
// k_vae_step at B <= 64 is one workgroup that also applies the optimizer (one launch per training
// step); at B > 64 every 64-row block writes its partial gradient to the workspace and
// k_vae_reduce_adam, ordered behind it by the stream alone, sums the blocks and applies Adam.  No
// kernel here waits on another workgroup.
//
// The kernels come in forms of one body: k_vae_fwd_cat / k_vae_step_cat read the input through a
// VaeCat (column segments, each optionally row-indexed; p3d.h p3d_vae_cat) instead of x, in the
// same order of operations; k_vae_step_dx is the core of the wide form (p3d_vae_wide.h), whose
// input is layer 0's output and whose backward also leaves the data gradient at that input.
//
// The bones filter (models.py:544-573 VAEBones, losses.py:113-156 loss_bones) is the same body
// with another loss kind: its decoder ends dec_dim -> mag1 (16, ReLU) -> {mag2 (16), cos2 (48)},
// the two linear heads one packed layer [16, 64] split at column 16 like the mean / log_varianze
// head, and k_vae_bones_fwd / _step and their _cat and _dx forms form the four-term loss and its
// backward in place of the ELBO's.
#pragma once
#include "p3d_kernels.h"
#include "p3d_layers.h"   // p3d_adam1
#include "p3d_vae_desc.h"
#include <math.h>
#include <stdint.h>

#define P3D_VAE_SITE 0x564145     // Philox site id of the eps stream (dropout sites are < 64)

__device__ __forceinline__ void vae_wsync() {   // LDS hand-off between the lanes of one wave
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// parent joint + 1 of bone a in nibble a (0: the bone is the joint itself), losses.py:74-94
#define P3D_VAE_PAR 0xFE8CB89870540210ull
__device__ __forceinline__ int vae_par(int a) { return (int)((P3D_VAE_PAR >> (4 * a)) & 15) - 1; }

// Four standard normals of eps row `row`, columns 4 c4 .. 4 c4 + 3: one Philox4x32-10 block keyed
// (seed, ctr, site, row, c4) through TF's Box-Muller (random_distributions.h BoxMullerFloat).
// vae_eps4_site is the construction over any site: the noise stream (p3d_vae_noise.h) draws from it.
__device__ __forceinline__ void vae_eps4_site(uint64_t seed, uint64_t ctr, uint32_t site, int64_t row, int c4,
                                              float e[4]) {
#pragma clang fp contract(off)
  const uint4 w = p3d_philox(make_uint4((uint32_t)row, (uint32_t)c4, site, (uint32_t)ctr),
                             (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t xs[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float u1 = __uint_as_float((xs[2 * h] & 0x7FFFFFu) | 0x3F800000u) - 1.0f;
    const float u2 = __uint_as_float((xs[2 * h + 1] & 0x7FFFFFu) | 0x3F800000u) - 1.0f;
    u1 = fmaxf(u1, 1.0e-7f);
    const float r = sqrtf(-2.0f * logf(u1));
    const float ang = 6.28318530717958647692f * u2;
    e[2 * h] = sinf(ang) * r;
    e[2 * h + 1] = cosf(ang) * r;
  }
}
__device__ __forceinline__ void vae_eps4(uint64_t seed, uint64_t ctr, int64_t row, int c4, float e[4]) {
  vae_eps4_site(seed, ctr, (uint32_t)P3D_VAE_SITE, row, c4, e);
}

__global__ __launch_bounds__(256) void k_vae_eps(uint64_t seed, uint64_t ctr, int64_t row0, int64_t B, int latent,
                                                 float* __restrict__ out) {
  const int c4n = latent >> 2;
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= B * c4n) return;
  const int64_t r = u / c4n;
  const int c4 = (int)(u - r * c4n);
  float e[4];
  vae_eps4(seed, ctr, row0 + r, c4, e);
  *(f32x4*)(out + r * latent + 4 * c4) = f32x4{e[0], e[1], e[2], e[3]};
}

// (p0 + p1) + (p2 + p3) over the four lanes i, i + 16, i + 32, i + 48 that share a row
__device__ __forceinline__ float vae_rowsum4(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// Element (row, col) of the concatenated input.  An index is clamped into its table: a bad one
// never becomes a wild read.  (Unrolled selects: no dynamic index into the kernel arguments.)
__device__ __forceinline__ const float* vae_cat_at(const VaeCat& c, int64_t row, int col) {
  const float* p = c.p[0];
  const int64_t* ix = c.idx[0];
  int64_t rows = c.rows[0];
  int w = c.w[0], off = 0;
#pragma unroll
  for (int s = 1; s < 4; ++s)
    if (s < c.n && col >= c.off[s]) { p = c.p[s]; ix = c.idx[s]; rows = c.rows[s]; w = c.w[s]; off = c.off[s]; }
  int64_t r = row;
  if (ix) {
    r = ix[row];
    r = r < 0 ? 0 : (r > rows - 1 ? rows - 1 : r);
  }
  return p + r * w + (col - off);
}

struct VaeArgs {
  const VaeDesc* desc;
  const float* pk;            // packed parameters [Ppk]
  const float* x;             // [B, in]
  const float* t;             // [B, out] or null (forward without loss terms)
  const float* eps;           // [B, latent] or null (draw from Philox)
  int64_t B;
  uint64_t seed, ctr;
  const VaeState* ctr_dev;    // if set, ctr = the device step counter
  // forward outputs (any may be null)
  float* y; float* mean; float* log_var; float* z; float* row_terms;
  // step
  int backward, adam, nblk;
  int tail;                   // one-launch form: k_vae_step forms the loss and applies Adam itself (nblk == 1)
  float c_like, c_kcs, c_kl;  // 2 likef / (B out), kcsf / B, dklf / B; bones: 2 magf / (16 B), angf / (256 B), dklf / B
  float c_cos;                // bones: cosf / (8 B)
  int nterm;                  // row terms and loss entries: 3, bones 4
  float f[4];                 // likef, kcsf, dklf; bones: magf, cosf, dklf, angf
  float lr;
  float* gout;                // block b's partial gradient at gout + b * P
  float* lpart;               // block b's loss sums at lpart + 4 b
  float* loss3;               // the loss vector [nterm]
  float* w; float* m; float* v; float* pk_out; VaeState* st;
  const int* pkidx;           // flat element -> its place in the packed copy
  float* dx;                  // k_vae_step_dx: d(loss sum) / dx, [B, in]
  VaeCat cat;                 // the _cat kernels: the input in place of x
};

// One layer of one 16-row tile: out = act(A W + b).  `arow` is this lane's row of A (global x or
// LDS), `W` the packed parameters in LDS.
__device__ __forceinline__ void vae_layer_fwd(const VaeLayer& L, const float* arow, const float* W, float* out) {
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const int K = L.K, ld = L.ld, ldo = L.ldo, relu = L.relu, nct = L.Np >> 4;   // (locals: the loops' bounds stay put)
  const float* ap = arow + q;
  for (int ct = 0; ct < nct; ++ct) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wp = W + L.wpk + q * ld + 16 * ct + i;
    for (int k = 0; k < K; k += 8) {   // (every width is a multiple of 8: two k-steps' operands in flight)
      const float a0 = ap[k], b0 = wp[k * ld], a1 = ap[k + 4], b1 = wp[(k + 4) * ld];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc, 0, 0, 0);
    }
    const float b = W[L.bpk + 16 * ct + i];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[r] + b;
      if (relu) v = p3d_relu(v);
      out[(4 * q + r) * ldo + 16 * ct + i] = v;
    }
  }
}

// Layer 0 of one tile on a concatenated input that is not staged in LDS: the same k order, each
// operand through vae_cat_at.
__device__ __forceinline__ void vae_layer_fwd_cat(const VaeLayer& L, const VaeCat& c, int64_t row, const float* W,
                                                  float* out) {
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const int K = L.K, ld = L.ld, ldo = L.ldo, relu = L.relu, nct = L.Np >> 4;
  for (int ct = 0; ct < nct; ++ct) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wp = W + L.wpk + q * ld + 16 * ct + i;
    for (int k = 0; k < K; k += 8) {
      const float a0 = *vae_cat_at(c, row, k + q), b0 = wp[k * ld];
      const float a1 = *vae_cat_at(c, row, k + 4 + q), b1 = wp[(k + 4) * ld];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc, 0, 0, 0);
    }
    const float b = W[L.bpk + 16 * ct + i];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[r] + b;
      if (relu) v = p3d_relu(v);
      out[(4 * q + r) * ldo + 16 * ct + i] = v;
    }
  }
}

// The bones loss of one tile (losses.py:113-156) on y = [mag (16) | cos (16 x 3)] in `yb` against the
// target row [tm | tc]: row terms MAG = mean_16 (tm - pm)^2, COS = 3 mean_48 (tc - pc)^2 and ANG =
// mean_16x16 |G(tc) - G(pc)|, G(c)[a][b] = c[a] . c[b] -- the KCS block on the 16 cosine triples
// themselves (no parent subtraction).  With `train`, dy = d(loss sum) / dy in place of y:
//   d / dpm = c_like (pm - tm), d / dpc = c_cos (pc - tc) + c_kcs 2 sum_b sign(phi[a][b]) pc[b],
// phi = G(pc) - G(tc), sign(0) = 0, sign(NaN) = NaN.
__device__ __forceinline__ void vae_bones_terms(const VaeArgs& a, const VaeDesc* d, float* act, float* yb, int ldy,
                                                int64_t row0, bool train, float terms[4]) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const int64_t Bm1 = a.B - 1;
  const int64_t myrow = row0 + i < a.B ? row0 + i : Bm1;
  const bool myvalid = row0 + i < a.B;
  const float* trow = a.t + myrow * 64;
  {
    float p = 0.0f;
    for (int c = q; c < 16; c += 4) {
      const float df = trow[c] - yb[i * ldy + c];
      p += df * df;
    }
    terms[0] = vae_rowsum4(p) / 16.0f;
    p = 0.0f;
    for (int c = q; c < 48; c += 4) {
      const float df = trow[16 + c] - yb[i * ldy + 16 + c];
      p += df * df;
    }
    terms[1] = 3.0f * (vae_rowsum4(p) / 48.0f);
  }
  float* bt = act + d->bt;
  const int ldb = d->ldb;
  for (int idx = lane; idx < 16 * 48; idx += 64) {
    const int r = idx / 48, e = idx - r * 48;
    const int64_t grow = row0 + r < a.B ? row0 + r : Bm1;
    bt[r * ldb + e] = a.t[grow * 64 + 16 + e];
  }
  vae_wsync();
  const float* yc = yb + i * ldy + 16;
  float pa[4][3], ta[4][3], dB[4][3];
#pragma unroll
  for (int a4 = 0; a4 < 4; ++a4) {
    const int bn = 4 * q + a4;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pa[a4][c] = yc[3 * bn + c];
      ta[a4][c] = bt[i * ldb + 3 * bn + c];
      dB[a4][c] = 0.0f;
    }
  }
  float s = 0.0f;
  for (int b = 0; b < 16; ++b) {
    float pb[3], tb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pb[c] = yc[3 * b + c];
      tb[c] = bt[i * ldb + 3 * b + c];
    }
#pragma unroll
    for (int a4 = 0; a4 < 4; ++a4) {
      const float pp = (pa[a4][0] * pb[0] + pa[a4][1] * pb[1]) + pa[a4][2] * pb[2];
      const float tt = (ta[a4][0] * tb[0] + ta[a4][1] * tb[1]) + ta[a4][2] * tb[2];
      const float phi = pp - tt;
      s += fabsf(phi);
      const float sg = phi > 0.0f ? 1.0f : (phi < 0.0f ? -1.0f : (phi == 0.0f ? 0.0f : phi));   // as the KCS block
#pragma unroll
      for (int c = 0; c < 3; ++c) dB[a4][c] += sg * pb[c];
    }
  }
  terms[3] = vae_rowsum4(s) * 0.00390625f;   // / 256
  vae_wsync();   // every lane has read the target cosines
  if (!train) return;
  const float ck = myvalid ? 2.0f * a.c_kcs : 0.0f;
#pragma unroll
  for (int a4 = 0; a4 < 4; ++a4)
#pragma unroll
    for (int c = 0; c < 3; ++c) bt[i * ldb + 3 * (4 * q + a4) + c] = ck * dB[a4][c];
  vae_wsync();
  for (int idx = lane; idx < 16 * 64; idx += 64) {
    const int r = idx >> 6, e = idx & 63;
    const bool valid = row0 + r < a.B;
    const int64_t grow = valid ? row0 + r : Bm1;
    float g = 0.0f;
    float cl = a.c_like;
    if (e >= 16) { g = bt[r * ldb + (e - 16)]; cl = a.c_cos; }
    cl = valid ? cl : 0.0f;
    g += cl * (yb[r * ldy + e] - a.t[grow * 64 + e]);
    yb[r * ldy + e] = g;
  }
}

// Forward of one tile (rows row0 .. row0 + 15) through every layer, the reparametrisation, the
// requested global outputs and the three per-row loss terms (when a.t is set); with `train` also
// 0.5 eps std, and dy = d(loss sum) / dy in place of y.  Returns this lane's row terms (lanes of
// one row hold the same values).  KIND picks the loss at compile time: the ELBO's three terms, or
// the bones filter's four (vae_bones_terms; terms[2], the KL term, is common).
template <bool CAT, int KIND>
__device__ __forceinline__ void vae_tile_fwd(const VaeArgs& a, const VaeDesc* d, const float* W, float* act,
                                             int64_t row0, uint64_t ctr, bool train, float terms[4]) {
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const int lat = d->latent, out = d->out;
  const int64_t Bm1 = a.B - 1;
  const int64_t myrow = row0 + i < a.B ? row0 + i : Bm1;     // (clamped: rows past B repeat the last)
  const bool myvalid = row0 + i < a.B;
  // ---- encoder ----
  if (d->xbuf >= 0) {   // the input tile through LDS: one round of coalesced loads
    float* xb = act + d->xbuf;
    const int in = d->in, ldx = d->ldx;
    for (int idx = lane; idx < 16 * in; idx += 64) {
      const int r = idx / in, c = idx - r * in;
      const int64_t grow = row0 + r < a.B ? row0 + r : Bm1;
      xb[r * ldx + c] = CAT ? *vae_cat_at(a.cat, grow, c) : a.x[grow * in + c];
    }
    vae_wsync();
    vae_layer_fwd(d->L[0], xb + i * ldx, W, act + d->L[0].aout);
  } else if (CAT) {
    vae_layer_fwd_cat(d->L[0], a.cat, myrow, W, act + d->L[0].aout);
  } else {
    vae_layer_fwd(d->L[0], a.x + myrow * d->in, W, act + d->L[0].aout);
  }
  vae_wsync();
  for (int l = 1; l <= d->head; ++l) {
    const VaeLayer& L = d->L[l];
    vae_layer_fwd(L, act + L.ain + i * L.lda, W, act + L.aout);
    vae_wsync();
  }
  // ---- z = eps exp(0.5 log_var) + mean (models.py:68-71) ----
  float* ml = act + d->L[d->head].aout;
  const int ldm = d->L[d->head].ldo;
  float* zb = act + d->zbuf;
  float* eb = act + d->ebuf;
  {
#pragma clang fp contract(off)
    const int c4n = lat >> 2;
    for (int u = lane; u < 16 * c4n; u += 64) {
      const int r = u / c4n, c4 = u - r * c4n;
      const bool valid = row0 + r < a.B;
      const int64_t grow = valid ? row0 + r : Bm1;
      float e[4];
      if (a.eps) {
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = a.eps[grow * lat + 4 * c4 + j];
      } else {
        vae_eps4(a.seed, ctr, grow, c4, e);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * c4 + j;
        const float mu = ml[r * ldm + c], lv = ml[r * ldm + lat + c];
        const float sd = expf(0.5f * lv);
        const float es = e[j] * sd;
        const float zz = es + mu;
        zb[r * d->ldz + c] = zz;
        if (train) eb[r * d->lde + c] = 0.5f * es;
        if (valid) {
          if (a.mean) a.mean[grow * lat + c] = mu;
          if (a.log_var) a.log_var[grow * lat + c] = lv;
          if (a.z) a.z[grow * lat + c] = zz;
        }
      }
    }
  }
  terms[0] = terms[1] = terms[2] = terms[3] = 0.0f;
  if (a.t) {   // KL row term 0.5 sum(exp(lv) + mean^2 - 1 - lv) (losses.py:29)
#pragma clang fp contract(off)
    float p = 0.0f;
    for (int c = q; c < lat; c += 4) {
      const float mu = ml[i * ldm + c], lv = ml[i * ldm + lat + c];
      p += ((expf(lv) + mu * mu) - 1.0f) - lv;
    }
    terms[2] = 0.5f * vae_rowsum4(p);
  }
  vae_wsync();
  // ---- decoder ----
  for (int l = d->head + 1; l < d->nl; ++l) {
    const VaeLayer& L = d->L[l];
    vae_layer_fwd(L, act + L.ain + i * L.lda, W, act + L.aout);
    vae_wsync();
  }
  float* yb = act + d->L[d->nl - 1].aout;
  const int ldy = d->L[d->nl - 1].ldo;
  if (a.y) {
    for (int idx = lane; idx < 16 * out; idx += 64) {
      const int r = idx / out, c = idx - r * out;
      if (row0 + r < a.B) a.y[(row0 + r) * out + c] = yb[r * ldy + c];
    }
  }
  if (!a.t) return;
  if (KIND == P3D_VAE_KIND_BONES) {
    vae_bones_terms(a, d, act, yb, ldy, row0, train, terms);
    return;
  }
  const float* trow = a.t + myrow * out;
  {   // likelihood row term mean_D (t - y)^2 (losses.py:31)
#pragma clang fp contract(off)
    float p = 0.0f;
    for (int c = q; c < out; c += 4) {
      const float df = trow[c] - yb[i * ldy + c];
      p += df * df;
    }
    terms[0] = vae_rowsum4(p) / (float)out;
  }
  const bool kcs = out == 48;
  float* bt = act + d->bt;
  const int ldb = d->ldb;
  if (kcs) {   // KCS row term sum |B^T B (pred) - B^T B (target)| (losses.py:60-109)
#pragma clang fp contract(off)
    for (int idx = lane; idx < 16 * 48; idx += 64) {
      const int r = idx / 48, e = idx - r * 48, jn = e / 3, c = e - 3 * jn;
      const int p = vae_par(jn);
      const int64_t grow = row0 + r < a.B ? row0 + r : Bm1;
      const float tv = a.t[grow * 48 + e];
      const float tp = p >= 0 ? a.t[grow * 48 + 3 * p + c] : 0.0f;
      bt[r * ldb + e] = tv - tp;
    }
    vae_wsync();
    float pa[4][3], ta[4][3], dB[4][3];
#pragma unroll
    for (int a4 = 0; a4 < 4; ++a4) {
      const int bn = 4 * q + a4, p = vae_par(bn);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        pa[a4][c] = yb[i * ldy + 3 * bn + c] - (p >= 0 ? yb[i * ldy + 3 * p + c] : 0.0f);
        ta[a4][c] = bt[i * ldb + 3 * bn + c];
        dB[a4][c] = 0.0f;
      }
    }
    float s = 0.0f;
    for (int b = 0; b < 16; ++b) {
      const int p = vae_par(b);
      float pb[3], tb[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        pb[c] = yb[i * ldy + 3 * b + c] - (p >= 0 ? yb[i * ldy + 3 * p + c] : 0.0f);
        tb[c] = bt[i * ldb + 3 * b + c];
      }
#pragma unroll
      for (int a4 = 0; a4 < 4; ++a4) {
        const float pp = (pa[a4][0] * pb[0] + pa[a4][1] * pb[1]) + pa[a4][2] * pb[2];
        const float tt = (ta[a4][0] * tb[0] + ta[a4][1] * tb[1]) + ta[a4][2] * tb[2];
        const float phi = pp - tt;
        s += fabsf(phi);
        const float sg = phi > 0.0f ? 1.0f : (phi < 0.0f ? -1.0f : (phi == 0.0f ? 0.0f : phi));   // tf.abs gradient: sign, sign(0) = 0, sign(NaN) = NaN
#pragma unroll
        for (int c = 0; c < 3; ++c) dB[a4][c] += sg * pb[c];
      }
    }
    terms[1] = vae_rowsum4(s);
    vae_wsync();   // every lane has read the target bones
    if (train) {   // d kcs / d bone = 2 sum_b sign(phi[a][b]) bone_b (phi is symmetric)
      const float ck = myvalid ? 2.0f * a.c_kcs : 0.0f;
#pragma unroll
      for (int a4 = 0; a4 < 4; ++a4)
#pragma unroll
        for (int c = 0; c < 3; ++c) bt[i * ldb + 3 * (4 * q + a4) + c] = ck * dB[a4][c];
      vae_wsync();
    }
  }
  if (train) {   // dy in place of y: joint j receives its own bone's gradient and minus its children's
#pragma clang fp contract(off)
    for (int idx = lane; idx < 16 * out; idx += 64) {
      const int r = idx / out, e = idx - r * out;
      const bool valid = row0 + r < a.B;
      const int64_t grow = valid ? row0 + r : Bm1;
      float g = 0.0f;
      if (kcs) {
        const int jn = e / 3, c = e - 3 * jn;
        g = bt[r * ldb + e];
        for (int ch = jn + 1; ch < 16; ++ch)
          if (vae_par(ch) == jn) g -= bt[r * ldb + 3 * ch + c];
      }
      const float cl = valid ? a.c_like : 0.0f;
      g += cl * (yb[r * ldy + e] - a.t[grow * out + e]);
      yb[r * ldy + e] = g;
    }
  }
}

// Parameters into LDS, the z buffers' pad columns zeroed (a latent of 8 mod 16 pads the k tile of
// the first decoder layer's weight gradient).
__device__ __forceinline__ void vae_load_params(const VaeArgs& a, const VaeDesc* d, float* sm) {
  for (int idx = threadIdx.x; idx < (d->Ppk >> 2); idx += 256) ((f32x4*)sm)[idx] = ((const f32x4*)a.pk)[idx];
  const int zp = d->ldz - d->latent;
  for (int idx = threadIdx.x; idx < 4 * 16 * zp; idx += 256) {
    const int w = idx / (16 * zp), rem = idx - w * 16 * zp, r = rem / zp, c = rem - r * zp;
    sm[d->Ppk + w * d->act + d->zbuf + r * d->ldz + d->latent + c] = 0.0f;
  }
  __syncthreads();
}

// The filter: x -> mean, log_var -> z -> y, every output optional.  Waves stride over the 16-row
// tiles on their own: no barrier after the parameter load.
template <bool CAT, int KIND>
__device__ __forceinline__ void vae_fwd_body(const VaeArgs& a) {
  extern __shared__ f32x4 vae_smem[];
  float* sm = (float*)vae_smem;
  const VaeDesc* d = a.desc;
  vae_load_params(a, d, sm);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* act = sm + d->Ppk + wave * d->act;
  const uint64_t ctr = a.ctr_dev ? (uint64_t)a.ctr_dev->step : a.ctr;
  const int64_t ntiles = (a.B + 15) >> 4;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
    constexpr int NTERM = KIND == P3D_VAE_KIND_BONES ? 4 : 3;
    float terms[4];
    vae_tile_fwd<CAT, KIND>(a, d, sm, act, tile * 16, ctr, false, terms);
    const int64_t row = tile * 16 + (lane & 15);
    if (a.row_terms && a.t && lane < 16 && row < a.B) {
#pragma unroll
      for (int j = 0; j < NTERM; ++j) a.row_terms[row * NTERM + j] = terms[j];
    }
    vae_wsync();
  }
}
__global__ __launch_bounds__(256) void k_vae_fwd(VaeArgs a) { vae_fwd_body<false, P3D_VAE_KIND_ELBO>(a); }
__global__ __launch_bounds__(256) void k_vae_fwd_cat(VaeArgs a) { vae_fwd_body<true, P3D_VAE_KIND_ELBO>(a); }
__global__ __launch_bounds__(256) void k_vae_bones_fwd(VaeArgs a) { vae_fwd_body<false, P3D_VAE_KIND_BONES>(a); }
__global__ __launch_bounds__(256) void k_vae_bones_fwd_cat(VaeArgs a) { vae_fwd_body<true, P3D_VAE_KIND_BONES>(a); }

__device__ __forceinline__ float vae_alpha(const VaeState* st, float lr) {
#pragma clang fp contract(off)
  return lr * sqrtf(1.0f - st->b2p) / (1.0f - st->b1p);
}
__device__ __forceinline__ void vae_advance(VaeState* st) {
  st->b1p = st->b1p * 0.9f;
  st->b2p = st->b2p * 0.999f;
  st->step = st->step + 1;
}

// Keras Adam (TF2's fused ResourceApplyAdam, every operation rounded on its own: p3d_adam1) on
// flat element e with gradient g, and the updated weight into the packed copy.
__device__ __forceinline__ void vae_adam_elem(const VaeArgs& a, const VaeDesc* d, int e, float g, float alpha) {
  float w1 = a.w[e], m1 = a.m[e], v1 = a.v[e];
  p3d_adam1(w1, m1, v1, g, alpha, 1.0f - 0.9f, 1.0f - 0.999f, 1.0e-7f);
  a.w[e] = w1; a.m[e] = m1; a.v[e] = v1;
  a.pk_out[a.pkidx[e]] = w1;
}

// The same on elements e .. e + 3 of two float4 groups per round (the one-launch tail: one
// workgroup walks the whole parameter set, so the loads of two groups go out together).
__device__ __forceinline__ void vae_adam_tail(const VaeArgs& a, int P, float alpha) {
  for (int e0 = 4 * threadIdx.x; e0 < P; e0 += 2048) {
    const int e1 = e0 + 1024;
    const bool two = e1 < P;
    const int es[2] = {e0, two ? e1 : e0};
    f32x4 g[2], w[2], m[2], v[2];
    int4 ix[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      g[h] = *(const f32x4*)(a.gout + es[h]); w[h] = *(const f32x4*)(a.w + es[h]);
      m[h] = *(const f32x4*)(a.m + es[h]); v[h] = *(const f32x4*)(a.v + es[h]);
      ix[h] = *(const int4*)(a.pkidx + es[h]);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (h == 1 && !two) break;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float w1 = w[h][c], m1 = m[h][c], v1 = v[h][c];
        p3d_adam1(w1, m1, v1, g[h][c], alpha, 1.0f - 0.9f, 1.0f - 0.999f, 1.0e-7f);
        w[h][c] = w1; m[h][c] = m1; v[h][c] = v1;
      }
      *(f32x4*)(a.w + es[h]) = w[h]; *(f32x4*)(a.m + es[h]) = m[h]; *(f32x4*)(a.v + es[h]) = v[h];
      a.pk_out[ix[h].x] = w[h][0]; a.pk_out[ix[h].y] = w[h][1];
      a.pk_out[ix[h].z] = w[h][2]; a.pk_out[ix[h].w] = w[h][3];
    }
  }
}

// loss[j] = factor * (sum over blocks, in block order, of the blocks' row-term sums) / B
__device__ __forceinline__ void vae_loss3(const VaeArgs& a, int j) {
#pragma clang fp contract(off)
  float s = a.lpart[j];
  for (int b = 1; b < a.nblk; ++b) s += a.lpart[4 * b + j];
  a.loss3[j] = (s / (float)a.B) * a.f[j];
}

// The training step: forward, the three loss terms, backward to every parameter's gradient and --
// in the one-workgroup form (nblk == 1, a.adam) -- Adam and the new packed copy.
// CAT: the input through a.cat.  DX (the wide form's core, whose input is layer 0's ReLU output):
// the data gradient runs for layer 0 too and goes to a.dx; alpha is always left
// in the state for the layer-0 optimizer behind this launch.
template <bool CAT, bool DX, int KIND>
__device__ __forceinline__ void vae_step_body(const VaeArgs& a) {
  constexpr int NTERM = KIND == P3D_VAE_KIND_BONES ? 4 : 3;
  extern __shared__ f32x4 vae_smem[];
  float* sm = (float*)vae_smem;
  const VaeDesc* d = a.desc;
  vae_load_params(a, d, sm);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, q = lane >> 4;
  float* act0 = sm + d->Ppk;
  float* act = act0 + wave * d->act;
  float* rt = sm + d->Ppk + 4 * d->act;   // [64][4] row terms of the block
  const uint64_t ctr = a.ctr_dev ? (uint64_t)a.ctr_dev->step : a.ctr;
  float alpha = 0.0f;
  if (a.adam) {
    alpha = vae_alpha(a.st, a.lr);
    if ((DX || !a.tail) && blockIdx.x == 0 && tid == 0) a.st->alpha = alpha;   // for k_vae_reduce_adam
  }
  const int nl = d->nl;
  for (int blk = blockIdx.x; blk < a.nblk; blk += gridDim.x) {
    const int64_t row0 = (int64_t)blk * 64 + wave * 16;
    float terms[4];
    vae_tile_fwd<CAT, KIND>(a, d, sm, act, row0, ctr, a.backward != 0, terms);
    if (lane < 16) {
      const bool valid = row0 + i < a.B;
#pragma unroll
      for (int j = 0; j < NTERM; ++j) rt[(wave * 16 + i) * 4 + j] = valid ? terms[j] : 0.0f;
    }
    __syncthreads();
    if (tid < NTERM) {   // the block's row-term sums, rows in order
      float s = rt[tid];
      for (int r = 1; r < 64; ++r) s += rt[4 * r + tid];
      a.lpart[4 * blk + tid] = s;
    }
    __syncthreads();   // (the next block's row terms overwrite rt)
    if (a.backward) {
      float* g = a.gout + (int64_t)blk * d->P;
      for (int l = nl - 1; l >= 0; --l) {
        const VaeLayer& L = d->L[l];
        // ---- dW = act^T dz over the block's 64 rows: one chain per output tile ----
        const int KT = (L.K + 15) >> 4, NT = L.Np >> 4;
        for (int tl = wave; tl < KT * NT; tl += 4) {
          const int kt = tl / NT, nt = tl - kt * NT;
          const int kc = 16 * kt + i;
          f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
          for (int t = 0; t < 4; ++t) {
            const float* zt = act0 + t * d->act + L.aout;
            if (L.ain < 0) {   // layer 0 with x in global memory
#pragma unroll
              for (int s = 0; s < 4; ++s) {
                int64_t row = (int64_t)blk * 64 + 16 * t + 4 * s + q;
                row = row < a.B ? row : a.B - 1;   // (dz is zero on rows past B)
                const int xc = kc < L.K ? kc : L.K - 1;
                const float xv = CAT ? *vae_cat_at(a.cat, row, xc) : a.x[row * d->in + xc];
                const float av = kc < L.K ? xv : 0.0f;
                acc =__builtin_amdgcn_mfma_f32_16x16x4f32(av, zt[(4 * s + q) * L.ldo + 16 * nt + i], acc, 0, 0, 0);
              }
            } else {
              const float* at = act0 + t * d->act + L.ain;
#pragma unroll
              for (int s = 0; s < 4; ++s)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(at[(4 * s + q) * L.lda + kc],
                                                           zt[(4 * s + q) * L.ldo + 16 * nt + i], acc, 0, 0, 0);
            }
          }
          const int n = 16 * nt + i;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = 16 * kt + 4 * q + r;
            if (k < L.K && n < L.N) {
              if (n < L.split) g[L.fw + k * L.split + n] = acc[r];
              else g[L.fw2 + k * (L.N - L.split) + (n - L.split)] = acc[r];
            }
          }
        }
        // ---- db = sum over the 64 rows, in row order ----
        if (tid < L.N) {
          float s = 0.0f;
          for (int t = 0; t < 4; ++t) {
            const float* zt = act0 + t * d->act + L.aout;
            for (int r = 0; r < 16; ++r) s += zt[r * L.ldo + tid];
          }
          if (tid < L.split) g[L.fb + tid] = s;
          else g[L.fb2 + (tid - L.split)] = s;
        }
        __syncthreads();   // every wave is done with this layer's input activations
        if (l > 0) {
          // ---- da = dz W^T, then dz of the layer below in place of the activation ----
          const bool to_head = l == d->head + 1;
          const float* dz = act + L.aout;
          const int KTp = (L.K + 15) >> 4;
          for (int kt = 0; kt < KTp; ++kt) {
            const int kc = 16 * kt + i;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* ap = dz + i * L.ldo + q;
            // (rows of W past K read row K - 1 and are replaced by zero: no MFMA under a lane mask)
            const float* wp = sm + L.wpk + (kc < L.K ? kc : L.K - 1) * L.ld + q;
            const bool inK = kc < L.K;
            const int N = L.N;
            for (int n = 0; n < N; n += 8) {
              const float a0 = ap[n], w0 = wp[n], a1 = ap[n + 4], w1 = wp[n + 4];
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, inK ? w0 : 0.0f, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, inK ? w1 : 0.0f, acc, 0, 0, 0);
            }
            if (to_head) {   // through z = eps std + mean, plus the KL term's own gradient
#pragma clang fp contract(off)
              const VaeLayer& H = d->L[d->head];
              float* ml = act + H.aout;
              const float* eb = act + d->ebuf;
              if (kc < d->latent) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const int row = 4 * q + r;
                  const float ck = row0 + row < a.B ? a.c_kl : 0.0f;
                  const float mu = ml[row * H.ldo + kc], lv = ml[row * H.ldo + d->latent + kc];
                  ml[row * H.ldo + kc] = acc[r] + ck * mu;
                  ml[row * H.ldo + d->latent + kc] = acc[r] * eb[row * d->lde + kc] + ck * (0.5f * (expf(lv) - 1.0f));
                }
              }
            } else {
              float* ab = act + L.ain;
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = 4 * q + r;
                const float av = ab[row * L.lda + kc];
                ab[row * L.lda + kc] = acc[r] * (av > 0.0f ? 1.0f : 0.0f);   // a product (ReluGrad): a NaN gradient stays NaN
              }
            }
          }
          __syncthreads();   // every wave's dz of the layer below is written
        }
      }
      if (DX) {   // layer 0's da = dz W^T (the loop's own data-gradient arithmetic) leaves for the layer-0 weight gradient
        const VaeLayer& L = d->L[0];
        const float* ap = act + L.aout + i * L.ldo + q;
        const int N = L.N, din = d->in;
        for (int kt = 0; kt < ((L.K + 15) >> 4); ++kt) {
          const int kc = 16 * kt + i;
          const bool inK = kc < L.K;
          const float* wp = sm + L.wpk + (inK ? kc : L.K - 1) * L.ld + q;
          f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
          for (int n = 0; n < N; n += 8) {
            const float a0 = ap[n], w0 = wp[n], a1 = ap[n + 4], w1 = wp[n + 4];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, inK ? w0 : 0.0f, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, inK ? w1 : 0.0f, acc, 0, 0, 0);
          }
          if (inK) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int64_t grow = row0 + 4 * q + r;
              if (grow < a.B) a.dx[grow * din + kc] = acc[r];
            }
          }
        }
        __syncthreads();   // (the next block's forward overwrites the activations)
      }
    }
  }
  if (a.tail) {   // one-launch forms: the loss, and the optimizer behind the gradient
    if (a.backward && a.adam) {
      vae_adam_tail(a, d->P, alpha);
    }
    if (tid < NTERM) vae_loss3(a, tid);
    if (a.backward && a.adam) {
      __syncthreads();   // every thread has formed alpha from the old state
      if (tid == 0) vae_advance(a.st);
    }
  }
}
__global__ __launch_bounds__(256) void k_vae_step(VaeArgs a) { vae_step_body<false, false, P3D_VAE_KIND_ELBO>(a); }
__global__ __launch_bounds__(256) void k_vae_step_cat(VaeArgs a) { vae_step_body<true, false, P3D_VAE_KIND_ELBO>(a); }
__global__ __launch_bounds__(256) void k_vae_step_dx(VaeArgs a) { vae_step_body<false, true, P3D_VAE_KIND_ELBO>(a); }
__global__ __launch_bounds__(256) void k_vae_bones_step(VaeArgs a) { vae_step_body<false, false, P3D_VAE_KIND_BONES>(a); }
__global__ __launch_bounds__(256) void k_vae_bones_step_cat(VaeArgs a) { vae_step_body<true, false, P3D_VAE_KIND_BONES>(a); }
__global__ __launch_bounds__(256) void k_vae_bones_step_dx(VaeArgs a) { vae_step_body<false, true, P3D_VAE_KIND_BONES>(a); }

// B > 64: block partials summed in block order into the gradient buffer, then Adam.  Also the
// stand-alone optimizer over the gradient buffer (nblk == 1, partials == the buffer itself).
__global__ __launch_bounds__(256) void k_vae_reduce_adam(VaeArgs a, float* __restrict__ grads) {
  const VaeDesc* d = a.desc;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (a.backward && e < d->P) {
    float g = a.gout[e];
    for (int b = 1; b < a.nblk; ++b) g += a.gout[(int64_t)b * d->P + e];
    grads[e] = g;
    if (a.adam) vae_adam_elem(a, d, e, g, a.st->alpha);
  }
  if (blockIdx.x == 0) {
    if (a.loss3 && threadIdx.x < a.nterm) vae_loss3(a, threadIdx.x);
    if (a.adam && threadIdx.x == 0) vae_advance(a.st);   // (nothing in this launch reads the beta powers)
  }
}

__global__ void k_vae_alpha(VaeState* st, float lr) { st->alpha = vae_alpha(st, lr); }

// The packed copy from the masters (after a host write): pad columns and rows are zero.
__global__ __launch_bounds__(256) void k_vae_pack(int P, const int* __restrict__ pkidx, const float* __restrict__ params,
                                                  float* __restrict__ pk) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < P) pk[pkidx[e]] = params[e];
}
