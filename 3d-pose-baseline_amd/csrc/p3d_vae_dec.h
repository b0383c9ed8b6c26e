// p3d_vae_dec.h -- the VAE filters' decoder on its own (gfx950): VAE.decode of
// src/top_vae_3d_pose/models.py:74-76, and poses drawn from the prior (z ~ N(0, I), the commented
// gen_sample of models.py:55-59).  Device code only; the host side is in p3d_vae_host.h.
//
// vae_layout packs the layers in order, so the decoder's parameters -- layers head + 1 .. nl - 1 --
// are ONE contiguous range of the packed copy, from L[head + 1].wpk to Ppk.  Only that range goes
// into LDS (the default filter: 4736 of 8960 packed floats), and behind it come four per-wave areas
// that hold nothing but the z tile and the decoder's activations.  The host describes this in a
// decoder-only VaeDesc (p3d_vae_layout.h vae_dec_layout: wpk / bpk rebased to the range, ain / aout into the
// shrunk area) that lives on the device beside the full one.
//
// A wave runs a 16-row tile through the decoder with vae_layer_fwd itself, layers and k-steps in
// the forward's order on the same packed weights: y is bit-identical to the y p3d_vae_forward
// writes for the same z.  Waves stride over the tiles on their own, as in vae_fwd_body.
//
// z comes from global memory, or (a.z null) from the PRIOR stream: vae_eps4_site over the site
// P3D_VAE_PRIOR_SITE at the global row a.row0 + r -- a site of its own, so a sample is never the
// eps a training step draws at the same (seed, ctr, row).
#pragma once
#include "p3d_vae.h"

#define P3D_VAE_PRIOR_SITE 0x505249   // Philox site id of the prior stream ("PRI"; eps 0x564145, noise 0x4E4F49 / 0x4E4F52)

struct VaeDecArgs {
  const VaeDesc* desc;    // the decoder-only descriptor
  const float* pk;        // the packed copy at the decoder's range [desc->Ppk]
  const float* z;         // [B, latent] or null (draw from the prior stream)
  int64_t B, row0;        // row r of this call is row row0 + r of the prior stream
  uint64_t seed, ctr;
  float* y;               // [B, out]
  float* z_out;           // [B, latent] or null: the drawn z
};

template <int KIND>
__device__ __forceinline__ void vae_dec_body(const VaeDecArgs& a) {
  extern __shared__ f32x4 vae_smem[];
  float* sm = (float*)vae_smem;
  const VaeDesc* d = a.desc;
  const int lat = d->latent, ldz = d->ldz;
  const int out = KIND == P3D_VAE_KIND_BONES ? 64 : d->out;
  // the decoder's parameters into LDS, the z buffers' pad columns zeroed
  for (int idx = threadIdx.x; idx < (d->Ppk >> 2); idx += 256) ((f32x4*)sm)[idx] = ((const f32x4*)a.pk)[idx];
  const int zp = ldz - lat;
  for (int idx = threadIdx.x; idx < 4 * 16 * zp; idx += 256) {
    const int w = idx / (16 * zp), rem = idx - w * 16 * zp, r = rem / zp, c = rem - r * zp;
    sm[d->Ppk + w * d->act + d->zbuf + r * ldz + lat + c] = 0.0f;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15;
  float* act = sm + d->Ppk + wave * d->act;
  float* zb = act + d->zbuf;
  const int64_t Bm1 = a.B - 1;
  const int64_t ntiles = (a.B + 15) >> 4;
  const int c4n = lat >> 2;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row0 = tile * 16;
    // ---- the z tile (rows past B repeat the last row) ----
    for (int u = lane; u < 16 * c4n; u += 64) {
      const int r = u / c4n, c4 = u - r * c4n;
      const bool valid = row0 + r < a.B;
      const int64_t grow = valid ? row0 + r : Bm1;
      float e[4];
      if (a.z) {
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = a.z[grow * lat + 4 * c4 + j];
      } else {
        vae_eps4_site(a.seed, a.ctr, (uint32_t)P3D_VAE_PRIOR_SITE, a.row0 + grow, c4, e);
        if (valid && a.z_out) {
#pragma unroll
          for (int j = 0; j < 4; ++j) a.z_out[grow * lat + 4 * c4 + j] = e[j];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) zb[r * ldz + 4 * c4 + j] = e[j];
    }
    vae_wsync();
    // ---- decoder: the forward's own layer function, layers in order ----
    for (int l = d->head + 1; l < d->nl; ++l) {
      const VaeLayer& L = d->L[l];
      vae_layer_fwd(L, act + L.ain + i * L.lda, sm, act + L.aout);
      vae_wsync();
    }
    const float* yb = act + d->L[d->nl - 1].aout;
    const int ldy = d->L[d->nl - 1].ldo;
    for (int idx = lane; idx < 16 * out; idx += 64) {
      const int r = idx / out, c = idx - r * out;
      if (row0 + r < a.B) a.y[(row0 + r) * out + c] = yb[r * ldy + c];
    }
    vae_wsync();   // (the next tile's z and activations overwrite this one's)
  }
}
__global__ __launch_bounds__(256) void k_vae_dec(VaeDecArgs a) { vae_dec_body<P3D_VAE_KIND_ELBO>(a); }
__global__ __launch_bounds__(256) void k_vae_bones_dec(VaeDecArgs a) { vae_dec_body<P3D_VAE_KIND_BONES>(a); }
