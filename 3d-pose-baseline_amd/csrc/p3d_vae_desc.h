// p3d_vae_desc.h -- the plain data the VAE filter's kernels take and its host side fills: limits,
// the descriptor of a laid-out filter, the step state and the concatenated input.  No HIP header:
// p3d_vae_layout.h plans over these without a device, p3d_vae.h and p3d_vae_seq.h read them on one.
// The structs are kernel arguments (or live in device memory): their layouts are fixed.
#pragma once
#include <stdint.h>

#define P3D_VAE_MAX_L 11          // 4 encoder layers + the head + 4 decoder layers (+ mag1) + the output
#define P3D_VAE_MAX_T 26          // kernel + bias of every dense layer (the head and the bones output are two layers)
#define P3D_VAE_KIND_ELBO 0       // y [out] against the joints: likelihood, KCS, KL
#define P3D_VAE_KIND_BONES 1      // y [64] = [mag | cos] against the bones: MAG, COS, KL, ANG (models.py:544-573)
#define P3D_VAE_LDS_LIMIT 163840  // one workgroup's LDS on gfx950
#define P3D_VAE_SEQ_MAX_LEN 5     // the sequence filter's in / out

struct VaeLayer {
  int K, N, Np, ld;      // true dims, N padded to 16, row stride of the packed weight
  int wpk, bpk;          // float offsets in the packed copy
  int ain, lda;          // input activation: float offset in the wave's LDS area (-1: x), row stride
  int aout, ldo;         // output activation (and, in the backward, this layer's dz)
  int relu;
  int fw, fb;            // flat (master) offsets of kernel and bias
  int split, fw2, fb2;   // columns >= split belong to a second tensor (the head's log_varianze)
};
struct VaeTensor { int flat, K, N, pk, ld; };   // master tensor [K, N] <-> packed copy
struct VaeDesc {
  int nl, head, in, latent, out, P, Ppk, act, nt;
  int zbuf, ldz, ebuf, lde, bt, ldb;   // z, 0.5 eps std and the target bones, per wave
  int xbuf, ldx;                       // the input tile staged in LDS (-1: layer 0 reads x from global memory)
  VaeLayer L[P3D_VAE_MAX_L];
  VaeTensor T[P3D_VAE_MAX_T];
};
struct VaeState {          // device-resident step state: a training step replays from a HIP graph
  int64_t step;
  float b1p, b2p;          // beta^(step + 1)
  float alpha;             // the step's lr_t, formed by k_vae_step / k_vae_alpha for k_vae_reduce_adam
  int pad[3];
};

// The input as 1 .. 4 column segments, each a table [rows, w] read at row r or at row idx[r]
// (p3d.h p3d_vae_cat); off[s] = w[0] + .. + w[s - 1].
struct VaeCat {
  int n;
  int w[4], off[4];
  const float* p[4];
  const int64_t* idx[4];
  int64_t rows[4];
};
