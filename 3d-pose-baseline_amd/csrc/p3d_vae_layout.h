// p3d_vae_layout.h -- everything p3d_vae_create derives from a filter's shape without a device: the
// shape checks, the LDS layouts (full, decoder-only, sequence), the parameter table, the workspace
// size, and the list of the built VAE kernels with its index.  Host-only (no HIP header): all of it
// is a pure function of the shape, so it compiles and is tested on its own
// (tests/host/vae_plan_main.cpp, tests/test_vae_plan.py).  A refusal comes back as a status and its
// text; p3d_vae_host.h hands them to fail() and attaches the kernel pointers to the list.
// Every function is static: the unity build's library exports none of them.
#pragma once
#include "p3d_vae_desc.h"
#include "../../include/p3d.h"
#include <string>
#include <vector>

// ---- the built kernels, each written down once: X(kernel, family, kind, cat, dx, waves, lds) ----
// family: the forward, the loss / gradient / training step, the decoder alone, the sequence filter,
// and the forward and the sequence filter averaged over K samples (p3d_vae_mc.h).
// cat: the input comes through a VaeCat; dx: the wide form's core, which also leaves d loss / d input;
// waves per workgroup; lds: which of a plan's sizes is the launch's dynamic LDS.
enum VaeFamily { VF_FWD, VF_STEP, VF_DEC, VF_SEQ, VF_FWDMC, VF_SEQMC };
enum VaeLdsOf { VL_FULL, VL_DEC, VL_SEQ };
#define P3D_VAE_KERNELS(X)                                                                      \
  X(k_vae_fwd, FWD, ELBO, 0, 0, 4, FULL) X(k_vae_fwd_cat, FWD, ELBO, 1, 0, 4, FULL)             \
  X(k_vae_bones_fwd, FWD, BONES, 0, 0, 4, FULL) X(k_vae_bones_fwd_cat, FWD, BONES, 1, 0, 4, FULL) \
  X(k_vae_step, STEP, ELBO, 0, 0, 4, FULL) X(k_vae_step_cat, STEP, ELBO, 1, 0, 4, FULL)         \
  X(k_vae_step_dx, STEP, ELBO, 0, 1, 4, FULL)                                                   \
  X(k_vae_bones_step, STEP, BONES, 0, 0, 4, FULL) X(k_vae_bones_step_cat, STEP, BONES, 1, 0, 4, FULL) \
  X(k_vae_bones_step_dx, STEP, BONES, 0, 1, 4, FULL)                                            \
  X(k_vae_dec, DEC, ELBO, 0, 0, 4, DEC) X(k_vae_bones_dec, DEC, BONES, 0, 0, 4, DEC)            \
  X(k_vae_seq, SEQ, ELBO, 0, 0, 1, SEQ) X(k_vae_seq4, SEQ, ELBO, 0, 0, 4, SEQ)                \
  X(k_vae_fwd_mc, FWDMC, ELBO, 0, 0, 4, FULL) X(k_vae_fwd_mc_cat, FWDMC, ELBO, 1, 0, 4, FULL)   \
  X(k_vae_seq4_mc, SEQMC, ELBO, 0, 0, 4, SEQ)

struct VaeKernelRow {
  const char* name;
  int family, kind, cat, dx, waves, lds;
};
#define P3D_VAE_KERNEL_ROW(NAME, FAMILY, KIND, CAT, DX, WAVES, LDS) \
  {#NAME, VF_##FAMILY, P3D_VAE_KIND_##KIND, CAT, DX, WAVES, VL_##LDS},
constexpr VaeKernelRow kVaeKernels[] = {P3D_VAE_KERNELS(P3D_VAE_KERNEL_ROW)};
#undef P3D_VAE_KERNEL_ROW
constexpr int kVaeKernelCount = (int)(sizeof(kVaeKernels) / sizeof(kVaeKernels[0]));

// A kernel's row in the list, by arithmetic (a batch-64 step is launch-bound: no search per call).
static constexpr int vae_kernel_index(int family, int kind, int cat, int dx, int waves) {
  return family == VF_FWD ? 2 * kind + cat
       : family == VF_STEP ? 4 + 3 * kind + (dx ? 2 : cat)
       : family == VF_DEC ? 10 + kind
       : family == VF_SEQ ? 12 + (waves == 4)
       : family == VF_FWDMC ? 14 + cat
                            : 16;
}
static constexpr bool vae_kernels_in_index_order() {
  for (int i = 0; i < kVaeKernelCount; ++i) {
    const VaeKernelRow& k = kVaeKernels[i];
    if (vae_kernel_index(k.family, k.kind, k.cat, k.dx, k.waves) != i) return false;
  }
  return true;
}
static_assert(kVaeKernelCount == 17 && vae_kernels_in_index_order(), "P3D_VAE_KERNELS is not in vae_kernel_index's order");

// ---- the shape ----------------------------------------------------------------------------------
struct VaeShape {
  int kind = P3D_VAE_KIND_ELBO;
  int in = 0, n_enc = 0, enc[4] = {}, latent = 0, n_dec = 0, dec[4] = {}, out = 0;
};

// p3d_vae_create's arguments checked and gathered into `s`; else P3D_ERR_ARG and the text.
static inline int vae_check_shape(int kind, int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent, int32_t n_dec,
                           const int32_t* dec_dims, int32_t out, VaeShape& s, std::string& err) {
  const auto refuse = [&](const char* msg) { err = msg; return P3D_ERR_ARG; };
  if (!enc_dims || !dec_dims) return refuse("p3d_vae_create: null argument");
  auto width = [](int w, int hi) { return w >= 8 && w <= hi && w % 8 == 0; };
  if (!width(in, 2048)) return refuse("p3d_vae_create: in must be a multiple of 8 in 8 .. 2048");
  if (n_enc < 1 || n_enc > 4 || n_dec < 1 || n_dec > 4) return refuse("p3d_vae_create: 1 to 4 hidden layers on each side");
  for (int e = 0; e < n_enc + n_dec; ++e)
    if (!width(e < n_enc ? enc_dims[e] : dec_dims[e - n_enc], 256))
      return refuse("p3d_vae_create: hidden widths must be multiples of 8 in 8 .. 256");
  if (!width(latent, 64)) return refuse("p3d_vae_create: latent must be a multiple of 8 in 8 .. 64");
  if (!width(out, 64)) return refuse("p3d_vae_create: out must be a multiple of 8 in 8 .. 64");
  s = VaeShape{};
  s.kind = kind; s.in = in; s.n_enc = n_enc; s.latent = latent; s.n_dec = n_dec; s.out = out;
  for (int e = 0; e < n_enc; ++e) s.enc[e] = enc_dims[e];
  for (int e = 0; e < n_dec; ++e) s.dec[e] = dec_dims[e];
  return P3D_OK;
}

// ---- the layouts ----------------------------------------------------------------------------------
static inline int vae_ceil16(int n) { return (n + 15) / 16 * 16; }

// The layout of a narrow filter (or a wide one's core): layers, the packed copy, a wave's LDS area,
// the master tensors.  wpad = 4 staggers the packed rows over the LDS banks for the data-gradient
// reads; 0 is the fall-back when that does not fit; stage_x keeps the 16-row input tile in LDS too
// (else layer 0 reads x from global memory).  kind = bones: behind the dec_dim layers come mag1 (16,
// ReLU) and one packed output layer [16, 64] = {mag2 | cos2} (models.py:555-566; cos1 is not
// reachable from the decoder's outputs and is not part of the model).  The checked shape bounds the
// arrays: at most 4 + 1 + 4 + 2 = P3D_VAE_MAX_L layers and 8 + 4 + 10 + 4 = P3D_VAE_MAX_T tensors.
// Returns the dynamic LDS bytes.
static inline size_t vae_layout(VaeDesc& d, std::vector<std::string>& names, const VaeShape& s, int wpad, int stage_x) {
  d = VaeDesc{};
  names.clear();
  d.in = s.in; d.latent = s.latent; d.out = s.out;
  int pk = 0, act = 0, flat = 0, prev = s.in;
  auto tensor = [&](const std::string& name, int K, int N, int pkoff, int ld) {
    d.T[d.nt++] = VaeTensor{flat, K, N, pkoff, ld};
    names.push_back(name);
    flat += K * N;
    return flat - K * N;
  };
  // a dense layer on `prev`: its packed weight and bias, its output tile and its master tensors --
  // `name`'s kernel and bias, or two layers side by side (columns < split `name`'s, the rest `name2`'s)
  auto dense = [&](const std::string& name, int N, int relu, int split = 0, const char* name2 = "") {
    VaeLayer& L = d.L[d.nl++];
    L.K = prev; L.N = N; L.Np = vae_ceil16(N); L.ld = L.Np + wpad; L.relu = relu;
    L.wpk = pk; pk += L.K * L.ld;
    L.bpk = pk; pk += L.Np;
    L.aout = act; L.ldo = L.Np + 2; act += 16 * L.ldo;
    L.split = split ? split : N;
    L.fw = tensor(name + "/kernel", L.K, L.split, L.wpk, L.ld);
    L.fb = tensor(name + "/bias", 1, L.split, L.bpk, L.Np);
    if (split) {
      L.fw2 = tensor(std::string(name2) + "/kernel", L.K, N - split, L.wpk + split, L.ld);
      L.fb2 = tensor(std::string(name2) + "/bias", 1, N - split, L.bpk + split, L.Np);
    }
    prev = N;
  };
  for (int e = 0; e < s.n_enc; ++e) dense("enc_h_" + std::to_string(s.enc[e]), s.enc[e], 1);
  d.head = d.nl;
  dense("mean", 2 * s.latent, 0, s.latent, "log_varianze");
  prev = s.latent;
  for (int e = 0; e < s.n_dec; ++e) dense("dec_f_" + std::to_string(s.dec[e]), s.dec[e], 1);
  const bool bones = s.kind == P3D_VAE_KIND_BONES;
  if (bones) {   // mag1, then mag2 (16) and cos2 (48), both on mag1's output: one packed layer split like the head
    dense("mag1", 16, 1);
    dense("mag2", 64, 0, 16, "cos2");
  } else {
    dense("dec_f_out", s.out, 0);
  }
  d.ldz = vae_ceil16(s.latent) + 2; d.zbuf = act; act += 16 * d.ldz;
  d.lde = d.ldz; d.ebuf = act; act += 16 * d.lde;
  d.ldb = 50; d.bt = act;
  if (s.out == 48 || bones) act += 16 * d.ldb;   // (bones: the 48 target cosines of the ANG term)
  d.ldx = vae_ceil16(s.in) + 2; d.xbuf = -1;
  if (stage_x) { d.xbuf = act; act += 16 * d.ldx; }
  for (int l = 0; l < d.nl; ++l) {
    VaeLayer& L = d.L[l];
    if (l == 0) { L.ain = d.xbuf; L.lda = d.xbuf >= 0 ? d.ldx : s.in; }
    else if (l == d.head + 1) { L.ain = d.zbuf; L.lda = d.ldz; }
    else { L.ain = d.L[l - 1].aout; L.lda = d.L[l - 1].ldo; }
  }
  d.P = flat;
  d.Ppk = (pk + 3) / 4 * 4;
  d.act = (act + 3) / 4 * 4;
  return sizeof(float) * ((size_t)d.Ppk + 4 * (size_t)d.act + 64 * 4);
}

// The sequence filter's LDS behind the packed copy (float offsets): ONE tile's activation area, the
// [16, in] state tile (the area's own input tile where the layout stages one), the frame's target
// tile and the 16 rows' first frame (int64) and frame count (int).  Returns the dynamic LDS bytes.
static inline size_t vae_seq_layout(const VaeDesc& d, int& xoff, int& toff, int& ldt, int& moff) {
  int act = d.act;
  xoff = d.xbuf;
  if (xoff < 0) { xoff = act; act += (16 * d.ldx + 3) / 4 * 4; }
  ldt = vae_ceil16(d.out) + 2;
  toff = act; act += 16 * ldt;
  moff = act; act += 16 * 2 + 16;   // (act stays a multiple of 4: the int64 offsets are aligned)
  return sizeof(float) * ((size_t)d.Ppk + (size_t)act);
}

// The decoder-only descriptor of a laid-out filter: the packed range of layers head + 1 .. nl - 1
// (`base` floats into the packed copy; vae_layout packs the layers in order, which is checked here)
// with wpk / bpk rebased to it, and a wave's area shrunk to the z tile and the decoder's
// activations.  Returns the dynamic LDS bytes of k_vae_dec, 0 if the range is not contiguous.
static inline size_t vae_dec_layout(const VaeDesc& full, VaeDesc& dd, int& base) {
  dd = full;
  base = full.L[full.head + 1].wpk;
  int pk = base, act = 0;
  dd.zbuf = act; act += 16 * dd.ldz;
  dd.ebuf = dd.bt = dd.xbuf = -1;
  for (int l = 0; l <= full.head; ++l) dd.L[l] = VaeLayer{};
  for (int l = full.head + 1; l < full.nl; ++l) {
    VaeLayer& L = dd.L[l];
    if (L.wpk != pk || L.bpk != pk + L.K * L.ld) return 0;
    pk = L.bpk + L.Np;
    L.wpk -= base; L.bpk -= base;
    L.ain = l == full.head + 1 ? dd.zbuf : dd.L[l - 1].aout;
    L.lda = l == full.head + 1 ? dd.ldz : dd.L[l - 1].ldo;
    L.aout = act; act += 16 * L.ldo;
  }
  if ((pk + 3) / 4 * 4 != full.Ppk || base % 4 != 0) return 0;
  dd.Ppk = full.Ppk - base;
  dd.act = (act + 3) / 4 * 4;
  return sizeof(float) * ((size_t)dd.Ppk + 4 * (size_t)dd.act);
}

// p3d_vae_dec_lds_bytes' answer: the decoder's layout behind a dummy encoder (the decoder's layout
// does not depend on the encoder) at the FIRST layout's (wpad, stage_x) = (4, 1), whatever a real
// filter of these widths would get -- one that only fits unstaggered (wpad = 0) has a smaller
// dec_lds in its plan than this answers.  0 above the limit.
static inline size_t vae_dec_bytes_staggered(VaeShape s) {
  s.in = 8; s.n_enc = 1; s.enc[0] = 8;
  VaeDesc d, dd;
  std::vector<std::string> names;
  int base;
  vae_layout(d, names, s, 4, 1);
  const size_t lds = vae_dec_layout(d, dd, base);
  return lds <= P3D_VAE_LDS_LIMIT ? lds : 0;
}

// flat element of the (core's) master buffers -> its place in the packed copy
static inline std::vector<int> vae_pack_index(const VaeDesc& d) {
  std::vector<int> idx((size_t)d.P);
  for (int t = 0; t < d.nt; ++t) {
    const VaeTensor& T = d.T[t];
    for (int k = 0; k < T.K; ++k)
      for (int n = 0; n < T.N; ++n) idx[(size_t)T.flat + (size_t)k * T.N + n] = T.pk + k * T.ld + n;
  }
  return idx;
}

// ---- the plan -------------------------------------------------------------------------------------
struct VaePlan {
  VaeShape shape;
  // Narrow (in <= 256): `desc` is the filter.  Wide (kernels in p3d_vae_wide.h): `desc` is the core
  // -- the filter behind layer 0, whose input is h0 [B, n0] -- and layer 0 (P0 = (in + 1) n0 floats)
  // leads the flat buffers; the core's tensors follow at flat + P0.  Narrow: P0 = 0, Ptot = desc.P.
  VaeDesc desc{};
  int wide = 0, n0 = 0, P0 = 0, Ptot = 0;
  std::vector<std::string> names;   // Keras order; tensor i is tensors[i]
  std::vector<VaeTensor> tensors;   // the full parameter table (flat offsets into the master buffers)
  size_t lds = 0;                   // dynamic LDS bytes of the forward and step kernels
  // the decoder on its own: its descriptor, the float offset of its parameters in the packed copy,
  // its dynamic LDS and the default workgroups per CU
  VaeDesc dec{};
  int dec_base = 0, dec_wgs = 0;
  size_t dec_lds = 0;
  // the sequence filter: seq_lds = 0 where this shape has none
  int seq_len = 0, seq_xoff = 0, seq_toff = 0, seq_ldt = 0, seq_moff = 0;
  size_t seq_lds = 0;

  // The workspace for up to B rows, in floats: per 64-row block the core's partial gradient and four
  // loss sums, four more floats, and (wide) h0 and dz0 [B, n0] behind them at offsets that are
  // multiples of 4.
  int64_t h0_off(int64_t B) const { return (B + 63) / 64 * ((int64_t)desc.P + 4) + 4; }
  int64_t ws_floats(int64_t B) const { return h0_off(B) + (wide ? 2 * B * n0 : 0); }
};

// Everything above for a checked shape.  The plan is filled whatever the answer (the *_lds_bytes
// calls read the sizes of shapes p3d_vae_create refuses); the refusals, in the order they answer:
// no layout fits the LDS limit, the decoder is not one range of the packed copy, two layers share a
// name.
static inline int vae_plan(const VaeShape& s, VaePlan& p, std::string& err) {
  p = VaePlan{};
  p.shape = s;
  p.wide = s.in > 256;
  p.n0 = s.enc[0];
  VaeShape core = s;
  if (p.wide) {   // the core: layer 0's output is its input
    core.in = s.enc[0];
    core.n_enc = s.n_enc - 1;
    for (int e = 0; e < core.n_enc; ++e) core.enc[e] = s.enc[e + 1];
    p.P0 = (s.in + 1) * s.enc[0];
    const std::string n = "enc_h_" + std::to_string(s.enc[0]);
    p.names = {n + "/kernel", n + "/bias"};
    p.tensors = {VaeTensor{0, s.in, s.enc[0], -1, 0}, VaeTensor{s.in * s.enc[0], 1, s.enc[0], -1, 0}};
  }
  // the roomiest layout that fits one workgroup's LDS (else the last one's size, over the limit)
  std::vector<std::string> names;
  const int tries[3][2] = {{4, 1}, {4, 0}, {0, 0}};
  for (auto& t : tries) {
    p.lds = vae_layout(p.desc, names, core, t[0], t[1]);
    if (p.lds <= P3D_VAE_LDS_LIMIT) break;
  }
  p.names.insert(p.names.end(), names.begin(), names.end());
  for (int t = 0; t < p.desc.nt; ++t) {
    VaeTensor T = p.desc.T[t];
    T.flat += p.P0;
    p.tensors.push_back(T);
  }
  p.Ptot = p.P0 + p.desc.P;
  p.dec_lds = vae_dec_layout(p.desc, p.dec, p.dec_base);
  const int fit = (int)(P3D_VAE_LDS_LIMIT / (p.dec_lds ? p.dec_lds : 1));   // as many as a CU's LDS holds,
  p.dec_wgs = fit < 1 ? 1 : (fit > 4 ? 4 : fit);                            // four at the most
  if (p.lds <= P3D_VAE_LDS_LIMIT && s.kind == P3D_VAE_KIND_ELBO && !p.wide && s.in % s.out == 0 &&
      s.in / s.out <= P3D_VAE_SEQ_MAX_LEN) {
    const size_t sl = vae_seq_layout(p.desc, p.seq_xoff, p.seq_toff, p.seq_ldt, p.seq_moff);
    if (sl <= P3D_VAE_LDS_LIMIT) { p.seq_len = s.in / s.out; p.seq_lds = sl; }
  }
  if (p.lds > P3D_VAE_LDS_LIMIT) {
    err = "p3d_vae_create: parameters and working space need " + std::to_string(p.lds) +
          " bytes of LDS, a workgroup has " + std::to_string(P3D_VAE_LDS_LIMIT);
    return P3D_ERR_ARG;
  }
  if (!p.dec_lds || p.dec_lds > p.lds) {
    err = "p3d_vae_create: the decoder's parameters are not one range of the packed copy";
    return P3D_ERR_STATE;
  }
  for (size_t i = 0; i < p.names.size(); ++i)
    for (size_t j = 0; j < i; ++j)
      if (p.names[i] == p.names[j]) {   // keras: "All layers added to a Model must have unique names"
        err = "p3d_vae_create: two layers of one side share the width in " + p.names[i] +
              " (keras layer names must be unique)";
        return P3D_ERR_ARG;
      }
  return P3D_OK;
}

// ---- the concatenated input -----------------------------------------------------------------------
// A caller's p3d_vae_cat checked against (in, B) and turned into the kernels' form.
static inline int vae_cat_check(const p3d_vae_cat* c, int32_t in, int64_t B, const char* what, VaeCat* out, std::string& err) {
  const std::string w(what);
  const auto refuse = [&](const std::string& msg) { err = w + msg; return P3D_ERR_ARG; };
  if (!c) return refuse(": null argument");
  if (c->n < 1 || c->n > 4) return refuse(": 1 to 4 segments");
  VaeCat k{};
  k.n = c->n;
  int sum = 0;
  for (int s = 0; s < c->n; ++s) {
    if (c->w[s] < 8 || c->w[s] % 8 != 0) return refuse(": segment widths must be multiples of 8");
    if (!c->p[s]) return refuse(": null segment pointer");
    if ((uintptr_t)c->p[s] % 16 != 0) return refuse(": segments must be 16-byte aligned");
    if (c->rows[s] < 1 || c->rows[s] > (INT64_MAX >> 16)) return refuse(": a segment's table needs at least one row");
    if (!c->idx[s] && c->rows[s] < B) return refuse(": a segment without an index needs B rows");
    k.w[s] = c->w[s]; k.off[s] = sum; k.p[s] = c->p[s]; k.idx[s] = c->idx[s]; k.rows[s] = c->rows[s];
    sum += c->w[s];
    if (sum > 2048) break;
  }
  if (in >= 0 && sum != in)   // (in < 0: no filter to compare with)
    return refuse(": segment widths must sum to in (" + std::to_string(in) + ")");
  if (out) *out = k;
  return P3D_OK;
}
