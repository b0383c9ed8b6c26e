// p3d_vae_host.h -- the VAE pose filter's host side (include/p3d.h): the handle, create / destroy,
// the launches and every extern "C" entry point of the filter, its noise and its bones.  Host code;
// included by p3d.hip behind p3d_host.h (fail(), LAUNCH_CHECK, HIP_TRY, aligned16).  What needs no device --
// shape checks, layouts, the kernel list -- is p3d_vae_layout.h; the kernels are in p3d_vae*.h and
// p3d_bones.h.
#pragma once
#include "p3d_vae_layout.h"

struct p3d_vae {
  VaePlan plan;                         // everything the shape alone decides
  int max_batch = 0, form = 0, cus = 0;
  uint64_t seed = 0;
  // the sequence filter's form: 1 is the default by measurement (MEASUREMENTS.md §14: 5.5 against
  // 14.6 us per frame step at H3.6M size); the decoder's workgroups per CU
  int seq_form = 1, dec_wgs = 0;
  // device memory: the master buffers [Ptot], the packed copy, the workspace, flat element -> packed
  // copy, the full and the decoder-only descriptor, the step state
  float* params = nullptr; float* grads = nullptr; float* am = nullptr; float* av = nullptr;
  float* pk = nullptr; float* ws = nullptr;
  int* pkidx = nullptr;
  VaeDesc* d_desc = nullptr; VaeDesc* d_dec = nullptr;
  VaeState* st = nullptr;
};

namespace {

// the kernel pointers of P3D_VAE_KERNELS, in its order
#define P3D_VAE_KERNEL_FN(NAME, FAMILY, KIND, CAT, DX, WAVES, LDS) reinterpret_cast<void (*)()>(NAME),
void (*const kVaeKernelFns[])() = {P3D_VAE_KERNELS(P3D_VAE_KERNEL_FN)};
#undef P3D_VAE_KERNEL_FN

// One launch of the list's kernel `idx` (vae_kernel_index) with the dynamic LDS its row names; Args
// is the family's argument struct.
template <class Args>
int vae_launch(const p3d_vae* v, int idx, unsigned grid, void* stream, const Args& a) {
  const VaeKernelRow& k = kVaeKernels[idx];
  const size_t lds[3] = {v->plan.lds, v->plan.dec_lds, v->plan.seq_lds};
  hipLaunchKernelGGL(reinterpret_cast<void (*)(Args)>(kVaeKernelFns[idx]), dim3(grid), dim3(64 * k.waves), lds[k.lds],
                     (hipStream_t)stream, a);
  LAUNCH_CHECK(k.name);
  return P3D_OK;
}

int vae_check_call(const p3d_vae* v, const void* x, int64_t B, const char* what) {
  if (!v || !x) return fail(P3D_ERR_ARG, std::string(what) + ": null argument");
  if (B < 1 || B > (1 << 20)) return fail(P3D_ERR_ARG, std::string(what) + ": B must be in 1 .. 2^20");
  return P3D_OK;
}

VaeArgs vae_args(const p3d_vae* v, const float* x, const float* t, int64_t B, const float* eps, uint64_t ctr) {
  const int P0 = v->plan.P0;
  VaeArgs a{};
  a.desc = v->d_desc; a.pk = v->pk; a.x = x; a.t = t; a.eps = eps; a.B = B;
  a.seed = v->seed; a.ctr = ctr;
  a.ctr_dev = ctr == P3D_CTR_GLOBAL_STEP ? v->st : nullptr;
  a.w = v->params + P0; a.m = v->am + P0; a.v = v->av + P0; a.pk_out = v->pk; a.st = v->st;
  a.pkidx = v->pkidx;
  a.nblk = 1;
  a.nterm = v->plan.shape.kind == P3D_VAE_KIND_BONES ? 4 : 3;
  return a;
}

// The wide form's first launch, h0 = relu(x W0 + b0) over x or the segments; the core then reads h0
// (h0 and dz0 [max_batch, n0] lie behind the core's block partials in the workspace).
int vae_wide_fwd(const p3d_vae* v, const float*& x, const VaeCat*& cat, int64_t B, int adam, VaeWideArgs& wa,
                 hipStream_t st, const char* what) {
  if (B > v->max_batch) return fail(P3D_ERR_ARG, std::string(what) + ": B exceeds max_batch");
  wa.B = B; wa.in = v->plan.shape.in; wa.n0 = v->plan.n0; wa.adam = adam;
  if (cat) wa.cat = *cat;
  else { wa.cat.n = 1; wa.cat.w[0] = wa.in; wa.cat.p[0] = x; wa.cat.rows[0] = B; }   // (x as one segment)
  wa.w0 = v->params; wa.h0 = v->ws + v->plan.h0_off(v->max_batch); wa.dz0 = wa.h0 + (int64_t)v->max_batch * wa.n0;
  wa.g = v->grads; wa.w = v->params; wa.m = v->am; wa.v = v->av; wa.st = v->st;
  const int64_t units = ((B + 15) / 16) * ((wa.n0 + 15) / 16);
  const int64_t nwg = (units + 3) / 4, cap = (int64_t)v->cus * 8;
  hipLaunchKernelGGL(k_vae_wide_fwd, dim3((unsigned)(nwg < cap ? nwg : cap)), dim3(256), 0, st, wa);
  LAUNCH_CHECK("k_vae_wide_fwd");
  x = wa.h0;
  cat = nullptr;
  return P3D_OK;
}

int vae_forward(p3d_vae* v, const float* x, const VaeCat* cat, int64_t B, const float* eps, uint64_t ctr, float* y,
                float* mean, float* log_var, float* z, const float* target, float* row_terms, void* stream,
                const char* what) {
  if ((row_terms != nullptr) != (target != nullptr))
    return fail(P3D_ERR_ARG, std::string(what) + ": row_terms and target go together");
  const hipStream_t st = (hipStream_t)stream;
  VaeWideArgs wa{};
  if (v->plan.wide)
    if (int rc = vae_wide_fwd(v, x, cat, B, 0, wa, st, what)) return rc;
  VaeArgs a = vae_args(v, x, target, B, eps, ctr);
  a.y = y; a.mean = mean; a.log_var = log_var; a.z = z; a.row_terms = row_terms;
  if (cat) a.cat = *cat;
  const int64_t nwg = (B + 63) / 64;
  const int grid = (int)(nwg < v->cus ? nwg : v->cus);
  return vae_launch(v, vae_kernel_index(VF_FWD, v->plan.shape.kind, cat != nullptr, 0, 4), grid, st, a);
}

// loss (backward = 0), gradient (backward = 1) or training step (adam = 1) over B rows; the input
// is x or, where `cat` is set, the concatenated segments
int vae_step(p3d_vae* v, const float* x, const VaeCat* cat, const float* t, int64_t B, const float* eps, uint64_t ctr,
             const float* factors, int backward, int adam, float lr, float* loss3, void* stream,
             const char* what) {
  const VaePlan& p = v->plan;
  if (!t || !factors || !loss3) return fail(P3D_ERR_ARG, std::string(what) + ": null argument");
  if (B > v->max_batch) return fail(P3D_ERR_ARG, std::string(what) + ": B exceeds max_batch");
  const bool bones = p.shape.kind == P3D_VAE_KIND_BONES;
  if (!bones && factors[1] != 0.0f && p.desc.out != 48)
    return fail(P3D_ERR_ARG, std::string(what) + ": the KCS term needs out == 48 (kcs_factor must be 0)");
  const hipStream_t st = (hipStream_t)stream;
  VaeWideArgs wa{};
  if (p.wide)
    if (int rc = vae_wide_fwd(v, x, cat, B, adam, wa, st, what)) return rc;
  VaeArgs a = vae_args(v, x, t, B, eps, ctr);
  if (cat) a.cat = *cat;
  const int nblk = (int)((B + 63) / 64);
  const bool one = nblk == 1 && v->form == 0;
  a.backward = backward; a.adam = adam; a.lr = lr;
  a.nblk = nblk;
  if (bones) {   // factors = {mag, cos, dkl, ang} (losses.py:143-152)
    a.c_like = (float)(2.0 * (double)factors[0] / (16.0 * (double)B));
    a.c_cos = (float)((double)factors[1] / (8.0 * (double)B));
    a.c_kcs = (float)((double)factors[3] / (256.0 * (double)B));
  } else {
    a.c_like = (float)(2.0 * (double)factors[0] / ((double)B * p.desc.out));
    a.c_kcs = (float)((double)factors[1] / (double)B);
  }
  a.c_kl = (float)((double)factors[2] / (double)B);
  for (int j = 0; j < a.nterm; ++j) a.f[j] = factors[j];
  a.lpart = v->ws + (int64_t)nblk * p.desc.P;
  a.loss3 = loss3;
  a.gout = one ? v->grads + p.P0 : v->ws;
  a.tail = one;
  a.dx = const_cast<float*>(wa.dz0);   // (null unless wide: the core writes what layer 0's gradient reads)
  const int grid = nblk < v->cus ? nblk : v->cus;
  if (int rc = vae_launch(v, vae_kernel_index(VF_STEP, p.shape.kind, cat != nullptr, p.wide, 4), grid, st, a)) return rc;
  if (!one) {
    // the partials form: block sums (gradient and loss) and the optimizer, behind it on the stream
    hipLaunchKernelGGL(k_vae_reduce_adam, dim3(backward ? (p.desc.P + 255) / 256 : 1), dim3(256), 0, st, a,
                       v->grads + p.P0);
    LAUNCH_CHECK("k_vae_reduce_adam");
  }
  if (p.wide && backward) {   // layer 0's gradient (and optimizer), behind dz0 and alpha on the stream
    const int units = ((p.shape.in + 15) / 16 + 1) * ((p.n0 + 15) / 16);
    hipLaunchKernelGGL(k_vae_wide_wgrad_adam, dim3((units + 3) / 4), dim3(256), 0, st, wa);
    LAUNCH_CHECK("k_vae_wide_wgrad_adam");
  }
  return P3D_OK;
}

// A p3d_vae_*lds_bytes call: the size `which` of the shape's plan (filled whatever vae_plan answers),
// or, `which` null, the decoder's staggered size; 0 for a shape the checks refuse.
int64_t vae_lds_answer(int kind, int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent, int32_t n_dec,
                       const int32_t* dec_dims, int32_t out, size_t VaePlan::*which) {
  VaeShape s;
  VaePlan p;
  std::string err;
  if (int rc = vae_check_shape(kind, in, n_enc, enc_dims, latent, n_dec, dec_dims, out, s, err)) return fail(rc, err), 0;
  if (!which) return (int64_t)vae_dec_bytes_staggered(s);
  (void)vae_plan(s, p, err);
  return (int64_t)(p.*which);
}

// `bytes` of device memory at *p, zeroed or filled from `src`; on an error, the call that failed
const char* vae_alloc(void** p, size_t bytes, const void* src, hipError_t& e) {
  if ((e = hipMalloc(p, bytes)) != hipSuccess) return "hipMalloc";
  if (!src) return (e = hipMemset(*p, 0, bytes)) != hipSuccess ? "hipMemset" : nullptr;
  return (e = hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice)) != hipSuccess ? "hipMemcpy" : nullptr;
}

int vae_create(int kind, int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent, int32_t n_dec,
               const int32_t* dec_dims, int32_t out, int32_t max_batch, uint64_t seed, p3d_vae** vout) {
  if (!vout) return fail(P3D_ERR_ARG, "p3d_vae_create: null argument");
  VaeShape s;
  std::string err;
  if (int rc = vae_check_shape(kind, in, n_enc, enc_dims, latent, n_dec, dec_dims, out, s, err)) return fail(rc, err);
  if (max_batch < 1 || max_batch > (1 << 20)) return fail(P3D_ERR_ARG, "p3d_vae_create: max_batch must be in 1 .. 2^20");
  p3d_vae* v = new p3d_vae();
  VaePlan& p = v->plan;
  if (int rc = vae_plan(s, p, err)) {
    delete v;
    return fail(rc, err);
  }
  v->max_batch = max_batch;
  v->seed = seed;
  v->dec_wgs = p.dec_wgs;
  auto bail = [&](hipError_t e, const std::string& what) {
    p3d_vae_destroy(v);
    return fail(P3D_ERR_HIP, what + ": " + hipGetErrorString(e));
  };
  hipError_t e;
  int dev = 0;
  if ((e = hipGetDevice(&dev)) != hipSuccess) return bail(e, "hipGetDevice");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, dev)) != hipSuccess) return bail(e, "hipGetDeviceProperties");
  v->cus = prop.multiProcessorCount;
  const std::vector<int> idx = vae_pack_index(p.desc);
  const VaeState s0{0, 0.9f, 0.999f, 0.0f, {0, 0, 0}};
  const size_t pb = sizeof(float) * (size_t)p.Ptot;
  const struct { void** p; size_t bytes; const void* src; } allocs[] = {
      {(void**)&v->params, pb, nullptr}, {(void**)&v->grads, pb, nullptr},
      {(void**)&v->am, pb, nullptr}, {(void**)&v->av, pb, nullptr},
      {(void**)&v->pk, sizeof(float) * (size_t)p.desc.Ppk, nullptr},
      {(void**)&v->ws, sizeof(float) * (size_t)p.ws_floats(max_batch), nullptr},
      {(void**)&v->d_desc, sizeof(VaeDesc), &p.desc},
      {(void**)&v->pkidx, sizeof(int) * idx.size(), idx.data()},
      {(void**)&v->d_dec, sizeof(VaeDesc), &p.dec},
      {(void**)&v->st, sizeof(VaeState), &s0}};
  for (const auto& a : allocs)
    if (const char* what = vae_alloc(a.p, a.bytes, a.src, e)) return bail(e, what);
  // Every listed kernel may use the whole of a workgroup's LDS -- the bound vae_plan has checked each
  // layout against -- so no filter's launches depend on which other filters the process has created
  // (the attribute is the process's, not the handle's).
  for (int k = 0; k < kVaeKernelCount; ++k)
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(kVaeKernelFns[k]), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 P3D_VAE_LDS_LIMIT)) != hipSuccess)
      return bail(e, std::string("hipFuncSetAttribute(") + kVaeKernels[k].name + ")");
  *vout = v;
  return P3D_OK;
}

int vae_cat_checked(const p3d_vae_cat* cat, int32_t in, int64_t B, const char* what, VaeCat* k) {
  std::string err;
  const int rc = vae_cat_check(cat, in, B, what, k, err);
  return rc ? fail(rc, err) : P3D_OK;
}

// a _cat call's checks: the struct's own errors answer before the null handle (they need no filter)
int vae_cat_call(const p3d_vae* v, const p3d_vae_cat* cat, int64_t B, const char* what, VaeCat* k) {
  if (!cat) return fail(P3D_ERR_ARG, std::string(what) + ": null argument");
  if (B < 1 || B > (1 << 20)) return fail(P3D_ERR_ARG, std::string(what) + ": B must be in 1 .. 2^20");
  if (int rc = vae_cat_checked(cat, v ? v->plan.shape.in : -1, B, what, k)) return rc;
  return vae_check_call(v, cat, B, what);
}

int vae_add_noise(const float* src, int64_t rows, int32_t d, const int64_t* starts, int32_t width, int64_t B,
                  uint64_t seed, uint64_t ctr, int64_t row0, float noise, float offset, float joint_scale,
                  uint64_t thr, float* out, void* stream, const char* what) {
  const std::string w(what);
  if (!src || !out) return fail(P3D_ERR_ARG, w + ": null argument");
  if (width < 12 || width > P3D_NOISE_MAX_WIDTH || width % 12 != 0)
    return fail(P3D_ERR_ARG, w + ": width must be a multiple of 12 in 12 .. 240");
  if (d < 4 || d % 4 != 0) return fail(P3D_ERR_ARG, w + ": d must be a positive multiple of 4");
  if (width % d != 0) return fail(P3D_ERR_ARG, w + ": width must be a multiple of d");
  if (B < 1 || B > (1 << 20)) return fail(P3D_ERR_ARG, w + ": B must be in 1 .. 2^20");
  if (!aligned16(src) || !aligned16(out)) return fail(P3D_ERR_ARG, w + ": src and out must be 16-byte aligned");
  if (((uintptr_t)starts & 7) != 0) return fail(P3D_ERR_ARG, w + ": starts must be 8-byte aligned");
  const uintptr_t s0 = (uintptr_t)src, o0 = (uintptr_t)out;
  const bool overlap = rows > 0 && s0 < o0 + (uintptr_t)B * width * 4 && o0 < s0 + (uintptr_t)rows * d * 4;
  if (starts) {
    if (rows < width / d) return fail(P3D_ERR_ARG, w + ": the table has fewer rows than a window");
    if (overlap) return fail(P3D_ERR_ARG, w + ": in the window form out may not overlap src");
  } else {
    if (width != d) return fail(P3D_ERR_ARG, w + ": without starts width must equal d");
    if (rows < B) return fail(P3D_ERR_ARG, w + ": without starts the table needs at least B rows");
    if (overlap && src != out) return fail(P3D_ERR_ARG, w + ": out may be src itself, not another overlapping range");
  }
  NoiseArgs a;
  a.src = src; a.rows = rows; a.starts = starts; a.B = B; a.row0 = row0; a.seed = seed; a.ctr = ctr; a.thr = thr;
  a.noise = noise; a.offset = offset; a.joint_scale = joint_scale; a.d = d; a.width = width;
  const uint64_t c4n = (uint64_t)(width / 4);
  a.magic = (uint32_t)(((1ull << 32) + c4n - 1) / c4n);
  a.out = out;
  hipLaunchKernelGGL(k_vae_noise, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK("k_vae_noise");
  return P3D_OK;
}

// why no K-sample call takes a bones filter
const char* const kVaeMcBones =
    "a bones filter's outputs are lengths and direction cosines, and direction cosines do not average";

// Why a filter cannot run over sequences of U3 values per frame (U3 < 0: of any width), in the
// order every caller reports it
enum VaeSeqFault { VAE_SEQ_OK, VAE_SEQ_BONES, VAE_SEQ_SHAPE, VAE_SEQ_LDS };
VaeSeqFault vae_seq_fault(const VaePlan& p, int32_t U3) {
  if (p.shape.kind != P3D_VAE_KIND_ELBO) return VAE_SEQ_BONES;
  if (p.wide || (U3 >= 0 && p.desc.out != U3) || p.desc.in % p.desc.out != 0 ||
      p.desc.in / p.desc.out > P3D_VAE_SEQ_MAX_LEN)
    return VAE_SEQ_SHAPE;
  return p.seq_lds ? VAE_SEQ_OK : VAE_SEQ_LDS;
}

// The checks and the VaeSeqArgs of the two sequence-filter calls.  bones: the caller's words for a
// bones filter; ptrs: its alignment list by name (the K-sample form's has ref_var, else null here).
int vae_seq_args(const char* what, const char* bones, const char* ptrs, p3d_vae* v, const float* pred,
                 const int64_t* seq_off, int64_t S, int64_t N, const float* eps, uint64_t ctr, int64_t eps_row0,
                 const float* target, float* state, int32_t* started, float* ref, const float* ref_var, float* frame_err,
                 double* seq_err, VaeSeqArgs& a) {
  auto bad = [what](const std::string& msg) { return fail(P3D_ERR_ARG, what + (": " + msg)); };
  if (!v || !pred || !seq_off || !ref) return bad("null argument");
  const VaePlan& p = v->plan;
  const VaeSeqFault f = vae_seq_fault(p, -1);
  if (f == VAE_SEQ_BONES) return bad(bones);
  if (f == VAE_SEQ_SHAPE)
    return bad("in must be seq_len * out with seq_len in 1 .. " + std::to_string(P3D_VAE_SEQ_MAX_LEN));
  if (f == VAE_SEQ_LDS) return bad("parameters, one tile and the state tile exceed a workgroup's LDS");
  if (S < 1 || S > (1 << 20)) return bad("S must be in 1 .. 2^20");
  if (N < 1 || N > (1 << 20)) return bad("N must be in 1 .. 2^20");
  if (eps_row0 < 0) return bad("eps_row0 must be >= 0");
  if ((state != nullptr) != (started != nullptr)) return bad("state and started go together");
  if ((frame_err || seq_err) && !target) return bad("frame_err and seq_err need a target");
  for (const void* q : {(const void*)pred, (const void*)eps, (const void*)target, (const void*)state, (const void*)ref,
                        (const void*)ref_var})
    if ((uintptr_t)q % 16 != 0) return bad(ptrs + std::string(" must be 16-byte aligned"));
  a.desc = p.desc; a.desc_dev = v->d_desc; a.pk = v->pk; a.pred = pred; a.seq_off = seq_off; a.S = S; a.N = N;
  a.eps = eps; a.seed = v->seed; a.ctr = ctr; a.eps_row0 = eps_row0; a.target = target;
  a.state = state; a.started = started; a.ref = ref; a.frame_err = frame_err; a.seq_err = seq_err;
  a.seq_len = p.seq_len; a.xoff = p.seq_xoff; a.toff = p.seq_toff; a.ldt = p.seq_ldt; a.moff = p.seq_moff;
  return P3D_OK;
}

}  // namespace

extern "C" int64_t p3d_vae_lds_bytes(int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent, int32_t n_dec,
                                     const int32_t* dec_dims, int32_t out) {
  return vae_lds_answer(P3D_VAE_KIND_ELBO, in, n_enc, enc_dims, latent, n_dec, dec_dims, out, &VaePlan::lds);
}

extern "C" int64_t p3d_vae_bones_lds_bytes(int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent,
                                           int32_t n_dec, const int32_t* dec_dims) {
  return vae_lds_answer(P3D_VAE_KIND_BONES, in, n_enc, enc_dims, latent, n_dec, dec_dims, 64, &VaePlan::lds);
}

extern "C" int64_t p3d_vae_dec_lds_bytes(int32_t latent, int32_t n_dec, const int32_t* dec_dims, int32_t out,
                                         int32_t bones) {
  const int32_t enc[1] = {8};   // (a dummy encoder: vae_dec_bytes_staggered)
  if (bones != 0 && bones != 1) return 0;
  return vae_lds_answer(bones ? P3D_VAE_KIND_BONES : P3D_VAE_KIND_ELBO, 8, 1, enc, latent, n_dec, dec_dims,
                        bones ? 64 : out, nullptr);
}

extern "C" int64_t p3d_vae_seq_lds_bytes(int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent,
                                         int32_t n_dec, const int32_t* dec_dims, int32_t out, int32_t form) {
  if (form != 0 && form != 1) return 0;   // (both forms run one tile per workgroup)
  return vae_lds_answer(P3D_VAE_KIND_ELBO, in, n_enc, enc_dims, latent, n_dec, dec_dims, out, &VaePlan::seq_lds);
}

extern "C" int p3d_vae_create(int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent, int32_t n_dec,
                              const int32_t* dec_dims, int32_t out, int32_t max_batch, uint64_t seed, p3d_vae** vout) {
  return vae_create(P3D_VAE_KIND_ELBO, in, n_enc, enc_dims, latent, n_dec, dec_dims, out, max_batch, seed, vout);
}

extern "C" int p3d_vae_create_bones(int32_t in, int32_t n_enc, const int32_t* enc_dims, int32_t latent, int32_t n_dec,
                                    const int32_t* dec_dims, int32_t max_batch, uint64_t seed, p3d_vae** vout) {
  return vae_create(P3D_VAE_KIND_BONES, in, n_enc, enc_dims, latent, n_dec, dec_dims, 64, max_batch, seed, vout);
}

extern "C" int p3d_vae_destroy(p3d_vae* v) {
  if (!v) return P3D_OK;
  void* bufs[] = {v->params, v->grads, v->am, v->av, v->pk, v->ws, v->d_desc, v->pkidx, v->d_dec, v->st};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  delete v;
  return P3D_OK;
}

extern "C" int32_t p3d_vae_kind(const p3d_vae* v) { return v ? v->plan.shape.kind : -1; }

extern "C" int p3d_bones_from_joints(const float* joints, int64_t B, int32_t precise, float* out64, void* stream) {
  if (!joints || !out64) return fail(P3D_ERR_ARG, "p3d_bones_from_joints: null argument");
  if (B < 1 || B > (1 << 20)) return fail(P3D_ERR_ARG, "p3d_bones_from_joints: B must be in 1 .. 2^20");
  if (precise != 0 && precise != 1) return fail(P3D_ERR_ARG, "p3d_bones_from_joints: precise must be 0 or 1");
  const unsigned grid = (unsigned)((B * 16 + 255) / 256);
  if (precise) hipLaunchKernelGGL(k_bones_from_joints<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, joints, B, out64);
  else hipLaunchKernelGGL(k_bones_from_joints<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, joints, B, out64);
  LAUNCH_CHECK("k_bones_from_joints");
  return P3D_OK;
}

extern "C" int p3d_bones_to_joints(const float* bones64, int64_t B, double* joints_f64, void* stream) {
  if (!bones64 || !joints_f64) return fail(P3D_ERR_ARG, "p3d_bones_to_joints: null argument");
  if (B < 1 || B > (1 << 20)) return fail(P3D_ERR_ARG, "p3d_bones_to_joints: B must be in 1 .. 2^20");
  hipLaunchKernelGGL(k_bones_to_joints, dim3((unsigned)((B * 16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bones64,
                     B, joints_f64);
  LAUNCH_CHECK("k_bones_to_joints");
  return P3D_OK;
}

extern "C" int p3d_vae_param_count(const p3d_vae* v, int32_t* count) {
  if (!v || !count) return fail(P3D_ERR_ARG, "p3d_vae_param_count: null argument");
  *count = (int32_t)v->plan.tensors.size();
  return P3D_OK;
}

extern "C" int p3d_vae_param_info(const p3d_vae* v, int32_t idx, const char** name, int64_t* numel, int32_t* rows,
                                  int32_t* cols, int64_t* offset) {
  if (!v) return fail(P3D_ERR_ARG, "p3d_vae_param_info: null argument");
  if (idx < 0 || idx >= (int)v->plan.tensors.size()) return fail(P3D_ERR_ARG, "p3d_vae_param_info: index out of range");
  const VaeTensor& T = v->plan.tensors[idx];
  if (name) *name = v->plan.names[idx].c_str();
  if (numel) *numel = (int64_t)T.K * T.N;
  if (rows) *rows = T.K;
  if (cols) *cols = T.N;
  if (offset) *offset = T.flat;
  return P3D_OK;
}

extern "C" int p3d_vae_param_ptr(p3d_vae* v, const char* name, void** dptr, int64_t* numel) {
  if (!v || !name || !dptr) return fail(P3D_ERR_ARG, "p3d_vae_param_ptr: null argument");
  for (size_t i = 0; i < v->plan.tensors.size(); ++i)
    if (v->plan.names[i] == name) {
      const VaeTensor& T = v->plan.tensors[i];
      *dptr = v->params + T.flat;
      if (numel) *numel = (int64_t)T.K * T.N;
      return P3D_OK;
    }
  return fail(P3D_ERR_NOTFOUND, std::string("p3d_vae_param_ptr: no parameter named ") + name);
}

extern "C" int p3d_vae_flat_ptr(p3d_vae* v, int32_t which, void** dptr, int64_t* numel) {
  if (!v || !dptr) return fail(P3D_ERR_ARG, "p3d_vae_flat_ptr: null argument");
  float* const bufs[6] = {v->params, v->grads, v->am, v->av, v->ws, v->pk};
  if (which < 0 || which > 5) return fail(P3D_ERR_ARG, "p3d_vae_flat_ptr: which must be 0 .. 5");
  *dptr = bufs[which];
  if (numel) *numel = which == 4 ? v->plan.ws_floats(v->max_batch) : which == 5 ? v->plan.desc.Ppk : v->plan.Ptot;
  return P3D_OK;
}

extern "C" int p3d_vae_params_updated(p3d_vae* v, void* stream) {
  if (!v) return fail(P3D_ERR_ARG, "p3d_vae_params_updated: null argument");
  const int P = v->plan.desc.P;
  hipLaunchKernelGGL(k_vae_pack, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, (const int*)v->pkidx,
                     (const float*)(v->params + v->plan.P0), v->pk);
  LAUNCH_CHECK("k_vae_pack");
  return P3D_OK;
}

extern "C" int p3d_vae_cat_check(const p3d_vae_cat* cat, int32_t in, int64_t B) {
  if (B < 1 || B > (1 << 20)) return fail(P3D_ERR_ARG, "p3d_vae_cat_check: B must be in 1 .. 2^20");
  return vae_cat_checked(cat, in, B, "p3d_vae_cat_check", nullptr);
}

extern "C" int p3d_vae_forward(p3d_vae* v, const float* x, int64_t B, const float* eps, uint64_t ctr, float* y,
                               float* mean, float* log_var, float* z, const float* target, float* row_terms,
                               void* stream) {
  if (int rc = vae_check_call(v, x, B, "p3d_vae_forward")) return rc;
  return vae_forward(v, x, nullptr, B, eps, ctr, y, mean, log_var, z, target, row_terms, stream, "p3d_vae_forward");
}

// The errors that need no filter answer first (and without a GPU).
extern "C" int p3d_vae_decode(p3d_vae* v, const float* z, int64_t B, uint64_t ctr, int64_t row0, float* y,
                              float* z_out, void* stream) {
  if (!y) return fail(P3D_ERR_ARG, "p3d_vae_decode: y is null");
  if (B < 1 || B > (1 << 20)) return fail(P3D_ERR_ARG, "p3d_vae_decode: B must be in 1 .. 2^20");
  if (z && z_out) return fail(P3D_ERR_ARG, "p3d_vae_decode: z_out receives the drawn z: give z or z_out, not both");
  if (row0 < 0) return fail(P3D_ERR_ARG, "p3d_vae_decode: row0 must be >= 0");
  if (ctr == P3D_CTR_GLOBAL_STEP)
    return fail(P3D_ERR_ARG, "p3d_vae_decode: the prior stream has no device counter (ctr may not be P3D_CTR_GLOBAL_STEP)");
  if (!v) return fail(P3D_ERR_ARG, "p3d_vae_decode: null handle");
  VaeDecArgs a{};
  a.desc = v->d_dec; a.pk = v->pk + v->plan.dec_base; a.z = z; a.B = B; a.row0 = row0;
  a.seed = v->seed; a.ctr = ctr; a.y = y; a.z_out = z_out;
  const int64_t nwg = (B + 63) / 64, cap = (int64_t)v->cus * v->dec_wgs;
  const int grid = (int)(nwg < cap ? nwg : cap);
  return vae_launch(v, vae_kernel_index(VF_DEC, v->plan.shape.kind, 0, 0, 4), grid, stream, a);
}

extern "C" int p3d_vae_dec_set_grid(p3d_vae* v, int32_t wgs_per_cu) {
  if (!v) return fail(P3D_ERR_ARG, "p3d_vae_dec_set_grid: null handle");
  const int fit = (int)(P3D_VAE_LDS_LIMIT / v->plan.dec_lds);
  if (wgs_per_cu < 0 || wgs_per_cu > (fit < 16 ? fit : 16))
    return fail(P3D_ERR_ARG, "p3d_vae_dec_set_grid: workgroups per CU must be 0 (the default) or 1 .. " +
                                 std::to_string(fit < 16 ? fit : 16) + " (what a CU's LDS holds)");
  v->dec_wgs = wgs_per_cu ? wgs_per_cu : v->plan.dec_wgs;
  return P3D_OK;
}

extern "C" int p3d_vae_loss(p3d_vae* v, const float* x, const float* t, int64_t B, const float* eps, uint64_t ctr,
                            const float* factors, float* loss3_dev, void* stream) {
  if (int rc = vae_check_call(v, x, B, "p3d_vae_loss")) return rc;
  return vae_step(v, x, nullptr, t, B, eps, ctr, factors, 0, 0, 0.0f, loss3_dev, stream, "p3d_vae_loss");
}

extern "C" int p3d_vae_grad(p3d_vae* v, const float* x, const float* t, int64_t B, const float* eps, uint64_t ctr,
                            const float* factors, float* loss3_dev, void* stream) {
  if (int rc = vae_check_call(v, x, B, "p3d_vae_grad")) return rc;
  return vae_step(v, x, nullptr, t, B, eps, ctr, factors, 1, 0, 0.0f, loss3_dev, stream, "p3d_vae_grad");
}

extern "C" int p3d_vae_train_step(p3d_vae* v, const float* x, const float* t, int64_t B, const float* eps,
                                  const float* factors, float lr, float* loss3_dev, void* stream) {
  if (!(lr >= 0.0f)) return fail(P3D_ERR_ARG, "p3d_vae_train_step: lr must be >= 0");
  if (int rc = vae_check_call(v, x, B, "p3d_vae_train_step")) return rc;
  return vae_step(v, x, nullptr, t, B, eps, P3D_CTR_GLOBAL_STEP, factors, 1, 1, lr, loss3_dev, stream,
                  "p3d_vae_train_step");
}

// The _cat twins.  The struct's own errors answer first: they need no filter (and no GPU).
extern "C" int p3d_vae_forward_cat(p3d_vae* v, const p3d_vae_cat* cat, int64_t B, const float* eps, uint64_t ctr,
                                   float* y, float* mean, float* log_var, float* z, const float* target,
                                   float* row_terms, void* stream) {
  VaeCat k;
  if (int rc = vae_cat_call(v, cat, B, "p3d_vae_forward_cat", &k)) return rc;
  return vae_forward(v, nullptr, &k, B, eps, ctr, y, mean, log_var, z, target, row_terms, stream, "p3d_vae_forward_cat");
}

extern "C" int p3d_vae_loss_cat(p3d_vae* v, const p3d_vae_cat* cat, const float* t, int64_t B, const float* eps,
                                uint64_t ctr, const float* factors, float* loss3_dev, void* stream) {
  VaeCat k;
  if (int rc = vae_cat_call(v, cat, B, "p3d_vae_loss_cat", &k)) return rc;
  return vae_step(v, nullptr, &k, t, B, eps, ctr, factors, 0, 0, 0.0f, loss3_dev, stream, "p3d_vae_loss_cat");
}

extern "C" int p3d_vae_grad_cat(p3d_vae* v, const p3d_vae_cat* cat, const float* t, int64_t B, const float* eps,
                                uint64_t ctr, const float* factors, float* loss3_dev, void* stream) {
  VaeCat k;
  if (int rc = vae_cat_call(v, cat, B, "p3d_vae_grad_cat", &k)) return rc;
  return vae_step(v, nullptr, &k, t, B, eps, ctr, factors, 1, 0, 0.0f, loss3_dev, stream, "p3d_vae_grad_cat");
}

extern "C" int p3d_vae_train_step_cat(p3d_vae* v, const p3d_vae_cat* cat, const float* t, int64_t B, const float* eps,
                                      const float* factors, float lr, float* loss3_dev, void* stream) {
  if (!(lr >= 0.0f)) return fail(P3D_ERR_ARG, "p3d_vae_train_step_cat: lr must be >= 0");
  VaeCat k;
  if (int rc = vae_cat_call(v, cat, B, "p3d_vae_train_step_cat", &k)) return rc;
  return vae_step(v, nullptr, &k, t, B, eps, P3D_CTR_GLOBAL_STEP, factors, 1, 1, lr, loss3_dev, stream,
                  "p3d_vae_train_step_cat");
}

extern "C" int p3d_vae_adam_apply(p3d_vae* v, float lr, void* stream) {
  if (!v || !(lr >= 0.0f)) return fail(P3D_ERR_ARG, "p3d_vae_adam_apply: bad argument");
  const VaePlan& p = v->plan;
  VaeArgs a = vae_args(v, nullptr, nullptr, 1, nullptr, 0);
  a.backward = 1; a.adam = 1; a.nblk = 1; a.gout = v->grads + p.P0; a.loss3 = nullptr;
  hipLaunchKernelGGL(k_vae_alpha, dim3(1), dim3(1), 0, (hipStream_t)stream, v->st, lr);
  LAUNCH_CHECK("k_vae_alpha");
  hipLaunchKernelGGL(k_vae_reduce_adam, dim3((p.desc.P + 255) / 256), dim3(256), 0, (hipStream_t)stream, a,
                     v->grads + p.P0);
  LAUNCH_CHECK("k_vae_reduce_adam");
  if (p.wide) {
    hipLaunchKernelGGL(k_vae_wide_adam, dim3((p.P0 + 255) / 256), dim3(256), 0, (hipStream_t)stream, p.P0,
                       (const float*)v->grads, v->params, v->am, v->av, (const VaeState*)v->st);
    LAUNCH_CHECK("k_vae_wide_adam");
  }
  return P3D_OK;
}

extern "C" int p3d_vae_set_form(p3d_vae* v, int32_t form) {
  if (!v || (form != 0 && form != 1)) return fail(P3D_ERR_ARG, "p3d_vae_set_form: form must be 0 or 1");
  v->form = form;
  return P3D_OK;
}

extern "C" int p3d_vae_get_step(const p3d_vae* v, int64_t* step, float* beta1_power, float* beta2_power) {
  if (!v) return fail(P3D_ERR_ARG, "p3d_vae_get_step: null argument");
  VaeState s;
  HIP_TRY(hipMemcpy(&s, v->st, sizeof(s), hipMemcpyDeviceToHost));
  if (step) *step = s.step;
  if (beta1_power) *beta1_power = s.b1p;
  if (beta2_power) *beta2_power = s.b2p;
  return P3D_OK;
}

extern "C" int p3d_vae_set_step(p3d_vae* v, int64_t step, float beta1_power, float beta2_power) {
  if (!v || step < 0) return fail(P3D_ERR_ARG, "p3d_vae_set_step: bad argument");
  const VaeState s{step, beta1_power, beta2_power, 0.0f, {0, 0, 0}};
  HIP_TRY(hipMemcpy(v->st, &s, sizeof(s), hipMemcpyHostToDevice));
  return P3D_OK;
}

extern "C" int p3d_vae_eps(uint64_t seed, uint64_t ctr, int64_t row0, int64_t B, int32_t latent, float* out,
                           void* stream) {
  if (!out) return fail(P3D_ERR_ARG, "p3d_vae_eps: null argument");
  if (B < 1 || B > (1 << 20) || row0 < 0) return fail(P3D_ERR_ARG, "p3d_vae_eps: B must be in 1 .. 2^20, row0 >= 0");
  if (latent < 4 || latent > 64 || latent % 4 != 0) return fail(P3D_ERR_ARG, "p3d_vae_eps: latent must be a multiple of 4 in 4 .. 64");
  const int64_t units = B * (latent / 4);
  hipLaunchKernelGGL(k_vae_eps, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, ctr,
                     row0, B, (int)latent, out);
  LAUNCH_CHECK("k_vae_eps");
  return P3D_OK;
}

extern "C" int p3d_vae_add_noise(const float* src, int64_t rows, int32_t d, const int64_t* starts, int32_t width,
                                 int64_t B, uint64_t seed, uint64_t ctr, int64_t row0, float noise, float offset,
                                 float joint_scale, float* out, void* stream) {
  return vae_add_noise(src, rows, d, starts, width, B, seed, ctr, row0, noise, offset, joint_scale,
                       P3D_NOISE_THRESHOLD, out, stream, "p3d_vae_add_noise");
}

extern "C" int p3d_vae_add_noise_thr(const float* src, int64_t rows, int32_t d, const int64_t* starts, int32_t width,
                                     int64_t B, uint64_t seed, uint64_t ctr, int64_t row0, float noise, float offset,
                                     float joint_scale, uint64_t threshold, float* out, void* stream) {
  if (threshold > (1ull << 32)) return fail(P3D_ERR_ARG, "p3d_vae_add_noise_thr: threshold must be in 0 .. 2^32");
  return vae_add_noise(src, rows, d, starts, width, B, seed, ctr, row0, noise, offset, joint_scale, threshold, out,
                       stream, "p3d_vae_add_noise_thr");
}

extern "C" int p3d_vae_seq_set_form(p3d_vae* v, int32_t form) {
  if (!v || (form != 0 && form != 1)) return fail(P3D_ERR_ARG, "p3d_vae_seq_set_form: form must be 0 or 1");
  v->seq_form = form;
  return P3D_OK;
}

extern "C" int p3d_vae_seq_filter(p3d_vae* v, const float* pred, const int64_t* seq_off, int64_t S, int64_t N,
                                  const float* eps, uint64_t ctr, int64_t eps_row0, const float* target,
                                  float* state, int32_t* started, float* ref, float* frame_err, double* seq_err,
                                  void* stream) {
  VaeSeqArgs a{};
  if (int rc = vae_seq_args("p3d_vae_seq_filter", "a bones filter has no sequence form", "pred, eps, target, state and ref",
                            v, pred, seq_off, S, N, eps, ctr, eps_row0, target, state, started, ref, nullptr, frame_err,
                            seq_err, a))
    return rc;
  return vae_launch(v, vae_kernel_index(VF_SEQ, P3D_VAE_KIND_ELBO, 0, 0, v->seq_form ? 4 : 1), (unsigned)((S + 15) / 16),
                    stream, a);
}

namespace {

// What the K-sample calls refuse before anything else, without a filter (and without a GPU): a null
// output, K out of range, the device counter.
int vae_mc_check(const void* out, const char* out_name, int32_t K, uint64_t ctr, const char* what) {
  const std::string w(what);
  if (!out) return fail(P3D_ERR_ARG, w + ": " + out_name + " is null");
  if (K < 1 || K > P3D_VAE_MC_MAX_K)
    return fail(P3D_ERR_ARG, w + ": K must be in 1 .. " + std::to_string(P3D_VAE_MC_MAX_K));
  if (ctr == P3D_CTR_GLOBAL_STEP)
    return fail(P3D_ERR_ARG, w + ": draw k uses the counter ctr + k (ctr may not be P3D_CTR_GLOBAL_STEP)");
  return P3D_OK;
}

int vae_mc_bones(const p3d_vae* v, const char* what) {
  if (v->plan.shape.kind != P3D_VAE_KIND_ELBO) return fail(P3D_ERR_ARG, what + (": " + std::string(kVaeMcBones)));
  return P3D_OK;
}

int vae_forward_mc(p3d_vae* v, const float* x, const VaeCat* cat, int64_t B, int32_t K, const float* eps, uint64_t ctr,
                   float* y_mean, float* y_var, float* mean, float* log_var, void* stream, const char* what) {
  const hipStream_t st = (hipStream_t)stream;
  VaeWideArgs wa{};
  if (v->plan.wide)
    if (int rc = vae_wide_fwd(v, x, cat, B, 0, wa, st, what)) return rc;
  VaeMcArgs a{};
  a.a = vae_args(v, x, nullptr, B, eps, ctr);
  a.a.y = y_mean; a.a.mean = mean; a.a.log_var = log_var;
  if (cat) a.a.cat = *cat;
  a.y_var = y_var; a.K = K;
  const int64_t nwg = (B + 63) / 64;
  const int grid = (int)(nwg < v->cus ? nwg : v->cus);
  return vae_launch(v, vae_kernel_index(VF_FWDMC, P3D_VAE_KIND_ELBO, cat != nullptr, 0, 4), grid, st, a);
}

}  // namespace

extern "C" int p3d_vae_forward_mc(p3d_vae* v, const float* x, int64_t B, int32_t K, const float* eps, uint64_t ctr,
                                  float* y_mean, float* y_var, float* mean, float* log_var, void* stream) {
  if (int rc = vae_mc_check(y_mean, "y_mean", K, ctr, "p3d_vae_forward_mc")) return rc;
  if (int rc = vae_check_call(v, x, B, "p3d_vae_forward_mc")) return rc;
  if (int rc = vae_mc_bones(v, "p3d_vae_forward_mc")) return rc;
  return vae_forward_mc(v, x, nullptr, B, K, eps, ctr, y_mean, y_var, mean, log_var, stream, "p3d_vae_forward_mc");
}

extern "C" int p3d_vae_forward_mc_cat(p3d_vae* v, const p3d_vae_cat* cat, int64_t B, int32_t K, const float* eps,
                                      uint64_t ctr, float* y_mean, float* y_var, float* mean, float* log_var,
                                      void* stream) {
  if (int rc = vae_mc_check(y_mean, "y_mean", K, ctr, "p3d_vae_forward_mc_cat")) return rc;
  VaeCat k;
  if (int rc = vae_cat_call(v, cat, B, "p3d_vae_forward_mc_cat", &k)) return rc;
  if (int rc = vae_mc_bones(v, "p3d_vae_forward_mc_cat")) return rc;
  return vae_forward_mc(v, nullptr, &k, B, K, eps, ctr, y_mean, y_var, mean, log_var, stream, "p3d_vae_forward_mc_cat");
}

extern "C" int p3d_vae_seq_filter_mc(p3d_vae* v, const float* pred, const int64_t* seq_off, int64_t S, int64_t N,
                                     int32_t K, const float* eps, uint64_t ctr, int64_t eps_row0, const float* target,
                                     float* state, int32_t* started, float* ref, float* ref_var, float* frame_err,
                                     double* seq_err, void* stream) {
  const char* what = "p3d_vae_seq_filter_mc";
  if (int rc = vae_mc_check(ref, "ref", K, ctr, what)) return rc;
  VaeSeqMcArgs m{};
  if (int rc = vae_seq_args(what, kVaeMcBones, "pred, eps, target, state, ref and ref_var", v, pred, seq_off, S, N, eps, ctr,
                            eps_row0, target, state, started, ref, ref_var, frame_err, seq_err, m.s))
    return rc;
  m.ref_var = ref_var; m.K = K;
  return vae_launch(v, vae_kernel_index(VF_SEQMC, P3D_VAE_KIND_ELBO, 0, 0, 4), (unsigned)((S + 15) / 16), stream, m);
}

extern "C" int64_t p3d_vae_workspace(const p3d_vae* v, int64_t B) {
  return v && B >= 1 ? (int64_t)sizeof(float) * v->plan.ws_floats(B) : 0;
}
