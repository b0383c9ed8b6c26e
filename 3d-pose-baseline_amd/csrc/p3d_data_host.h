// p3d_data_host.h -- the entry points around the network (include/p3d.h): the MPJPE accumulation,
// DLPack aliases, the empty launch, the H3.6M data pipeline (camera, normalise / unnormalise,
// p3d_sample_world, moments), p3d_lift and CRC-32C.  Host code (and the one-line k_empty);
// included by p3d.hip behind p3d_forward_host.h (forward_impl, forward_gemv) and p3d_model.h; the
// kernels are in p3d_eval.h, p3d_data.h and p3d_sample.h.  The clip calls: p3d_clip_host.h.
#pragma once

extern "C" int p3d_mpjpe_accum_ex(const float* pred_n, const float* gt_n, int32_t D, const double* mean96,
                                  const double* std96, const int32_t* dims, int64_t B, int32_t n_joints,
                                  int32_t procrustes, double* joint_sum, double* sq_sum, void* stream) {
  if (!pred_n || !gt_n || !mean96 || !std96 || !dims || !joint_sum)
    return fail(P3D_ERR_ARG, "p3d_mpjpe_accum: null argument");
  if (B <= 0) return fail(P3D_ERR_ARG, "p3d_mpjpe_accum: batch must be positive");
  if (n_joints < 1 || n_joints > P3D_MAX_JOINTS || D <= 0 || D % 3 != 0 ||
      (3 * n_joints - D != 0 && 3 * n_joints - D != 3))
    return fail(P3D_ERR_ARG, "p3d_mpjpe_accum: need D == 3*n_joints (predict_14) or 3*(n_joints-1) (root prepended)");
  MpjpeArgs a{};
  a.pred = pred_n; a.gt = gt_n; a.D = D; a.J = n_joints; a.root = (3 * n_joints - D) / 3;
  a.mean = mean96; a.stdv = std96; a.dims = dims; a.B = B; a.joint_sum = joint_sum; a.sq_sum = sq_sum;
  const unsigned grid = (unsigned)((B + 63) / 64);
  if (procrustes) k_mpjpe<true><<<grid, 64, 0, (hipStream_t)stream>>>(a);
  else k_mpjpe<false><<<grid, 64, 0, (hipStream_t)stream>>>(a);
  LAUNCH_CHECK("k_mpjpe");
  return P3D_OK;
}

extern "C" int p3d_mpjpe_accum(const float* pred_n, const float* gt_n, const double* mean96,
                               const double* std96, const int32_t* dims48, int64_t B, double* joint_sum17,
                               void* stream) {
  return p3d_mpjpe_accum_ex(pred_n, gt_n, 48, mean96, std96, dims48, B, 17, 0, joint_sum17, nullptr, stream);
}

// DLPack (v0.8 ABI) alias of device memory for the host binding (torch.from_dlpack):
// the managed-tensor record and its deleter live here, so freeing the view never calls
// back into Python (a ctypes-callback deleter crashed interpreter teardown).
namespace {
struct DlDevice { int32_t device_type; int32_t device_id; };
struct DlDType { uint8_t code; uint8_t bits; uint16_t lanes; };
struct DlTensor {
  void* data; DlDevice device; int32_t ndim; DlDType dtype; int64_t* shape; int64_t* strides;
  uint64_t byte_offset;
};
struct DlManaged { DlTensor dl_tensor; void* manager_ctx; void (*deleter)(DlManaged*); };
void dl_free(DlManaged* t) {
  if (!t) return;
  free(t->dl_tensor.shape);
  free(t);
}
}  // namespace

extern "C" void* p3d_dlpack_alias(void* data, int32_t ndim, const int64_t* shape, int32_t device_id,
                                  int32_t dtype_code, int32_t bits) {
  if (ndim <= 0 || !shape) return nullptr;
  DlManaged* t = (DlManaged*)calloc(1, sizeof(DlManaged));
  if (!t) return nullptr;
  t->dl_tensor.shape = (int64_t*)malloc(sizeof(int64_t) * (size_t)ndim);
  if (!t->dl_tensor.shape) { free(t); return nullptr; }
  for (int i = 0; i < ndim; ++i) t->dl_tensor.shape[i] = shape[i];
  t->dl_tensor.data = data;
  t->dl_tensor.device.device_type = 10;   // kDLROCM
  t->dl_tensor.device.device_id = device_id;
  t->dl_tensor.ndim = ndim;
  t->dl_tensor.dtype.code = (uint8_t)dtype_code;
  t->dl_tensor.dtype.bits = (uint8_t)bits;
  t->dl_tensor.dtype.lanes = 1;
  t->deleter = dl_free;
  return t;
}

__global__ void k_empty() {}

// (include/p3d.h) an empty launch through the model's launch path: the fixed cost of a launch +
// synchronise round trip that the headline's timed region pays beside its kernel (bench.py)
extern "C" int p3d_empty_launch(p3d_model* m, int32_t grid, void* stream) {
  if (!m || grid <= 0) return fail(P3D_ERR_ARG, "p3d_empty_launch: bad argument");
  ProfScope ps(m, "empty");
  HP_START
  go(ps, k_empty, dim3((unsigned)grid), dim3(256), (hipStream_t)stream);
  HP(8);
  LAUNCH_CHECK("k_empty");
  return P3D_OK;
}

// =====================================================================================
// H3.6M data pipeline (p3d_data.h)
// =====================================================================================
static int64_t p3d_moments_blocks(int64_t F) {
  int64_t g = (F + 255) / 256;
  return g < 1 ? 1 : (g > 4096 ? 4096 : g);
}

extern "C" int p3d_cam_transform(const double* P, int64_t n, int64_t in_cam_stride, const double* cams,
                                 int32_t C, int32_t inverse, double* out, void* stream) {
  if (n < 0 || C < 0) return fail(P3D_ERR_ARG, "p3d_cam_transform: negative size");
  if (n == 0 || C == 0) return 0;
  if (!P || !cams || !out) return fail(P3D_ERR_ARG, "p3d_cam_transform: null argument");
  if (in_cam_stride != 0 && in_cam_stride < 3 * n) return fail(P3D_ERR_ARG, "p3d_cam_transform: in_cam_stride < 3n");
  if (in_cam_stride == 0 && inverse == 0 && (const double*)out == P) return fail(P3D_ERR_ARG, "p3d_cam_transform: out aliases P");
  CamArgs a{P, in_cam_stride, n, cams, C, out, nullptr, nullptr, nullptr, nullptr};
  const dim3 grid((unsigned)((n + 255) / 256));
  if (inverse) k_cam_points<1><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  else k_cam_points<0><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  LAUNCH_CHECK("k_cam_points");
  return 0;
}

extern "C" int p3d_cam_project(const double* P, int64_t n, const double* cams, int32_t C, double* proj,
                               double* depth, double* radial, double* tan, double* r2, void* stream) {
  if (n < 0 || C < 0) return fail(P3D_ERR_ARG, "p3d_cam_project: negative size");
  if (n == 0 || C == 0) return 0;
  if (!P || !cams || !proj) return fail(P3D_ERR_ARG, "p3d_cam_project: null argument");
  CamArgs a{P, 0, n, cams, C, proj, depth, radial, tan, r2};
  k_cam_points<2><<<dim3((unsigned)((n + 255) / 256)), 256, 0, (hipStream_t)stream>>>(a);
  LAUNCH_CHECK("k_cam_points");
  return 0;
}

extern "C" int p3d_root_center(const double* poses, int64_t F, int32_t width, double* out, double* root,
                               void* stream) {
  if (F < 0 || width < 3 || width % 3) return fail(P3D_ERR_ARG, "p3d_root_center: width must be 3 * joints");
  if (F == 0) return 0;
  if (!poses || !out) return fail(P3D_ERR_ARG, "p3d_root_center: null argument");
  if ((const double*)out == poses) return fail(P3D_ERR_ARG, "p3d_root_center: out must not alias poses");
  const int64_t total = F * width;
  k_root_center<<<dim3((unsigned)((total + 255) / 256)), 256, 0, (hipStream_t)stream>>>(poses, F, width, out, root);
  LAUNCH_CHECK("k_root_center");
  return 0;
}

extern "C" int p3d_normalize(const double* x, int64_t F, int32_t D, const double* mean, const double* stdv,
                             const int32_t* dims_to_use, int32_t U, void* out, int32_t out_dtype, void* stream) {
  if (F < 0 || D <= 0 || U < 0) return fail(P3D_ERR_ARG, "p3d_normalize: bad size");
  if (out_dtype != P3D_DTYPE_F32 && out_dtype != P3D_DTYPE_F64) return fail(P3D_ERR_ARG, "p3d_normalize: out_dtype F32 or F64");
  if (F == 0 || U == 0) return 0;
  if (!x || !mean || !stdv || !dims_to_use || !out) return fail(P3D_ERR_ARG, "p3d_normalize: null argument");
  const int64_t total = F * U;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (out_dtype == P3D_DTYPE_F32) k_normalize<true><<<grid, 256, 0, (hipStream_t)stream>>>(x, F, D, mean, stdv, dims_to_use, U, out);
  else k_normalize<false><<<grid, 256, 0, (hipStream_t)stream>>>(x, F, D, mean, stdv, dims_to_use, U, out);
  LAUNCH_CHECK("k_normalize");
  return 0;
}

extern "C" int p3d_unnormalize(const void* xn, int32_t in_dtype, int64_t F, int32_t U, const double* mean,
                               const double* stdv, const int32_t* dims_to_use, int32_t D, double* out, void* stream) {
  if (F < 0 || U < 0 || D <= 0 || D > 256 || U > D) return fail(P3D_ERR_ARG, "p3d_unnormalize: need 0 <= U <= D <= 256");
  if (in_dtype != P3D_DTYPE_F32 && in_dtype != P3D_DTYPE_F64) return fail(P3D_ERR_ARG, "p3d_unnormalize: in_dtype F32 or F64");
  if (F == 0) return 0;
  if (!mean || !stdv || !out || (U > 0 && (!xn || !dims_to_use))) return fail(P3D_ERR_ARG, "p3d_unnormalize: null argument");
  const int64_t total = F * D;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (in_dtype == P3D_DTYPE_F32) k_unnormalize<true><<<grid, 256, 0, (hipStream_t)stream>>>(xn, F, U, mean, stdv, dims_to_use, D, out);
  else k_unnormalize<false><<<grid, 256, 0, (hipStream_t)stream>>>(xn, F, U, mean, stdv, dims_to_use, D, out);
  LAUNCH_CHECK("k_unnormalize");
  return 0;
}

// sample()'s numbers (src/predict_3dpose.py:512-546) for N rows in one launch: p3d_unnormalize,
// + root, p3d_cam_transform(inverse = 1) with each row's camera, p3d_root_center -- the same bits.
extern "C" int p3d_sample_world(const void* yn, int32_t in_dtype, int64_t N, int32_t U, const double* mean96,
                                const double* std96, const int32_t* dims_to_use, const double* root,
                                const double* cams, int32_t C, const int32_t* cam_of_row, double* out,
                                void* stream) {
  if (!yn || !mean96 || !std96 || !dims_to_use || !cams || !out)
    return fail(P3D_ERR_ARG, "p3d_sample_world: null argument");
  if (N < 1 || N > (1 << 20)) return fail(P3D_ERR_ARG, "p3d_sample_world: N must be in 1 .. 2^20");
  if (U < 1 || U > P3D_SAMPLE_W) return fail(P3D_ERR_ARG, "p3d_sample_world: U must be in 1 .. 96");
  if (C < 1 || C > P3D_SAMPLE_MAX_CAMS) return fail(P3D_ERR_ARG, "p3d_sample_world: C must be in 1 .. 64");
  if (in_dtype != P3D_DTYPE_F32 && in_dtype != P3D_DTYPE_F64)
    return fail(P3D_ERR_ARG, "p3d_sample_world: in_dtype F32 or F64");
  if (!aligned16(out)) return fail(P3D_ERR_ARG, "p3d_sample_world: out must be 16-byte aligned");
  if (((uintptr_t)root & 7) != 0) return fail(P3D_ERR_ARG, "p3d_sample_world: root must be 8-byte aligned");
  SampleArgs a{yn, N, U, mean96, std96, dims_to_use, root, cams, C, cam_of_row, out};
  const int64_t tiles = (N + P3D_SAMPLE_ROWS - 1) / P3D_SAMPLE_ROWS;
  const dim3 grid((unsigned)(tiles < P3D_SAMPLE_MAX_BLOCKS ? tiles : P3D_SAMPLE_MAX_BLOCKS));
  hipStream_t s = (hipStream_t)stream;
  if (in_dtype == P3D_DTYPE_F64) k_sample_world<false, false><<<grid, 256, 0, s>>>(a);
  else if (aligned16(yn)) k_sample_world<true, true><<<grid, 256, 0, s>>>(a);
  else k_sample_world<true, false><<<grid, 256, 0, s>>>(a);
  LAUNCH_CHECK("k_sample_world");
  return 0;
}

// src/openpose_3dpose_sandbox.py:347-356 per call: normalise the mapped 2D rows (float32, the
// placeholder cast), the eval forward, unNormalizeData -- as ONE launch where the batch-1 chain
// runs (B <= 4, the model's hidden layers on the device at once), else as p3d_normalize +
// p3d_forward_ex + p3d_unnormalize; the same bits either way.
extern "C" int p3d_lift(p3d_model* m, const double* raw, int64_t B, int32_t D2, const double* mean2,
                        const double* std2, const int32_t* use2, int32_t U2, const double* mean3, const double* std3,
                        const int32_t* use3, int32_t U3, int32_t D3, double* out, void* stream) {
  if (!m || !raw || !mean2 || !std2 || !use2 || !mean3 || !std3 || !use3 || !out)
    return fail(P3D_ERR_ARG, "p3d_lift: null argument");
  const p3d_cfg& c = m->cfg;
  if (B <= 0 || B > c.max_batch) return fail(P3D_ERR_ARG, "p3d_lift: batch must be in 1..max_batch");
  if (U2 != c.input_size || U3 != c.output_size || D2 < U2 || D3 < U3 || D3 > 256)
    return fail(P3D_ERR_ARG, "p3d_lift: dimension sets do not match the model");
  if (c.dtype != P3D_DTYPE_F32 || !m->gemv.lift_x) return fail(P3D_ERR_ARG, "p3d_lift: float32 models only");
  hipStream_t st = (hipStream_t)stream;
  if (B <= m->knobs.gemv_maxb) {
    GemvFrames fr{};
    fr.raw = raw; fr.ldraw = D2; fr.mean2 = mean2; fr.std2 = std2; fr.use2 = use2;
    fr.out = out; fr.D3 = D3; fr.mean3 = mean3; fr.std3 = std3; fr.use3 = use3;
    if (m->host.hwait) { fr.hflag = m->host.hflag_dev; fr.hcnt = m->host.hcnt; fr.hseq = m->host.hwait; }
    const int r = forward_gemv(m, nullptr, B, nullptr, 1.0f, 0, 0, 0, 0, st, &fr);   // (keep 1: no dropout, seed unused)
    if (r == P3D_OK && m->host.hwait) m->host.harmed = true;
    if (r != 1) return r;
  }
  int r = p3d_normalize(raw, B, D2, mean2, std2, use2, U2, m->gemv.lift_x, P3D_DTYPE_F32, stream);
  if (r) return r;
  r = forward_impl(m, m->gemv.lift_x, B, m->gemv.lift_y, 0, 1.0f, 0, 0, 0, 0, stream, nullptr);
  if (r) return r;
  return p3d_unnormalize(m->gemv.lift_y, P3D_DTYPE_F32, B, U3, mean3, std3, use3, D3, out, stream);
}

extern "C" int64_t p3d_moments_workspace(int64_t F, int32_t D) {
  if (F <= 0 || D <= 0) return 0;
  return p3d_moments_blocks(F) * (int64_t)D * (int64_t)sizeof(double);
}

extern "C" int p3d_moments(const double* x, int64_t F, int32_t D, double* mean, double* stdv, void* work,
                           int64_t work_bytes, void* stream) {
  if (F <= 0 || D <= 0 || D > 256) return fail(P3D_ERR_ARG, "p3d_moments: need F >= 1 and 1 <= D <= 256");
  if (!x || !mean || !stdv || !work) return fail(P3D_ERR_ARG, "p3d_moments: null argument");
  if (work_bytes < p3d_moments_workspace(F, D)) return fail(P3D_ERR_ARG, "p3d_moments: workspace too small");
  const int64_t G = p3d_moments_blocks(F), chunk = (F + G - 1) / G;
  const hipStream_t st = (hipStream_t)stream;
  double* part = (double*)work;
  const dim3 gf((unsigned)D);
  k_col_partial<1><<<dim3((unsigned)G), 256, 0, st>>>(x, F, D, chunk, nullptr, part);
  k_col_final<1><<<gf, 256, 0, st>>>(part, (int)G, D, F, mean);
  k_col_partial<2><<<dim3((unsigned)G), 256, 0, st>>>(x, F, D, chunk, mean, part);
  k_col_final<2><<<gf, 256, 0, st>>>(part, (int)G, D, F, stdv);
  LAUNCH_CHECK("k_col_partial");
  return 0;
}

// ---------------------------------------------------------------------------------------
// CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) of host memory, slicing-by-8: the
// checksum of TF's tensor bundles (every tensor's bytes and every index-table block,
// checkpoint_io.py / tf_bundle.py), far too slow byte by byte in Python for 51 MB of state.
// crc = p3d_crc32c(data, n, 0) for a whole buffer; pass the previous result to continue.
// ---------------------------------------------------------------------------------------
namespace {
struct Crc32cTables {
  uint32_t t[8][256];
  Crc32cTables() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xFFu];
  }
};
const Crc32cTables& crc32c_tables() {
  static const Crc32cTables tb;
  return tb;
}
}  // namespace

extern "C" uint32_t p3d_crc32c(const void* data, int64_t n, uint32_t crc) {
  const Crc32cTables& tb = crc32c_tables();
  const unsigned char* p = (const unsigned char*)data;
  uint32_t c = ~crc;
  while (n > 0 && ((uintptr_t)p & 7)) { c = (c >> 8) ^ tb.t[0][(c ^ *p++) & 0xFFu]; --n; }
  while (n >= 8) {
    uint64_t v;
    memcpy(&v, p, 8);
    const uint32_t lo = (uint32_t)v ^ c, hi = (uint32_t)(v >> 32);
    c = tb.t[7][lo & 0xFF] ^ tb.t[6][(lo >> 8) & 0xFF] ^ tb.t[5][(lo >> 16) & 0xFF] ^ tb.t[4][lo >> 24] ^
        tb.t[3][hi & 0xFF] ^ tb.t[2][(hi >> 8) & 0xFF] ^ tb.t[1][(hi >> 16) & 0xFF] ^ tb.t[0][hi >> 24];
    p += 8;
    n -= 8;
  }
  while (n-- > 0) c = (c >> 8) ^ tb.t[0][(c ^ *p++) & 0xFFu];
  return ~c;
}
