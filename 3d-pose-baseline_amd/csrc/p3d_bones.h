// p3d_bones.h -- joints <-> bones of the bones filter (gfx950): src/top_vae_3d_pose/bones.py:71-98
// (convert_to_bones_tf), :101-121 (convert_to_bones) and :124-153 (convert_to_joints).  Device code
// only; the host side is in p3d_vae_host.h.
//
// The skeleton has joints 0 .. 16 with the hip, joint 0, at the origin; joint k >= 1 is columns
// 3 (k - 1) .. 3 (k - 1) + 2 of a 48-vector.  Bone b runs from joint BJA[b] to joint BJB[b]
// (bones.py:74-75, and what get_bones_joints yields on src/bones_mapping.yml); a bone's parent
// joint is produced by an earlier bone.
//
// A row of bones is [mag (16) | cos (16 x 3)], 64 floats: model.concat([mags, dir_cos])
// (models.py:528-530), so one buffer is the filter's input segment and the loss's target.
//
// One lane per (row, bone): the 16 lanes of a row read 192 and write 256 (384 for the joints)
// contiguous bytes between them.  No LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// BJA[b], BJB[b] in nibble b
#define P3D_BONES_JA 0xCB9FE99870540210ull
#define P3D_BONES_JB 0xDCB0FEA987654321ull   // (16 does not fit a nibble: see bones_jb)
// the bone that produces BJA[b], plus 1 (0: the hip), in nibble b
#define P3D_BONES_PB 0xFE9CB99870540210ull

__device__ __forceinline__ int bones_ja(int b) { return (int)((P3D_BONES_JA >> (4 * b)) & 15); }
__device__ __forceinline__ int bones_jb(int b) { return b == 12 ? 16 : (int)((P3D_BONES_JB >> (4 * b)) & 15); }
__device__ __forceinline__ int bones_pb(int b) { return (int)((P3D_BONES_PB >> (4 * b)) & 15) - 1; }

// [B, 48] float32 joints -> [B, 64] = [mag | cos].  v = J[BJB] - J[BJA], mag = sqrt((vx^2 + vy^2) +
// vz^2), cos = v / mag; a zero-length bone gives 0 / 0 = NaN cosines.  PRECISE: float64 throughout,
// rounded to float32 once at the end (convert_to_bones: the float32 joints are widened by the
// concatenation with the float64 hip); else float32 throughout (convert_to_bones_tf).  Every
// operation is rounded on its own: no FMA contraction.
template <bool PRECISE>
__global__ __launch_bounds__(256) void k_bones_from_joints(const float* __restrict__ joints, int64_t B,
                                                           float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= B * 16) return;
  const int64_t row = u >> 4;
  const int b = (int)(u & 15);
  const int ja = bones_ja(b), jb = bones_jb(b);
  const float* j = joints + row * 48;
  float pb[3], pa[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    pb[c] = j[3 * (jb - 1) + c];
    pa[c] = ja > 0 ? j[3 * (ja - 1) + c] : 0.0f;
  }
  float* o = out + row * 64;
  if (PRECISE) {
    double v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (double)pb[c] - (double)pa[c];
    const double mag = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    o[b] = (float)mag;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[16 + 3 * b + c] = (float)(v[c] / mag);
  } else {
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = pb[c] - pa[c];
    const float mag = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    o[b] = mag;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[16 + 3 * b + c] = v[c] / mag;
  }
}

// [B, 64] = [mag | cos] -> float64 [B, 48] joints: in bone order J[BJB[b]] = J[BJA[b]] +
// (double)(cos[b] * mag[b]), the product float32 and rounded once, the running position float64
// from the hip's 0.0 on (convert_to_joints).  A lane walks its own bone's path from the hip, so
// joint BJB[b] is the same chain of additions whichever lane forms it.
__global__ __launch_bounds__(256) void k_bones_to_joints(const float* __restrict__ bones, int64_t B,
                                                         double* __restrict__ joints) {
#pragma clang fp contract(off)
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= B * 16) return;
  const int64_t row = u >> 4;
  const int b = (int)(u & 15);
  uint32_t path = 0;   // the bones from the hip to b, the hip's first, one nibble each (at most 6)
  int n = 0;
  for (int p = b; p >= 0 && n < 6; p = bones_pb(p), ++n) path = (path << 4) | (uint32_t)p;
  const float* r = bones + row * 64;
  double pos[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < n; ++k, path >>= 4) {
    const int bb = (int)(path & 15);
    const float mg = r[bb];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float pr = r[16 + 3 * bb + c] * mg;
      pos[c] = pos[c] + (double)pr;
    }
  }
  double* o = joints + row * 48 + 3 * (bones_jb(b) - 1);
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = pos[c];
}
