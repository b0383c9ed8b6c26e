// p3d_skel.h -- lifted rows as a rigid skeleton (gfx950; include/p3d.h: p3d_skel_*):
// constant bone lengths per clip, one shortest-arc rotation per bone and frame, Euler angles in
// BVH's Z X Y order and the forward kinematics with the constant lengths.  Device code only; the
// host side is in p3d_skel_host.h.
//
//   k_skel_len_part   per chunk of one clip: the per-bone sums of |J[jb] - J[ja]| over the frames
//                     that count, and their number
//   k_skel_len_fold   per clip: the chunks' partials in a fixed order -> lengths [S, 16], n_used [S]
//   k_skel_pose       per frame: quat [N, 16, 4], euler [N, 16, 3], rigid [N, 17, 3], root [N, 3]
//
// A row is a `poses` row of the clip calls, [96] float64 = 32 joints in exported coordinates; the 17
// skeleton joints are the H3.6M joints of skel_h36m(), joint 0 the hip, in skeleton coordinates
// (X, Y, Z) = (x, z, -y).  The bones are p3d_bones.h's (bones_ja / bones_jb / bones_pb); the rest
// direction of bone b is skel_rest(b).  The lengths' chunks are the clip kernels' (P3D_CLIP_CHUNK
// frames, starting again at every clip: ClipSeg, k_clips_index, clip_where of p3d_clips.h), so a
// clip's sums are formed in the same order alone and inside a batch.  No atomics, no waiting
// between workgroups.  All arithmetic float64, every operation rounded on its own (tests/skel_oracle.py
// states the same operations).
#pragma once
#include "p3d_bones.h"
#include "p3d_clips.h"

#define P3D_SKEL_THREADS 256
#define P3D_SKEL_ROWS (P3D_SKEL_THREADS / 16)     // rows of one pass: 16 lanes per row, one per bone
#define P3D_SKEL_LDS_ROW 97                       // doubles per staged row (96 and one of padding)

// the H3.6M joint of skeleton joint j (0 .. 16), five bits each: {0,1,2,3,6,7,8,12,13,14,15,17} | {18,19,25,26,27}
#define P3D_SKEL_H36M_LO 0x8BDCD620E618820ull
#define P3D_SKEL_H36M_HI 0x1BD6672ull
__device__ __forceinline__ int skel_h36m(int j) {
  return j < 12 ? (int)((P3D_SKEL_H36M_LO >> (5 * j)) & 31) : (int)((P3D_SKEL_H36M_HI >> (5 * (j - 12))) & 31);
}

// The rest direction of bone b, by its child joint: hips, shoulders, elbows and wrists along -X
// (right) / +X (left), knees and feet along -Y, spine, thorax, neck and head along +Y.  Z is 0.
#define P3D_SKEL_REST_Y 0x03F6u     // bit b: the rest direction is along Y (else X)
#define P3D_SKEL_REST_NEG 0x1C37u   // bit b: it points to the negative side
__device__ __forceinline__ void skel_rest(int b, double& rx, double& ry) {
  const double s = (P3D_SKEL_REST_NEG >> b) & 1 ? -1.0 : 1.0;
  const bool y = (P3D_SKEL_REST_Y >> b) & 1;
  rx = y ? 0.0 : s;
  ry = y ? s : 0.0;
}

// skeleton joint j of a row (exported coordinates, `row` = 32 joints x 3) in skeleton coordinates
__device__ __forceinline__ void skel_joint(const double* row, int j, double p[3]) {
  const double* q = row + 3 * skel_h36m(j);
  p[0] = q[0];
  p[1] = q[2];
  p[2] = -q[1];
}

// bone bb of a row: v = J[jb] - J[ja], len = sqrt((vx^2 + vy^2) + vz^2)
__device__ __forceinline__ double skel_bone(const double* row, int bb, double v[3]) {
#pragma clang fp contract(off)
  double a[3], c[3];
  skel_joint(row, bones_ja(bb), a);
  skel_joint(row, bones_jb(bb), c);
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = c[k] - a[k];
  return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

// ---- the lengths ------------------------------------------------------------------------------
struct SkelLenArgs {
  const double* poses;   // [N, 96]
  const int32_t* src;    // [N] or null (every row its own)
  int64_t N;
  double* psum;          // workspace [chunks, 16]
  int64_t* pcnt;         // workspace [chunks]
  double* lengths;       // [S, 16]
  int64_t* n_used;       // [S]
  int32_t nch;           // the grid's chunk total: psum / pcnt hold that many
};

// One workgroup per chunk k of a clip, 16 lanes per frame, 16 frames per pass.  A frame counts
// when src says it carries its own pose and its 17 joints are finite.  Thread (g, b) sums bone b
// over frames g, g + 16, ... of the chunk in that order, then lane b of the first 16 adds the 16
// values in the order of g: the order depends on the position inside the chunk alone.
__global__ __launch_bounds__(P3D_SKEL_THREADS) void k_skel_len_part(SkelLenArgs a, ClipSeg sg) {
#pragma clang fp contract(off)
  constexpr int C = P3D_CLIP_CHUNK, R = P3D_SKEL_ROWS;
  __shared__ double ssum[R][16];
  __shared__ int scnt[R];
  const int t = threadIdx.x, b = t & 15, g = t >> 4;
  const int64_t k = blockIdx.x;
  ClipWhere cw;
  if (!clip_where(sg, a.N, k, cw)) return;   // (uniform)
  const int nf = (int)min((int64_t)C, cw.hi - cw.c0);
  double sum = 0.0;
  int cnt = 0;
  for (int i = g; i < C; i += R) {           // (every lane runs every trip: the ballot)
    const bool in = i < nf;
    const int64_t n = cw.c0 + (in ? i : 0);  // (a frame of the clip: cw.c0 < cw.hi)
    const double* row = a.poses + n * P3D_CLIP_D3;
    double v[3], h[3], c[3];
    const double len = skel_bone(row, b, v);
    // lane b vouches for the bone's child joint and for the hip: the 16 lanes for the 17 joints
    skel_joint(row, 0, h);
    skel_joint(row, bones_jb(b), c);
    const bool ok = isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(h[0]) && isfinite(h[1]) && isfinite(h[2]);
    const unsigned long long m = __ballot(ok);
    const bool all = ((m >> (t & 48)) & 0xFFFFull) == 0xFFFFull;
    const bool own = a.src ? a.src[n] == (int32_t)n : true;
    if (in && all && own) {
      sum = sum + len;
      ++cnt;
    }
  }
  ssum[g][b] = sum;
  if (b == 0) scnt[g] = cnt;
  __syncthreads();
  if (t < 16) {
    double s = ssum[0][t];
    int c = scnt[0];
    for (int q = 1; q < R; ++q) { s = s + ssum[q][t]; c += scnt[q]; }
    a.psum[k * 16 + t] = s;
    if (t == 0) a.pcnt[k] = c;
  }
}

// One workgroup per clip: thread (g, b) sums bone b over the g-th of 16 contiguous spans of the
// clip's chunks in chunk order, lane b of the first 16 adds the spans in order and divides by the
// count (no frame counts: zeros).  The spans depend on the clip's chunk count alone.
__global__ __launch_bounds__(P3D_SKEL_THREADS) void k_skel_len_fold(SkelLenArgs a, ClipSeg sg) {
#pragma clang fp contract(off)
  constexpr int R = P3D_SKEL_ROWS;
  __shared__ double ssum[R][16];
  __shared__ int64_t scnt[R];
  const int t = threadIdx.x, b = t & 15, g = t >> 4;
  const int64_t s = blockIdx.x;
  if (s >= sg.S) return;
  // the clip's chunks, whatever the device offsets gave, inside what k_skel_len_part wrote
  const int k0 = min(max(sg.chunk_base[s], 0), a.nch);
  const int k1 = min(max(sg.chunk_base[s + 1], k0), a.nch);
  const int per = (k1 - k0 + R - 1) / R;
  const int q0 = min(k0 + g * per, k1), q1 = min(q0 + per, k1);
  double sum = 0.0;
  int64_t cnt = 0;
  for (int q = q0; q < q1; q += 8) {   // eight loads in flight (addresses clamped), added in chunk order
    double v[8];
    int64_t c[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t i = min(q + u, q1 - 1);
      v[u] = a.psum[i * 16 + b];
      c[u] = a.pcnt[i];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (q + u < q1) {
        sum = sum + v[u];
        cnt += c[u];
      }
  }
  ssum[g][b] = sum;
  if (b == 0) scnt[g] = cnt;
  __syncthreads();
  if (t < 16) {
    double v = ssum[0][t];
    int64_t c = scnt[0];
    for (int q = 1; q < R; ++q) { v = v + ssum[q][t]; c += scnt[q]; }
    a.lengths[s * 16 + t] = c > 0 ? v / (double)c : 0.0;
    if (t == 0) a.n_used[s] = c;
  }
}

// ---- the pose of a frame ----------------------------------------------------------------------
struct SkelPoseArgs {
  const double* poses;    // [N, 96]
  const int32_t* src;     // [N] or null; src[n] < 0: the row counts as zeros
  const int64_t* off;     // device [S + 1], read clamped into [0, N]
  const double* lengths;  // [S, 16]
  int64_t S, N;
  double *quat, *euler, *rigid, *root;   // each may be null
};

// the shortest arc from the unit rest direction (rx, ry, 0) to the unit direction d, (w, x, y, z):
// normalize(1 + r.d, r x d); antiparallel: half a turn about Z
__device__ __forceinline__ void skel_arc(double rx, double ry, const double d[3], double g[4]) {
#pragma clang fp contract(off)
  const double w = 1.0 + (rx * d[0] + ry * d[1]);
  if (w < 1e-12) {
    g[0] = 0.0; g[1] = 0.0; g[2] = 0.0; g[3] = 1.0;
    return;
  }
  const double cx = ry * d[2], cy = -(rx * d[2]), cz = rx * d[1] - ry * d[0];
  const double inv = 1.0 / sqrt((w * w + cx * cx) + (cy * cy + cz * cz));
  g[0] = w * inv; g[1] = cx * inv; g[2] = cy * inv; g[3] = cz * inv;
}

// 16 rows per workgroup, staged through LDS with whole-row loads; lane b of a row walks the path
// of bone b from the hip (at most 6 bones: k_bones_to_joints' walk), so its joint's rigid position
// and its parent's direction need no exchange between lanes.  A row's 16 lanes store 512 (quat),
// 384 (euler) and 408 (rigid) contiguous bytes between them.
__global__ __launch_bounds__(P3D_SKEL_THREADS) void k_skel_pose(SkelPoseArgs a) {
#pragma clang fp contract(off)
  constexpr int R = P3D_SKEL_ROWS, D = P3D_CLIP_D3, W = P3D_SKEL_LDS_ROW, PER = R * D / P3D_SKEL_THREADS;
  static_assert(R * D % P3D_SKEL_THREADS == 0, "whole values per thread");
  __shared__ double srow[R * W];
  const int t = threadIdx.x, b = t & 15, g = t >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  if (r0 >= a.N) return;   // (uniform)
  {   // the 16 rows are contiguous: every load issued before the first is waited for (addresses clamped)
    const int64_t last = a.N * D - 1;
    double v[PER];
    int32_t sv[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int64_t e = min(r0 * D + t + q * P3D_SKEL_THREADS, last);
      v[q] = a.poses[e];
      sv[q] = a.src ? a.src[e / D] : 0;
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int idx = t + q * P3D_SKEL_THREADS;
      srow[(idx / D) * W + idx % D] = sv[q] < 0 ? 0.0 : v[q];
    }
  }
  __syncthreads();
  const int64_t n = r0 + g;
  if (n >= a.N) return;
  const double* row = srow + g * W;

  // the row's clip: off[s] <= n < off[s + 1] over the clamped offsets (S = 1: no loads)
  int64_t s = 0;
  for (int64_t hi = a.S; hi - s > 1;) {
    const int64_t mid = (s + hi) >> 1;
    if (min(max(a.off[mid], (int64_t)0), a.N) <= n) s = mid; else hi = mid;
  }
  const double* L = a.lengths + s * 16;

  uint32_t path = 0;   // the bones from the hip to b, the hip's first, one nibble each (at most 6)
  int np = 0;
  for (int p = b; p >= 0 && np < 6; p = bones_pb(p), ++np) path = (path << 4) | (uint32_t)p;
  double hip[3], pos[3];
  skel_joint(row, 0, hip);
#pragma unroll
  for (int c = 0; c < 3; ++c) pos[c] = hip[c];
  double d[3] = {0.0, 0.0, 0.0}, dp[3] = {0.0, 0.0, 0.0};   // the bone's direction and its parent's
  bool z = true, zp = true;                                    // ... of zero length: the rest direction
  for (int k = 0; k < np; ++k, path >>= 4) {
    const int bb = (int)(path & 15);
    double v[3], rx, ry;
    const double len = skel_bone(row, bb, v);
    skel_rest(bb, rx, ry);
    zp = z;
#pragma unroll
    for (int c = 0; c < 3; ++c) dp[c] = d[c];
    z = len == 0.0;
    const double inv = 1.0 / len;
    d[0] = z ? rx : v[0] * inv;
    d[1] = z ? ry : v[1] * inv;
    d[2] = z ? 0.0 : v[2] * inv;
    const double Lb = L[bb];
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[c] = pos[c] + Lb * d[c];
  }

  if (a.rigid) {
    double* o = a.rigid + n * 51;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[3 * bones_jb(b) + c] = pos[c];
    if (b == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = hip[c];
    }
  }
  if (a.root && b == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.root[n * 3 + c] = hip[c];
  }
  if (!a.quat && !a.euler) return;   // (uniform)

  // g_b and g_pb: a zero-length bone is the identity; q_b = conj(g_pb) (x) g_b
  double rx, ry, gb[4] = {1.0, 0.0, 0.0, 0.0}, gp[4] = {1.0, 0.0, 0.0, 0.0}, q[4];
  const int pb = bones_pb(b);
  skel_rest(b, rx, ry);
  if (!z) skel_arc(rx, ry, d, gb);
  if (pb >= 0) {
    skel_rest(pb, rx, ry);
    if (!zp) skel_arc(rx, ry, dp, gp);
    const double pw = gp[0], px = -gp[1], py = -gp[2], pz = -gp[3];
    q[0] = ((pw * gb[0] - px * gb[1]) - py * gb[2]) - pz * gb[3];
    q[1] = ((pw * gb[1] + px * gb[0]) + py * gb[3]) - pz * gb[2];
    q[2] = ((pw * gb[2] - px * gb[3]) + py * gb[0]) + pz * gb[1];
    q[3] = ((pw * gb[3] + px * gb[2]) - py * gb[1]) + pz * gb[0];
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = gb[c];
  }
  if (a.quat) {
    double* o = a.quat + n * 64 + 4 * b;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = q[c];
  }
  if (!a.euler) return;   // (uniform)

  // R = Rz Rx Ry of the matrix of q, degrees; atan2 throughout (asin loses half the digits near 90)
  const double w = q[0], x = q[1], y = q[2], zz = q[3];
  const double r00 = 1.0 - 2.0 * (y * y + zz * zz), r01 = 2.0 * (x * y - w * zz);
  const double r10 = 2.0 * (x * y + w * zz), r11 = 1.0 - 2.0 * (x * x + zz * zz);
  const double r20 = 2.0 * (x * zz - w * y), r21 = 2.0 * (y * zz + w * x), r22 = 1.0 - 2.0 * (x * x + y * y);
  const double hx = hypot(r01, r11);
  const bool gimbal = hx < 1e-12;
  const double ex = atan2(r21, hx);
  const double ez = gimbal ? atan2(r10, r00) : atan2(-r01, r11);
  const double ey = gimbal ? 0.0 : atan2(-r20, r22);
  constexpr double DEG = 57.29577951308232;   // 180 / pi
  double* o = a.euler + n * 48 + 3 * b;
  o[0] = ez * DEG;   // the channel order: Zrotation Xrotation Yrotation
  o[1] = ex * DEG;
  o[2] = ey * DEG;
}
