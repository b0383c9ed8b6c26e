// p3d_vae_seq.h -- the temporal VAE filter run as a recurrence over whole sequences in ONE launch
// (src/3d_pose_vae_filter_kin.py:285-361 evaluate(), gfx950).  Device code only; the host side is
// in p3d_vae_host.h.
//
// The filter reads the last seq_len = in / out poses concatenated; frame f's refined pose r_f is
// written back into the buffer that feeds the next seq_len - 1 frames:
//
//   buffer = [p_0] * seq_len;  per frame: buffer = buffer[1:] + [p_f]; r_f = VAE(buffer); buffer[-1] = r_f
//
// Frame f needs frame f - 1, sequences need nothing of each other: a tile is 16 SEQUENCES (a row
// is a sequence, not a frame), the packed parameters go to LDS once, and the tile loops over the
// frames of its longest sequence with the [16, in] input tile -- the recurrence's state -- kept in
// LDS.  Rows whose sequence has ended run on their frozen state and write nothing.  The layers are
// vae_layer_fwd's arithmetic and the reparametrisation is vae_tile_fwd's, so row r of frame f is
// bit-identical to what k_vae_fwd returns for the same input row and eps row: an output element's
// MFMA k-chain depends on its own row only.
//
// Frame f + 1's pred, eps and target rows are global loads on a serial chain: pred and target are
// issued before frame f's layers and consumed behind them, eps behind frame f's reparametrisation
// and consumed by frame f + 1's, from registers.
//
// Two launch forms, bit-identical: k_vae_seq runs a tile on one wave, k_vae_seq4 on four waves
// that deal a layer's 16-column tiles among themselves (K is never split) with a workgroup barrier
// per layer; all four run the tile's common frame count, so the barrier is uniform.  No workgroup
// waits on another.
#pragma once
#include "p3d_vae.h"
#include "p3d_vae_desc.h"   // P3D_VAE_SEQ_MAX_LEN, VaeDesc

struct VaeSeqArgs {
  VaeDesc desc;               // by value: kernel arguments are uniform and invariant, so the layers' dimensions
                              // are scalar loads the frame loop does not wait on memory for (form 1)
  const VaeDesc* desc_dev;    // the device copy (form 0: one wave holds four times the per-thread state of
                              // form 1, and the scalars hoisted from a by-value copy do not fit beside it)
  const float* pk;            // packed parameters [Ppk]
  const float* pred;          // [N, out]
  const int64_t* seq_off;     // [S + 1]
  int64_t S, N;
  const float* eps;           // [N, latent] or null (draw from Philox)
  uint64_t seed, ctr;
  int64_t eps_row0;
  const float* target;        // [N, out] or null
  float* state;               // [S, (seq_len - 1) out] or null
  int32_t* started;           // [S] or null
  float* ref;                 // [N, out]
  float* frame_err;           // [N, 2] or null
  double* seq_err;            // [S, 2] or null
  int seq_len;
  int xoff, toff, ldt, moff;  // float offsets behind the packed copy: state tile, target tile, row metadata
};

template <int NW>
__device__ __forceinline__ void vae_seq_sync() {
  if (NW == 1) vae_wsync();
  else __syncthreads();
}

// vae_layer_fwd with the layer's column tiles dealt to the NW waves of the workgroup.  The k-chain of
// an output element is vae_layer_fwd's (k ascending, one accumulator); only the operand loads differ:
// the chain is serial and nothing else runs beside it, so its LDS latency is all there is to hide --
// four k-steps' operands are loaded one round ahead of the MFMAs that use them, and the operands
// of an odd last pair of k-steps before the first round.
template <int NW>
__device__ __forceinline__ void vae_seq_layer(const VaeLayer& L, const float* arow, const float* W, float* out) {
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4, wave = threadIdx.x >> 6;
  const int K = L.K, ld = L.ld, ldo = L.ldo, relu = L.relu, nct = L.Np >> 4;
  const int K16 = K & ~15;          // (every width is a multiple of 8)
  const bool tail = (K & 8) != 0;
  const float* ap = arow + q;
  for (int ct = wave; ct < nct; ct += NW) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wp = W + L.wpk + q * ld + 16 * ct + i;
    const float b = W[L.bpk + 16 * ct + i];
    const int kt = tail ? K16 : 0;  // (without a tail: any valid place, the values are not used)
    const float ta0 = ap[kt], tb0 = wp[kt * ld], ta1 = ap[kt + 4], tb1 = wp[(kt + 4) * ld];
    float av[4], bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kk = K16 ? 4 * j : 0;
      av[j] = ap[kk]; bv[j] = wp[kk * ld];
    }
    for (int k = 0; k < K16; k += 16) {
      const int kn = k + 16 < K16 ? k + 16 : k;   // (the last round loads its own operands again, unused)
      float an[4], bn[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { an[j] = ap[kn + 4 * j]; bn[j] = wp[(kn + 4 * j) * ld]; }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) { av[j] = an[j]; bv[j] = bn[j]; }
    }
    if (tail) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ta0, tb0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ta1, tb1, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[r] + b;
      if (relu) v = p3d_relu(v);
      out[(4 * q + r) * ldo + 16 * ct + i] = v;
    }
  }
}

template <int NW>
__device__ __forceinline__ void vae_seq_body(const VaeSeqArgs& a) {
  constexpr int NT = 64 * NW;
  constexpr int PER = 256 / NT;   // float4 units of a [16, <= 64] tile per thread
  extern __shared__ f32x4 vae_smem[];
  float* sm = (float*)vae_smem;
  const VaeDesc* d = NW == 1 ? a.desc_dev : &a.desc;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int lat = d->latent, out = d->out, SL = a.seq_len;
  float* act = sm + d->Ppk;
  float* xb = act + a.xoff;     // [16, ldx]: the state
  float* tg = act + a.toff;     // [16, ldt]: the frame's target rows
  int64_t* moff = (int64_t*)(act + a.moff);   // first frame of the row's sequence
  int* mlen = (int*)(moff + 16);              // its frame count
  const int ldx = d->ldx, ldt = a.ldt;
  const int64_t s0 = (int64_t)blockIdx.x * 16;

  for (int idx = tid; idx < (d->Ppk >> 2); idx += NT) ((f32x4*)sm)[idx] = ((const f32x4*)a.pk)[idx];
  {
    const int zp = d->ldz - lat;
    for (int idx = tid; idx < 16 * zp; idx += NT) {
      const int r = idx / zp, c = idx - r * zp;
      act[d->zbuf + r * d->ldz + lat + c] = 0.0f;
    }
  }
  if (tid < 16) {   // offsets clamped into [0, N]: a malformed table can touch no frame outside the arrays
    const int64_t s = s0 + tid;
    int64_t o0 = 0, o1 = 0;
    if (s < a.S) {
      o0 = a.seq_off[s]; o1 = a.seq_off[s + 1];
      o0 = o0 < 0 ? 0 : (o0 > a.N ? a.N : o0);
      o1 = o1 < o0 ? o0 : (o1 > a.N ? a.N : o1);
    }
    moff[tid] = o0;
    mlen[tid] = (int)(o1 - o0);
  }
  __syncthreads();
  int T = 0;
  for (int r = 0; r < 16; ++r) T = mlen[r] > T ? mlen[r] : T;
  const int64_t mys = s0 + i;
  const int mylen = mlen[i];
  const int64_t myoff = moff[i];
  const bool w_pred = wave == 0, w_ref = wave == (NW == 1 ? 0 : 1);   // the waves that form err_pred / err_ref
  if (T == 0) {
    if (a.seq_err && q == 0 && mys < a.S) {
      if (w_pred) a.seq_err[2 * mys] = 0.0;
      if (w_ref) a.seq_err[2 * mys + 1] = 0.0;
    }
    return;
  }

  // this thread's float4 units of the [16, out] tiles (pred, target, ref) and of the [16, latent] eps tile
  const int o4 = out >> 2, l4 = lat >> 2;
  int pr[PER], pc[PER], plen[PER], er[PER], ec[PER], elen[PER];
  int poff[PER], eoff[PER];   // (N <= 2^20: a frame index fits an int)
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int u = tid + j * NT;
    const int r = u / o4, r2 = u / l4;
    const bool pv = u < 16 * o4, ev = u < 16 * l4;
    pr[j] = pv ? r : 0; pc[j] = 4 * (u - r * o4);
    plen[j] = pv ? mlen[pr[j]] : 0; poff[j] = (int)moff[pr[j]];
    er[j] = ev ? r2 : 0; ec[j] = u - r2 * l4;
    elen[j] = ev ? mlen[er[j]] : 0; eoff[j] = (int)moff[er[j]];
  }
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 pN[PER], tN[PER], eN[PER];
  // frame f's rows into registers (rows whose sequence has ended: zero, never used): pred and target
  // before frame f - 1's encoder, eps behind frame f - 1's reparametrisation (its registers are free then)
  auto fetch_pt = [&](int f) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      pN[j] = zero4; tN[j] = zero4;
      if (f < plen[j]) {
        const int64_t g = (int64_t)(poff[j] + f) * out + pc[j];
        pN[j] = *(const f32x4*)(a.pred + g);
        if (a.target) tN[j] = *(const f32x4*)(a.target + g);
      }
    }
  };
  auto fetch_e = [&](int f) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      eN[j] = zero4;
      if (f < elen[j]) {
        const int64_t g = (int64_t)(eoff[j] + f);
        if (a.eps) {
          eN[j] = *(const f32x4*)(a.eps + g * lat + 4 * ec[j]);
        } else {
          float e[4];
          vae_eps4(a.seed, a.ctr, a.eps_row0 + g, ec[j], e);
          eN[j] = f32x4{e[0], e[1], e[2], e[3]};
        }
      }
    }
  };

  // ---- the state before frame 0: the carried groups, or frame 0's pred in every group ----
  fetch_pt(0);
  fetch_e(0);
  const int sw = (SL - 1) * out;   // floats of state per sequence
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (plen[j] > 0) {
      const int64_t s = s0 + pr[j];
      const bool carried = a.started && a.started[s] != 0;
      float* xr = xb + pr[j] * ldx + pc[j];
      for (int g = 0; g < SL - 1; ++g) {
        const f32x4 v = carried ? *(const f32x4*)(a.state + s * sw + g * out + pc[j]) : pN[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) xr[g * out + k] = v[k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xr[(SL - 1) * out + k] = pN[j][k];
        tg[pr[j] * ldt + pc[j] + k] = tN[j][k];
      }
    }
  }
  __syncthreads();

  const VaeLayer& H = d->L[d->head];
  float* ml = act + H.aout;
  const int ldm = H.ldo, ldz = d->ldz;
  float* zb = act + d->zbuf;
  float* yb = act + d->L[d->nl - 1].aout;
  const int ldy = d->L[d->nl - 1].ldo;
  double acc_pred = 0.0, acc_ref = 0.0;
  float e_pred = 0.0f, e_ref = 0.0f;
  // Frame fr's global writes: r_f from the output layer's tile (it stands until the next frame's last
  // layer) and the two errors from registers.  They are issued at the top of frame fr + 1, beside its
  // loads: the memory counter that the loads' consumers wait on counts stores too, so a store issued
  // at a frame's end would be waited for in full.
  auto flush = [&](int fr) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (fr < plen[j]) {
        const float* yr = yb + pr[j] * ldy + pc[j];
        *(f32x4*)(a.ref + (int64_t)(poff[j] + fr) * out + pc[j]) = f32x4{yr[0], yr[1], yr[2], yr[3]};
      }
    }
    if (a.frame_err && q == 0 && fr < mylen) {
      if (w_pred) a.frame_err[2 * (myoff + fr)] = e_pred;
      if (w_ref) a.frame_err[2 * (myoff + fr) + 1] = e_ref;
    }
  };

  for (int f = 0; f < T; ++f) {
    fetch_pt(f + 1);   // (in flight under this frame's layers)
    if (f > 0) flush(f - 1);
    // ---- encoder ----
    vae_seq_layer<NW>(d->L[0], xb + i * ldx, sm, act + d->L[0].aout);
    vae_seq_sync<NW>();
    for (int l = 1; l <= d->head; ++l) {
      const VaeLayer& L = d->L[l];
      vae_seq_layer<NW>(L, act + L.ain + i * L.lda, sm, act + L.aout);
      vae_seq_sync<NW>();
    }
    // ---- z = eps exp(0.5 log_var) + mean, as vae_tile_fwd forms it ----
    {
#pragma clang fp contract(off)
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        if (tid + j * NT < 16 * l4) {
          const int r = er[j];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int c = 4 * ec[j] + k;
            const float mu = ml[r * ldm + c], lv = ml[r * ldm + lat + c];
            const float sd = expf(0.5f * lv);
            const float es = eN[j][k] * sd;
            const float zz = es + mu;
            zb[r * ldz + c] = zz;
          }
        }
      }
    }
    fetch_e(f + 1);    // (in flight under the decoder and the next frame's encoder)
    vae_seq_sync<NW>();
    // ---- decoder ----
    for (int l = d->head + 1; l < d->nl; ++l) {
      const VaeLayer& L = d->L[l];
      vae_seq_layer<NW>(L, act + L.ain + i * L.lda, sm, act + L.aout);
      vae_seq_sync<NW>();
    }
    // ---- err_pred = mean (y - p)^2, err_ref = mean (y - r)^2, associated as vae_tile_fwd's terms[0] ----
    if (a.target) {
#pragma clang fp contract(off)
      const float* trow = tg + i * ldt;
      if (w_pred) {
        const float* prow = xb + i * ldx + (SL - 1) * out;
        float p = 0.0f;
        for (int c = q; c < out; c += 4) {
          const float df = trow[c] - prow[c];
          p += df * df;
        }
        const float e = vae_rowsum4(p) / (float)out;
        e_pred = e;
        if (q == 0 && f < mylen) acc_pred += (double)e;
      }
      if (w_ref) {
        const float* rrow = yb + i * ldy;
        float p = 0.0f;
        for (int c = q; c < out; c += 4) {
          const float df = trow[c] - rrow[c];
          p += df * df;
        }
        const float e = vae_rowsum4(p) / (float)out;
        e_ref = e;
        if (q == 0 && f < mylen) acc_ref += (double)e;
      }
      vae_seq_sync<NW>();   // (the state's last group and the target tile have been read)
    }
    // ---- the state of frame f + 1: groups shifted left, r_f behind them, then p_{f+1} ----
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (f < plen[j]) {
        float* xr = xb + pr[j] * ldx + pc[j];
        const float* yr = yb + pr[j] * ldy + pc[j];
        const bool more = f + 1 < plen[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          for (int g = 0; g < SL - 1; ++g) xr[g * out + k] = g + 1 < SL - 1 ? xr[(g + 1) * out + k] : yr[k];
          if (more) {
            xr[(SL - 1) * out + k] = pN[j][k];
            tg[pr[j] * ldt + pc[j] + k] = tN[j][k];
          }
        }
      }
    }
    vae_seq_sync<NW>();
  }

  flush(T - 1);
  // ---- the carried groups, the started flags, the sequences' error sums ----
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (plen[j] > 0 && a.state) {
      const int64_t s = s0 + pr[j];
      const float* xr = xb + pr[j] * ldx + pc[j];
      for (int g = 0; g < SL - 1; ++g)
        *(f32x4*)(a.state + s * sw + g * out + pc[j]) = f32x4{xr[g * out], xr[g * out + 1], xr[g * out + 2], xr[g * out + 3]};
      if (pc[j] == 0) a.started[s] = 1;
    }
  }
  if (a.seq_err && q == 0 && mys < a.S) {
    if (w_pred) a.seq_err[2 * mys] = acc_pred;
    if (w_ref) a.seq_err[2 * mys + 1] = acc_ref;
  }
}

__global__ __launch_bounds__(64) void k_vae_seq(VaeSeqArgs a) { vae_seq_body<1>(a); }
__global__ __launch_bounds__(256) void k_vae_seq4(VaeSeqArgs a) { vae_seq_body<4>(a); }
