// p3d_vae_mc.h -- the VAE filter averaged over K posterior samples inside one launch (gfx950):
// the encoder runs once per row, the decoder K times on the tile that is already in LDS, and the
// running mean and the sum of squared deviations of the K outputs are folded in registers.  Device
// code only; the host side is in p3d_vae_host.h.
//
// For a row with encoder outputs mean, log_var and K draws eps_k, sample k is
//
//   y_k = decoder(eps_k exp(0.5 log_var) + mean)
//
// in exactly the arithmetic of vae_tile_fwd and vae_layer_fwd (the layers ARE vae_layer_fwd, the
// reparametrisation is vae_tile_fwd's, k-chains included): with the caller's eps_k, y_k has the bits
// p3d_vae_forward writes for that eps; with eps null, draw k is the library's stream at counter
// ctr + k (same seed, same site, row r of the call).  Per output element, in float32 with every
// operation rounded once and no division on the device:
//
//   m = y_0;  M = 0
//   for k = 1 .. K - 1:   d = y_k - m;   m = m + d c_k;   M = M + d (y_k - m)
//   y_mean = m            y_var = M c_{K-1}              c_j = (float)(1.0 / (double)(j + 1))
//
// K = 1 gives y_mean = y_0 bit for bit and y_var = 0.
//
// k_vae_fwd_mc / k_vae_fwd_mc_cat: the forward's FULL LDS layout, four waves that stride over the
// 16-row tiles.  A lane folds the elements idx = lane + 64 j of its wave's y tile (the mapping of the
// forward's y store; at most 16 at out = 64) and holds their m and M in registers over the K
// passes.  The head's tile (mean | log_var) is no layer's input buffer but the reparametrisation's,
// so it stands through the passes; each pass overwrites only the z tile and the decoder's tiles.
//
// k_vae_seq4_mc: the four-wave sequence form (p3d_vae_seq.h).  Per frame the encoder runs once on
// the state tile, then K decoder passes; a thread folds its own float4 unit of the [16, out] tile
// (16 out / 256 <= 4 elements).  r_f = y_mean goes to ref, into the y tile (err_ref is taken of it)
// and into the state tile as the recurrence's feedback.  pred and target keep their places on the
// serial chain; ONE eps unit per thread is in flight at a time: draw k + 1's is requested behind
// draw k's reparametrisation, frame f + 1's first behind frame f's last (a runtime K of up to 64
// units does not fit the registers beside the frame's state).
#pragma once
#include "p3d_vae.h"
#include "p3d_vae_seq.h"

#define P3D_VAE_MC_MAX_K 64

// c_j = (float)(1.0 / (double)(j + 1)), formed at compile time
struct VaeMcC { float c[P3D_VAE_MC_MAX_K]; };
constexpr VaeMcC vae_mc_make_c() {
  VaeMcC t{};
  for (int j = 0; j < P3D_VAE_MC_MAX_K; ++j) t.c[j] = (float)(1.0 / (double)(j + 1));
  return t;
}
__device__ const VaeMcC kVaeMcC = vae_mc_make_c();

// one step of the fold: sample y at draw k >= 1 into (m, M)
__device__ __forceinline__ void vae_mc_fold(float y, float ck, float& m, float& M) {
#pragma clang fp contract(off)
  const float d = y - m;
  const float dc = d * ck;
  m = m + dc;
  const float d2 = y - m;
  const float p = d * d2;
  M = M + p;
}

struct VaeMcArgs {
  VaeArgs a;        // the forward's arguments: a.y is y_mean; a.eps is [K, B, latent] or null; a.t, a.z, a.row_terms unused
  float* y_var;     // [B, out] or null
  int K;
};

template <bool CAT>
__device__ __forceinline__ void vae_mc_body(const VaeMcArgs& ma) {
  extern __shared__ f32x4 vae_smem[];
  float* sm = (float*)vae_smem;
  const VaeArgs& a = ma.a;
  const VaeDesc* d = a.desc;
  vae_load_params(a, d, sm);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15;
  float* act = sm + d->Ppk + wave * d->act;
  const float* W = sm;
  const int lat = d->latent, out = d->out, K = ma.K;
  const int64_t Bm1 = a.B - 1;
  const float* ml = act + d->L[d->head].aout;
  const int ldm = d->L[d->head].ldo;
  float* zb = act + d->zbuf;
  const float* yb = act + d->L[d->nl - 1].aout;
  const int ldy = d->L[d->nl - 1].ldo;
  const int nel = 16 * out;
  // this lane's elements of the y tile: their places in LDS and in a [16, out] tile of the output
  int yo[16], go[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int idx = lane + 64 * j;
    const int r = idx / out, c = idx - r * out;
    yo[j] = idx < nel ? r * ldy + c : 0;
    go[j] = idx < nel ? r : 16;            // (row of the tile; 16: not an element)
  }
  const float cl = kVaeMcC.c[K - 1];
  const int64_t ntiles = (a.B + 15) >> 4;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row0 = tile * 16;
    const int64_t myrow = row0 + i < a.B ? row0 + i : Bm1;
    // ---- encoder: vae_tile_fwd's ----
    if (d->xbuf >= 0) {
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
    float m[16], M[16];
    for (int k = 0; k < K; ++k) {
      // ---- z_k = eps_k exp(0.5 log_var) + mean, as vae_tile_fwd forms it ----
      {
#pragma clang fp contract(off)
        const int c4n = lat >> 2;
        const float* ek = a.eps ? a.eps + (int64_t)k * a.B * lat : nullptr;
        for (int u = lane; u < 16 * c4n; u += 64) {
          const int r = u / c4n, c4 = u - r * c4n;
          const bool valid = row0 + r < a.B;
          const int64_t grow = valid ? row0 + r : Bm1;
          float e[4];
          if (ek) {
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = ek[grow * lat + 4 * c4 + j];
          } else {
            vae_eps4(a.seed, a.ctr + (uint64_t)k, grow, c4, e);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = 4 * c4 + j;
            const float mu = ml[r * ldm + c], lv = ml[r * ldm + lat + c];
            const float sd = expf(0.5f * lv);
            const float es = e[j] * sd;
            const float zz = es + mu;
            zb[r * d->ldz + c] = zz;
            if (k == 0 && valid) {
              if (a.mean) a.mean[grow * lat + c] = mu;
              if (a.log_var) a.log_var[grow * lat + c] = lv;
            }
          }
        }
      }
      vae_wsync();
      // ---- decoder ----
      for (int l = d->head + 1; l < d->nl; ++l) {
        const VaeLayer& L = d->L[l];
        vae_layer_fwd(L, act + L.ain + i * L.lda, W, act + L.aout);
        vae_wsync();
      }
      // ---- the fold, in registers ----
      if (k == 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) { m[j] = yb[yo[j]]; M[j] = 0.0f; }
      } else {
        const float ck = kVaeMcC.c[k];
#pragma unroll
        for (int j = 0; j < 16; ++j) vae_mc_fold(yb[yo[j]], ck, m[j], M[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int idx = lane + 64 * j;
      if (go[j] < 16 && row0 + go[j] < a.B) {
#pragma clang fp contract(off)
        a.y[row0 * out + idx] = m[j];       // ((row0 + r) out + c = row0 out + idx)
        if (ma.y_var) ma.y_var[row0 * out + idx] = M[j] * cl;
      }
    }
    vae_wsync();   // (the next tile's layers overwrite what the last fold read)
  }
}
__global__ __launch_bounds__(256) void k_vae_fwd_mc(VaeMcArgs a) { vae_mc_body<false>(a); }
__global__ __launch_bounds__(256) void k_vae_fwd_mc_cat(VaeMcArgs a) { vae_mc_body<true>(a); }

struct VaeSeqMcArgs {
  VaeSeqArgs s;     // the sequence filter's arguments: s.ref is the mean; s.eps is [K, N, latent] or null
  float* ref_var;   // [N, out] or null
  int K;
};

// vae_seq_body<4> with K decoder passes per frame and the fold between them.
__global__ __launch_bounds__(256) void k_vae_seq4_mc(VaeSeqMcArgs ma) {
  constexpr int NW = 4, NT = 256;
  extern __shared__ f32x4 vae_smem[];
  float* sm = (float*)vae_smem;
  const VaeSeqArgs& a = ma.s;
  const VaeDesc* d = &a.desc;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int lat = d->latent, out = d->out, SL = a.seq_len, K = ma.K;
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
  const bool w_pred = wave == 0, w_ref = wave == 1;   // the waves that form err_pred / err_ref
  if (T == 0) {
    if (a.seq_err && q == 0 && mys < a.S) {
      if (w_pred) a.seq_err[2 * mys] = 0.0;
      if (w_ref) a.seq_err[2 * mys + 1] = 0.0;
    }
    return;
  }

  // this thread's float4 unit of the [16, out] tiles (pred, target, ref) and of the [16, latent] eps tile
  const int o4 = out >> 2, l4 = lat >> 2;
  const int up = tid / o4, ue = tid / l4;
  const bool pv = tid < 16 * o4, ev = tid < 16 * l4;
  const int pr = pv ? up : 0, pc = 4 * (tid - up * o4);
  const int plen = pv ? mlen[pr] : 0, poff = (int)moff[pr];   // (N <= 2^20: a frame index fits an int)
  const int er = ev ? ue : 0, ec = tid - ue * l4;
  const int elen = ev ? mlen[er] : 0, eoff = (int)moff[er];
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 pN = zero4, tN = zero4, eN = zero4;
  auto fetch_pt = [&](int f) {
    pN = zero4; tN = zero4;
    if (f < plen) {
      const int64_t g = (int64_t)(poff + f) * out + pc;
      pN = *(const f32x4*)(a.pred + g);
      if (a.target) tN = *(const f32x4*)(a.target + g);
    }
  };
  // draw k of frame f (rows whose sequence has ended: zero, never used)
  auto fetch_e = [&](int f, int k) {
    eN = zero4;
    if (f < elen) {
      const int64_t g = (int64_t)(eoff + f);
      if (a.eps) {
        eN = *(const f32x4*)(a.eps + ((int64_t)k * a.N + g) * lat + 4 * ec);
      } else {
        float e[4];
        vae_eps4(a.seed, a.ctr + (uint64_t)k, a.eps_row0 + g, ec, e);
        eN = f32x4{e[0], e[1], e[2], e[3]};
      }
    }
  };

  // ---- the state before frame 0: the carried groups, or frame 0's pred in every group ----
  fetch_pt(0);
  fetch_e(0, 0);
  const int sw = (SL - 1) * out;   // floats of state per sequence
  if (plen > 0) {
    const int64_t s = s0 + pr;
    const bool carried = a.started && a.started[s] != 0;
    float* xr = xb + pr * ldx + pc;
    for (int g = 0; g < SL - 1; ++g) {
      const f32x4 v = carried ? *(const f32x4*)(a.state + s * sw + g * out + pc) : pN;
#pragma unroll
      for (int k = 0; k < 4; ++k) xr[g * out + k] = v[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xr[(SL - 1) * out + k] = pN[k];
      tg[pr * ldt + pc + k] = tN[k];
    }
  }
  __syncthreads();

  const VaeLayer& H = d->L[d->head];
  const float* ml = act + H.aout;
  const int ldm = H.ldo, ldz = d->ldz;
  float* zb = act + d->zbuf;
  float* yb = act + d->L[d->nl - 1].aout;
  const int ldy = d->L[d->nl - 1].ldo;
  float* yr = yb + pr * ldy + pc;   // this thread's unit of the y tile
  double acc_pred = 0.0, acc_ref = 0.0;
  float e_pred = 0.0f, e_ref = 0.0f;
  float m[4] = {0.f, 0.f, 0.f, 0.f}, M[4] = {0.f, 0.f, 0.f, 0.f};
  // Frame fr's global writes, from registers (m and M stand until the next frame's first fold); they
  // are issued at the top of frame fr + 1, beside its loads, as in vae_seq_body.
  auto flush = [&](int fr) {
    if (fr < plen) {
#pragma clang fp contract(off)
      const int64_t g = (int64_t)(poff + fr) * out + pc;
      const float cl = kVaeMcC.c[K - 1];   // (read here: one scalar less to keep over the frame)
      *(f32x4*)(a.ref + g) = f32x4{m[0], m[1], m[2], m[3]};
      if (ma.ref_var) *(f32x4*)(ma.ref_var + g) = f32x4{M[0] * cl, M[1] * cl, M[2] * cl, M[3] * cl};
    }
    if (a.frame_err && q == 0 && fr < mylen) {
      if (w_pred) a.frame_err[2 * (myoff + fr)] = e_pred;
      if (w_ref) a.frame_err[2 * (myoff + fr) + 1] = e_ref;
    }
  };

  for (int f = 0; f < T; ++f) {
    fetch_pt(f + 1);   // (in flight under this frame's layers)
    if (f > 0) flush(f - 1);
    // ---- encoder, once ----
    vae_seq_layer<NW>(d->L[0], xb + i * ldx, sm, act + d->L[0].aout);
    __syncthreads();
    for (int l = 1; l <= d->head; ++l) {
      const VaeLayer& L = d->L[l];
      vae_seq_layer<NW>(L, act + L.ain + i * L.lda, sm, act + L.aout);
      __syncthreads();
    }
    for (int k = 0; k < K; ++k) {
      // ---- z_k = eps_k exp(0.5 log_var) + mean, as vae_tile_fwd forms it ----
      if (ev) {
#pragma clang fp contract(off)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = 4 * ec + j;
          const float mu = ml[er * ldm + c], lv = ml[er * ldm + lat + c];
          const float sd = expf(0.5f * lv);
          const float es = eN[j] * sd;
          const float zz = es + mu;
          zb[er * ldz + c] = zz;
        }
      }
      // the next draw's eps unit: in flight under this pass's decoder (and, behind the last pass,
      // under the next frame's encoder)
      {
        const bool last = k + 1 == K;
        fetch_e(last ? f + 1 : f, last ? 0 : k + 1);
      }
      __syncthreads();
      // ---- decoder ----
      for (int l = d->head + 1; l < d->nl; ++l) {
        const VaeLayer& L = d->L[l];
        vae_seq_layer<NW>(L, act + L.ain + i * L.lda, sm, act + L.aout);
        __syncthreads();
      }
      // ---- the fold of this thread's unit ----
      if (pv) {
        if (k == 0) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { m[j] = yr[j]; M[j] = 0.0f; }
        } else {
          const float ck = kVaeMcC.c[k];
#pragma unroll
          for (int j = 0; j < 4; ++j) vae_mc_fold(yr[j], ck, m[j], M[j]);
        }
      }
    }
    // ---- err_pred = mean (y - p)^2, err_ref = mean (y - r)^2 of r_f = y_mean, as vae_seq_body's ----
    if (a.target) {
#pragma clang fp contract(off)
      if (pv && K > 1) {   // r_f into the y tile (a thread writes the unit only it has read)
#pragma unroll
        for (int j = 0; j < 4; ++j) yr[j] = m[j];
      }
      __syncthreads();
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
      __syncthreads();   // (the state's last group and the target tile have been read)
    }
    // ---- the state of frame f + 1: groups shifted left, r_f behind them, then p_{f+1} ----
    if (f < plen) {
      float* xr = xb + pr * ldx + pc;
      const bool more = f + 1 < plen;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        for (int g = 0; g < SL - 1; ++g) xr[g * out + k] = g + 1 < SL - 1 ? xr[(g + 1) * out + k] : m[k];
        if (more) {
          xr[(SL - 1) * out + k] = pN[k];
          tg[pr * ldt + pc + k] = tN[k];
        }
      }
    }
    __syncthreads();
  }

  flush(T - 1);
  // ---- the carried groups, the started flags, the sequences' error sums ----
  if (plen > 0 && a.state) {
    const int64_t s = s0 + pr;
    const float* xr = xb + pr * ldx + pc;
    for (int g = 0; g < SL - 1; ++g)
      *(f32x4*)(a.state + s * sw + g * out + pc) = f32x4{xr[g * out], xr[g * out + 1], xr[g * out + 2], xr[g * out + 3]};
    if (pc == 0) a.started[s] = 1;
  }
  if (a.seq_err && q == 0 && mys < a.S) {
    if (w_pred) a.seq_err[2 * mys] = acc_pred;
    if (w_ref) a.seq_err[2 * mys + 1] = acc_ref;
  }
}
