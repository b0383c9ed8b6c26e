// p3d_serve6.h -- k_serve6: the persistent XCD-local batch-64 evaluation sized for launches of
// a few dozen steps (the driver's `bench.py --steps 20`), and k_serve6_rounds: its pair form on
// longer launches, the rounds run back to back (the comment in front of the kernels).
//
// k_serve5 (p3d_serve.h) is built for throughput over long launches: two 16-CU groups per XCD,
// each running its steps one after another.  With 20 steps per launch that leaves 4 of its 16
// groups running a second step while the other 12 idle: the launch costs two steps of latency
// (8 hidden phases, each ~20 us) for 1.25 steps of work.  The critical path of a launch of nb
// steps is (rounds of steps) x (phases) x (column tiles per CU + fixed cost per phase), so
// k_serve6 takes the groups-per-XCD S as a launch argument, chosen on the host for nb
// (p3d_serve_plan.h): at nb = 20, S = 3 groups of 11/11/10 CUs run all 20 steps at once,
// each CU contracting <= 7 of a layer's 64 column tiles per phase -- 28 16x16 tiles of K = 1024
// on the critical path and 4 phases, instead of 32 tiles and 8 phases.
//
// One launch per call: the sync words alternate between two banks picked on the device (the
// launch's groups each read their epoch word, use bank epoch & 1, zero their flags of the other for
// the next launch; each group's rank-0 member advances the group's word at its end, when every
// member has provably read it),
// so a launch needs no memset in front and captured graphs replay correctly.  The epilogue
// constants come from a table k_serve_prep forms per parameter version.
//
// What differs from k_serve5 (everything else -- XCD-local groups (k_serve6: placed by the
// dispatcher's round-robin, checked against the hardware XCD id), flag hand-offs in
// the XCD's L2, sc1 reads of other CUs' data, 4-wave K-split contraction with a register ring,
// epilogue constants in LDS, steps pipelined when a group has several -- is the same design):
//   * work is dealt in 16-column tiles, not 32-column units: member r of a group of n owns the
//     contiguous tiles [T r / n, T (r+1) / n) (T = L / 16), i.e. floor or ceil of T / n, and
//     contracts them (all 4 row tiles) as one contraction of NCM tiles (a member with fewer
//     computes a copy of its last tile and stores nothing for it; one with more loops);
//   * the output layer is a phase of its own (round 5; it was fused into the last hidden epilogue
//     as one 64 x 48 partial per column tile, summed by a reduction: 15.7 MB of partials per
//     20-step launch and a full-group wait): its RT x NDT tiles are dealt over the members and
//     contracted like hidden tiles, K split over the 4 waves, slices summed in order -- the
//     association is fixed by the tile, independent of n and S, so every launch shape gives the
//     same bits.
#pragma once
#include "p3d_serve.h"

#ifndef P3D_S6_PIN_ARGS
#define P3D_S6_PIN_ARGS 1          // the prologue's kernel arguments fetched in one round (round 5)
#endif
#ifndef P3D_S6_COMBINE_BATCH
#define P3D_S6_COMBINE_BATCH 1     // the K-combine's LDS reads issued before the first add (round 5)
#endif
#ifndef P3D_S6_OUT_PRE
#define P3D_S6_OUT_PRE 1           // the output layer's first weight fragments requested before the last hand-off
#endif
#ifndef P3D_S6_LATE_EPOCH
#define P3D_S6_LATE_EPOCH 1        // the epoch read off the prologue's critical path (round 5)
#endif
#ifndef P3D_S6_HELPER_NAP
#define P3D_S6_HELPER_NAP 8        // k_serve6_rounds: s_sleep between a helper wave's polls of the partials word (x 64 clocks)
#endif
#ifndef P3D_S6_HELPER_PRIO
#define P3D_S6_HELPER_PRIO 2       // k_serve6_rounds: static s_setprio 1 for its helper waves (0 none, 1 the contraction waves; MEASUREMENTS 22)
#endif


// Timeline stamps for development (-DP3D_TRACE, tools/trace_serve6.py): for every group, its
// rank-0 member (row 0) and its first member with the most tiles (row 1), first step only:
// [0] start, [1] placement, [2] input layer, [3] first hand-off; per hidden phase ph at 8 ph:
// [0] begin, [1] contraction, [2] K-combine, [3] epilogue, [4] hand-off; at 8 (NH + 1): [0]
// the output reduction.  wall_clock64 (100 MHz).
#ifdef P3D_TRACE
#define P3D_S6_STAMP(row, k)                                                              \
  do {                                                                                    \
    if (tr6 && (row) && threadIdx.x == 0) {                                               \
      tr6[(k)] = wall_clock64();                                                          \
      tr6[64 + (k)] = __builtin_amdgcn_s_memtime();                                       \
    }                                                                                     \
  } while (0)
#else
#define P3D_S6_STAMP(row, k) do { } while (0)
#endif

// The epilogue-constant table of the serve launches, formed when the parameters changed (and
// inside every captured graph): bias, inv = gamma / sqrt(var + eps), shift = beta - mean * inv
// -- the arithmetic of every other path -- of every layer 0..2N and column, laid out per
// 16-column tile as k_serve6 keeps them in LDS, so its workgroups copy them with one round of
// loads instead of forming them (five dependent operand loads per element) in every launch.
__global__ __launch_bounds__(256) void k_serve_prep(ServeArgs p, float* ecg) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int L = p.L, nl = 2 * p.nblk + 1;
  if (i >= nl * L) return;
  const int l = i / L, col = i % L, t = col >> 4, j = col & 15;
  const ServeLayer& ly = p.ly[l];
  float inv = 1.f, shift = 0.f;
  if (p.bn) {
    inv = (1.0f / sqrtf(ly.mvar[col] + p.eps)) * ly.gamma[col];
    shift = ly.beta[col] - ly.mmean[col] * inv;
  }
  float* e = ecg + ((int64_t)l * (L >> 4) + t) * 48;
  e[j] = ly.bias[col]; e[16 + j] = inv; e[32 + j] = shift;
  if (col == 0)   // the layer's max-norm divisor max(||W||, 1) (1 without --max_norm)
    ecg[(int64_t)nl * (L >> 4) * 48 + l] = ly.wsq ? fmaxf(sqrtf(*ly.wsq), 1.0f) : 1.0f;
}

// owner of column tile t when T tiles are dealt contiguously over n members
__device__ __forceinline__ int p3d_tile_owner(int t, int n, int T) { return ((t + 1) * n - 1) / T; }

// RT: row tiles per unit.  Rows are independent in evaluation, so the rows of a launch need
// not go in batch-64 steps: a unit of 16 RT rows is what one group runs through all layers.
// RT = 4 is the batch-64 step; RT = 2 half a step (20 steps = 40 units = 5 groups per XCD);
// RT = 6 .. 16 with S = 1 gives each XCD ONE unit of all its rows and all 32 of its CUs, each
// CU 2 of a layer's 64 column tiles for every row tile (20 steps: 160 rows per XCD, RT = 10):
// no group idles, no CU holds more tiles than another, and each weight fragment is read by one
// CU per XCD and serves 10 row tiles (p3d_serve_plan.h serve_plan picks the form per launch).
// The epilogue / input-layer work of a chunk, RT x NCM 16 x 16 tiles, is dealt to the waves
// round-robin: unit u = w + 4 j is row tile u / NCM of column tile u % NCM (UMAX per wave).
//
// PAIR (round 5): each group runs TWO units of RT row tiles side by side, alternating their
// phases -- A's phase ph, B's phase ph, A's phase ph + 1, ... -- so the hand-off of one unit runs
// under the other's contraction instead of in front of the next: a member's next contraction
// reads the other unit's previous phase, published a whole contraction earlier.  Per block
// (one unit's phase): the contraction, whose last DEPTH k-groups refill the register ring with
// the next block's first ones (its producers' flags checked a round earlier); partial sums to
// LDS; K-combine, epilogue, stores; the next contraction at once, its ring full.  A block's
// stores are published from inside the next contraction, after its first DEPTH k-groups (a
// vmcnt wait that leaves that contraction's refills in flight), each wave on its own, the fourth
// to arrive (an LDS counter) posting the member's flag -- no barrier, no store round trip and no
// ring fill between contractions.
//
// ROUNDS (the pair form on launches of more than one round of units per group): the block
// sequence runs on from round to round.  The next round's input layers are computed at the
// boundaries of this round's last two blocks, into the slab of each unit's rotation that its last
// phase reads nothing from, and published by the following blocks' in-contraction posts like any
// block's stores; the last block refills the ring with the next round's block 0.  A round's output
// layer runs at a block boundary of the next round, when both units' last hidden layers were
// posted (and checked by this wave) more than a block ago: no prologue, no drain, no wait between
// rounds.  Only a group's first round runs the prologue and only its last the closing post / wait /
// output phase.  Output tiles keep their association, so rows have the bits of the one-round
// launches.
//
// The body (p3d_serve6_body.h) is compiled into each kernel as text, ROUNDS a constant of the kernel:
// k_serve6 is the same function as before the ROUNDS form existed -- name, arguments and code (its
// register allocation does not survive being called through a wrapper: 509 + 253 registers and other
// code where the kernel itself has 512 + 256).
template <int DEPTH, int NDT, int NCM, int RT = 4, bool PAIR = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_serve6(ServeArgs p) {
  constexpr bool ROUNDS = false, HELPERS = false;
#include "p3d_serve6_body.h"
}

// the pair form with its rounds run back to back: launches of more than one round per group.
// Two waves per SIMD (p3d_serve6_helpers.h): waves 0-3 contract and never stop between blocks, waves
// 4-7 do the work between contractions; one register allocation for both roles, 256 registers.
template <int DEPTH, int NDT, int NCM, int RT>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_serve6_rounds(ServeArgs p) {
  constexpr bool PAIR = true, ROUNDS = true, HELPERS = true;
#include "p3d_serve6_body.h"
}

// the same with one wave per SIMD, each doing its own boundary work (P3D_SERVE6_HELPERS=0): the form
// the helper waves were measured against, and the yardstick of their tests
template <int DEPTH, int NDT, int NCM, int RT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_serve6_rounds_w4(ServeArgs p) {
  constexpr bool PAIR = true, ROUNDS = true, HELPERS = false;
#include "p3d_serve6_body.h"
}
