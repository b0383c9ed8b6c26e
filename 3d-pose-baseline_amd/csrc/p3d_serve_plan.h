// p3d_serve_plan.h -- which serve kernel a p3d_serve / p3d_serve_mse launch runs: the list of the
// built forms and the planner that picks one.  Host-only (no HIP header): the decision is a pure
// function of (model shape, CU count, knobs, batch, with-loss), so it is tested without a GPU
// (p3d_serve_plan, tests/test_serve_plan.py).  p3d_serve_host.h attaches the kernel pointers to the list.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>

// ---- the built forms, each written down once: X(kind, DEPTH, NDT, NCM, RT, PAIR) ------------
// k_serve (models without residual blocks, p3d_serve.h): 4 K slices per unit, a 2-deep register ring.
// k_serve5: 4-wave workgroups, two groups per XCD, paired units, steps pipelined; a 4-deep ring
// where each wave's L / 64 k-groups allow it, else 2 (p3d_serve needs L % 128 == 0, so L / 64 is
// even); depth 8 spilled 186 registers and measured 8.1 M poses/s vs 12.9 M at depth 4, so it is
// not built.  (Both run batch-64 steps, RT = 4, and are not dealt in column tiles: NCM = 0.)
// k_serve6 (p3d_serve6.h), by (RT, NCM): batch-64 units with 2 / 4 / 7 / 8 column tiles per CU,
// half-step units with 11 (S = 5) or 2 (S = 1), 16-row units with 2 (S = 1: a lone batch-64 request
// on four XCDs), and XCD-wide units (S = 1, 2 tiles per CU) of 6 .. 16 row tiles.  Ring depth 4 for
// the narrow forms; 2 for 7 / 8 tiles (depth 4 spills there: 77 / 136 registers; depth 2 none / 38;
// the 7-tile form with weights 4 ahead, 53 spills, is built for P3D_SERVE6_DEPTH=4); an 8-deep
// weight ring measured 117 vs 107-112 us at RT = 10.  The pair form: two units of 5 row tiles per
// group; k_serve6_rounds: the pair form on long launches, its rounds run back to back, with helper
// waves for the work between contractions (512 threads); k_serve6_rounds_w4: the same on one wave
// per SIMD (P3D_SERVE6_HELPERS=0).
#define P3D_SERVE_FORMS(X)                                                                      \
  X(k_serve, 2, 1, 0, 4, false) X(k_serve, 2, 2, 0, 4, false) X(k_serve, 2, 3, 0, 4, false)      \
  X(k_serve, 2, 4, 0, 4, false)                                                                 \
  X(k_serve5, 4, 1, 0, 4, false) X(k_serve5, 4, 2, 0, 4, false) X(k_serve5, 4, 3, 0, 4, false)  \
  X(k_serve5, 4, 4, 0, 4, false)                                                                \
  X(k_serve5, 2, 1, 0, 4, false) X(k_serve5, 2, 2, 0, 4, false) X(k_serve5, 2, 3, 0, 4, false)  \
  X(k_serve5, 2, 4, 0, 4, false)                                                                \
  X(k_serve6, 4, 3, 2, 4, false) X(k_serve6, 2, 3, 2, 4, false) X(k_serve6, 4, 3, 4, 4, false)  \
  X(k_serve6, 2, 3, 4, 4, false) X(k_serve6, 4, 3, 7, 4, false) X(k_serve6, 2, 3, 7, 4, false)  \
  X(k_serve6, 2, 3, 8, 4, false)                                                                \
  X(k_serve6, 4, 3, 2, 1, false) X(k_serve6, 4, 3, 2, 2, false) X(k_serve6, 2, 3, 11, 2, false) \
  X(k_serve6, 4, 3, 2, 6, false) X(k_serve6, 4, 3, 2, 8, false) X(k_serve6, 4, 3, 2, 10, false) \
  X(k_serve6, 4, 3, 2, 12, false) X(k_serve6, 4, 3, 2, 16, false)                               \
  X(k_serve6, 4, 3, 2, 5, true) X(k_serve6_rounds, 4, 3, 2, 5, true)                             \
  X(k_serve6_rounds_w4, 4, 3, 2, 5, true)

enum ServeKind { SK_k_serve, SK_k_serve5, SK_k_serve6, SK_k_serve6_rounds, SK_k_serve6_rounds_w4 };
// (k_serve6 and both rounds kernels: the k_serve6 launch -- banks by epoch, no memset, its slabs)
inline bool serve_kind_is6(ServeKind k) { return k == SK_k_serve6 || k == SK_k_serve6_rounds || k == SK_k_serve6_rounds_w4; }
// threads per workgroup: k_serve splits K over 8 waves; k_serve6_rounds runs two waves per SIMD,
// contraction waves and helper waves (p3d_serve6_helpers.h); every other form one wave per SIMD
inline int serve_kind_threads(ServeKind k) { return k == SK_k_serve || k == SK_k_serve6_rounds ? 512 : 256; }

struct ServeForm {
  ServeKind kind;
  int depth, ndt, ncm, rt;
  bool pair;
};

#define P3D_SERVE_FORM_ROW(KIND, DEPTH, NDT, NCM, RT, PAIR) {SK_##KIND, DEPTH, NDT, NCM, RT, PAIR},
constexpr ServeForm kServeForms[] = {P3D_SERVE_FORMS(P3D_SERVE_FORM_ROW)};
#undef P3D_SERVE_FORM_ROW

// The built form with these parameters, or nullptr: the planner returns nothing else.
inline const ServeForm* serve_form_find(ServeKind kind, int depth, int ndt, int ncm, int rt, bool pair) {
  for (const ServeForm& f : kServeForms)
    if (f.kind == kind && f.depth == depth && f.ndt == ndt && f.ncm == ncm && f.rt == rt && f.pair == pair) return &f;
  return nullptr;
}

// The kernel's name as rocprofv3 prints it, up to k_serve6's trailing ", false>" (bench.py and the
// tests compare these strings with profiler symbols).
inline std::string serve_kernel_name(ServeKind kind, int depth, int ndt, int ncm, int rt, bool pair) {
  const std::string dn = std::to_string(depth) + ", " + std::to_string(ndt);
  const std::string cr = ", " + std::to_string(ncm) + ", " + std::to_string(rt);
  switch (kind) {
    case SK_k_serve: return "k_serve<" + dn + ", 4>";
    case SK_k_serve5: return "k_serve5<" + dn + ", 2, 2>";
    case SK_k_serve6_rounds: return "k_serve6_rounds<" + dn + cr + ">";
    case SK_k_serve6_rounds_w4: return "k_serve6_rounds_w4<" + dn + cr + ">";
    default: return "k_serve6<" + dn + cr + (pair ? ", true>" : ">");
  }
}
inline std::string serve_form_name(const ServeForm& f) {
  return serve_kernel_name(f.kind, f.depth, f.ndt, f.ncm, f.rt, f.pair);
}

// The form of launches no k_serve6 form takes (and p3d_kernel_name's answer before any launch).
inline ServeKind serve_fallback_kind(int num_layers) { return num_layers > 0 ? SK_k_serve5 : SK_k_serve; }
inline int serve_fallback_depth(int L, int num_layers) { return num_layers > 0 && (L / 64) % 4 == 0 ? 4 : 2; }

// ---- sizes the plan must respect -------------------------------------------------------------
constexpr int kServe6Rows = 4096;   // rows in flight k_serve6's activation slabs hold (P3D_SERVE6_ROWS)
// the fused MSE's partials buffer: one word per 16-row x 16-column output tile (serve_loss)
constexpr int64_t kServeLossTiles = kServe6Rows / 16 * 4;

// ---- the knobs (environment, read at p3d_create and by p3d_serve_plan) -------------------------
struct ServeKnobs {
  int serve6 = 1;    // k_serve6 for launches of <= max_nb steps (P3D_SERVE6: 0 off, 1 auto, 2 always)
  int max_nb = 32;   // (P3D_SERVE6_MAX_NB)
  int split = 0;     // k_serve6 groups per XCD, 0 = chosen per launch (P3D_SERVE6_SPLIT: 1..8)
  int rt = 0;        // k_serve6 row tiles per unit, 0 = chosen per launch (P3D_SERVE6_RT)
  int depth = 2;     // k_serve6 weight-ring depth of the 7-tile form (P3D_SERVE6_DEPTH: 2 or 4)
  int pair = 1;      // XCD-wide units of 10 row tiles as two 5-row-tile units run side by side (P3D_SERVE6_PAIR: 0 off)
  // launches of more than max_nb steps on the pair form with its rounds run back to back
  // (k_serve6_rounds) where the pair form's conditions hold (P3D_SERVE6_ROUNDS: 0 off -- k_serve5)
  int rounds = 1;
  // the rounds form with helper waves (P3D_SERVE6_HELPERS: 0 -- one wave per SIMD, k_serve6_rounds_w4)
  int helpers = 1;
};

inline ServeKnobs serve_knobs_from_env() {
  ServeKnobs k;
  const auto read = [](const char* name, int& v) { if (const char* ev = getenv(name)) v = atoi(ev); };
  read("P3D_SERVE6", k.serve6);
  read("P3D_SERVE6_MAX_NB", k.max_nb);
  read("P3D_SERVE6_SPLIT", k.split);
  read("P3D_SERVE6_RT", k.rt);
  read("P3D_SERVE6_DEPTH", k.depth);
  read("P3D_SERVE6_PAIR", k.pair);
  read("P3D_SERVE6_ROUNDS", k.rounds);
  read("P3D_SERVE6_HELPERS", k.helpers);
  return k;
}

// ---- the choice --------------------------------------------------------------------------------
// What one launch runs: the form, S groups per XCD (k_serve6; 0 otherwise) and nb units of 16 RT
// rows; or a refusal (P3D_ERR_ARG) with its reason.
struct ServeChoice {
  const ServeForm* form = nullptr;
  int S = 0, nb = 0;
  const char* refused = nullptr;
};

// A k_serve6 launch shape: S groups per XCD, RT row tiles per unit (4: batch-64 steps, 2:
// 32-row half steps), NCM column tiles per contraction (the built form covering a member of the
// smallest group; its epilogue constants of at most ECT tiles sit in LDS, p3d_serve6.h).
// The plan minimising (rounds of units) x (fixed cost per phase + cost per column tile x tiles
// per CU), 32 CUs per XCD (cus / 8): a phase's fixed cost (hand-off, ring fill, K-combine,
// epilogue) ~4 us, a column tile of K = 1024 ~3.9 us at 4 row tiles, proportional to the row
// tiles (round-1 phase traces).  20 batch-64 steps (1280 rows): RT = 10, S = 1 --
// 160 rows per XCD, 2 column tiles per CU (the half-step form, RT = 2 with 5 groups per XCD,
// costs 11 tiles of 2 row tiles per CU: 22 vs 20 tile-units and 5x the weight reads).  A
// wide form (NCM >= 7) is priced at its full width: its register ring and epilogue run NCM
// tiles whatever share of them a member owns.  One batch-64 request: RT = 1, four 16-row units
// on four XCDs, 2 tiles per CU (vs one XCD at RT = 4).  nb = 20 at RT = 4 -> S = 3 (all steps at
// once, <= 7 tiles per CU); nb <= 8 -> S = 1; nb = 16 -> S = 2.
struct Serve6Shape { int S = 0, rt = 4, ncm = 0; };

inline Serve6Shape serve6_price(int T, int cus, const ServeKnobs& k, int64_t B) {
  // the narrowest built NCM covering `need` tiles at RT row tiles (0: none)
  const auto ncm_for = [](int rt, int need) {
    int best = 0;
    for (const ServeForm& f : kServeForms)
      if (f.kind == SK_k_serve6 && !f.pair && f.rt == rt && f.ncm >= need && (!best || f.ncm < best)) best = f.ncm;
    return best;
  };
  static const int rts[] = {4, 2, 1, 6, 8, 10, 12, 16};
  const int cx = std::max(1, cus / 8);
  const double cfix = 4.0;
  Serve6Shape best;
  double bt = 1e30;
  for (int rt : rts) {
    if (k.rt && k.rt != rt) continue;
    if ((rt > 4 || rt == 1) && (T / 4) % 4 != 0) continue;   // these forms run a 4-deep weight ring
    const int64_t nb = (B + 16 * rt - 1) / (16 * rt);
    const double ctile = 3.9 * (rt / 4.0) * T / 64.0;
    for (int S = 1; S <= 8; ++S) {
      if (k.split && k.split != S) continue;
      const int nmin = cx / S;
      if (nmin < 1) continue;
      // the plan's activation slabs must fit (8 S groups of 16 RT rows, kServe6Rows): only plans
      // that fit are priced (a cap applied after the choice dropped a launch whose
      // best plan did not fit to k_serve5 instead of the best plan that did)
      if ((int64_t)8 * S * 16 * rt > kServe6Rows) continue;
      const int need = (T + nmin - 1) / nmin, ncm = ncm_for(rt, need);
      if (!ncm || need > (ncm >= 7 ? ncm : 2 * ncm)) continue;
      const double rounds = (double)((nb + 8 * S - 1) / (8 * S));
      if (rt == 2 && ncm == 2 && (T / 4) % 4 != 0) continue;
      const double t = rounds * (cfix + ctile * (ncm >= 7 ? ncm : need));
      if (t < bt - 1e-9) { bt = t; best.S = S; best.rt = rt; best.ncm = ncm; }
    }
  }
  return best;
}

// The launch of B rows on a model of hidden width L (a multiple of 128), num_layers residual
// blocks and NDT 16-column output tiles, on a device of `cus` compute units.
inline ServeChoice serve_plan(int L, int num_layers, int NDT, int cus, const ServeKnobs& k, int64_t B, bool with_loss) {
  const int T = L / 16;
  ServeChoice c;
  c.nb = (int)((B + 63) / 64);   // batch-64 steps (k_serve6 may deal other units)
  // the loss partials must fit their buffer whatever the knobs let through
  if (with_loss && (B + 15) / 16 * NDT > kServeLossTiles) {
    c.refused = "p3d_serve_mse: more 16 x 16 output tiles than the loss partials buffer holds: use p3d_serve + p3d_mse";
    return c;
  }
  // A launch of more than max_nb steps: the pair form with its rounds run back to back
  // (k_serve6_rounds) where the pair form's conditions hold -- 12 or more k-groups per wave in whole
  // ring rounds, at most 2 column tiles per member, nothing forcing another shape -- else k_serve5.
  // (The fused MSE keeps to launches of at most max_nb steps.)
  const bool long_launch = c.nb > (int64_t)k.max_nb;
  const bool long_pair = long_launch && k.serve6 == 1 && k.rounds && k.pair && !with_loss && num_layers > 0 &&
                         NDT == 3 && L / 64 >= 12 && (L / 64) % 4 == 0 && cus >= 8 &&
                         (T + cus / 8 - 1) / (cus / 8) <= 2 && T >= cus / 8 && (k.split == 0 || k.split == 1) &&
                         (k.rt == 0 || k.rt == 10);
  if (k.serve6 && num_layers > 0 && NDT == 3 && (k.serve6 == 2 || !long_launch || long_pair)) {
    Serve6Shape s;
    if (long_pair) { s.S = 1; s.rt = 10; s.ncm = 2; }
    else s = serve6_price(T, cus, k, B);
    if (s.S > 0) {
      // the pair form: an XCD-wide unit of 10 row tiles run as two units of 5 side by side, phases
      // alternating (p3d_serve6.h; the same bits; 20 steps: 99.2 vs 101.1 us, six alternating pairs)
      const bool pair = k.pair && s.S == 1 && s.rt == 10 && L / 64 >= 12;
      if (pair) s.rt = 5;
      // the ring depth each (RT, NCM) is built with (the list above)
      int depth = ((s.ncm <= 4 || (s.ncm == 7 && k.depth == 4)) && (T / 4) % 4 == 0) ? 4 : 2;
      if (s.rt == 2) depth = s.ncm == 2 ? 4 : 2;
      if (s.rt == 1 || s.rt > 4) depth = 4;
      // (a forced k_serve6 -- P3D_SERVE6=2 -- whose plan is the pair form runs a long launch's rounds
      // back to back as well)
      const bool rounds = pair && long_launch && k.rounds && !with_loss;
      const ServeKind kind = !rounds ? SK_k_serve6 : k.helpers ? SK_k_serve6_rounds : SK_k_serve6_rounds_w4;
      c.form = serve_form_find(kind, depth, NDT, s.ncm, s.rt, pair);
      if (!c.form) { c.refused = "p3d_serve: the planned k_serve6 form is not built"; return c; }
      c.S = s.S;
      c.nb = (int)((B + 16 * s.rt - 1) / (16 * s.rt));   // units of 16 RT rows
      return c;
    }
  }
  // no k_serve6 form covers this launch: k_serve5 / k_serve, which carry no loss
  if (with_loss) {
    c.refused = "p3d_serve_mse: no k_serve6 form covers this launch (more than 32 batch-64 steps, "
                "or a model shape k_serve6 is not built for): use p3d_serve + p3d_mse";
    return c;
  }
  c.form = serve_form_find(serve_fallback_kind(num_layers), serve_fallback_depth(L, num_layers), NDT, 0, 4, false);
  if (!c.form) c.refused = "p3d_serve: no serve kernel is built for this many output columns";
  return c;
}
