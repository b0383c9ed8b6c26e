// p3d_live_host.h -- the host side of S live OpenPose streams (include/p3d.h: p3d_live_*): the
// tick planner's export, the per-slot state, the two kernels of p3d_live.h as calls of their own and
// p3d_live_push, one tick from pushed frames to final poses.  Included by p3d.hip behind
// p3d_clips_host.h; the stage it shares with the clip calls is in p3d_clip_host.h.
//
// p3d_live_push's workspace: LiftLayout's rows without a head, cap = 5 S rows.
#pragma once

namespace {

int64_t live_cap(int64_t S) { return S * P3D_LIVE_SLOT_ROWS; }

// everything a tick's table can be refused for, without touching the GPU (the table is host memory)
int live_check(const char* what, const int64_t* row_off, const int32_t* row_frame, const int32_t* row_kind, int64_t S,
               int64_t N, const void* state, LiveTick& t) {
  const std::string w(what);
  if (S < 1 || S > P3D_LIVE_MAX_S) return fail(P3D_ERR_ARG, w + ": S must be in 1.." + std::to_string(P3D_LIVE_MAX_S) + " slots");
  if (N < 0 || N > live_cap(S)) return fail(P3D_ERR_ARG, w + ": N must be in 0..5 S rows");
  if (!row_off) return fail(P3D_ERR_ARG, w + ": null row_off");
  if (N > 0 && !row_frame) return fail(P3D_ERR_ARG, w + ": null row_frame");
  if (!state || ((uintptr_t)state & 7)) return fail(P3D_ERR_ARG, w + ": null or misaligned state");
  if (row_off[0] != 0 || row_off[S] != N) return fail(P3D_ERR_ARG, w + ": row_off must start at 0 and end at N");
  for (int64_t s = 0; s < S; ++s) {
    const int64_t n = row_off[s + 1] - row_off[s];
    if (n < 0) return fail(P3D_ERR_ARG, w + ": row_off must not decrease (slot " + std::to_string(s) + ")");
    if (n > P3D_LIVE_SLOT_ROWS)
      return fail(P3D_ERR_ARG, w + ": row_off gives slot " + std::to_string(s) + " more than 5 rows");
    if (row_off[s + 1] > N) return fail(P3D_ERR_ARG, w + ": row_off must end at N");
  }
  for (int64_t r = 0; r < N; ++r) {
    if (row_frame[r] < 0) return fail(P3D_ERR_ARG, w + ": row_frame must be >= 0 (row " + std::to_string(r) + ")");
    if (row_kind && (row_kind[r] < P3D_LIVE_KIND_NONE || row_kind[r] > P3D_LIVE_KIND_TAIL))
      return fail(P3D_ERR_ARG, w + ": row_kind must be in 0..3 (row " + std::to_string(r) + ")");
  }
  t.off = row_off; t.frame = row_frame; t.kind = row_kind; t.S = S; t.N = N;
  return P3D_OK;
}

int live_prepare_check(const char* what, const double* xy_in, const int32_t* push_frame, const int32_t* row_kind,
                       int64_t S, int64_t N, int32_t smooth, int32_t U2) {
  const std::string w(what);
  if (!xy_in || !push_frame) return fail(P3D_ERR_ARG, w + ": null xy_in or push_frame");
  if (N > 0 && !row_kind) return fail(P3D_ERR_ARG, w + ": null row_kind");
  if (U2 < 1 || U2 > 64) return fail(P3D_ERR_ARG, w + ": U2 must be in 1..64");
  if (!smooth)
    for (int64_t r = 0; r < N; ++r)
      if (row_kind[r] != P3D_LIVE_KIND_NONE)
        return fail(P3D_ERR_ARG, w + ": row_kind must be 0 without smoothing (row " + std::to_string(r) + ")");
  (void)S;
  return P3D_OK;
}

unsigned live_grid(int64_t S) { return (unsigned)((S + P3D_LIVE_WAVES - 1) / P3D_LIVE_WAVES); }

int live_prepare(const LiveTick& t, const double* xy_in, const int32_t* push_frame, const Stat2& s2, void* state,
                 float* x, double* xy_s, hipStream_t st) {
  LiveInArgs a{};
  a.c = lift_in_args(s2, t.N, x, xy_s);
  a.xy = xy_in; a.push_frame = push_frame; a.t = t; a.st = live_state(state, t.S);
  k_live_in<<<dim3(live_grid(t.S)), P3D_LIVE_WAVES * 64, 0, st>>>(a);
  LAUNCH_CHECK("k_live_in");
  return P3D_OK;
}

int live_finish(const LiveTick& t, const float* y, const double* xy_s, const Stat3& s3, void* state, double* poses,
                int32_t* src, hipStream_t st) {
  if (t.N == 0) return P3D_OK;   // (no row: no state changes)
  LiveOutArgs a{};
  a.c = lift_out_args(s3, y, t.N, xy_s, poses, src);
  a.t = t; a.st = live_state(state, t.S);
  k_live_out<<<dim3(live_grid(t.S)), P3D_LIVE_WAVES * 64, 0, st>>>(a);
  LAUNCH_CHECK("k_live_out");
  return P3D_OK;
}

}  // namespace

extern "C" int p3d_live_plan(int64_t S, int32_t smooth, int32_t* count, const uint8_t* push, const uint8_t* close,
                             int64_t* row_off, int32_t* row_slot, int32_t* row_frame, int32_t* row_kind,
                             int32_t* push_frame, int32_t* is_short, int64_t* n_rows) {
  if (S < 1 || S > P3D_LIVE_MAX_S) return fail(P3D_ERR_ARG, "p3d_live_plan: S must be in 1.." + std::to_string(P3D_LIVE_MAX_S) + " slots");
  if (!count || !push || !close || !row_off || !row_slot || !row_frame || !row_kind || !push_frame || !is_short || !n_rows)
    return fail(P3D_ERR_ARG, "p3d_live_plan: null argument");
  const int64_t n = live_plan(S, smooth, count, push, close, row_off, row_slot, row_frame, row_kind, push_frame, is_short);
  if (n < 0)
    return fail(P3D_ERR_ARG, "p3d_live_plan: slot " + std::to_string(-1 - n) +
                                 " is pushed and closed in one tick, or its count is out of range");
  *n_rows = n;
  return P3D_OK;
}

extern "C" int64_t p3d_live_state_bytes(int64_t S, int32_t U3) {
  if (S < 1 || S > P3D_LIVE_MAX_S || U3 < 1 || U3 > P3D_CLIP_D3) return 0;
  return align256(S * ((P3D_LIVE_RING + 1) * P3D_CLIP_COLS + P3D_CLIP_D3) * (int64_t)sizeof(double) +
                  S * (int64_t)sizeof(int32_t));
}

// slot < 0: every slot.  A reset slot has no last smoothed row and no last good pose; its ring is
// never read before it is written again (a window reads only frames of the new stream).
extern "C" int p3d_live_reset(void* state, int64_t S, int64_t slot, void* stream) {
  if (!state || ((uintptr_t)state & 7)) return fail(P3D_ERR_ARG, "p3d_live_reset: null or misaligned state");
  if (S < 1 || S > P3D_LIVE_MAX_S) return fail(P3D_ERR_ARG, "p3d_live_reset: S must be in 1.." + std::to_string(P3D_LIVE_MAX_S) + " slots");
  if (slot >= S) return fail(P3D_ERR_ARG, "p3d_live_reset: slot must be below S (or negative: all)");
  const LiveState ls = live_state(state, S);
  hipStream_t st = (hipStream_t)stream;
  if (slot < 0) {
    HIP_TRY(hipMemsetAsync(state, 0, (size_t)((char*)ls.good_pos - (char*)state), st));
    HIP_TRY(hipMemsetAsync(ls.good_pos, 0xff, (size_t)S * sizeof(int32_t), st));
  } else {
    HIP_TRY(hipMemsetAsync(ls.last + slot * P3D_CLIP_COLS, 0, P3D_CLIP_COLS * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(ls.good_pos + slot, 0xff, sizeof(int32_t), st));
  }
  return P3D_OK;
}

extern "C" int p3d_live_prepare(const double* xy_in, const int32_t* push_frame, const int64_t* row_off,
                                const int32_t* row_frame, const int32_t* row_kind, int64_t S, int64_t N, int32_t smooth,
                                const double* mean2, const double* std2, const int32_t* use2, int32_t U2, void* state,
                                float* x, double* xy_s, void* stream) {
  const char* what = "p3d_live_prepare";
  if (!mean2 || !std2 || !use2) return fail(P3D_ERR_ARG, "p3d_live_prepare: null statistics");
  LiveTick t;
  if (int rc = live_check(what, row_off, row_frame, row_kind, S, N, state, t)) return rc;
  if (int rc = live_prepare_check(what, xy_in, push_frame, row_kind, S, N, smooth, U2)) return rc;
  if (N > 0 && (!x || !xy_s)) return fail(P3D_ERR_ARG, "p3d_live_prepare: null x or xy_s");
  return live_prepare(t, xy_in, push_frame, {mean2, std2, use2, U2}, state, x, xy_s, (hipStream_t)stream);
}

extern "C" int p3d_live_finish(const float* y, const int64_t* row_off, const int32_t* row_frame, int64_t S, int64_t N,
                               const double* xy_s, const double* mean3, const double* std3, const int32_t* use3,
                               int32_t U3, int32_t D3, int32_t cache_on_fail, void* state, double* poses, int32_t* src,
                               void* stream) {
  const char* what = "p3d_live_finish";
  if (!mean3 || !std3 || !use3) return fail(P3D_ERR_ARG, "p3d_live_finish: null statistics");
  LiveTick t;
  if (int rc = live_check(what, row_off, row_frame, nullptr, S, N, state, t)) return rc;
  if (D3 != P3D_CLIP_D3) return fail(P3D_ERR_ARG, "p3d_live_finish: D3 must be 96 (32 joints)");
  if (U3 < 1 || U3 > D3) return fail(P3D_ERR_ARG, "p3d_live_finish: U3 must be in 1..96");
  if (N > 0 && (!y || !xy_s || !poses)) return fail(P3D_ERR_ARG, "p3d_live_finish: null y, xy_s or poses");
  return live_finish(t, y, xy_s, {mean3, std3, use3, U3, cache_on_fail}, state, poses, src, (hipStream_t)stream);
}

extern "C" int64_t p3d_live_push_workspace(int64_t S, int32_t U2, int32_t U3, int32_t with_filter) {
  if (S < 1 || S > P3D_LIVE_MAX_S || U2 <= 0 || U3 <= 0) return 0;
  return LiftLayout(nullptr, 0, live_cap(S), U2, U3, with_filter != 0).total;
}

// One tick on `stream`: prepare; the forward tiles over the tick's rows in slot order; the temporal
// filter over the slots as its sequences (slots without rows are empty sequences) on the carried
// state; finish on the refined rows.
extern "C" int p3d_live_push(p3d_model* m, p3d_vae* v, int32_t K, uint64_t ctr, int64_t eps_row0, void* state,
                             float* filter_state, int32_t* filter_started, const double* xy_in,
                             const int32_t* push_frame, const int64_t* row_off, const int32_t* row_frame,
                             const int32_t* row_kind, int64_t S, int64_t N, const double* mean2, const double* std2,
                             const int32_t* use2, int32_t U2, const double* mean3, const double* std3,
                             const int32_t* use3, int32_t U3, int32_t D3, int32_t cache_on_fail, int32_t smooth,
                             double* xy_s, double* poses, int32_t* src, float* ref_var, void* work, int64_t work_bytes,
                             void* stream) {
  const char* what = "p3d_live_push";
  // what needs neither the model nor the filter first: the test without a GPU reaches all of it
  if (!mean2 || !std2 || !use2 || !mean3 || !std3 || !use3) return fail(P3D_ERR_ARG, "p3d_live_push: null statistics");
  if (!xy_s || !poses) return fail(P3D_ERR_ARG, "p3d_live_push: null xy_s or poses");
  if (U3 < 1 || U3 > P3D_CLIP_D3) return fail(P3D_ERR_ARG, "p3d_live_push: U3 must be in 1..96");
  if (D3 != P3D_CLIP_D3) return fail(P3D_ERR_ARG, "p3d_live_push: D3 must be 96 (32 joints)");
  if (K < 0 || K > P3D_VAE_MC_MAX_K)
    return fail(P3D_ERR_ARG, "p3d_live_push: K must be in 1 .. " + std::to_string(P3D_VAE_MC_MAX_K) + " (0: one draw)");
  if (eps_row0 < 0) return fail(P3D_ERR_ARG, "p3d_live_push: eps_row0 must be >= 0");
  LiveTick t;
  if (int rc = live_check(what, row_off, row_frame, row_kind, S, N, state, t)) return rc;
  if (int rc = live_prepare_check(what, xy_in, push_frame, row_kind, S, N, smooth, U2)) return rc;
  if (!work || ((uintptr_t)work & 255)) return fail(P3D_ERR_ARG, "p3d_live_push: null workspace, or not 256-byte aligned");
  const LiftLayout l(work, 0, live_cap(S), U2, U3, v != nullptr);
  if (work_bytes < l.total) return fail(P3D_ERR_ARG, "p3d_live_push: workspace too small");
  if (!v) {
    if (K || ref_var || filter_state || filter_started)
      return fail(P3D_ERR_ARG, "p3d_live_push: K, ref_var and the filter state need a filter");
  } else {
    if (int rc = lift_check_filter(what, v, U3)) return rc;
    if (ctr == P3D_CTR_GLOBAL_STEP)
      return fail(P3D_ERR_ARG, "p3d_live_push: ctr may not be P3D_CTR_GLOBAL_STEP (draw k uses the counter ctr + k)");
    if (ref_var && K < 1) return fail(P3D_ERR_ARG, "p3d_live_push: ref_var needs K >= 1");
    if (!filter_state || !filter_started) return fail(P3D_ERR_ARG, "p3d_live_push: null filter_state or filter_started");
    if ((uintptr_t)filter_state % 16 != 0 || (uintptr_t)ref_var % 16 != 0)
      return fail(P3D_ERR_ARG, "p3d_live_push: filter_state and ref_var must be 16-byte aligned");
  }
  if (!m) return fail(P3D_ERR_ARG, "p3d_live_push: null model");
  if (int rc = lift_check_model(what, m, U2, U3)) return rc;
  const Stat3 s3{mean3, std3, use3, U3, cache_on_fail};
  hipStream_t st = (hipStream_t)stream;
  int rc = live_prepare(t, xy_in, push_frame, {mean2, std2, use2, U2}, state, l.x, xy_s, st);
  if (rc || N == 0) return rc;
  if ((rc = lift_forward(m, l.x, l.y, 0, N, stream))) return rc;
  if (!v) return live_finish(t, l.y, xy_s, s3, state, poses, src, st);
  if ((rc = lift_filter_run(v, K, l.y, row_off, S, N, nullptr, ctr, eps_row0, filter_state, filter_started, l.ref,
                            ref_var, stream)))
    return rc;
  return live_finish(t, l.ref, xy_s, s3, state, poses, src, st);
}
