"""The table of bad calls behind tests/golden/lift_errors_parent.json: p3d_clip_*, p3d_clips_*,
p3d_skel_lengths / _pose, p3d_live_prepare / _finish / _push and the two sequence-filter calls, every
one refused before anything is launched, most with two faults at once so that the pair (return code, p3d_last_error)
pins WHICH fault answers.  tools/record_lift_errors.py runs the table against a library and writes
the fixture; tests/test_lift_errors.py runs it against the built library and compares.

No call has a model or a filter handle (both need a GPU), and a row is named after what it can
reach.  The prepare / finish calls, the skeleton calls and p3d_clips_resample take no handle: their
rows reach every check.  p3d_live_push asks for the model last: its rows reach everything but the
checks of a live filter.  p3d_clip_lift, p3d_clips_lift and p3d_clips_lift_resampled ask for the model first, and the sequence-filter calls read the filter before
they look at sizes, state, targets or alignment: their few rows (`null_model*`, `null_filter*`) pin
that the null handle answers before the other fault, and the K-sample call's rows what it refuses
before it reads the handle.  Nothing in this table reaches the checks behind a handle: those are
handle_cases and lift_handle_cases below."""
import ctypes

import numpy as np

GLOBAL_STEP = 0xFFFFFFFFFFFFFFFF

# argument names in call order (include/p3d.h); `stream` is always null
ORDER = {
    "p3d_clip_prepare": "xy N smooth mean2 std2 use2 U2 x xy_s work work_bytes",
    "p3d_clip_finish": "y N xy_s mean3 std3 use3 U3 D3 cache poses src work work_bytes",
    "p3d_clip_lift": "m xy N smooth mean2 std2 use2 U2 mean3 std3 use3 U3 D3 cache xy_s poses src work work_bytes",
    "p3d_clips_prepare": "xy off_host off_dev S N smooth mean2 std2 use2 U2 x xy_s work work_bytes",
    "p3d_clips_finish": "y off_host off_dev S N xy_s mean3 std3 use3 U3 D3 cache poses src work work_bytes",
    "p3d_clips_lift": "m v K eps ctr eps_row0 xy off_host off_dev S N smooth mean2 std2 use2 U2 mean3 std3 use3 U3 D3 "
                      "cache xy_s poses src poses_u src_u ref_var work work_bytes",
    "p3d_live_prepare": "xy push_frame row_off row_frame row_kind S N smooth mean2 std2 use2 U2 state x xy_s",
    "p3d_live_finish": "y row_off row_frame S N xy_s mean3 std3 use3 U3 D3 cache state poses src",
    "p3d_live_push": "m v K ctr eps_row0 state fstate fstarted xy push_frame row_off row_frame row_kind S N mean2 std2 "
                     "use2 U2 mean3 std3 use3 U3 D3 cache smooth xy_s poses src ref_var work work_bytes",
    "p3d_skel_lengths": "poses src off_host off_dev S N lengths n_used work work_bytes",
    "p3d_skel_pose": "poses src off_host off_dev S N lengths quat euler rigid root",
    "p3d_clips_resample": "xy_s off_host off_dev S N R mean2 std2 use2 U2 x xy_r off_out info work work_bytes",
    "p3d_clips_lift_resampled": "m v K eps ctr eps_row0 xy off_host off_dev S N smooth mean2 std2 use2 U2 mean3 std3 use3 "
                                "U3 D3 cache xy_s poses src poses_u src_u ref_var R xy_r off_out info work work_bytes",
    "p3d_vae_seq_filter": "v pred seq_off S N eps ctr eps_row0 target fstate fstarted ref frame_err seq_err",
    "p3d_vae_seq_filter_mc": "v pred seq_off S N K eps ctr eps_row0 target fstate fstarted ref ref_var frame_err seq_err",
}

I64 = lambda *v: np.array(v, np.int64)   # noqa: E731
I32 = lambda *v: np.array(v, np.int32)   # noqa: E731


def cases():
    """[(id, function name, {argument: value})]: the overrides of a call that is in order but for
    its null model / filter.  A value that is an int is a byte offset into the fake device buffer
    when the argument is a pointer (None: null); numpy arrays are host tables passed as they are."""
    c = []

    def add(fn, name, **kw):
        # prepare / finish take no handle: a row stays only where one of its faults is theirs
        names = ORDER[fn].split()
        kw = {k: v for k, v in kw.items() if k in names}
        if kw or "m" in names or "v" in names:
            c.append(("%s/%s" % (fn[4:], name), fn, kw))

    more = dict(ref_var=8192 + 4, K=65, ctr=GLOBAL_STEP)
    for fn, more in (("p3d_clip_lift", {}), ("p3d_clips_lift", more), ("p3d_clips_lift_resampled", more)):
        add(fn, "null_model")                                # the model is asked for first: whatever else is wrong
        add(fn, "null_model_N0", N=0)
        add(fn, "null_model_null_statistics", mean2=None, mean3=None)
        add(fn, "null_model_null_work_bad_D3", work=None, D3=48)
        add(fn, "null_model_smooth_2_frames", N=2, off_host=I64(0, 2, 30))
        if more:
            add(fn, "null_model_bad_filter_arguments", **more)
    add("p3d_clip_prepare", "alias_bad_U2", xy_s=0, xy=0, U2=0)
    for fn in ("p3d_clip_prepare", "p3d_clip_finish"):
        add(fn, "N0", N=0)
        add(fn, "N0_null_work", N=0, work=None)
        add(fn, "null_mean_N0", mean2=None, mean3=None, N=0)
        add(fn, "small_work", work_bytes=1)
        add(fn, "bad_D3_small_work", D3=48, work_bytes=1)
        add(fn, "bad_D3_U3", D3=48, U3=97)
        add(fn, "bad_U_small_work", U2=65, U3=97, work_bytes=1)
        add(fn, "misaligned_work_small", work=4096 + 4, work_bytes=1)
        for n in (2, 8):
            add(fn, "smooth_%d_frames_null_work" % n, N=n, work=None)
            add(fn, "smooth_%d_frames_null_xy" % n, N=n, xy=None, y=None)
        add(fn, "no_smooth_2_frames_null_work", N=2, smooth=0, work=None)
    for fn in ("p3d_clips_prepare", "p3d_clips_finish"):
        add(fn, "N0", N=0)
        add(fn, "null_statistics_N0", mean2=None, mean3=None, N=0)
        add(fn, "null_offsets_N0", off_host=None, N=0)
        add(fn, "null_xy_null_offsets", xy=None, y=None, off_dev=None)
        add(fn, "bad_S_bad_offsets", S=0, off_host=I64(1, 9, 30))
        add(fn, "offsets_start_and_end", off_host=I64(1, 9, 29))
        add(fn, "empty_clip_null_work", off_host=I64(0, 0, 30), work=None)
        add(fn, "decreasing_small_work", off_host=I64(0, 31, 30), work_bytes=1)
        add(fn, "bad_D3_small_work", D3=48, work_bytes=1)
        add(fn, "bad_D3_U3", D3=48, U3=97)
        add(fn, "bad_U_null_work", U2=65, U3=0, work=None)
        add(fn, "alias_small_work", xy_s=0, xy=0, work_bytes=1)
        add(fn, "misaligned_work_small", work=4096 + 4, work_bytes=1)
        for n in (2, 8):
            add(fn, "smooth_clip_of_%d_null_work" % n, off_host=I64(0, n, 30), work=None)
            add(fn, "smooth_clip_of_%d_bad_U" % n, off_host=I64(0, 30 - n, 30), U2=65, U3=97)
    for fn in ("p3d_skel_lengths", "p3d_skel_pose", "p3d_clips_resample"):   # no handle: every check is reached
        add(fn, "null_argument_bad_N", poses=None, xy_s=None, N=0)
        add(fn, "null_offsets_bad_N", off_host=None, N=0)
        add(fn, "null_offsets_bad_S", off_dev=None, S=0)
        add(fn, "bad_N_bad_S", N=0, S=0)
        add(fn, "bad_S_bad_offsets", S=0, off_host=I64(1, 9, 30))
        add(fn, "S_above_N_bad_offsets", S=31, off_host=I64(1, 9, 30))
        add(fn, "offsets_start_and_end", off_host=I64(1, 9, 29))
        add(fn, "offsets_end_empty_clip", off_host=I64(0, 0, 29))
        add(fn, "empty_then_decreasing", S=3, off_host=I64(0, 0, -1, 30))
        add(fn, "decreasing_then_empty", S=4, off_host=I64(0, 10, 9, 9, 30))
        add(fn, "past_the_end_then_decreasing", off_host=I64(0, 31, 30))
        add(fn, "empty_clip_null_work", off_host=I64(0, 0, 30), work=None)
        add(fn, "null_work_small", work=None, work_bytes=1)
        add(fn, "misaligned_work_small", work=WORK + 4, work_bytes=1)
        add(fn, "small_work", work_bytes=1)
    add("p3d_skel_pose", "null_argument_no_outputs", lengths=None, quat=None, euler=None, rigid=None, root=None)
    add("p3d_skel_pose", "no_outputs_null_offsets", quat=None, euler=None, rigid=None, root=None, off_dev=None)
    add("p3d_skel_pose", "one_output_null_offsets", quat=None, euler=None, rigid=None, off_host=None)
    R = "p3d_clips_resample"
    add(R, "null_off_out_bad_R", off_out=None, R=0)
    add(R, "empty_clip_bad_R", off_host=I64(0, 0, 30), R=0)
    for r in (0, 17):
        add(R, "R%d_clip_of_3" % r, R=r, off_host=I64(0, 3, 30))
    add(R, "clip_of_3_bad_U2", off_host=I64(0, 27, 30), U2=65)
    add(R, "bad_U2_alias", U2=0, xy_r=0)
    add(R, "alias_null_work", xy_r=0, work=None)
    add(R, "R17_too_many_rows", R=17, N=1 << 20, off_host=I64(0, 9, 1 << 20))
    add(R, "too_many_rows_long_clip", R=2, N=1 << 20, off_host=I64(0, 9, 1 << 20))
    add(R, "long_clip_bad_U2", R=1, N=1 << 20, off_host=I64(0, 9, 1 << 20), U2=0)
    for fn in ("p3d_live_prepare", "p3d_live_finish", "p3d_live_push"):
        add(fn, "in_order_but_for_the_model")
        add(fn, "null_statistics", mean2=None, mean3=None)
        add(fn, "null_statistics_bad_S", use2=None, use3=None, S=0)
        add(fn, "bad_S_bad_N", S=0, N=-1)
        add(fn, "bad_N_null_row_off", N=16, row_off=None)
        add(fn, "null_row_off_null_state", row_off=None, state=None)
        add(fn, "null_row_frame_misaligned_state", row_frame=None, state=256 + 4)
        add(fn, "null_state_bad_offsets", state=None, row_off=I64(1, 5, 5, 6))
        add(fn, "five_rows_negative_frame", row_off=I64(0, 6, 6, 6), row_frame=I32(0, 1, 2, -3, 4, 9))
        add(fn, "bad_kind_bad_U", row_kind=I32(1, 1, 1, 1, 2, 4), U2=65, U3=97)
        add(fn, "bad_D3_U3", D3=48, U3=97)
        add(fn, "bad_D3_null_outputs", D3=48, poses=None, x=None)
        add(fn, "bad_U_null_outputs", U2=0, U3=0, xy_s=None)
        add(fn, "null_xy_null_kind", xy=None, y=None, row_kind=None)
        add(fn, "no_smoothing_kinds_bad_U2", smooth=0, U2=65)
    P = "p3d_live_push"
    add(P, "null_model_N0", N=0, row_off=I64(0, 0, 0, 0))
    add(P, "bad_D3_small_work", D3=48, work_bytes=1)
    add(P, "bad_K_null_row_off", K=65, row_off=None)
    add(P, "bad_K_bad_row0", K=-1, eps_row0=-1)
    add(P, "bad_row0_bad_S", eps_row0=-1, S=0)
    add(P, "null_work_small", work=None, work_bytes=1)
    add(P, "misaligned_work_filter_arguments", work=4096 + 8, K=2, fstate=8192)
    add(P, "small_work_filter_arguments", work_bytes=1, ref_var=8192)
    add(P, "misaligned_work_bad_U2", work=4096 + 8, U2=65)
    add(P, "ref_var_without_filter", ref_var=8192)
    add(P, "fstate_without_filter", fstate=8192 + 4)
    add(P, "fstarted_without_filter", fstarted=8192)
    add(P, "global_step_K0", ctr=GLOBAL_STEP, K=0)
    add(P, "global_step_K1", ctr=GLOBAL_STEP, K=1)
    add(P, "K1_without_filter_small_work", K=1, work_bytes=1)
    for fn in ("p3d_vae_seq_filter", "p3d_vae_seq_filter_mc"):   # the filter is read before anything but ref, K, ctr
        add(fn, "null_filter")
        add(fn, "null_filter_null_ref", ref=None)
        add(fn, "null_filter_global_step", ctr=GLOBAL_STEP)
        add(fn, "null_filter_global_step_null_ref", ctr=GLOBAL_STEP, ref=None)
        add(fn, "null_filter_bad_sizes", S=0, N=0, eps_row0=-1)
        add(fn, "null_filter_misaligned_pointers", pred=8192 + 4, ref=8192 + 260, fstate=8192 + 520)
    for K in (0, 65):                                        # the K-sample call: ref, then K, then ctr, then the filter
        add("p3d_vae_seq_filter_mc", "K%d_null_ref" % K, K=K, ref=None)
        add("p3d_vae_seq_filter_mc", "K%d_global_step" % K, K=K, ctr=GLOBAL_STEP)
        add("p3d_vae_seq_filter_mc", "K%d_null_filter" % K, K=K)
    assert len({i for i, _, _ in c}) == len(c)
    return c


WORK = 16384                                             # the fake workspace's byte offset: behind every 256 * k
INTS = {"N", "S", "K", "R", "smooth", "U2", "U3", "D3", "cache", "ctr", "eps_row0", "work_bytes"}


def run(lib):
    """Every case against `lib` -> [{"id", "rc", "msg"}].  The fake device pointers are addresses
    inside one zeroed host buffer, 256-byte aligned at offset 0: nothing may follow them."""
    buf = (ctypes.c_double * 8192)()
    base = ctypes.addressof(buf)
    base += (-base) % 256
    N, S = 30, 2
    clip = dict(N=N, S=S, R=2, smooth=1, U2=32, U3=48, D3=96, cache=1, K=0, ctr=0, eps_row0=0, off_host=I64(0, 9, 30),
                work_bytes=1 << 16, m=None, v=None, eps=None, src=None, poses_u=None, src_u=None, ref_var=None)
    live = dict(clip, N=6, S=3, row_off=I64(0, 5, 5, 6), row_frame=I32(0, 1, 2, 3, 4, 9), row_kind=I32(1, 1, 1, 1, 2, 2),
                push_frame=I32(8, -1, 13), fstate=None, fstarted=None)
    seq = dict(v=None, N=N, S=S, K=2, ctr=0, eps_row0=0, seq_off=I64(0, 9, 30), eps=None, target=None, fstate=None,
               fstarted=None, ref_var=None, frame_err=None, seq_err=None)
    out = []
    for cid, fn, kw in cases():
        names = ORDER[fn].split()
        d = dict(seq if "seq_filter" in fn else live if "live" in fn else clip)
        for k, name in enumerate(names):                 # a distinct aligned address for every other pointer
            d.setdefault(name, 256 * k if name != "work" else WORK)
        d.update(kw)
        args = []
        for name in names:
            v = d[name]
            if name in INTS:
                args.append(v)
            elif isinstance(v, np.ndarray):
                args.append(ctypes.c_void_p(v.ctypes.data))
            else:
                args.append(None if v is None else ctypes.c_void_p(base + v))
        rc = getattr(lib, fn)(*args, None)
        out.append({"id": cid, "rc": int(rc), "msg": lib.p3d_last_error().decode() if rc else ""})
    del buf
    return out


# --------------------------------------------------------------------------------------
# behind a live filter (needs a GPU): the order inside the two sequence-filter calls
# --------------------------------------------------------------------------------------


def handle_cases():
    """[(id, function name, filter, {argument: value})] for the two sequence-filter calls with a live
    handle: 'seq' a sequence filter (144 -> 48, seq_len 3), 'bones' a bones filter, 'flat' a filter
    whose input (104) is no multiple of its output.  Every row is refused; consecutive checks are
    paired so that each pair pins which of the two answers, and every pointer of the alignment list
    is misaligned once on its own."""
    c = []
    for fn in ("p3d_vae_seq_filter", "p3d_vae_seq_filter_mc"):
        add = lambda name, flt="seq", **kw: c.append(("%s/%s" % (fn[4:], name), fn, flt, kw))   # noqa: E731
        add("bones_bad_S", "bones", S=0)
        add("no_sequence_shape_bad_S", "flat", S=0)
        add("null_pred_bones", "bones", pred=None)
        add("bad_S_bad_N", S=0, N=0)
        add("bad_N_bad_row0", N=0, eps_row0=-1)
        add("bad_row0_state_without_started", eps_row0=-1, fstarted=None)
        add("state_without_started_errors_without_target", fstarted=None, target=None)
        add("started_without_state", fstate=None)
        add("errors_without_target_misaligned_pred", target=None, pred=4)
        for name in ("pred", "eps", "target", "fstate", "ref"):
            add("misaligned_%s" % name, **{name: 4})
        add("misaligned_pred_and_ref", pred=8, ref=12)
    add("misaligned_ref_var", ref_var=4)                     # (the K-sample call alone has it)
    add("K0_bones", "bones", K=0)
    add("global_step_bones", "bones", ctr=GLOBAL_STEP)
    add("null_ref_misaligned_pred", ref=None, pred=4)
    return c


def run_handles(lib, filters, base, seq_off):
    """handle_cases against `lib`.  filters: {name: p3d_vae handle}; base: a 256-byte aligned device
    address with 16 KiB of real memory per pointer argument behind it (a value in a row is a byte
    offset INTO the argument's own block: were a row ever launched, it would stay inside); seq_off:
    the device offsets [0, 9, 30]."""
    out = []
    for cid, fn, flt, kw in handle_cases():
        names = ORDER[fn].split()
        d = dict(N=30, S=2, K=2, ctr=0, eps_row0=0)
        d.update({name: 0 for name in names if name not in d})
        d.update(kw)
        args = []
        for k, name in enumerate(names):
            v = d[name]
            if name == "v":
                args.append(filters[flt])
            elif name == "seq_off":
                args.append(ctypes.c_void_p(seq_off))
            elif name in INTS:
                args.append(v)
            else:
                args.append(None if v is None else ctypes.c_void_p(base + 16384 * k + v))
        rc = getattr(lib, fn)(*args, None)
        out.append({"id": cid, "rc": int(rc), "msg": lib.p3d_last_error().decode() if rc else ""})
    return out


# --------------------------------------------------------------------------------------
# behind a live model and a live filter (needs a GPU): the order inside the two batched lift calls
# --------------------------------------------------------------------------------------


def lift_handle_cases():
    """[(id, function name, filter, {argument: value})] for p3d_clips_lift and p3d_clips_lift_resampled
    with a live model (32 -> 48) and, but where `filter` is None, a live filter: 'seq', 'bones', 'flat'
    as in handle_cases.  Every row is refused; consecutive checks are paired so that each pair pins
    which of the two answers.  A pointer's value is a byte offset into its own block, or '=name': the
    address of another argument; work_bytes may be 'clips' (p3d_clips_workspace(N, S), the head of
    either workspace) or 'short' (one byte less than the call needs)."""
    c = []
    for fn in ("p3d_clips_lift", "p3d_clips_lift_resampled"):
        add = lambda name, flt="seq", **kw: c.append(("%s/%s" % (fn[4:], name), fn, flt, kw))   # noqa: E731
        add("dimension_sets_bad_U2", U2=65)
        add("dimension_sets_bad_U3_bad_D3", U3=97, D3=48)
        add("bad_D3_alias", D3=48, xy_s="=xy")
        add("alias_outputs_without_filter", None, xy_s="=xy")
        add("outputs_without_filter_bad_K", None, K=65)
        add("ref_var_without_filter", None, poses_u=None, src_u=None)
        add("src_unfiltered_without_filter", None, poses_u=None, ref_var=None)
        add("bones_bad_K", "bones", K=65)
        add("no_sequence_shape_bad_K", "flat", K=65)
        add("bad_K_global_step", K=65, ctr=GLOBAL_STEP)
        add("negative_K_global_step", K=-1, ctr=GLOBAL_STEP)
        add("global_step_K1_src_without_poses", K=1, ctr=GLOBAL_STEP, poses_u=None)
        add("global_step_K0_ref_var", K=0, ctr=GLOBAL_STEP)
        add("ref_var_K0_src_without_poses", K=0, poses_u=None)
        add("src_without_poses_bad_row0", poses_u=None, eps_row0=-1)
        add("bad_row0_misaligned_eps", eps_row0=-1, eps=4)
        add("misaligned_eps_null_offsets", eps=4, off_host=None)
        add("misaligned_ref_var_null_offsets", ref_var=4, off_dev=None)
        for n in (2, 8):
            add("smooth_clip_of_%d_null_work" % n, off_host=I64(0, n, 30), work=None)
        add("null_work_small", work=None, work_bytes=1)
        add("misaligned_work_small", work=4, work_bytes=1)
        add("not_256_small_for_the_clips", work=8, work_bytes=1)
        add("not_256_small_for_the_call", work=8, work_bytes="clips")
        add("not_256", work=8)
        add("small_for_the_call", work_bytes="short")
        add("small_for_the_call_no_filter", None, poses_u=None, src_u=None, ref_var=None, work_bytes="clips")
    add("null_xy_r_bad_U2", xy_r=None, U2=65)                # (the resampled call alone from here on)
    add("null_off_out_bad_D3", off_out=None, D3=48)
    add("alias_xy_r_xy_s_bad_K", xy_r="=xy_s", K=65)
    add("alias_xy_r_xy_bad_K", xy_r="=xy", K=65)
    add("smooth_clip_of_8_bad_R", off_host=I64(0, 8, 30), R=0)
    for r in (0, 17):
        add("R%d_clip_of_3" % r, smooth=0, off_host=I64(0, 3, 30), R=r)
    add("clip_of_3_not_256", smooth=0, off_host=I64(0, 27, 30), work=8)
    add("clip_of_3_small_for_the_call", smooth=0, off_host=I64(0, 3, 30), work_bytes="clips")
    return c


def run_lift_handles(lib, model, filters, base, off_dev, block=32768):
    """lift_handle_cases against `lib`.  model: a p3d_model handle with 32 inputs and 48 outputs;
    filters: {name: p3d_vae handle}; base: a 256-byte aligned device address with `block` bytes of real
    memory per argument behind it and, behind those, the larger call's workspace; off_dev: the device
    offsets [0, 9, 30].  Were a row ever launched, it would stay inside its blocks."""
    out = []
    for cid, fn, flt, kw in lift_handle_cases():
        names = ORDER[fn].split()
        d = dict(N=30, S=2, R=2, K=2, ctr=1, eps_row0=0, smooth=1, U2=32, U3=48, D3=96, cache=1, off_host=I64(0, 9, 30))
        need = int(lib.p3d_clips_lift_workspace(30, 2, 32, 48, int(flt is not None)) if fn == "p3d_clips_lift" else
                   lib.p3d_clips_lift_resampled_workspace(30, 2, 2, 32, 48, int(flt is not None)))
        d["work_bytes"] = need
        d.update({name: 0 for name in names if name not in d})
        d.update(kw)
        d["work_bytes"] = {"clips": int(lib.p3d_clips_workspace(30, 2)), "short": need - 1}.get(d["work_bytes"], d["work_bytes"])
        addr = {name: None if d[name] is None else base + block * k + d[name]
                for k, name in enumerate(names) if not isinstance(d[name], (str, np.ndarray)) and name not in INTS}
        args = []
        for name in names:
            v = d[name]
            if name == "m":
                args.append(model)
            elif name == "v":
                args.append(None if flt is None else filters[flt])
            elif name == "off_dev" and v is not None:
                args.append(ctypes.c_void_p(off_dev))
            elif name in INTS:
                args.append(v)
            elif isinstance(v, np.ndarray):
                args.append(ctypes.c_void_p(v.ctypes.data))
            else:
                a = addr[v[1:]] if isinstance(v, str) else addr[name]
                args.append(None if a is None else ctypes.c_void_p(a))
        rc = getattr(lib, fn)(*args, None)
        out.append({"id": cid, "rc": int(rc), "msg": lib.p3d_last_error().decode() if rc else ""})
    return out
