"""Live OpenPose streams lifted tick by tick (include/p3d.h: p3d_live_prepare / p3d_live_finish /
p3d_live_push; openpose_frontend.LiveLifter; openpose_3dpose_sandbox_realtime.py), bit for bit
against the clip path on the streams' whole frame lists: p3d_clips_prepare, the existing forward
on each tick's rows, filter_sequences with carried state, p3d_clips_finish.  Four slots, streams of
13, 1, 9 and 20 frames opened at staggered ticks, and the one-frame stream's slot reused by a
stream of 10.  Nothing here has a tolerance: NaN positions and the signs of zeros are compared too."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
sys.path.insert(0, HERE)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import _p3d  # noqa: E402
import clip_oracle  # noqa: E402
import data_pipeline as dp  # noqa: E402
import live_oracle  # noqa: E402
import openpose_frontend as of  # noqa: E402
import test_gpu_clip as tc  # noqa: E402
import test_gpu_clips as tcs  # noqa: E402
from top_vae_3d_pose import models  # noqa: E402

USE2, USE3, IGN3 = tc.USE2, tc.USE3, tc.IGN3
assert_same_bits = tc.assert_same_bits
S = 4
SCHED = [(0, 0, 0, 13), (1, 3, 3, 1), (2, 1, 1, 9), (3, 2, 2, 20), (4, 3, 6, 10)]   # (stream, slot, first tick, frames)
LENS = [n for _, _, _, n in SCHED]
OFF = tcs.offsets(LENS)


def ticks(sched=SCHED, smooth=True, slots=S):
    """The schedule tick by tick: [(push {slot: (stream, frame)}, close [(slot, stream)], rows
    [(slot, stream, frame, kind)] in slot order)].  A stream is closed in the tick after its last
    frame.  The rows come from the numpy restatement of the rule (tests/live_oracle.py)."""
    sent, closed, out, t = {i: 0 for i, _, _, _ in sched}, set(), [], 0
    while len(closed) < len(sched):
        push, close = {}, []
        for i, slot, t0, n in sched:
            if i in closed or t < t0:
                continue
            if sent[i] == n:
                close.append((slot, i))
            else:
                assert slot not in push
                push[slot] = (i, sent[i])
        rows = []
        for slot in range(slots):
            if slot in push:
                i = push[slot][0]
                sent[i] += 1
                rows += [(slot, i, f, k) for f, k in live_oracle.plan_push(sent[i], smooth)]
            for sl, i in close:
                if sl == slot:
                    rows += [(slot, i, f, k) for f, k in live_oracle.plan_close(sent[i], smooth)]
                    closed.add(i)
        out.append((push, close, rows))
        t += 1
    return out


class Raw:
    """The tick's pinned table and the slots' device state for the two kernels' own calls."""

    def __init__(self, slots=S):
        pin = lambda shape, dt: torch.zeros(shape, dtype=dt, pin_memory=True)   # noqa: E731
        self.S = slots
        self.hin, self.push = pin((slots, 36), torch.float64), pin((slots,), torch.int32)
        self.off, self.frame, self.kind = pin((slots + 1,), torch.int64), pin((5 * slots,), torch.int32), pin((5 * slots,), torch.int32)
        self.state = torch.empty(int(_p3d.lib().p3d_live_state_bytes(slots, len(USE3))), dtype=torch.uint8, device="cuda")
        self.state.fill_(0x5a)                                        # (garbage: the reset must do its work)
        self.reset(-1)

    def reset(self, slot):
        _p3d.check(_p3d.lib().p3d_live_reset(self.state.data_ptr(), self.S, slot, _p3d.stream_handle()), "p3d_live_reset")

    def table(self, push, rows, streams=None):
        """Fill the table; a stream's first push resets its slot.  Returns the row count."""
        self.push.fill_(-1)
        for slot, (i, f) in push.items():
            self.push[slot] = f
            if streams is not None:
                self.hin[slot] = torch.from_numpy(streams[i][f])
            if f == 0:
                self.reset(slot)
        off = np.zeros(self.S + 1, np.int64)
        for r, (slot, _, f, k) in enumerate(rows):
            off[slot + 1:] = r + 1
            self.frame[r], self.kind[r] = f, k
        self.off.copy_(torch.from_numpy(off))
        return len(rows)


def clips_prepare(streams, smooth, mean2, std2):
    """p3d_clips_prepare of the whole streams, one clip each -> (xy_s [N, 36], x [N, U2]) on the host."""
    xy = np.concatenate(streams)
    N = xy.shape[0]
    d_xy, m2, s2, u2 = tc.dev(xy), tc.dev(mean2), tc.dev(std2), dp._dims(USE2, 64, "t")
    d_off = torch.from_numpy(OFF).cuda()
    x = torch.full((N, len(USE2)), 7.0, dtype=torch.float32, device="cuda")
    xy_s = torch.full((N, 36), 7.0, dtype=torch.float64, device="cuda")
    work, nbytes = tcs.work_for(N, len(streams))
    p = _p3d.ptr
    _p3d.check(_p3d.lib().p3d_clips_prepare(p(d_xy), OFF.ctypes.data, p(d_off), len(streams), N, int(smooth), p(m2), p(s2),
                                            p(u2), len(USE2), p(x), p(xy_s), p(work), nbytes, _p3d.stream_handle()),
               "p3d_clips_prepare")
    torch.cuda.synchronize()
    return xy_s.cpu().numpy(), x.cpu().numpy()


def clips_finish(y, xy_s, mean3, std3, cache):
    """p3d_clips_finish of the whole streams -> (poses [N, 96], src [N] stream-local) on the host."""
    N = y.shape[0]
    d_y, d_xy, m3, s3, u3 = tc.dev(y, torch.float32), tc.dev(xy_s), tc.dev(mean3), tc.dev(std3), dp._dims(USE3, 96, "t")
    d_off = torch.from_numpy(OFF).cuda()
    poses = torch.full((N, 96), 7.0, dtype=torch.float64, device="cuda")
    src = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    work, nbytes = tcs.work_for(N, len(LENS))
    p = _p3d.ptr
    _p3d.check(_p3d.lib().p3d_clips_finish(p(d_y), OFF.ctypes.data, p(d_off), len(LENS), N, p(d_xy), p(m3), p(s3), p(u3),
                                           len(USE3), 96, int(cache), p(poses), p(src), p(work), nbytes,
                                           _p3d.stream_handle()), "p3d_clips_finish")
    torch.cuda.synchronize()
    src = src.cpu().numpy()
    local = np.concatenate([np.where(src[OFF[i]:OFF[i + 1]] >= 0, src[OFF[i]:OFF[i + 1]] - OFF[i], -1) for i in range(len(LENS))])
    return poses.cpu().numpy(), local.astype(np.int32)


@pytest.mark.parametrize("smooth", [1, 0])
def test_prepare_tick_by_tick_equals_clips_prepare(smooth):
    rng = np.random.default_rng(31)
    mean2, std2 = rng.uniform(200, 600, 64), rng.uniform(50, 150, 64)
    streams = [tcs.crafted_clip(i, n, 700 + i) for i, n in enumerate(LENS)]
    want_s, want_x = clips_prepare(streams, smooth, mean2, std2)
    raw = Raw()
    m2, s2, u2 = tc.dev(mean2), tc.dev(std2), dp._dims(USE2, 64, "t")
    x = torch.empty((5 * S, len(USE2)), dtype=torch.float32, device="cuda")
    xy_s = torch.empty((5 * S, 36), dtype=torch.float64, device="cuda")
    got_s, got_x, order = np.full_like(want_s, 7.0), np.full_like(want_x, 7.0), {i: [] for i in range(len(LENS))}
    p = _p3d.ptr
    for push, close, rows in ticks(smooth=bool(smooth)):
        N = raw.table(push, rows, streams)
        x.fill_(7.0)
        xy_s.fill_(7.0)
        _p3d.check(_p3d.lib().p3d_live_prepare(p(raw.hin), p(raw.push), p(raw.off), p(raw.frame), p(raw.kind), S, N, smooth,
                                               p(m2), p(s2), p(u2), len(USE2), p(raw.state), p(x), p(xy_s),
                                               _p3d.stream_handle()), "p3d_live_prepare")
        torch.cuda.synchronize()                                      # (the table is rewritten for the next tick)
        hx, hs = x.cpu().numpy(), xy_s.cpu().numpy()
        assert (hx[N:] == 7.0).all() and (hs[N:] == 7.0).all()        # nothing past the tick's rows
        for r, (_, i, f, _) in enumerate(rows):
            got_s[OFF[i] + f], got_x[OFF[i] + f] = hs[r], hx[r]
            order[i].append(f)
    for i, n in enumerate(LENS):
        assert order[i] == list(range(n)), "stream %d" % i            # every frame once, in order
        assert_same_bits(got_s[OFF[i]:OFF[i + 1]], want_s[OFF[i]:OFF[i + 1]], "xy_s of stream %d (%d frames)" % (i, n))
        assert_same_bits(got_x[OFF[i]:OFF[i + 1]], want_x[OFF[i]:OFF[i + 1]], "x of stream %d (%d frames)" % (i, n))
    if smooth:   # the cases are there: held zeros from frame 0, a kept -0.0 at frame 0, NaN beside both ends
        for i, n in enumerate(LENS):
            if n >= 9:
                w = want_s[OFF[i]:OFF[i + 1]]
                assert not w[:, tcs.ZCOL(i)].any() and w[0, 6] == 0 and np.signbit(w[0, 6])
                assert np.isnan(streams[i][-3:, 7]).all() and np.isfinite(w[:3, 7]).all()
        assert not tcs.same(want_s, np.concatenate(streams))


def finish_streams(kind):
    """crafted_batch outputs per stream, with a failing run over frames 7 .. 11 of the 20-frame
    stream (one tick each: the run crosses five ticks); stream 1 is one failing frame."""
    parts, mean3, std3 = tcs.crafted_batch(LENS, kind, 900)
    xdim = list(USE3).index(int([d for d in USE3 if d % 3 == 0][0]))
    parts[3][0][7:12, xdim] = -100.0
    return [q[0] for q in parts], [q[1] for q in parts], mean3, std3


@pytest.mark.parametrize("kind", ["mixed", "high", "negative"])
@pytest.mark.parametrize("cache", [1, 0])
def test_finish_tick_by_tick_equals_clips_finish(kind, cache):
    ys, xs, mean3, std3 = finish_streams(kind)
    want, want_src = clips_finish(np.concatenate(ys), np.concatenate(xs), mean3, std3, cache)
    raw = Raw()
    m3, s3, u3 = tc.dev(mean3), tc.dev(std3), dp._dims(USE3, 96, "t")
    poses = torch.empty((5 * S, 96), dtype=torch.float64, device="cuda")
    src = torch.empty((5 * S,), dtype=torch.int32, device="cuda")
    got, got_src = np.full_like(want, 7.0), np.full_like(want_src, -7)
    p = _p3d.ptr
    for push, close, rows in ticks():
        N = raw.table(push, rows)
        if not N:
            continue
        y = tc.dev(np.stack([ys[i][f] for _, i, f, _ in rows]), torch.float32)
        xy_s = tc.dev(np.stack([xs[i][f] for _, i, f, _ in rows]))
        poses.fill_(7.0)
        src.fill_(-7)
        _p3d.check(_p3d.lib().p3d_live_finish(p(y), p(raw.off), p(raw.frame), S, N, p(xy_s), p(m3), p(s3), p(u3), len(USE3),
                                              96, cache, p(raw.state), p(poses), p(src), _p3d.stream_handle()),
                   "p3d_live_finish")
        torch.cuda.synchronize()
        hp, hs = poses.cpu().numpy(), src.cpu().numpy()
        assert (hp[N:] == 7.0).all() and (hs[N:] == -7).all()
        for r, (_, i, f, _) in enumerate(rows):
            got[OFF[i] + f], got_src[OFF[i] + f] = hp[r], hs[r]
    for i, n in enumerate(LENS):
        a, b = OFF[i], OFF[i + 1]
        np.testing.assert_array_equal(got_src[a:b], want_src[a:b], "src of stream %d" % i)
        assert_same_bits(got[a:b], want[a:b], "poses of stream %d (%d frames)" % (i, n))
    if cache:   # the cases are there (the clip call's results alone)
        assert (want_src[OFF[3] + 7:OFF[3] + 12] == 6).all()          # a failing run across ticks
        assert all(want_src[OFF[i]] == -1 and not want[OFF[i]].any() for i in (0, 2, 3, 4))   # a failing first frame
        assert want_src[OFF[1]] == -1 and not want[OFF[1]].any()      # the one-frame failing stream
        assert want_src[OFF[4] + 9] == 9                              # the reused slot's stream ends on its own pose
    else:
        np.testing.assert_array_equal(want_src, np.concatenate([np.arange(n) for n in LENS]))


# ------------------------------------------------------------------------------- LiveLifter
def make_lifter(m, s, slots=S, cache=True, smooth=True, vae=None, samples=None):
    return of.LiveLifter(m, s["mean2"], s["std2"], USE2, s["mean3"], s["std3"], IGN3, slots=slots, cache_on_fail=cache,
                         smooth=smooth, vae=vae, samples=samples)


def drive(lifter, streams, sched=SCHED, slots=S):
    """The schedule through LiveLifter -> per stream dict(frames, poses, xy_s, src[, ref_var]) concatenated."""
    got = {i: [] for i, _, _, _ in sched}
    for push, close, rows in ticks(sched, lifter.smooth, slots):
        for slot, (i, f) in sorted(push.items()):
            if f == 0:
                assert lifter.open() == slot
        out = lifter.push({slot: streams[i][f] for slot, (i, f) in push.items()}, close=[slot for slot, _ in close])
        by_slot = {}
        for slot, i, f, _ in rows:
            by_slot.setdefault(slot, (i, []))[1].append(f)
        assert sorted(out) == sorted(by_slot)
        for slot, (i, frames) in by_slot.items():
            assert out[slot]["frames"].tolist() == frames
            got[i].append(out[slot])
    return {i: {k: np.concatenate([g[k] for g in parts]) for k in parts[0]} for i, parts in got.items() if parts}


def chain(m, s, streams, vae=None, samples=None, ctr=0, cache=True, sched=SCHED, slots=S):
    """The same schedule through the existing calls: p3d_clips_prepare on the whole streams, each
    tick's rows through the existing forward at that batch, filter_sequences with carried state and
    the tick's keys, the rows scattered back into clip order, p3d_clips_finish."""
    xy_s, x = clips_prepare(streams, True, s["mean2"], s["std2"])
    N = x.shape[0]
    y = np.zeros((N, len(USE3)), np.float32)
    var = np.zeros((N, len(USE3)), np.float32)
    state = vae.new_seq_state(slots) if vae is not None else None
    emitted = 0
    for push, close, rows in ticks(sched, True, slots):
        for slot, (i, f) in push.items():
            if f == 0 and state is not None:
                state[1][slot] = 0                                     # a reopened slot: a fresh sequence
        if not rows:
            continue
        idx = [OFF[i] + f for _, i, f, _ in rows]
        out = m.forward_device(torch.from_numpy(x[idx]).cuda(), False, 1.0, ctr=0)
        if vae is not None:
            off = np.zeros(slots + 1, np.int64)
            for r, (slot, _, _, _) in enumerate(rows):
                off[slot + 1:] = r + 1
            o = vae.filter_sequences(out, off, ctr=ctr, eps_row0=emitted, state=state, samples=samples,
                                     want=("ref", "ref_var") if samples else ("ref",))
            out = o["ref"]
            if samples:
                var[idx] = o["ref_var"].cpu().numpy()
        y[idx] = out.cpu().numpy()
        emitted += len(rows)
    poses, src = clips_finish(y, xy_s, s["mean3"], s["std3"], cache)
    return dict(poses=poses, xy_s=xy_s, src=src, ref_var=var)


@pytest.fixture(scope="module")
def session():
    st, m, s = tc.model_setup(8)
    # a narrow 3D scale keeps every exported value near its mean whatever the fresh weights predict:
    # a frame then fails exactly where its smoothed spine_x is below 530 (model_setup), so every
    # stream of more than one frame has good frames behind its failing first ones
    s["std3"] = s["std3"] * 1e-3
    vae = models.VAE(144, 24, [40, 32], [32, 40], 48, max_batch=64, seed=17)
    streams = [tc.clip_for_model(n, 300 + i) for i, n in enumerate(LENS)]
    plain = drive(make_lifter(m, s), streams)
    yield dict(m=m, s=s, vae=vae, streams=streams, plain=plain)
    vae.close()
    m.close()


@pytest.mark.parametrize("mode", ["none", "filter", "samples"])
def test_live_lifter_equals_the_chain_of_existing_calls(session, mode):
    f = session
    m, s, streams = f["m"], f["s"], f["streams"]
    vae = None if mode == "none" else f["vae"]
    K = 2 if mode == "samples" else None
    if mode == "none":
        got, ctr = f["plain"], 0
    else:
        before = vae._calls
        lifter = make_lifter(m, s, vae=vae, samples=K)
        assert lifter.ctr == before + 1 and vae._calls == before + (K or 1) and lifter.latency() == 4
        got, ctr = drive(lifter, streams), lifter.ctr
    want = chain(m, s, streams, vae, K, ctr)
    for i, n in enumerate(LENS):
        a, b = OFF[i], OFF[i + 1]
        g = got[i]
        assert sorted(g) == sorted(["frames", "poses", "xy_s", "src"] + (["ref_var"] if K else []))
        assert g["frames"].tolist() == list(range(n))
        assert_same_bits(g["xy_s"], want["xy_s"][a:b], "xy_s of stream %d" % i)
        assert_same_bits(g["poses"], want["poses"][a:b], "poses of stream %d (%d frames)" % (i, n))
        np.testing.assert_array_equal(g["src"], want["src"][a:b])
        assert g["src"].dtype == np.int32
        if K:
            assert_same_bits(g["ref_var"], want["ref_var"][a:b], "ref_var of stream %d" % i)
            assert g["ref_var"].dtype == np.float32 and (n == 1 or g["ref_var"].any())
        if vae is not None and n > 1:                                 # the filter changed every stream's poses
            assert not tcs.same(g["poses"], f["plain"][i]["poses"]), "stream %d" % i
        assert g["src"][0] == -1 and not g["poses"][0].any()          # (clip_for_model: frame 0 fails)
        assert n == 1 or (g["src"][-1] >= 5 and g["poses"][-1].any())  # ... and good frames follow
    m.check_errors()


def test_a_reopened_slot_gives_the_bits_of_a_fresh_session(session):
    f = session
    m, s = f["m"], f["s"]
    first, second = tc.clip_for_model(13, 51), tc.clip_for_model(10, 52)
    assert (second[0:5, 2] == 450.0).all()                            # the second stream starts on failing frames
    both = drive(make_lifter(m, s, slots=1), [first, second], sched=[(0, 0, 0, 13), (1, 0, 14, 10)], slots=1)
    fresh = drive(make_lifter(m, s, slots=1), [second], sched=[(0, 0, 0, 10)], slots=1)
    assert both[0]["src"][-1] >= 5                                    # the first stream left a good pose behind
    for k in ("frames", "poses", "xy_s", "src"):
        assert_same_bits(both[1][k], fresh[0][k], k)
    assert (fresh[0]["src"][:5] == -1).all() and not fresh[0]["poses"][:5].any()
    m.check_errors()


def test_a_short_stream_raises_at_close_and_leaves_the_others_alone(session):
    f = session
    m, s = f["m"], f["s"]
    long_, short = tc.clip_for_model(13, 61), tc.clip_for_model(5, 62)
    alone = drive(make_lifter(m, s, slots=2), [long_], sched=[(0, 0, 0, 13)], slots=2)[0]
    lifter = make_lifter(m, s, slots=2)
    a, b = lifter.open(), lifter.open()
    parts = []
    for t in range(13):
        out = lifter.push({a: long_[t], b: short[t]} if t < 5 else {a: long_[t]})
        assert sorted(out) in ([], [a])                               # (the short stream never has a final row)
        if t == 6:
            with pytest.raises(ValueError, match="slot %d.*5 frames.*min 9 frames" % b):
                lifter.close(b)
            assert not lifter.is_open[b] and lifter.is_open[a]
            with pytest.raises(ValueError, match="not open"):
                lifter.push({b: short[0]})
            assert lifter.open() == b                                 # the slot is free again
        if a in out:
            parts.append(out[a])
    parts.append(lifter.close(a))
    for k in ("frames", "poses", "xy_s", "src"):
        assert_same_bits(np.concatenate([q[k] for q in parts]), alone[k], k)
    with pytest.raises(ValueError, match="36 keypoint values"):
        lifter.push({b: np.zeros(35)})
    with pytest.raises(ValueError, match="pushed and closed"):
        lifter.push({b: np.zeros(36)}, close=[b])
    assert make_lifter(m, s, smooth=False).latency() == 0
    m.check_errors()


# ------------------------------------------------------------------------------- the driver
def read_export(path, joints):
    data = json.load(open(path))
    frames = sorted(data, key=int)
    return frames, np.array([[data[fr][str(j)]["translate"] for j in range(joints)] for fr in frames]).reshape(len(frames), -1)


def test_realtime_driver_equals_the_clip_driver(tmp_path):
    import data_utils
    import openpose_3dpose_sandbox as sandbox
    import openpose_3dpose_sandbox_realtime as rt
    import predict_3dpose as p3
    with np.load(tc.GOLD, allow_pickle=False) as z:
        raw = z["raw_body25_23"][:13]
    frames = tmp_path / "json"
    tcs.write_clip(str(frames), raw)
    base = ["--synthetic", "--residual", "--batch_norm", "--max_batch", "128", "--verbose", "0",
            "--pose_estimation_json", str(frames)]
    live = ["--idle_exit", "0"]
    l3, l2 = rt.main(base + live + ["--out_dir", str(tmp_path / "live")])
    c3, c2 = sandbox.main(base + ["--out_dir", str(tmp_path / "clip")])
    names, two = read_export(l2, 18)
    assert names == [str(i) for i in range(13)] == read_export(c2, 18)[0]
    assert_same_bits(two, read_export(c2, 18)[1], "2d_data.json")    # exactly the clip driver's
    n3, n2 = rt.main(base + live + ["--no_smooth", "--out_dir", str(tmp_path / "live_raw")])
    _, xy = of.read_openpose_json(str(frames))
    assert_same_bits(read_export(n2, 18)[1], xy, "2d_data.json without smoothing")

    # 3d_data.json: the same model (the drivers' seeded weights), the forward at the ticks' batches
    flags = rt.build_parser().parse_args(base + live)
    p3.FLAGS = flags
    d = p3.load_data(flags)
    with p3.Session() as sess:
        model = p3.create_model(sess, data_utils.define_actions(flags.action), 128, flags)
        stats = (d["data_mean_2d"], d["data_std_2d"], d["dim_to_use_2d"], d["data_mean_3d"], d["data_std_3d"],
                 d["dim_to_ignore_3d"])
        use3 = np.setdiff1d(np.arange(96), np.asarray(d["dim_to_ignore_3d"], np.int64))
        # --no_smooth: one row per tick, FrameLifter's batch-1 bits
        fl = of.FrameLifter(model, *stats, batch=1)
        un = np.concatenate([fl.lift(row) for row in xy])
        want, _ = clip_oracle.post(un, xy, cache_on_fail=flags.cache_on_fail)
        assert_same_bits(read_export(n3, 32)[1], want, "3d_data.json without smoothing")
        # smoothing: ticks of 5, 1, 1, 1, 1 and 4 rows
        xy_s = clip_oracle.smooth(xy)
        x = dp.normalize(of.map_frames(xy_s), d["data_mean_2d"], d["data_std_2d"], d["dim_to_use_2d"], out_dtype=torch.float32)
        y = torch.cat([model.forward_device(x[a:b].contiguous(), False, 1.0, ctr=0)
                       for a, b in ((0, 5), (5, 6), (6, 7), (7, 8), (8, 9), (9, 13))]).cpu().numpy()
        want, _ = clip_oracle.post(clip_oracle.unnormalize(y, d["data_mean_3d"], d["data_std_3d"], use3), xy_s,
                                   cache_on_fail=flags.cache_on_fail)
        assert_same_bits(read_export(l3, 32)[1], want, "3d_data.json")
        model.close()
    for flag in ("--interpolation", "--write_gif", "--export_unfiltered"):
        with pytest.raises(SystemExit):
            rt.main(base + live + [flag])
