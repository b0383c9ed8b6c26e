"""A batch of OpenPose clips in one call (include/p3d.h: p3d_clips_prepare / p3d_clips_finish /
p3d_clips_lift; ClipLifter.lift_clips), bit for bit against tests/clip_oracle.py applied clip by
clip and against the existing per-clip calls (lift_clip, filter_sequences, p3d_clip_finish).
Nothing here has a tolerance: NaN positions and the signs of zeros are compared too."""
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
import linear_model  # noqa: E402
import openpose_frontend as of  # noqa: E402
import test_gpu_clip as tc  # noqa: E402  (crafted_outputs, check_crafted, model_setup, ...)
from top_vae_3d_pose import models  # noqa: E402

C = tc.C
USE2, USE3, IGN3 = tc.USE2, tc.USE3, tc.IGN3
assert_same_bits = tc.assert_same_bits
LAYOUTS = {
    "A": [9, 1, C - 1, C, C + 1, 2 * C + 5, 10],          # no clip starts on a multiple of C
    "B": [C, C + 1, 9, 3 * C + 5, 1, 1, 12],              # starts on and off multiples of C; one long clip
}
ZCOL = lambda s: s % 2   # noqa: E731  (the column that is zero from position 0 on in clip s)


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def work_for(n, s):
    nbytes = int(_p3d.lib().p3d_clips_workspace(n, s))
    return torch.empty(nbytes // 8, dtype=torch.float64, device="cuda"), nbytes


def crafted_clip(s, n, seed):
    """Clip s of a batch.  Columns 0-8 are never dropped at random and carry the cases:
    0 / 1  zero from position 0 on in the clips of >= 9 frames (column s % 2; the other column is
           non-zero everywhere, so the previous clip always ENDS non-zero in this clip's zero column)
    2      a zero run over whole chunks of the clip, 4: a short run across one chunk boundary
    6      a -0.0 median at position 0
    7      NaN in the clip's last three frames, 8: NaN in its first three (a neighbour's windows
           that reached across the boundary would turn NaN)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(40.0, 900.0, (n, 36))
    xy[:, 9:][rng.random((n, 27)) < 0.3] = 0.0
    xy[-3:, 7] = np.nan
    xy[:3, 8] = np.nan
    if n >= 9:
        xy[:, ZCOL(s)] = 0.0
        xy[0:6, 6] = -0.0
    if n >= 2 * C + 5:
        xy[C - 10:n - 2, 2] = 0.0                        # over every whole chunk past the first, ending mid-chunk
        xy[2 * C - 2:2 * C + 3, 4] = 0.0
    return xy


@pytest.fixture(scope="module")
def stats2():
    rng = np.random.default_rng(31)
    return rng.uniform(200, 600, 64), rng.uniform(50, 150, 64)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("smooth", [1, 0])
def test_prepare_matches_oracle_clip_by_clip(layout, smooth, stats2):
    mean2, std2 = stats2
    lens = LAYOUTS[layout]
    off, S, N = offsets(lens), len(lens), sum(lens)
    clips = [crafted_clip(s, n, 500 + 10 * s + len(layout)) for s, n in enumerate(lens)]
    per = [clip_oracle.smooth(c, smooth=bool(smooth)) for c in clips]
    want = np.concatenate(per)
    xy = np.concatenate(clips)

    d_xy, m2, s2, u2 = tc.dev(xy), tc.dev(mean2), tc.dev(std2), dp._dims(USE2, 64, "t")
    d_off = torch.from_numpy(off).cuda()
    x = torch.full((N, len(USE2)), 7.0, dtype=torch.float32, device="cuda")        # (sentinels: an unwritten
    xy_s = torch.full((N, 36), 7.0, dtype=torch.float64, device="cuda")            #  row fails)
    work, nbytes = work_for(N, S)
    p = _p3d.ptr
    _p3d.check(_p3d.lib().p3d_clips_prepare(p(d_xy), off.ctypes.data, p(d_off), S, N, smooth, p(m2), p(s2), p(u2),
                                            len(USE2), p(x), p(xy_s), p(work), nbytes, _p3d.stream_handle()),
               "p3d_clips_prepare")
    torch.cuda.synchronize()
    got, got_x = xy_s.cpu().numpy(), x.cpu().numpy()
    for s in range(S):
        assert_same_bits(got[off[s]:off[s + 1]], per[s], "xy_s of clip %d (%d frames)" % (s, lens[s]))
    want_x = dp.normalize(of.map_frames(want), mean2, std2, USE2, out_dtype=torch.float32).cpu().numpy()
    assert_same_bits(got_x, want_x, "x")

    if not smooth:
        assert same(want, xy)
        return
    # the cases are really there (properties of the oracle's results alone) ...
    for s, n in enumerate(lens):
        w = per[s]
        assert np.isnan(clips[s][-3:, 7]).all() and np.isnan(clips[s][:3, 8]).all()   # NaN beside both boundaries
        if n < 9:
            assert same(w, clips[s])                                  # a one-frame clip passes through
            continue
        assert not w[:, ZCOL(s)].any()                                # zero from position 0 on: stays zero
        if s > 0:
            assert per[s - 1][-1, ZCOL(s)] != 0                       # ... though the previous clip ended non-zero
        assert w[0, 6] == 0 and np.signbit(w[0, 6])                   # the -0.0 median at position 0, kept
        assert np.isfinite(w[:3, 7]).all() and np.isfinite(w[-3:, 8]).all()   # no neighbour's NaN got in
        if n >= 2 * C + 5:
            assert w[C - 1, 2] != 0 and np.all(w[C:n - 2, 2] == w[C - 1, 2])      # held over whole chunks
            assert w[2 * C, 4] == w[2 * C - 1, 4] != 0
    assert max(lens) >= 2 * C + 5
    # ... and a kernel that ignored the boundaries could not pass: the concatenation smoothed as
    # one clip differs from the per-clip result in every clip after the first
    whole = clip_oracle.smooth(xy)
    for s in range(1, S):
        assert not same(whole[off[s]:off[s + 1]], per[s]), "clip %d" % s


def crafted_batch(lens, kind, seed):
    """crafted_outputs clip by clip; a one-frame clip is one good (even s) or one failing frame."""
    parts = []
    for s, n in enumerate(lens):
        if n >= 9:
            y, xy_s, mean3, std3, fail, exact, lead, run = tc.crafted_outputs(n, kind, seed + s)
        else:
            rng = np.random.default_rng(seed + s)
            mean3, std3, _ = tc.stats3(kind)
            y = rng.uniform(-1, 1, (n, len(USE3))).astype(np.float32)
            xy_s = rng.uniform(400, 700, (n, 36))
            fail = np.full(n, s % 2 == 1)
            y[fail, list(USE3).index(int([d for d in USE3 if d % 3 == 0][0]))] = -100.0
            exact, lead, run = None, int(fail[0]), None
        parts.append((y, xy_s, fail, exact, lead, run))
    return parts, mean3, std3


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("kind", ["mixed", "high", "negative"])
@pytest.mark.parametrize("cache", [1, 0])
def test_finish_matches_oracle_clip_by_clip(layout, kind, cache):
    lens = LAYOUTS[layout]
    off, S, N = offsets(lens), len(lens), sum(lens)
    parts, mean3, std3 = crafted_batch(lens, kind, 900)
    y = np.concatenate([q[0] for q in parts])
    xy_s = np.concatenate([q[1] for q in parts])

    d_y, d_xy, m3, s3, u3 = tc.dev(y, torch.float32), tc.dev(xy_s), tc.dev(mean3), tc.dev(std3), dp._dims(USE3, 96, "t")
    d_off = torch.from_numpy(off).cuda()
    poses = torch.full((N, 96), 7.0, dtype=torch.float64, device="cuda")
    src = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    work, nbytes = work_for(N, S)
    p = _p3d.ptr
    _p3d.check(_p3d.lib().p3d_clips_finish(p(d_y), off.ctypes.data, p(d_off), S, N, p(d_xy), p(m3), p(s3), p(u3),
                                           len(USE3), 96, cache, p(poses), p(src), p(work), nbytes,
                                           _p3d.stream_handle()), "p3d_clips_finish")
    torch.cuda.synchronize()
    got, got_src = poses.cpu().numpy(), src.cpu().numpy()

    after_good, across = 0, 0
    for s, n in enumerate(lens):
        a, b = int(off[s]), int(off[s + 1])
        yq, xq, fail, exact, lead, run = parts[s]
        un = clip_oracle.unnormalize(yq, mean3, std3, USE3)
        want, want_src = clip_oracle.post(un, xq, cache_on_fail=bool(cache))
        np.testing.assert_array_equal(got_src[a:b], np.where(want_src >= 0, want_src + a, -1), "src of clip %d" % s)
        assert_same_bits(got[a:b], want, "poses of clip %d (%d frames)" % (s, n))
        # the cases are really there (the oracle's results alone)
        if n >= 9:
            tc.check_crafted(n, kind, cache, un, xq, want, want_src, fail, exact, lead, run)
        if cache and lead:
            assert np.all(want_src[:lead] == -1) and not want[:lead].any()      # zeros, src = -1 ...
            if s > 0 and not parts[s - 1][2][-1]:
                after_good += 1                                                  # ... right after a good frame
            across += lead > C or (run is not None)                              # a failing run over a chunk boundary
    if cache:
        assert after_good >= 3
        assert across >= 1 or kind != "negative"


def lifter_for(m, s, max_frames, cache=True):
    return of.ClipLifter(m, s["mean2"], s["std2"], USE2, s["mean3"], s["std3"], IGN3, max_frames=max_frames,
                         cache_on_fail=cache)


def per_clip(cl, clips):
    """lift_clip clip by clip: [(poses, xy_s, src, the network's rows)]."""
    out = []
    for xy in clips:
        poses, xy_s, src = cl.lift_clip(xy)
        out.append((poses, xy_s, src, cl.network_rows(len(xy)).clone()))
    return out


def test_lift_clips_equals_lift_clip_clip_by_clip():
    st, m, s = tc.model_setup()
    assert m.max_batch == 64
    lens = [23, 1, 69, 9, 64]
    off = offsets(lens)
    clips = [tc.clip_for_model(n, 40 + n) for n in lens]
    for cache in (True, False):
        cl = lifter_for(m, s, sum(lens), cache)
        want = per_clip(cl, clips)
        got = cl.lift_clips(clips)
        rows = cl.network_rows().cpu().numpy()
        assert len(got) == len(lens)
        for k, (g, (poses, xy_s, src, net)) in enumerate(zip(got, want)):
            assert sorted(g) == ["poses", "src", "xy_s"]
            assert_same_bits(g["xy_s"], xy_s, "xy_s of clip %d" % k)
            assert_same_bits(g["poses"], poses, "poses of clip %d" % k)
            np.testing.assert_array_equal(g["src"], src)
            assert g["src"].dtype == np.int32
            assert_same_bits(rows[off[k]:off[k + 1]], net.cpu().numpy(), "network rows of clip %d" % k)
        if cache:
            assert all(g["src"][0] == -1 for g in got)                 # (clip_for_model: position 0 fails)
        with pytest.raises(ValueError):
            cl.refined_rows()
        m.check_errors()
    m.close()


def finish_one(cl, y, xy_s):
    """p3d_clip_finish of one clip's rows y (device float32 [n, 48]) and smoothed 2D rows."""
    n = y.shape[0]
    d_xy = tc.dev(xy_s)
    poses = torch.empty((n, 96), dtype=torch.float64, device="cuda")
    src = torch.empty((n,), dtype=torch.int32, device="cuda")
    work, nbytes = tc.work_for(n)
    p = _p3d.ptr
    _p3d.check(_p3d.lib().p3d_clip_finish(p(y), n, p(d_xy), p(cl.m3), p(cl.s3), p(cl.u3), cl.u3.numel(), 96,
                                          int(cl.cache_on_fail), p(poses), p(src), p(work), nbytes,
                                          _p3d.stream_handle()), "p3d_clip_finish")
    torch.cuda.synchronize()
    return poses.cpu().numpy(), src.cpu().numpy()


FILTER_LENS = [9, 40, 17, 1, 23, 12, 31, 10, 9, 36, 28, 11, 19, 40, 14, 25, 9, 33, 22]   # 18 of 9..40 and a single frame


@pytest.fixture(scope="module")
def filtered():
    """The lifter, a seeded temporal filter, 19 clips (two 16-sequence tiles) and the per-clip
    results of the existing calls, computed once."""
    st, m, s = tc.model_setup(8)
    vae = models.VAE(144, 24, [40, 32], [32, 40], 48, max_batch=64, seed=17)
    lens = FILTER_LENS
    assert len(lens) == 19 and sorted(lens)[0] == 1 and sorted(lens)[1] == 9 and max(lens) == 40
    clips = [tc.clip_for_model(n, 300 + k) for k, n in enumerate(lens)]
    cl = lifter_for(m, s, sum(lens))
    base = per_clip(cl, clips)
    yield dict(m=m, vae=vae, cl=cl, lens=lens, off=offsets(lens), clips=clips, base=base)
    vae.close()
    m.close()


def chain(f, k, **kw):
    """Clip k through the existing calls: lift_clip's network rows -> filter_sequences -> p3d_clip_finish."""
    poses_u, xy_s, src_u, net = f["base"][k]
    n = f["lens"][k]
    o = f["vae"].filter_sequences(net, [0, n], want=("ref", "ref_var") if kw.get("samples") else ("ref",), **kw)
    poses, src = finish_one(f["cl"], o["ref"], xy_s)
    return poses, src, o["ref"].cpu().numpy(), (o["ref_var"].cpu().numpy() if "ref_var" in o else None)


@pytest.mark.parametrize("mode", ["eps", "stream", "samples_eps", "samples_stream"])
def test_filtered_lift_clips_equals_the_chain_of_existing_calls(filtered, mode):
    f = filtered
    cl, vae, off, lens = f["cl"], f["vae"], f["off"], f["lens"]
    N, K = int(off[-1]), (3 if mode.startswith("samples") else None)
    rng = np.random.default_rng(5)
    eps = None
    if mode.endswith("eps"):
        eps = rng.standard_normal((K, N, 24) if K else (N, 24)).astype(np.float32)
    ctr = None if eps is not None else 77
    got = cl.lift_clips(f["clips"], vae=vae, samples=K, eps=eps, ctr=ctr, unfiltered=True)
    refined = cl.refined_rows().cpu().numpy()
    differ = 0
    for k, g in enumerate(got):
        a, b = int(off[k]), int(off[k + 1])
        if eps is not None:
            kw = dict(eps=eps[:, a:b] if K else eps[a:b])
        else:
            kw = dict(ctr=ctr, eps_row0=a)
        poses, src, ref, ref_var = chain(f, k, samples=K, **kw)
        assert_same_bits(refined[a:b], ref, "refined rows of clip %d" % k)
        assert_same_bits(g["poses"], poses, "poses of clip %d (%d frames)" % (k, lens[k]))
        np.testing.assert_array_equal(g["src"], src)
        assert_same_bits(g["xy_s"], f["base"][k][1], "xy_s does not depend on the filter")
        assert_same_bits(g["poses_unfiltered"], f["base"][k][0], "unfiltered poses of clip %d" % k)
        np.testing.assert_array_equal(g["src_unfiltered"], f["base"][k][2])
        if K:
            assert_same_bits(g["ref_var"], ref_var, "ref_var of clip %d" % k)
            assert g["ref_var"].shape == (lens[k], 48) and g["ref_var"].dtype == np.float32
        else:
            assert "ref_var" not in g
        differ += not same(g["poses"], g["poses_unfiltered"])
    assert differ >= len(lens) - 1       # the filter changed every clip (the single frame fails either way: zeros)
    f["m"].check_errors()


def test_fresh_counter_advances_as_filter_sequences(filtered):
    f = filtered
    vae = f["vae"]
    before = vae._calls
    f["cl"].lift_clips(f["clips"][:2], vae=vae)
    assert vae._calls == before + 1
    f["cl"].lift_clips(f["clips"][:2], vae=vae, samples=4)
    assert vae._calls == before + 5
    f["cl"].lift_clips(f["clips"][:2], vae=vae, ctr=3)
    assert vae._calls == before + 5


def test_filtered_graph_replay_equals_eager(filtered):
    f = filtered
    cl, vae, off = f["cl"], f["vae"], f["off"]
    N = int(off[-1])
    got = cl.lift_clips(f["clips"], vae=vae, ctr=9, unfiltered=True)            # (sizes every buffer)
    want = {k: np.concatenate([g[k] for g in got]) for k in ("poses", "xy_s", "poses_unfiltered")}
    want_src = cl.hsrc.numpy()[:N].copy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cl.lift_clips_device(True, vae, None, None, 9, 0, True)
    torch.cuda.current_stream().wait_stream(side)
    cl.dout.fill_(3.0)
    cl.dout_u.fill_(3.0)
    cl.dxy.fill_(3.0)
    cl.dsrc.fill_(-9)
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(cl.dout.cpu().numpy()[:N], want["poses"])
    assert_same_bits(cl.dout_u.cpu().numpy()[:N], want["poses_unfiltered"])
    assert_same_bits(cl.dxy.cpu().numpy()[:N], want["xy_s"])
    np.testing.assert_array_equal(cl.dsrc.cpu().numpy()[:N], want_src)
    f["m"].check_errors()
    del graph


def test_argument_errors_in_c(filtered):
    f = filtered
    lib, E, p = _p3d.lib(), _p3d.P3D_ERR_ARG, _p3d.ptr
    cl, m, vae = f["cl"], f["m"], f["vae"]
    lens = [9, 1, 20]
    off = offsets(lens)
    N, S = int(off[-1]), len(lens)
    cl.lift_clips(f["clips"], vae=vae, samples=2, ctr=1, unfiltered=True)         # (every buffer exists)
    cl.set_offsets(off)
    torch.cuda.synchronize()
    good = dict(m=m._h, v=vae._h, K=2, eps=None, ctr=1, row0=0, xy=p(cl.din), offh=off, offd=p(cl.doff), S=S, N=N,
                smooth=1, U2=32, U3=48, D3=96, xy_s=p(cl.dxy), poses=p(cl.dout), src=p(cl.dsrc), pu=p(cl.dout_u),
                su=p(cl.dsrc_u), var=p(cl.dvar), w=cl.cwork_ptr, wb=cl.cwork_bytes)

    def call(**kw):
        a = dict(good, **kw)
        oh = None if a["offh"] is None else a["offh"].ctypes.data
        return lib.p3d_clips_lift(a["m"], a["v"], a["K"], a["eps"], a["ctr"], a["row0"], a["xy"], oh, a["offd"], a["S"],
                                  a["N"], a["smooth"], p(cl.m2), p(cl.s2), p(cl.u2), a["U2"], p(cl.m3), p(cl.s3),
                                  p(cl.u3), a["U3"], a["D3"], 1, a["xy_s"], a["poses"], a["src"], a["pu"], a["su"],
                                  a["var"], a["w"], a["wb"], m.stream())

    def bad(word, **kw):
        rc = call(**kw)
        msg = lib.p3d_last_error().decode()
        assert rc == E and msg.startswith("p3d_clips_lift: ") and word in msg, (kw, rc, msg)

    I = lambda *v: np.array(v, np.int64)   # noqa: E731,E741
    for name in ("m", "xy", "offh", "offd", "xy_s", "poses", "w"):
        bad("null", **{name: None})
    bad("start at 0", offh=I(1, 10, 11, 30))
    bad("decrease", offh=I(0, 20, 10, 30))
    bad("end at N", offh=I(0, 9, 10, 29))
    bad("empty", offh=I(0, 10, 10, 30))
    for n in range(2, 9):
        bad("min 9 frames", offh=I(0, 9, 9 + n, 30))
    bad("S must be", S=0)
    bad("N must be", N=0)
    bad("workspace too small", wb=int(lib.p3d_clips_lift_workspace(N, S, 32, 48, 1)) - 1)
    bad("workspace too small", wb=int(lib.p3d_clips_workspace(N, S)))
    bad("256-byte aligned", w=cl.cwork_ptr + 8)
    bad("96", D3=48)
    bad("do not match the model", U2=16)
    bad("do not match the model", U3=32)
    for K in (-1, 65):
        bad("K must be", K=K)
    bad("ref_var needs K", K=0)
    for name in ("var", "pu", "su"):                                              # asked for without a filter
        none = dict(v=None, var=None, pu=None, su=None)
        none[name] = good[name]
        bad("need a filter", **none)
    other = models.VAE(96, 8, [32], [32], 32, max_batch=64, seed=1)               # out = 32 != U3
    bad("sequence filter", v=other._h)
    other.close()
    other = models.VAE(56, 8, [32], [32], 48, max_batch=64, seed=1)               # in is no multiple of out
    bad("sequence filter", v=other._h)
    other.close()
    bones = models.VAEBones(64, 8, [32], [32], max_batch=64, seed=1)
    bad("bones filter", v=bones._h)
    bones.close()
    mb = linear_model.LinearModel(1024, 2, True, True, False, 64, 1e-3, "/tmp/p3d_clips", dtype="bfloat16", seed=3)
    bad("float32 models only", m=mb._h)
    mb.close()
    # nothing above was launched; the good calls run
    assert call() == 0 and call(K=0, var=None) == 0 and call(v=None, var=None, pu=None, su=None) == 0
    assert call(smooth=0, K=1) == 0
    torch.cuda.synchronize()
    m.check_errors()
    with pytest.raises(ValueError):
        _p3d.check(call(D3=48), "p3d_clips_lift")


def test_argument_errors_in_python(filtered):
    f = filtered
    cl, vae, clips = f["cl"], f["vae"], f["clips"]
    ok = clips[:3]
    with pytest.raises(ValueError, match="min 9 frames"):
        cl.lift_clips([clips[0], np.ones((5, 36))])
    assert len(cl.lift_clips([clips[0], np.ones((5, 36))], smooth=False)) == 2
    for wrong in ([], [np.ones((9, 35))], [np.ones((0, 36))], [np.ones(36)], clips + clips):
        with pytest.raises(ValueError):
            cl.lift_clips(wrong)
    for kw in (dict(samples=2), dict(eps=np.zeros((1, 24), np.float32)), dict(unfiltered=True)):     # need a filter
        with pytest.raises(ValueError, match="need a filter"):
            cl.lift_clips(ok, **kw)
    n = sum(len(c) for c in ok)
    for kw in (dict(samples=0), dict(samples=65), dict(samples=1.5), dict(eps=np.zeros((n + 1, 24), np.float32)),
               dict(eps=np.zeros((n, 16), np.float32)), dict(samples=2, eps=np.zeros((n, 24), np.float32))):
        with pytest.raises(ValueError):
            cl.lift_clips(ok, vae=vae, **kw)
    bones = models.VAEBones(64, 8, [32], [32], max_batch=64, seed=1)
    other = models.VAE(96, 8, [32], [32], 32, max_batch=64, seed=1)
    plain = models.VAE(56, 8, [32], [32], 48, max_batch=64, seed=1)
    for v in (bones, other, plain):
        with pytest.raises(ValueError):
            cl.lift_clips(ok, vae=v)
        v.close()
    with pytest.raises(ValueError):
        cl.set_offsets([0, 5, 5, 9])
    with pytest.raises(ValueError):
        cl.set_offsets([1, 5])
    with pytest.raises(ValueError):
        cl.set_offsets([0, cl.max_frames + 1])
    assert len(cl.lift_clips(ok, vae=vae)) == 3                                  # the lifter still works
    f["m"].check_errors()


def write_clip(d, raw):
    os.makedirs(d, exist_ok=True)
    for i, row in enumerate(raw):
        with open(os.path.join(d, "clip_%012d_keypoints.json" % i), "w") as fh:
            json.dump({"people": [{"pose_keypoints_2d": [float(v) for v in row]}]}, fh)


def read_export(path, joints):
    data = json.load(open(path))
    frames = sorted(data, key=int)
    return frames, np.array([[data[fr][str(j)]["translate"] for j in range(joints)] for fr in frames]).reshape(len(frames), -1)


def test_sandbox_driver_clips_root_and_filter(tmp_path):
    import openpose_3dpose_sandbox as sandbox
    with np.load(tc.GOLD, allow_pickle=False) as z:
        raw = {n: z["raw_body25_%d" % n] for n in (9, 10, 23)}
        sm = {n: z["sm_body25_%d" % n] for n in (9, 10, 23)}
    root = tmp_path / "clips"
    names = {"a_nine": 9, "b_ten": 10, "c_long": 23}
    for name, n in names.items():
        write_clip(str(root / name), raw[n])
    base = ["--synthetic", "--residual", "--batch_norm", "--max_batch", "128", "--verbose", "0",
            "--clips_root", str(root)]
    paths = sandbox.main(base + ["--out_dir", str(tmp_path / "plain")])
    assert len(paths) == 3
    plain = {}
    for (p3, p2), (name, n) in zip(paths, names.items()):
        assert os.path.dirname(p3) == str(tmp_path / "plain" / name) and os.path.basename(p3) == "3d_data.json"
        frames, two = read_export(p2, 18)
        assert frames == [str(i) for i in range(n)]
        assert_same_bits(two, sm[n], "2D export of %s" % name)                 # the reference's own smoothing
        plain[name] = read_export(p3, 32)[1]
        assert plain[name].shape == (n, 96) and np.isfinite(plain[name]).all()
    vae = models.VAE(144, 24, [40, 32], [32, 40], 48, max_batch=64, seed=23)
    weights = str(tmp_path / "filter.npz")
    vae.save_weights(weights)
    vae.close()
    paths = sandbox.main(base + ["--out_dir", str(tmp_path / "filtered"), "--vae_filter", weights,
                                 "--filter_samples", "2", "--export_unfiltered"])
    for (p3, p2, pu), (name, n) in zip(paths, names.items()):
        assert os.path.basename(pu) == "3d_data_unfiltered.json" and os.path.dirname(pu) == str(tmp_path / "filtered" / name)
        assert_same_bits(read_export(pu, 32)[1], plain[name], "unfiltered export of %s" % name)
        assert_same_bits(read_export(p2, 18)[1], sm[n])
        if plain[name].any():                # (frames that fail with and without the filter are zeros in both)
            assert not same(read_export(p3, 32)[1], plain[name])
    # a single --pose_estimation_json clip takes the filter too
    one = sandbox.main(["--synthetic", "--residual", "--batch_norm", "--max_batch", "128", "--verbose", "0",
                        "--pose_estimation_json", str(root / "c_long"), "--out_dir", str(tmp_path / "one"),
                        "--vae_filter", weights, "--export_unfiltered"])
    assert [os.path.basename(q) for q in one] == ["3d_data.json", "2d_data.json", "3d_data_unfiltered.json"]
    assert_same_bits(read_export(one[2], 32)[1], plain["c_long"])
