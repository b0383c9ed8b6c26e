"""ClipLifter's two batched device calls stand on one owner of their rows (openpose_frontend._RowBuffers)
and one checked binding of their shared arguments (ClipLifter._batch_args): a call that needs no more
than an earlier one keeps every address (a captured graph holds them), and the two calls refuse the
same bad arguments in the same words -- the words they had when each wrote its checks out."""
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

import test_gpu_clip as tc  # noqa: E402  (model_setup, clip_for_model, assert_same_bits)
import test_gpu_clips as tcs  # noqa: E402  (lifter_for)
from top_vae_3d_pose import models  # noqa: E402

LENS, R = [9, 23], 2
N = sum(LENS)


@pytest.fixture(scope="module")
def setup():
    st, m, s = tc.model_setup(8)
    vae = models.VAE(144, 24, [40, 32], [32, 40], 48, max_batch=64, seed=17)
    clips = [tc.clip_for_model(n, 500 + n) for n in LENS]
    yield dict(m=m, s=s, vae=vae, clips=clips)
    vae.close()
    m.close()


def addresses(cl):
    out = {"work": cl.work_ptr, "cwork": cl.cwork_ptr, "resampled work": cl.resampled.work_ptr}
    for name in "din dxy dout dsrc hin hxy hout hsrc dout_u dsrc_u dvar doff".split():
        out[name] = getattr(cl, name).data_ptr()
    for tag, b in (("rows", cl.rows), ("resampled", cl.resampled)):
        for side, tensors in (("h", b.h), ("d", b.d)):
            out.update({"%s.%s[%s]" % (tag, side, k): t.data_ptr() for k, t in tensors.items()})
    return out


def same_results(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        for k in w:
            tc.assert_same_bits(g[k], w[k], "%s: %s" % (what, k))


def test_repeated_and_smaller_batches_keep_every_address(setup):
    clips, kw = setup["clips"], dict(vae=setup["vae"], ctr=77, samples=3, unfiltered=True)
    cl = tcs.lifter_for(setup["m"], setup["s"], 64)
    plain, res = cl.lift_clips(clips, **kw), cl.lift_clips(clips, resample=R, **kw)
    assert sorted(res[0]) == sorted(list(plain[0]) + ["spline_info"]) and "ref_var" in plain[0]
    first = addresses(cl)
    assert len(first) == 3 + 12 + 2 * (7 + 8) and all(first.values())
    same_results(cl.lift_clips(clips, **kw), plain, "the batch again")
    same_results(cl.lift_clips(clips, resample=R, **kw), res, "the resampled batch again")
    assert addresses(cl) == first
    # a shorter batch: its one clip is the first clip of the longer one, rows and noise keys included
    same_results(cl.lift_clips(clips[:1], **kw), plain[:1], "a shorter batch")
    same_results(cl.lift_clips(clips[:1], resample=R, **kw), res[:1], "a shorter resampled batch")
    assert addresses(cl) == first
    setup["m"].check_errors()


def refusal(call, *a, **kw):
    with pytest.raises(ValueError) as e:
        call(*a, **kw)
    print("%s %s -> %s" % (call.__name__, sorted(kw), e.value))
    return str(e.value)


def test_the_two_device_calls_refuse_in_the_same_words(setup):
    vae, clips = setup["vae"], setup["clips"]
    cl = tcs.lifter_for(setup["m"], setup["s"], 64)
    calls = ((cl.lift_clips_device, (), N), (cl.lift_clips_resampled_device, (R,), R * N))
    for call, a, rows in calls:
        assert refusal(call, *a) == "set_offsets first"
    assert refusal(cl.lift_clips_resampled_device, 0) == "set_offsets first"     # (before the look at resample)
    cl.set_offsets(np.array([0, 9, N]))
    need = "samples, eps and unfiltered need a filter (vae=...)"
    resample = "resample must be a whole number in 1..16 (the reference's multiplier 1 / resample)"
    for call, a, rows in calls:
        assert refusal(call, *a, samples=3) == need
        assert refusal(call, *a, unfiltered=True) == need
        want = "eps: expected a contiguous float32 device tensor (3, %d, 24)" % rows
        for eps in (torch.zeros((3, rows + 1, 24), device="cuda"), torch.zeros((rows, 24), device="cuda"),
                    torch.zeros((3, rows, 24), dtype=torch.float64, device="cuda"), torch.zeros((3, rows, 24))):
            assert refusal(call, *a, vae=vae, samples=3, eps=eps) == want
        assert refusal(call, *a, vae=vae, eps=torch.zeros((3, rows, 24), device="cuda")) == \
            "eps: expected a contiguous float32 device tensor (%d, 24)" % rows
    for bad in (0, 17, 2.5):
        assert refusal(cl.lift_clips_resampled_device, bad) == resample
        assert refusal(cl.lift_clips_resampled_device, bad, samples=3) == resample   # (before the filter arguments)
        assert refusal(cl.lift_clips, clips, resample=bad) == resample
