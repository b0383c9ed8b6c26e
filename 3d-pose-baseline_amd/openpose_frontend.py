"""Per-frame lifting of the OpenPose front end, on the GPU.

src/openpose_3dpose_sandbox.py:317-356 lifts one frame at a time: map the OpenPose joints into
the 64-wide H3.6M 2D vector (``order`` of :25 plus the derived Hip / Neck-Nose / Thorax,
:336-342), normalise it with the 2D training statistics (:347-350), ``model.step`` at batch 1
(:353) and ``unNormalizeData`` of the 3D output (:356).

``FrameLifter`` runs everything after the joint mapping as ONE HIP graph per call: pinned H2D
of the mapped frame(s) -> ``p3d_lift`` (normalise, the float32 placeholder cast, the forward,
unNormalizeData: one persistent launch at batch <= 4, else ``p3d_normalize`` + the layer kernels +
``p3d_unnormalize``, the same bits) -> pinned D2H of the [B, 96] millimetre pose(s).  The mapping is
a host-side index shuffle of the OpenPose JSON values (as in the reference).

``ClipLifter`` lifts a whole clip -- the sandbox's own workflow (:39-227, 317-433) -- in one
``p3d_clip_lift``: the median smoothing and the hold of dropped joints, the mapping, the forward
in tiles of ``max_batch`` rows, the axis swap / flip / spine offset and ``--cache_on_fail``, from
pinned rows in to pinned rows out.  ``read_openpose_json`` parses the frame files and
``export_maya`` writes ``3d_data.json`` / ``2d_data.json``.  The plots and ``--write_gif`` stay out
of scope; ``--interpolation``'s spline resampling is ``lift_clips(resample=R)``.

``ClipLifter.lift_clips`` lifts a BATCH of clips in one ``p3d_clips_lift`` (every clip the bits of
``lift_clip`` on it alone), optionally with the temporal VAE filter (``models.VAE``, the filter
``3d_pose_vae_filter_kin.py`` trains) between the forward and the post-processing: the filter is
a serial chain per clip and runs 16 clips per workgroup, so it pays over many clips at once.
``read_clips`` / ``check_clips`` / ``export_maya_clips`` are the directory-of-clips forms of the
reader, the check and the export.

``LiveLifter`` lifts LIVE streams frame by frame (src/openpose_3dpose_sandbox_realtime.py; DESIGN.md
8d): S slots with carried state on the device, one ``p3d_live_push`` per tick, and for every stream
the rows of its lifetime are those of the clip path on the stream's whole frame list -- at a fixed
delay of four frames with smoothing (the median looks ahead), none without.
"""
from __future__ import annotations

import ctypes
import json
import os
import re

import numpy as np

import data_pipeline as dp

ORDER = [15, 12, 25, 26, 27, 17, 18, 19, 1, 2, 3, 6, 7, 8]   # src/openpose_3dpose_sandbox.py:25
# the per-joint copies of the mapping as one gather: H3.6M columns 2h, 2h+1 <- OpenPose 2i, 2i+1
_SRC = np.array([2 * i + k for i in range(len(ORDER)) for k in (0, 1)])
_DST = np.array([2 * h + k for h in ORDER for k in (0, 1)])


def map_frames(frames_xy):
    """OpenPose frames [N, >= 28] (x/y interleaved) -> H3.6M 2D vectors [N, 64] float64."""
    xy = np.asarray(frames_xy, np.float64)
    if xy.ndim == 1:
        xy = xy[None, :]
    if xy.ndim != 2 or xy.shape[1] < 2 * len(ORDER):
        raise ValueError("expected OpenPose frames [N, >= %d], got %s" % (2 * len(ORDER), xy.shape))
    e = np.zeros((xy.shape[0], 64))
    e[:, _DST] = xy[:, _SRC]
    e[:, 0:2] = (e[:, 2:4] + e[:, 12:14]) / 2            # Hip = mean(RHip, LHip)
    e[:, 28:30] = (e[:, 30:32] + e[:, 24:26]) / 2        # Neck/Nose = mean(Head, Spine)
    e[:, 26:28] = 2 * e[:, 24:26] - e[:, 28:30]          # Thorax = 2 Spine - Neck/Nose
    return e


def lift(model, raw, mean2, std2, use2, mean3, std3, use3, out):
    """Device rows raw [B, 64] float64 (mapped frames) -> out [B, D3] float64 millimetres:
    normalize_data, the float32 cast, the eval forward, unNormalizeData (p3d_lift).  mean/std:
    device float64; use2/use3: device int32 dimension sets (data_pipeline._dims)."""
    import _p3d
    p = lambda t: t.data_ptr()   # noqa: E731
    _p3d.check(_p3d.lib().p3d_lift(model._h, p(raw), raw.shape[0], raw.shape[1], p(mean2), p(std2), p(use2),
                                   use2.numel(), p(mean3), p(std3), p(use3), use3.numel(), out.shape[1], p(out),
                                   model.stream()), "p3d_lift")
    return out


def lift_layout(head, rows, U2, U3, with_filter=False):
    """Byte offsets (x, y, ref, total) of a lift call's workspace: behind the path's `head` bytes
    x [rows, U2] | y [rows, U3] | with a filter ref [rows, U3], float32, each 256-aligned -- the
    mirror of LiftLayout (csrc/p3d_clip_host.h)."""
    a256 = lambda b: (b + 255) // 256 * 256   # noqa: E731
    y = head + a256(rows * U2 * 4)
    ref = y + a256(rows * U3 * 4)
    return head, y, ref, ref + (a256(rows * U3 * 4) if with_filter else 0)


def _aligned_workspace(torch, nbytes, dev):
    """`nbytes` device bytes -> (the tensor that owns them, their 256-byte aligned address)."""
    t = torch.empty((nbytes + 256,), dtype=torch.uint8, device=dev)
    return t, (t.data_ptr() + 255) // 256 * 256


def _check_filter(vae, samples, out_size, who):
    """A lifter's filter arguments: a sequence filter (ValueError: bones, wide, not a sequence
    filter) of the lifter's width -> K, the number of draws (0: one draw, no variance)."""
    vae._seq_len()
    if vae.human_3d_size != out_size:
        raise ValueError("the filter refines %d values per frame, the lifter predicts %d" % (vae.human_3d_size, out_size))
    return 0 if samples is None else vae._samples(samples, who)


class _Lifter:
    """What the three lifters share: the statistics on the device and the result dicts."""

    def _load_stats(self, who, model, data_mean_2d, data_std_2d, dim_to_use_2d, data_mean_3d, data_std_3d,
                    dim_to_ignore_3d, wide=True, upload=True):
        """Check the statistics against the model (wide: and for the 64 / 96 columns of the clip
        kernels) and upload them (upload=False: the checks alone): m2 s2 m3 s3 (float64), u2 u3 (int32
        dimension sets).  Returns D3."""
        D3 = int(np.asarray(data_mean_3d).shape[0])
        use3 = np.setdiff1d(np.arange(D3), np.asarray(dim_to_ignore_3d, np.int64))
        if wide and (D3 != 96 or np.asarray(data_mean_2d).shape[0] != 64):
            raise ValueError("%s: needs the 64-wide 2D and 96-wide 3D statistics" % who)
        if len(use3) != model.output_size or len(dim_to_use_2d) != model.input_size:
            raise ValueError("statistics do not match the model's %d inputs / %d outputs"
                             % (model.input_size, model.output_size))
        if not upload:
            return D3
        with self.torch.cuda.device(model.device):
            self.m2, self.s2 = dp.as_device(data_mean_2d), dp.as_device(data_std_2d)
            self.m3, self.s3 = dp.as_device(data_mean_3d), dp.as_device(data_std_3d)
            self.u2 = dp._dims(dim_to_use_2d, 64, who)
            self.u3 = dp._dims(use3, D3, who)
        return D3

    @staticmethod
    def _results(off, views):
        """Result rows -> one dict of copies per row range [off[i], off[i + 1]) (None: an empty
        range).  views: [(key, rows as a numpy array, e.g. a pinned tensor's view)]."""
        return [{k: v[a:b].copy() for k, v in views} if b > a else None for a, b in zip(off[:-1], off[1:])]


class FrameLifter(_Lifter):
    """Lift mapped OpenPose frames to 3D (mm) with a LinearModel: one p3d_lift launch per call on
    pinned host rows (fp32 models; bf16 models: one HIP graph of the three calls per call)."""

    def __init__(self, model, data_mean_2d, data_std_2d, dim_to_use_2d, data_mean_3d, data_std_3d,
                 dim_to_ignore_3d, batch=1):
        import torch
        self.torch, self.model, self.B = torch, model, int(batch)
        if self.B < 1 or self.B > model.max_batch:
            raise ValueError("batch must be in [1, max_batch=%d]" % model.max_batch)
        dev = model.device
        D3 = self._load_stats("FrameLifter", model, data_mean_2d, data_std_2d, dim_to_use_2d, data_mean_3d, data_std_3d,
                              dim_to_ignore_3d, wide=False)
        with torch.cuda.device(dev):
            f32, f64 = torch.float32, torch.float64
            self.hin = torch.empty((self.B, 64), dtype=f64, pin_memory=True)
            self.hout = torch.empty((self.B, D3), dtype=f64, pin_memory=True)
            self.din = torch.empty((self.B, 64), dtype=f64, device=dev)
            self.x = torch.empty((self.B, model.input_size), dtype=f32, device=dev)
            self.y = torch.empty((self.B, model.output_size), dtype=f32, device=dev)
            self.p3 = torch.empty((self.B, D3), dtype=f64, device=dev)
            self.hin.zero_()
            self.graph, self._launch, self._host_wait = None, None, False
            if not model.bf16 and os.environ.get("P3D_LIFT_EAGER", "1") != "0":
                # fp32 (round 6): ONE p3d_lift launch per call that reads the pinned frame rows and
                # writes the pinned millimetre rows itself (mapped host memory), its ctypes
                # arguments bound once -- a graph replay costs more than the launch it would save
                import ctypes
                import _p3d
                c = ctypes.c_void_p
                args = (model._h, c(self.hin.data_ptr()), self.B, 64, c(self.m2.data_ptr()), c(self.s2.data_ptr()),
                        c(self.u2.data_ptr()), self.u2.numel(), c(self.m3.data_ptr()), c(self.s3.data_ptr()),
                        c(self.u3.data_ptr()), self.u3.numel(), D3, c(self.hout.data_ptr()))
                # p3d_lift_sync returns once the rows are in hout (the launch's output workgroups
                # store a completion word the host waits on); env P3D_HOST_WAIT=0: p3d_lift + a
                # stream synchronize
                self._host_wait = os.environ.get("P3D_HOST_WAIT", "1") != "0"
                fn, sh = (_p3d.lib().p3d_lift_sync if self._host_wait else _p3d.lib().p3d_lift), _p3d.stream_handle
                self._launch = lambda: fn(*args, c(sh()))   # noqa: E731
                _p3d.check(self._launch(), "p3d_lift")
                torch.cuda.current_stream(dev).synchronize()
            else:
                side = torch.cuda.Stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    self._body()                           # eager warm-up (no side effects)
                torch.cuda.current_stream(dev).wait_stream(side)
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph, stream=side):
                    self._body()
        self.hin_np, self.hout_np = self.hin.numpy(), self.hout.numpy()

    def _body(self):
        self.din.copy_(self.hin, non_blocking=True)
        if self.model.bf16:
            # p3d_lift is float32-only: the three calls it folds (the same arithmetic)
            dp.normalize(self.din, self.m2, self.s2, self.u2, out_dtype=self.torch.float32, out=self.x)
            self.model.forward_device(self.x, False, 1.0, out=self.y, ctr=0)
            dp.unnormalize(self.y, self.m3, self.s3, self.u3, self.p3.shape[1], out=self.p3)
        else:
            lift(self.model, self.din, self.m2, self.s2, self.u2, self.m3, self.s3, self.u3, out=self.p3)
        self.hout.copy_(self.p3, non_blocking=True)

    def lift_mapped(self, enc_in64):
        """Mapped H3.6M 2D vectors [n <= batch, 64] -> 3D poses [n, 96] (mm, float64)."""
        e = np.asarray(enc_in64, np.float64)
        n = e.shape[0]
        if e.ndim != 2 or e.shape[1] != 64 or not 1 <= n <= self.B:
            raise ValueError("expected [1..%d, 64] mapped frames, got %s" % (self.B, e.shape))
        self.hin_np[:n] = e
        if n < self.B:
            self.hin_np[n:] = 0.0
        if self._launch is not None:
            rc = self._launch()
            if rc:
                import _p3d
                self.model.check_errors()         # (raises with the kernels' own report, if any)
                _p3d.check(rc, "p3d_lift")
            if not self._host_wait:
                self.torch.cuda.current_stream(self.model.device).synchronize()
        else:
            self.graph.replay()
            self.torch.cuda.current_stream(self.model.device).synchronize()
        return self.hout_np[:n].copy()

    def lift(self, frames_xy):
        """OpenPose frames [N, >= 28] -> 3D poses [N, 96] (mm), in calls of `batch` frames."""
        e = map_frames(frames_xy)
        if e.shape[0] <= self.B:          # (the sandbox's per-frame call: one batch)
            return self.lift_mapped(e)
        return np.concatenate([self.lift_mapped(e[i:i + self.B]) for i in range(0, e.shape[0], self.B)])


# --------------------------------------------------------------------------------------
# a whole clip: src/openpose_3dpose_sandbox.py:39-227 (reading, smoothing), :317-433 (lifting, export)
# --------------------------------------------------------------------------------------


def parse_keypoints(data):
    """One person's OpenPose keypoint list -> the 36 COCO-18 x/y values (:58-124): lists of >= 53
    values carry confidences (x, y of every triple kept); more than 54 values is body_25, whose
    joints 0-7 and 9-18 are the COCO ones; anything shorter is tf-pose-estimation's plain x/y."""
    n = len(data)
    xy = [data[o + k] for o in range(0, n - 1, 3) for k in (0, 1)] if n >= 53 else list(data)
    if n > 54:
        xy = xy[0:16] + xy[18:38]
    return xy


def read_frame_file(path):
    """One frame file -> the 36 COCO-18 x/y values of its first person (key ``pose_keypoints_2d``
    or ``pose_keypoints``)."""
    with open(path) as f:
        person = json.load(f)["people"][0]
    xy = parse_keypoints(person["pose_keypoints_2d"] if "pose_keypoints_2d" in person else person["pose_keypoints"])
    if len(xy) != 36:
        raise ValueError("%s: expected 18 joints (36 values), got %d values" % (os.path.basename(path), len(xy)))
    return xy


def read_openpose_json(directory):
    """The frame files of `directory` (*.json, sorted by name) -> (frame_numbers [N] int64,
    xy [N, 36] float64), first person of each file, key ``pose_keypoints_2d`` or
    ``pose_keypoints``; the frame number is the last run of digits of the file name (:46-127)."""
    names = sorted(f for f in os.listdir(directory) if f.endswith(".json"))
    if not names:
        raise ValueError("no .json frame files in %s" % directory)
    numbers, rows = [], []
    for name in names:
        digits = re.findall(r"(\d+)", name)
        if not digits:
            raise ValueError("no frame number in file name %s" % name)
        numbers.append(int(digits[-1]))
        rows.append(read_frame_file(os.path.join(directory, name)))
    return np.array(numbers, np.int64), np.array(rows, np.float64)


def check_clip(frame_numbers, smooth=True):
    """The conditions under which the reference's smoothing runs (:140-173): one frame, or at
    least 9 with contiguous numbers (it indexes frame +- k and raises KeyError on a gap)."""
    fn = np.asarray(frame_numbers, np.int64)
    if not smooth or fn.shape[0] == 1:
        return
    if fn.shape[0] <= 8:
        raise ValueError("need more frames, min 9 frames/json files for smoothing")
    if np.any(np.diff(fn) != 1):
        raise ValueError("frame numbers must be contiguous for smoothing (a gap after frame %d)"
                         % fn[:-1][np.diff(fn) != 1][0])


def export_maya(out_dir, frame_numbers, poses, xy_s):
    """Write ``3d_data.json`` ({frame: {joint: {"translate": [x, y, z]}}}, 32 joints) and
    ``2d_data.json`` (the 18 smoothed 2D joints, [x, y]) into `out_dir` (:326-328, 406-408, 426-433).
    Returns the two paths."""
    poses, xy_s = np.asarray(poses, np.float64), np.asarray(xy_s, np.float64)
    if poses.ndim != 2 or poses.shape[1] != 96 or xy_s.shape != (poses.shape[0], 36) or len(frame_numbers) != poses.shape[0]:
        raise ValueError("expected poses [N, 96], xy_s [N, 36] and N frame numbers")
    three, two = {}, {}
    for n, frame in enumerate(frame_numbers):
        p, q = poses[n].tolist(), xy_s[n].tolist()
        three[int(frame)] = {j: {"translate": p[3 * j:3 * j + 3]} for j in range(32)}
        two[int(frame)] = {j: {"translate": q[2 * j:2 * j + 2]} for j in range(18)}
    os.makedirs(out_dir, exist_ok=True)
    paths = os.path.join(out_dir, "3d_data.json"), os.path.join(out_dir, "2d_data.json")
    for path, units in zip(paths, (three, two)):
        with open(path, "w") as f:
            json.dump(units, f)
    return paths


def read_clips(root):
    """Every immediate subdirectory of `root` that holds frame files (*.json) is one clip, in sorted
    order, each read by read_openpose_json -> (names [S], frame_numbers: S arrays, clips: S arrays
    [n_s, 36]).  Subdirectories without frame files and plain files are ignored."""
    names, numbers, clips = [], [], []
    for name in sorted(os.listdir(root)):
        d = os.path.join(root, name)
        if not os.path.isdir(d) or not any(f.endswith(".json") for f in os.listdir(d)):
            continue
        fn, xy = read_openpose_json(d)
        names.append(name)
        numbers.append(fn)
        clips.append(xy)
    if not names:
        raise ValueError("no clip directories with .json frame files in %s" % root)
    return names, numbers, clips


def check_clips(frame_numbers, smooth=True, names=None):
    """check_clip on every clip; the error names the clip."""
    for s, fn in enumerate(frame_numbers):
        try:
            check_clip(fn, smooth)
        except ValueError as e:
            raise ValueError("clip %s: %s" % (names[s] if names is not None else s, e)) from None


def export_maya_clips(out_dir, names, frame_numbers, results, unfiltered=False):
    """export_maya of every clip of a lift_clips result into <out_dir>/<clip name>/; with
    unfiltered=True also ``3d_data_unfiltered.json`` (the lift without the filter) beside them.
    Returns one tuple of paths per clip."""
    if not len(names) == len(frame_numbers) == len(results):
        raise ValueError("expected one name, one array of frame numbers and one result per clip")
    paths = []
    for name, fn, r in zip(names, frame_numbers, results):
        d = os.path.join(out_dir, name)
        p = export_maya(d, fn, r["poses"], r["xy_s"])
        if unfiltered:
            p += (export_unfiltered(d, fn, r["poses_unfiltered"]),)
        paths.append(p)
    return paths


def export_unfiltered(out_dir, frame_numbers, poses):
    """``3d_data_unfiltered.json``: the layout of ``3d_data.json`` for the poses before the filter."""
    poses = np.asarray(poses, np.float64)
    if poses.ndim != 2 or poses.shape[1] != 96 or len(frame_numbers) != poses.shape[0]:
        raise ValueError("expected poses [N, 96] and N frame numbers")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "3d_data_unfiltered.json")
    with open(path, "w") as f:
        json.dump({int(frame): {j: {"translate": poses[n, 3 * j:3 * j + 3].tolist()} for j in range(32)}
                   for n, frame in enumerate(frame_numbers)}, f)
    return path


# --------------------------------------------------------------------------------------
# lifted rows as a rigid skeleton: bone lengths, rotations, BVH
# --------------------------------------------------------------------------------------

SKEL_H36M = (0, 1, 2, 3, 6, 7, 8, 12, 13, 14, 15, 17, 18, 19, 25, 26, 27)   # the skeleton's joints among the 32


def skel_tables():
    """(names [17], ja [16], jb [16], pb [16], rest [16, 3]) of the skeleton: the bones filter's bone
    table, every bone's parent bone (-1: it leaves the hip) and its unit rest direction, keyed by
    the child joint -- right hip / arm bones along -X, left ones along +X, knees and feet along -Y,
    spine to head along +Y."""
    import data_utils
    from top_vae_3d_pose.bones import BJA, BJB
    names = [data_utils.H36M_NAMES[j].replace("/", "") for j in SKEL_H36M]
    pb = [BJB.index(a) if a else -1 for a in BJA]
    rest = np.zeros((16, 3))
    for b, j in enumerate(BJB):
        n = names[j]
        if n.endswith(("Knee", "Foot")):
            rest[b, 1] = -1.0
        elif n[0] in "RL":
            rest[b, 0] = -1.0 if n[0] == "R" else 1.0
        else:
            rest[b, 1] = 1.0
    return names, list(BJA), list(BJB), pb, rest


class _SkeletonBuffers:
    """The device and pinned rows of p3d_skel_lengths / p3d_skel_pose, grown on demand (a captured
    graph holds the addresses: size them with one eager call before capturing)."""

    OUT = (("quat", (16, 4)), ("euler", (16, 3)), ("rigid", (17, 3)), ("root", (3,)))

    def __init__(self, torch, device):
        self.torch, self.device = torch, device
        self.rows, self.clips, self.work_bytes = 0, 0, 0

    def _grow(self, N, S):
        import _p3d
        torch, dev = self.torch, self.device
        with torch.cuda.device(dev):
            if N > self.rows:
                self.d = {k: torch.empty((N,) + shp, dtype=torch.float64, device=dev) for k, shp in self.OUT}
                self.h = {k: torch.empty((N,) + shp, dtype=torch.float64, pin_memory=True) for k, shp in self.OUT}
                self.rows = N
            if S > self.clips:
                self.hoff = torch.empty((S + 1,), dtype=torch.int64, pin_memory=True)
                self.doff = torch.empty((S + 1,), dtype=torch.int64, device=dev)
                self.dlen, self.dmean = (torch.empty((S, 16), dtype=torch.float64, device=dev) for _ in range(2))
                self.hlen = torch.empty((S, 16), dtype=torch.float64, pin_memory=True)
                self.dused = torch.empty((S,), dtype=torch.int64, device=dev)
                self.hused = torch.empty((S,), dtype=torch.int64, pin_memory=True)
                self.clips = S
            need = int(_p3d.lib().p3d_skel_workspace(N, S))
            if need > self.work_bytes:
                self.work, self.work_ptr = _aligned_workspace(torch, need, dev)
                self.work_bytes = need

    def run(self, dposes, dsrc, off, lengths=None):
        """The two calls on device rows dposes [>= N, 96] / dsrc [>= N] int32 or None under the clip
        offsets `off` (int64 [S + 1]) -> one dict per clip."""
        import _p3d
        torch, lib, p = self.torch, _p3d.lib(), _p3d.ptr
        off = np.ascontiguousarray(off, np.int64)
        S, N = off.shape[0] - 1, int(off[-1])
        if lengths is not None:
            lengths = np.asarray(lengths, np.float64)
            if lengths.shape == (16,):
                lengths = np.tile(lengths, (S, 1))
            if lengths.shape != (S, 16) or not (lengths >= 0).all():
                raise ValueError("lengths: expected [16] or [%d, 16] bone lengths >= 0, got %s" % (S, lengths.shape))
        self._grow(N, S)
        with torch.cuda.device(self.device):
            st = _p3d.stream_handle()
            self.hoff.numpy()[:S + 1] = off
            self.doff[:S + 1].copy_(self.hoff[:S + 1], non_blocking=True)
            _p3d.check(lib.p3d_skel_lengths(p(dposes), p(dsrc), off.ctypes.data, p(self.doff), S, N, p(self.dmean),
                                            p(self.dused), self.work_ptr, self.work_bytes, st), "p3d_skel_lengths")
            dlen = self.dmean
            if lengths is not None:
                self.hlen.numpy()[:S] = lengths
                self.dlen[:S].copy_(self.hlen[:S], non_blocking=True)
                dlen = self.dlen
            _p3d.check(lib.p3d_skel_pose(p(dposes), p(dsrc), off.ctypes.data, p(self.doff), S, N, p(dlen),
                                         *(p(self.d[k]) for k, _ in self.OUT), st), "p3d_skel_pose")
            for k, _ in self.OUT:
                self.h[k][:N].copy_(self.d[k][:N], non_blocking=True)
            self.hused[:S].copy_(self.dused[:S], non_blocking=True)
            if lengths is None:
                self.hlen[:S].copy_(self.dmean[:S], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        out = _Lifter._results(off.tolist(), [(k, self.h[k].numpy()) for k, _ in self.OUT])
        for s, r in enumerate(out):
            r["lengths"], r["n_used"] = self.hlen.numpy()[s].copy(), int(self.hused[s])
        return out


def skeleton_rows(poses, src, offsets, lengths=None, device=None):
    """The rigid skeleton of host rows: poses [N, 96] float64 as the lifters return them (or as read
    back from ``3d_data.json``), S clips one after another under `offsets` [S + 1]; src [N]: each
    clip's 'src' as the lifters return it (positions inside the clip, -1: zeros), concatenated, or
    None (every row carries its own pose).  lengths: [16] or [S, 16] bone lengths to use instead of
    the clips' own means (a known actor; a live stream's earlier estimate).  Returns one dict per
    clip: 'lengths' [16] (the ones used), 'n_used' (the frames the clip's own mean is over), 'quat'
    [n, 16, 4] (w, x, y, z), 'euler' [n, 16, 3] (Z, X, Y degrees), 'rigid' [n, 17, 3], 'root' [n, 3],
    in skeleton coordinates (X, Y, Z) = (x, z, -y).  device: a torch device (default: the current one)."""
    import torch
    poses = np.ascontiguousarray(poses, np.float64)
    off = np.asarray(offsets)
    if poses.ndim != 2 or poses.shape[1] != 96 or poses.shape[0] < 1:
        raise ValueError("expected poses [N >= 1, 96] (32 joints), got %s" % (poses.shape,))
    if off.ndim != 1 or off.shape[0] < 2 or not np.issubdtype(off.dtype, np.integer) or off[0] != 0 \
            or (np.diff(off) <= 0).any() or off[-1] != poses.shape[0]:
        raise ValueError("clip offsets must be integers [S + 1] that start at 0, give every clip a frame and end at N")
    off = off.astype(np.int64)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        dposes, dsrc = torch.from_numpy(poses).to(dev), None
        if src is not None:
            src = np.asarray(src)
            if src.shape != (poses.shape[0],) or not np.issubdtype(src.dtype, np.integer):
                raise ValueError("src: expected %d integers, got %s %s" % (poses.shape[0], src.dtype, src.shape))
            first = np.repeat(off[:-1], np.diff(off))
            dsrc = torch.from_numpy(np.where(src >= 0, src + first, -1).astype(np.int32)).to(dev)
        return _SkeletonBuffers(torch, dev).run(dposes, dsrc, off, lengths)


def export_bvh(path, frame_numbers, lengths, euler, root, fps=30.0):
    """Write one clip as a BVH file: ``ROOT Hips`` (six channels, its rotation always zero) and one
    ``JOINT bone_<child joint>`` per bone, placed at the bone's START (OFFSET 0 for the three hip
    bones, else the parent bone's length times its rest direction) with channels ``Zrotation
    Xrotation Yrotation``; every leaf ends in an ``End Site`` at its own length times its rest
    direction.  lengths [16], euler [N, 16, 3] (Z, X, Y degrees) and root [N, 3] as skeleton_rows /
    ClipLifter.skeleton return them; one motion line per frame, values printed with repr.  Lengths
    that are all zero (a clip with n_used == 0) and non-finite values raise ValueError.  Returns path."""
    lengths, euler, root = np.asarray(lengths, np.float64), np.asarray(euler, np.float64), np.asarray(root, np.float64)
    n = len(frame_numbers)
    if lengths.shape != (16,) or euler.shape != (n, 16, 3) or root.shape != (n, 3) or n < 1:
        raise ValueError("%s: expected lengths [16], euler [N, 16, 3], root [N, 3] and N >= 1 frame numbers" % path)
    if not lengths.any():
        raise ValueError("%s: the clip has no frame to take bone lengths from (n_used == 0)" % path)
    if not (np.isfinite(lengths).all() and np.isfinite(euler).all() and np.isfinite(root).all()):
        raise ValueError("%s: non-finite lengths, angles or root positions" % path)
    if not fps > 0:
        raise ValueError("%s: fps must be > 0" % path)
    names, _, jb, pb, rest = skel_tables()
    vec = lambda v: " ".join(repr(float(x)) for x in v)   # noqa: E731
    lines, order = ["HIERARCHY", "ROOT Hips", "{", "  OFFSET 0.0 0.0 0.0",
                    "  CHANNELS 6 Xposition Yposition Zposition Zrotation Xrotation Yrotation"], []

    def joint(b, depth):
        pad = "  " * depth
        order.append(b)
        lines.extend([pad + "JOINT bone_" + names[jb[b]], pad + "{",
                      pad + "  OFFSET " + vec(lengths[pb[b]] * rest[pb[b]] if pb[b] >= 0 else np.zeros(3)),
                      pad + "  CHANNELS 3 Zrotation Xrotation Yrotation"])
        kids = [c for c in range(16) if pb[c] == b]
        for c in kids:
            joint(c, depth + 1)
        if not kids:
            lines.extend([pad + "  End Site", pad + "  {", pad + "    OFFSET " + vec(lengths[b] * rest[b]), pad + "  }"])
        lines.append(pad + "}")

    for b in range(16):
        if pb[b] < 0:
            joint(b, 1)
    lines.extend(["}", "MOTION", "Frames: %d" % n, "Frame Time: " + repr(1.0 / float(fps))])
    for f in range(n):
        lines.append(vec(root[f]) + " 0.0 0.0 0.0 " + vec(euler[f, order].reshape(-1)))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return path


def export_bvh_clips(out_dir, names, frame_numbers, skeletons, fps=30.0):
    """export_bvh of every clip of a ClipLifter.skeleton / skeleton_rows result into
    <out_dir>/<clip name>/skeleton.bvh, beside export_maya_clips' files.  Returns the paths."""
    if not len(names) == len(frame_numbers) == len(skeletons):
        raise ValueError("expected one name, one array of frame numbers and one skeleton per clip")
    return [export_bvh(os.path.join(out_dir, name, "skeleton.bvh"), fn, sk["lengths"], sk["euler"], sk["root"], fps)
            for name, fn, sk in zip(names, frame_numbers, skeletons)]


# --------------------------------------------------------------------------------------
# the root trajectory of lifted rows: the pinhole solve per frame, its windowed mean
# --------------------------------------------------------------------------------------

TRAJ_MAX_HALF = 32


def _check_camera(focal, center, smooth_half):
    """(focal, cx, cy, h) as the library takes them; ValueError for what it would refuse."""
    try:
        f = float(focal)
        cx, cy = (float(c) for c in center)
    except (TypeError, ValueError):
        raise ValueError("expected a focal length and a principal point (cx, cy) in pixels") from None
    if not (np.isfinite(f) and f > 0):
        raise ValueError("focal must be finite and > 0, got %r" % (focal,))
    if not (np.isfinite(cx) and np.isfinite(cy)):
        raise ValueError("the principal point must be finite, got %r" % (center,))
    h = int(smooth_half)
    if h != smooth_half or not 0 <= h <= TRAJ_MAX_HALF:
        raise ValueError("smooth_half must be a whole number in 0..%d" % TRAJ_MAX_HALF)
    return f, cx, cy, h


class _TrajectoryBuffers:
    """The device and pinned rows of p3d_root_trajectory, grown on demand (a captured graph holds the
    addresses: size them with one eager call before capturing)."""

    OUT = (("traj", (3,), "float64"), ("traj_raw", (3,), "float64"), ("resid", (), "float64"), ("valid", (), "int32"))

    def __init__(self, torch, device):
        self.torch, self.device = torch, device
        self.rows, self.clips, self.work_bytes, self.work_ptr = 0, 0, 0, None

    def _grow(self, N, S, h):
        import _p3d
        torch, dev = self.torch, self.device
        with torch.cuda.device(dev):
            if N > self.rows:
                self.d = {k: torch.empty((N,) + shp, dtype=getattr(torch, dt), device=dev) for k, shp, dt in self.OUT}
                self.h = {k: torch.empty((N,) + shp, dtype=getattr(torch, dt), pin_memory=True) for k, shp, dt in self.OUT}
                self.rows = N
            if S > self.clips:
                self.hoff = torch.empty((S + 1,), dtype=torch.int64, pin_memory=True)
                self.doff = torch.empty((S + 1,), dtype=torch.int64, device=dev)
                self.clips = S
            need = int(_p3d.lib().p3d_root_trajectory_workspace(N, h))
            if need > self.work_bytes:
                self.work, self.work_ptr = _aligned_workspace(torch, need, dev)
                self.work_bytes = need

    def run(self, dposes, dxy, dsrc, off, focal, center, smooth_half):
        """The call on device rows dposes [>= N, 96] / dxy [>= N, 36] / dsrc [>= N] int32 or None under
        the clip offsets `off` (int64 [S + 1]) -> one dict per clip."""
        import _p3d
        f, cx, cy, h = _check_camera(focal, center, smooth_half)
        torch, lib, p = self.torch, _p3d.lib(), _p3d.ptr
        off = np.ascontiguousarray(off, np.int64)
        S, N = off.shape[0] - 1, int(off[-1])
        self._grow(N, S, h)
        with torch.cuda.device(self.device):
            self.hoff.numpy()[:S + 1] = off
            self.doff[:S + 1].copy_(self.hoff[:S + 1], non_blocking=True)
            _p3d.check(lib.p3d_root_trajectory(p(dposes), p(dxy), p(dsrc), off.ctypes.data, p(self.doff), S, N, f, cx, cy,
                                               h, *(p(self.d[k]) for k, _, _ in self.OUT), self.work_ptr, self.work_bytes,
                                               _p3d.stream_handle()), "p3d_root_trajectory")
            for k, _, _ in self.OUT:
                self.h[k][:N].copy_(self.d[k][:N], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        out = _Lifter._results(off.tolist(), [(k, self.h[k].numpy()) for k, _, _ in self.OUT])
        for r in out:
            r["valid"] = r["valid"] != 0
            # skeleton coordinates (X, Y, Z) = (ex, ez, -ey) with ex = camera x, ey = camera z, ez = -camera y
            r["root_skel"] = r["traj"] * np.array([1.0, -1.0, -1.0]) + 0.0   # (no -0.0 in a BVH)
            r["camera"] = dict(focal=f, center=[cx, cy], smooth_half=h)
        return out


def trajectory_rows(poses, xy_s, src, offsets, focal, center, smooth_half=0, device=None):
    """The root trajectory of host rows: poses [N, 96] and xy_s [N, 36] float64 as the lifters return
    them (a LiveLifter stream's collected rows, ``3d_data.json`` / ``2d_data.json`` read back), S clips
    one after another under `offsets` [S + 1]; src [N]: each clip's 'src' as the lifters return it
    (positions inside the clip, -1: zeros), concatenated, or None (every row its own).  focal and
    center = (cx, cy) are the camera's, in the pixels of xy_s; smooth_half = h in 0..32 averages the
    valid rows at most h frames away inside the clip.  Returns one dict per clip: 'traj' [n, 3] and
    'traj_raw' [n, 3] (Tx, Ty, Tz in the camera's frame: x right, y down, z forward, the 3D
    statistics' unit), 'resid' [n] (the reprojection residual, pixels), 'valid' [n] bool, 'root_skel'
    [n, 3] = (Tx, -Ty, -Tz), the trajectory in the skeleton's coordinates (export_bvh's `root`), and
    'camera'.  The solve takes the 3D rows to be in the camera's frame (a model trained with
    --camera_frame) and the camera to be the video's; it cannot check either."""
    import torch
    poses = np.ascontiguousarray(poses, np.float64)
    xy_s = np.ascontiguousarray(xy_s, np.float64)
    off = np.asarray(offsets)
    if poses.ndim != 2 or poses.shape[1] != 96 or poses.shape[0] < 1:
        raise ValueError("expected poses [N >= 1, 96] (32 joints), got %s" % (poses.shape,))
    if xy_s.shape != (poses.shape[0], 36):
        raise ValueError("expected xy_s [%d, 36] (18 joints), got %s" % (poses.shape[0], xy_s.shape))
    if off.ndim != 1 or off.shape[0] < 2 or not np.issubdtype(off.dtype, np.integer) or off[0] != 0 \
            or (np.diff(off) <= 0).any() or off[-1] != poses.shape[0]:
        raise ValueError("clip offsets must be integers [S + 1] that start at 0, give every clip a frame and end at N")
    off = off.astype(np.int64)
    _check_camera(focal, center, smooth_half)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        dsrc = None
        if src is not None:
            src = np.asarray(src)
            if src.shape != (poses.shape[0],) or not np.issubdtype(src.dtype, np.integer):
                raise ValueError("src: expected %d integers, got %s %s" % (poses.shape[0], src.dtype, src.shape))
            if (src >= np.repeat(np.diff(off), np.diff(off))).any():
                raise ValueError("src: a position past its clip's end")
            first = np.repeat(off[:-1], np.diff(off))
            dsrc = torch.from_numpy(np.where(src >= 0, src + first, -1).astype(np.int32)).to(dev)
        return _TrajectoryBuffers(torch, dev).run(torch.from_numpy(poses).to(dev), torch.from_numpy(xy_s).to(dev), dsrc,
                                                  off, focal, center, smooth_half)


def export_trajectory(out_dir, frame_numbers, result):
    """Write ``trajectory.json`` into `out_dir` from one clip's trajectory_rows / ClipLifter.trajectory
    dict: {"trajectory": {frame: [Tx, Ty, Tz]}, "resid": [...], "valid": [...], "camera": {focal,
    center, smooth_half}}.  Returns the path."""
    traj, resid, valid = np.asarray(result["traj"], np.float64), np.asarray(result["resid"], np.float64), np.asarray(result["valid"])
    n = len(frame_numbers)
    if traj.shape != (n, 3) or resid.shape != (n,) or valid.shape != (n,) or n < 1:
        raise ValueError("expected traj [N, 3], resid [N], valid [N] and N >= 1 frame numbers")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "trajectory.json")
    with open(path, "w") as f:
        json.dump({"trajectory": {int(frame): traj[i].tolist() for i, frame in enumerate(frame_numbers)},
                   "resid": resid.tolist(), "valid": [bool(v) for v in valid], "camera": result["camera"]}, f)
    return path


def _check_resample(resample):
    R = int(resample)
    if R != resample or not 1 <= R <= 16:
        raise ValueError("resample must be a whole number in 1..16 (the reference's multiplier 1 / resample)")
    return R


class _RowBuffers:
    """Pinned (h) and device (d) tensors in pairs under the keys xy out src out_u src_u var (one row per
    frame), info (one per clip) and off (the clip offsets), plus a 256-byte aligned workspace.  Each
    grows on demand and never shrinks: a call that needs no more than an earlier one reallocates
    nothing (a captured graph holds the addresses: size them with one eager call of the same kind
    before capturing)."""

    def __init__(self, torch, dev, out_size, h=None, d=None):
        self.torch, self.dev, self.h, self.d = torch, dev, dict(h or {}), dict(d or {})
        f64, i32 = torch.float64, torch.int32
        self.kinds = dict(xy=((36,), f64), out=((96,), f64), src=((), i32), out_u=((96,), f64), src_u=((), i32),
                          var=((out_size,), torch.float32), info=((36, 5), i32), off=((), torch.int64))
        self.work, self.work_ptr, self.work_bytes = None, 0, 0

    def need(self, keys, rows, work_bytes=0):
        torch = self.torch
        with torch.cuda.device(self.dev):
            for k in keys:
                if k not in self.d or self.d[k].shape[0] < rows:
                    shape, dt = (rows,) + self.kinds[k][0], self.kinds[k][1]
                    self.h[k] = torch.empty(shape, dtype=dt, pin_memory=True)
                    self.d[k] = torch.empty(shape, dtype=dt, device=self.dev)
            if work_bytes > self.work_bytes:
                self.work, self.work_ptr = _aligned_workspace(torch, work_bytes, self.dev)
                self.work_bytes = work_bytes


class ClipLifter(_Lifter):
    """Lift whole OpenPose clips of up to `max_frames` frames with a float32 LinearModel: pinned
    rows in, ONE p3d_clip_lift (smoothing, mapping, forward tiles, post-processing), pinned rows
    out."""

    def __init__(self, model, data_mean_2d, data_std_2d, dim_to_use_2d, data_mean_3d, data_std_3d,
                 dim_to_ignore_3d, max_frames, cache_on_fail=True):
        import torch
        import _p3d
        self.torch, self.model, self.max_frames = torch, model, int(max_frames)
        self.cache_on_fail = bool(cache_on_fail)
        if model.bf16:
            raise ValueError("ClipLifter: float32 models only")
        if not 1 <= self.max_frames <= 1 << 20:
            raise ValueError("max_frames must be in [1, 2^20]")
        self._load_stats("ClipLifter", model, data_mean_2d, data_std_2d, dim_to_use_2d, data_mean_3d, data_std_3d,
                         dim_to_ignore_3d)
        dev, n = model.device, self.max_frames
        with torch.cuda.device(dev):
            f64 = torch.float64
            self.hin = torch.empty((n, 36), dtype=f64, pin_memory=True)
            self.hxy = torch.empty((n, 36), dtype=f64, pin_memory=True)
            self.hout = torch.empty((n, 96), dtype=f64, pin_memory=True)
            self.hsrc = torch.empty((n,), dtype=torch.int32, pin_memory=True)
            self.din = torch.empty((n, 36), dtype=f64, device=dev)
            self.dxy = torch.empty((n, 36), dtype=f64, device=dev)
            self.dout = torch.empty((n, 96), dtype=f64, device=dev)
            self.dsrc = torch.empty((n,), dtype=torch.int32, device=dev)
            self.work_bytes = int(_p3d.lib().p3d_clip_lift_workspace(n, model.input_size, model.output_size))
            self.work, self.work_ptr = _aligned_workspace(torch, self.work_bytes, dev)
        # the batched calls' rows, offsets and workspaces: the rows as given (the single clip's rows among
        # them) and the resampled rows
        self.rows = _RowBuffers(torch, dev, model.output_size, dict(xy=self.hxy, out=self.hout, src=self.hsrc),
                                dict(xy=self.dxy, out=self.dout, src=self.dsrc))
        self.resampled = _RowBuffers(torch, dev, model.output_size)
        self._off, self._clips = None, None                  # the offsets of the last set_offsets; the last batched lift
        self._last_off, self._skel = None, None              # the last lift's clip offsets; skeleton()'s buffers
        self._last_rows = None                               # the last lift's device rows where not dout / dsrc (resampled)
        self._traj = None                                    # trajectory()'s buffers

    # the batched call's optional rows, offsets and workspace under the names they had as attributes
    dout_u = property(lambda self: self.rows.d.get("out_u"))
    dsrc_u = property(lambda self: self.rows.d.get("src_u"))
    dvar = property(lambda self: self.rows.d.get("var"))
    doff = property(lambda self: self.rows.d.get("off"))
    cwork_ptr = property(lambda self: self.rows.work_ptr)
    cwork_bytes = property(lambda self: self.rows.work_bytes)

    def lift_device(self, n, smooth=True):
        """p3d_clip_lift of the first n rows of self.din into self.dxy / dout / dsrc (current stream)."""
        import _p3d
        p = lambda t: t.data_ptr()   # noqa: E731
        _p3d.check(_p3d.lib().p3d_clip_lift(
            self.model._h, p(self.din), n, int(bool(smooth)), p(self.m2), p(self.s2), p(self.u2), self.u2.numel(),
            p(self.m3), p(self.s3), p(self.u3), self.u3.numel(), 96, int(self.cache_on_fail), p(self.dxy),
            p(self.dout), p(self.dsrc), self.work_ptr, self.work_bytes, self.model.stream()), "p3d_clip_lift")
        self._last_off, self._last_rows = np.array([0, n], np.int64), None

    def network_rows(self, n=None):
        """View of the network's normalised outputs [n, output_size] float32 that the last
        lift of n frames left in the workspace (behind the scan's summaries and the input rows);
        n=None: the rows of the last lift_clips / lift_clips_device, all clips one after another."""
        import _p3d
        if n is None:
            return self._clips_rows(0)
        off = lift_layout(int(_p3d.lib().p3d_clip_workspace(n)), n, self.model.input_size, self.model.output_size)[1]
        return _p3d.device_view(self.work_ptr + off, (n, self.model.output_size), self.model.device.index)

    # ------------------------------------------------------------------ a batch of clips
    def _clips_rows(self, area):
        """View of area 0 (the network's rows) or 1 (the filter's) of the batched workspace."""
        import _p3d
        if self._clips is None:
            raise ValueError("no batched lift has run yet")
        S, N, filtered = self._clips
        if area == 1 and not filtered:
            raise ValueError("the last batched lift ran without a filter")
        off = lift_layout(int(_p3d.lib().p3d_clips_workspace(N, S)), N, self.model.input_size, self.model.output_size,
                          filtered)[1 + area]
        return _p3d.device_view(self.rows.work_ptr + off, (N, self.model.output_size), self.model.device.index)

    def refined_rows(self):
        """View of the filter's refined rows [N, output_size] float32 of the last batched lift."""
        return self._clips_rows(1)

    def set_offsets(self, offsets):
        """Check the clip offsets [S + 1] (start at 0, no empty clip, end <= max_frames) and put them
        where lift_clips_device reads them: a host copy for the library's checks and grids, and the
        device copy the kernels read (uploaded on the current stream).  Returns (S, N)."""
        torch = self.torch
        off = np.asarray(offsets)
        if off.ndim != 1 or off.shape[0] < 2 or not np.issubdtype(off.dtype, np.integer):
            raise ValueError("clip offsets: expected an integer vector [S + 1], got %s %s" % (off.dtype, off.shape))
        off = off.astype(np.int64)
        if off[0] != 0 or (np.diff(off) <= 0).any() or off[-1] > self.max_frames:
            raise ValueError("clip offsets must start at 0, every clip must have a frame, and at most "
                             "max_frames = %d frames in all" % self.max_frames)
        S = off.shape[0] - 1
        self.rows.need(("off",), S + 1)
        self.rows.h["off"].numpy()[:S + 1] = off
        with torch.cuda.device(self.model.device):
            self.doff[:S + 1].copy_(self.rows.h["off"][:S + 1], non_blocking=True)
        self._off = off
        return S, int(off[-1])

    def _batch_args(self, b, resample, smooth, vae, samples, eps, ctr, eps_row0, unfiltered):
        """What the two batched device calls share: the checks of their arguments (eps over R N rows),
        the rows and the workspace of b (a _RowBuffers) sized for the call, and the arguments up to the
        workspace that both library calls take -> (S, N, R, K, arguments)."""
        import _p3d
        if self._off is None:
            raise ValueError("set_offsets first")
        R = 1 if resample is None else _check_resample(resample)
        S, N, K = self._off.shape[0] - 1, int(self._off[-1]), 0
        if vae is None:
            if samples is not None or eps is not None or unfiltered:
                raise ValueError("samples, eps and unfiltered need a filter (vae=...)")
        else:
            K = _check_filter(vae, samples, self.model.output_size, "lift_clips")
            want = (K, R * N, vae.latent_dim) if K else (R * N, vae.latent_dim)
            if eps is not None and (tuple(eps.shape) != want or eps.dtype != self.torch.float32 or not eps.is_cuda
                                    or not eps.is_contiguous()):
                raise ValueError("eps: expected a contiguous float32 device tensor %s" % (want,))
        lib, n, sizes = _p3d.lib(), self.max_frames, (self.model.input_size, self.model.output_size, int(vae is not None))
        keys = ("xy", "out", "src") + (("out_u", "src_u") if unfiltered else ()) + (("var",) if K else ())
        if resample is None:                                 # (the rows as given: sized once, for max_frames)
            b.need(keys, n, int(lib.p3d_clips_lift_workspace(n, min(S, n), *sizes)))
        else:
            b.need(keys, R * N, int(lib.p3d_clips_lift_resampled_workspace(N, S, R, *sizes)))
            b.need(("info",), S)
            b.need(("off",), S + 1)
        p, d = _p3d.ptr, b.d
        return S, N, R, K, (
            self.model._h, None if vae is None else vae._h, K, p(eps), int(ctr), int(eps_row0),
            p(self.din), self._off.ctypes.data, p(self.doff), S, N, int(bool(smooth)),
            p(self.m2), p(self.s2), p(self.u2), self.u2.numel(), p(self.m3), p(self.s3), p(self.u3), self.u3.numel(), 96,
            int(self.cache_on_fail), p(self.dxy), p(d["out"]), p(d["src"]),
            p(d["out_u"]) if unfiltered else None, p(d["src_u"]) if unfiltered else None, p(d["var"]) if K else None)

    def lift_clips_device(self, smooth=True, vae=None, samples=None, eps=None, ctr=0, eps_row0=0, unfiltered=False):
        """ONE p3d_clips_lift of the rows self.din[:N] under the offsets of the last set_offsets, into
        self.dxy / dout / dsrc (and dout_u / dsrc_u, dvar), on the current stream; capturable.  vae:
        a models.VAE sequence filter run between the forward and the post-processing; samples=K:
        the mean of K draws; eps: a device tensor [N, latent] ([K, N, latent]) or None for the
        library's stream at (ctr, eps_row0 + row)."""
        import _p3d
        b = self.rows
        S, N, _, _, args = self._batch_args(b, None, smooth, vae, samples, eps, ctr, eps_row0, unfiltered)
        _p3d.check(_p3d.lib().p3d_clips_lift(*args, b.work_ptr, b.work_bytes, self.model.stream()), "p3d_clips_lift")
        self._clips = (S, N, vae is not None)
        self._last_off, self._last_rows = self._off, None

    def lift_clips_resampled_device(self, resample, smooth=True, vae=None, samples=None, eps=None, ctr=0, eps_row0=0,
                                    unfiltered=False):
        """ONE p3d_clips_lift_resampled of the rows self.din[:N] under the offsets of the last set_offsets:
        smoothing into self.dxy, the spline resampling (the reference's --interpolation --multiplier
        1 / resample) into the R N rows of self.resampled.d['xy'], and the lift of those rows into
        its ['out'] / ['src'] (['out_u'] / ['src_u'], ['var']); ['info'] [S, 36, 5] is the fits' record
        and ['off'] the resampled clips' offsets.  On the current stream; capturable.  eps rows count
        over the R N resampled rows."""
        import _p3d
        b, p = self.resampled, _p3d.ptr
        _, _, R, _, args = self._batch_args(b, resample, smooth, vae, samples, eps, ctr, eps_row0, unfiltered)
        _p3d.check(_p3d.lib().p3d_clips_lift_resampled(
            *args, R, p(b.d["xy"]), p(b.d["off"]), p(b.d["info"]), b.work_ptr, b.work_bytes, self.model.stream()),
            "p3d_clips_lift_resampled")
        self._last_off, self._last_rows = self._off * R, (b.d["out"], b.d["src"])

    def skeleton(self, lengths=None):
        """The rigid skeleton of the last lift_clip / lift_clips, from its device rows (dout, dsrc, the
        clip offsets): p3d_skel_lengths and p3d_skel_pose, no model involved.  lengths: [16] or
        [S, 16] bone lengths to use instead of each clip's own means.  Returns one dict per clip (one
        for lift_clip): 'lengths' [16], 'n_used', 'quat' [n, 16, 4], 'euler' [n, 16, 3] (Z, X, Y
        degrees), 'rigid' [n, 17, 3], 'root' [n, 3] -- see skeleton_rows."""
        if self._last_off is None:
            raise ValueError("no lift has run yet")
        if self.model.output_size != 48:
            raise ValueError("the skeleton needs the 17-joint model (48 outputs), this one predicts %d values"
                             % self.model.output_size)
        if self._skel is None:
            self._skel = _SkeletonBuffers(self.torch, self.model.device)
        dout, dsrc = self._last_rows or (self.dout, self.dsrc)
        return self._skel.run(dout, dsrc, self._last_off, lengths)

    def trajectory(self, focal, center, smooth_half=0):
        """The root trajectory of the last lift_clip / lift_clips (also with resample= and vae=), from its
        device rows (the poses, the 2D rows the network saw, src, the clip offsets): p3d_root_trajectory,
        no model involved and any joint count.  focal, center = (cx, cy): the camera's, in the pixels
        of the keypoints; smooth_half: the window's half width in frames, 0..32.  Returns one dict per
        clip (one for lift_clip): 'traj', 'traj_raw' [n, 3], 'resid' [n], 'valid' [n] bool, 'root_skel'
        [n, 3], 'camera' -- see trajectory_rows, which says what the solve assumes."""
        if self._last_off is None:
            raise ValueError("no lift has run yet")
        if self._traj is None:
            self._traj = _TrajectoryBuffers(self.torch, self.model.device)
        if self._last_rows is None:
            dout, dsrc, dxy = self.dout, self.dsrc, self.dxy
        else:                                                # (resampled: the rows the lifter saw are the resampled ones)
            dout, dsrc, dxy = self._last_rows + (self.resampled.d["xy"],)
        return self._traj.run(dout, dxy, dsrc, self._last_off, focal, center, smooth_half)

    def lift_clips(self, clips, smooth=True, vae=None, samples=None, eps=None, ctr=None, unfiltered=False,
                   resample=None):
        """A list of clips, each [n_s, 36] raw keypoints in position order (sum n_s <= max_frames), in
        ONE p3d_clips_lift: every clip is smoothed, lifted and post-processed as lift_clip does it
        alone, bit for bit.  vae: a models.VAE sequence filter (in = seq_len * out) that refines the
        network's rows before the post-processing, every clip a fresh sequence; samples=K: the mean of
        K draws; eps: [N, latent] ([K, N, latent]) rows over the concatenated clips, or None for the
        library's stream at counter ctr (None: a fresh one, as filter_sequences).  Returns one dict
        per clip: 'poses' [n_s, 96], 'xy_s' [n_s, 36], 'src' [n_s] (positions inside the clip, -1
        zeros), with unfiltered=True 'poses_unfiltered' / 'src_unfiltered' (the lift without the
        filter) and with samples 'ref_var' [n_s, out] float32 (the draws' variance).

        resample=R (1..16): the reference's --interpolation --multiplier 1/R in the same call
        (p3d_clips_lift_resampled): every smoothed track is fitted with the reference's
        cubic smoothing spline and sampled R times per frame, and the R n_s resampled rows are what the
        lifter, the filter and the post-processing see.  Every clip needs at least 4 frames.  Each
        result then holds R n_s rows -- 'poses', 'xy_s' (the resampled rows), 'src', the optional ones --
        plus 'spline_info' [36, 5] int32 (per track: knots after the first and the second fit, FITPACK's
        ier of each, the p iterations); eps rows count over the resampled rows."""
        rows = [np.asarray(c, np.float64) for c in clips]
        if not rows:
            raise ValueError("expected at least one clip")
        for r in rows:
            if r.ndim != 2 or r.shape[1] != 36 or r.shape[0] < 1:
                raise ValueError("expected clips of [n >= 1, 36] keypoint rows, got %s" % (r.shape,))
            if smooth and 2 <= r.shape[0] <= 8:
                raise ValueError("need more frames, min 9 frames for smoothing")
        off = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int64)
        N = int(off[-1])
        if N > self.max_frames:
            raise ValueError("%d frames in all, max_frames is %d" % (N, self.max_frames))
        R = 1
        if resample is not None:
            R = _check_resample(resample)
            if min(r.shape[0] for r in rows) < 4:
                raise ValueError("need more frames, min 4 frames for a cubic spline")
            if R * N > 1 << 20:
                raise ValueError("%d resampled rows in all, at most 2^20" % (R * N))
        N, N_in, off_in, off = R * N, N, off, off * R        # (rows and offsets of the results)
        torch, K = self.torch, None
        if vae is not None:
            vae._seq_len()
            K = None if samples is None else vae._samples(samples, "lift_clips")
            if eps is not None:
                eps = vae._eps_k(eps, K, N) if K else vae._dev(eps, vae.latent_dim, "eps")
                if eps.shape[-2] != N:
                    raise ValueError("eps: expected %d rows, got %d" % (N, eps.shape[-2]))
            if ctr is None:
                ctr = vae._calls + 1
                vae._calls += K or 1
        np.concatenate(rows, out=self.hin.numpy()[:N_in])
        with torch.cuda.device(self.model.device):
            self.set_offsets(off_in)
            self.din[:N_in].copy_(self.hin[:N_in], non_blocking=True)
            if resample is None:
                self.lift_clips_device(smooth, vae, samples, eps, ctr or 0, 0, unfiltered)
                h, d = self.rows.h, self.rows.d
            else:
                self.lift_clips_resampled_device(R, smooth, vae, samples, eps, ctr or 0, 0, unfiltered)
                h, d = self.resampled.h, self.resampled.d
                h["info"][:len(rows)].copy_(d["info"][:len(rows)], non_blocking=True)
            keys = ["xy", "out", "src"] + (["out_u", "src_u"] if unfiltered else []) + (["var"] if K else [])
            for k in keys:
                h[k][:N].copy_(d[k][:N], non_blocking=True)
            torch.cuda.current_stream(self.model.device).synchronize()
        self.model.check_errors()
        first = np.repeat(off[:-1], np.diff(off))            # every row's clip start: 'src' counts from it (-1 stays)
        local = lambda t: np.where(t.numpy()[:N] >= 0, t.numpy()[:N] - first, -1).astype(np.int32)   # noqa: E731
        views = [("poses", h["out"].numpy()), ("xy_s", h["xy"].numpy()), ("src", local(h["src"]))]
        if unfiltered:
            views += [("poses_unfiltered", h["out_u"].numpy()), ("src_unfiltered", local(h["src_u"]))]
        if K:
            views.append(("ref_var", h["var"].numpy()))
        res = self._results(off.tolist(), views)
        if resample is not None:
            for s, r in enumerate(res):
                r["spline_info"] = h["info"].numpy()[s].copy()
        return res

    def lift_clip(self, xy, smooth=True, resample=None):
        """xy [N <= max_frames, 36] raw keypoints in position order -> (poses [N, 96] float64 mm,
        xy_s [N, 36] float64, src [N] int32: the position each exported pose came from, -1 zeros).
        resample=R: the clip through lift_clips(resample=R) as a batch of one -> (poses [R N, 96], xy_s
        [R N, 36] the resampled rows, src [R N], spline_info [36, 5])."""
        xy = np.asarray(xy, np.float64)
        if xy.ndim != 2 or xy.shape[1] != 36 or not 1 <= xy.shape[0] <= self.max_frames:
            raise ValueError("expected [1..%d, 36] keypoint rows, got %s" % (self.max_frames, xy.shape))
        if resample is not None:
            r = self.lift_clips([xy], smooth, resample=resample)[0]
            return r["poses"], r["xy_s"], r["src"], r["spline_info"]
        n = xy.shape[0]
        if smooth and 2 <= n <= 8:
            raise ValueError("need more frames, min 9 frames for smoothing")
        self.hin.numpy()[:n] = xy
        with self.torch.cuda.device(self.model.device):
            self.din[:n].copy_(self.hin[:n], non_blocking=True)
            self.lift_device(n, smooth)
            self.hxy[:n].copy_(self.dxy[:n], non_blocking=True)
            self.hout[:n].copy_(self.dout[:n], non_blocking=True)
            self.hsrc[:n].copy_(self.dsrc[:n], non_blocking=True)
            self.torch.cuda.current_stream(self.model.device).synchronize()
        self.model.check_errors()
        return self.hout.numpy()[:n].copy(), self.hxy.numpy()[:n].copy(), self.hsrc.numpy()[:n].copy()


# --------------------------------------------------------------------------------------
# live streams: src/openpose_3dpose_sandbox_realtime.py, with the clip path's semantics
# --------------------------------------------------------------------------------------


class LiveLifter(_Lifter):
    """Lift up to `slots` live OpenPose streams frame by frame with a float32 LinearModel.  Every
    tick (``push``) takes at most one raw frame (36 values) per open slot and returns the rows that
    became final: with smoothing frame f once frame f + 4 has arrived (frames 0 .. 4 together at
    the ninth frame, the last four at ``close``), without smoothing at once.  Concatenated over a
    stream's lifetime the rows are ``poses`` / ``xy_s`` / ``src`` of ``ClipLifter.lift_clips`` on the
    stream's whole frame list, bit for bit up to the forward's tiling (a tick's rows, in slot order,
    in tiles of max_batch) and the filter's noise keys (the session's counter, row = rows emitted
    before the tick).  This is the clip path's --cache_on_fail (a failing frame shows the last good
    one from the stream's first frame on), not the realtime script's ``frame != 0`` variant.

    vae: a models.VAE sequence filter between the forward and the post-processing, its buffer
    carried per slot; samples=K: the mean of K draws (adds 'ref_var').  Pinned rows in and out, one
    p3d_live_push per tick, then a wait on the model's completion word."""

    def __init__(self, model, data_mean_2d, data_std_2d, dim_to_use_2d, data_mean_3d, data_std_3d,
                 dim_to_ignore_3d, slots, cache_on_fail=True, smooth=True, vae=None, samples=None):
        import torch
        import _p3d
        self.torch, self.model, self.S = torch, model, int(slots)
        self.cache_on_fail, self.smooth, self.vae = bool(cache_on_fail), bool(smooth), vae
        if model.bf16:
            raise ValueError("LiveLifter: float32 models only")
        if not 1 <= self.S <= 1 << 16:
            raise ValueError("slots must be in [1, 2^16]")
        stats = (data_mean_2d, data_std_2d, dim_to_use_2d, data_mean_3d, data_std_3d, dim_to_ignore_3d)
        self._load_stats("LiveLifter", model, *stats, upload=False)   # (the filter is vetted before anything is uploaded)
        self.K = 0
        if vae is None:
            if samples is not None:
                raise ValueError("samples needs a filter (vae=...)")
        else:
            self.K = _check_filter(vae, samples, model.output_size, "LiveLifter")
            self.ctr = vae._calls + 1                        # the session's noise counter(s), as a fresh
            vae._calls += self.K or 1                        # filter_sequences call takes them
        self._load_stats("LiveLifter", model, *stats)
        S, cap, dev, U3 = self.S, 5 * self.S, model.device, model.output_size
        lib = _p3d.lib()
        with torch.cuda.device(dev):
            pin = lambda shape, dt: torch.zeros(shape, dtype=dt, pin_memory=True)   # noqa: E731
            i32, f64 = torch.int32, torch.float64
            # the tick's table and the rows in and out: pinned, read and written by the kernels in place
            self.hin, self.hpush = pin((S, 36), f64), pin((S,), i32)
            self.hoff, self.hslot = pin((S + 1,), torch.int64), pin((cap,), i32)
            self.hframe, self.hkind = pin((cap,), i32), pin((cap,), i32)
            self.hxy, self.hout, self.hsrc = pin((cap, 36), f64), pin((cap, 96), f64), pin((cap,), i32)
            self.hvar = pin((cap, U3), torch.float32) if self.K else None
            self.state = torch.empty((int(lib.p3d_live_state_bytes(S, U3)),), dtype=torch.uint8, device=dev)
            self.work_bytes = int(lib.p3d_live_push_workspace(S, model.input_size, U3, int(vae is not None)))
            self.work, self.work_ptr = _aligned_workspace(torch, self.work_bytes, dev)
            self.fstate, self.fstarted = vae.new_seq_state(S) if vae is not None else (None, None)
            _p3d.check(lib.p3d_live_reset(self.state.data_ptr(), S, -1, model.stream()), "p3d_live_reset")
        self.count = np.zeros(S, np.int32)                   # frames received per slot
        self._push, self._close, self._short = np.zeros(S, np.uint8), np.zeros(S, np.uint8), np.zeros(S, np.int32)
        self.is_open = np.zeros(S, bool)
        self.emitted = 0                                     # rows emitted so far: the tick's eps_row0
        self.hin_np = self.hin.numpy()
        # the result rows' numpy views, taken once: push slices them per slot
        self._views = [(k, t.numpy()) for k, t in (("frames", self.hframe), ("poses", self.hout), ("xy_s", self.hxy),
                                                   ("src", self.hsrc), ("ref_var", self.hvar)) if t is not None]

    def latency(self):
        """Pushes between a frame and its row: 4 with smoothing, 0 without."""
        return 4 if self.smooth else 0

    def open(self):
        """A free slot, starting from nothing: no ring contents, no held joints, no last good pose, a
        fresh filter buffer."""
        import _p3d
        free = np.flatnonzero(~self.is_open)
        if not len(free):
            raise ValueError("LiveLifter: all %d slots are open" % self.S)
        slot = int(free[0])
        with self.torch.cuda.device(self.model.device):
            _p3d.check(_p3d.lib().p3d_live_reset(self.state.data_ptr(), self.S, slot, self.model.stream()),
                       "p3d_live_reset")
            if self.fstarted is not None:
                self.fstarted[slot:slot + 1].zero_()
        self.count[slot] = 0
        self.is_open[slot] = True
        return slot

    def _slot(self, slot):
        s = int(slot)
        if s != slot or not 0 <= s < self.S or not self.is_open[s]:
            raise ValueError("LiveLifter: slot %r is not open" % (slot,))
        return s

    def push(self, frames, close=()):
        """One tick.  frames: {slot: the 36 raw keypoint values of the slot's next frame}; close:
        slots whose stream ends (not among `frames`).  Returns {slot: dict(frames [n], poses [n, 96],
        xy_s [n, 36], src [n] int32 stream-local, -1 zeros[, ref_var [n, out]])} for the slots with
        rows that became final.  Closing a stream of 2 .. 8 frames under smoothing raises ValueError
        naming the slot -- after freeing it, before anything of the tick has run: the other streams
        are untouched and the tick can be pushed again without it."""
        import _p3d
        lib, model, S = _p3d.lib(), self.model, self.S
        rows = {self._slot(s): np.asarray(xy, np.float64) for s, xy in frames.items()}
        closing = sorted({self._slot(s) for s in close})
        for s, xy in rows.items():
            if xy.shape != (36,):
                raise ValueError("LiveLifter: slot %d: expected 36 keypoint values, got %s" % (s, xy.shape))
            if s in closing:
                raise ValueError("LiveLifter: slot %d is pushed and closed in one tick" % s)
        short = [s for s in closing if self.smooth and 2 <= self.count[s] <= 8]
        if short:
            n = int(self.count[short[0]])
            self.count[short], self.is_open[short] = 0, False
            raise ValueError("stream in slot %d: %d frames: need more frames, min 9 frames for smoothing" % (short[0], n))
        self._push[:], self._close[:] = 0, 0
        for s, xy in rows.items():
            self._push[s] = 1
            self.hin_np[s] = xy
        self._close[closing] = 1
        n_rows = ctypes.c_int64()
        P = lambda t: t.data_ptr()   # noqa: E731
        _p3d.check(lib.p3d_live_plan(S, int(self.smooth), self.count.ctypes.data, self._push.ctypes.data,
                                     self._close.ctypes.data, P(self.hoff), P(self.hslot), P(self.hframe), P(self.hkind),
                                     P(self.hpush), self._short.ctypes.data, ctypes.byref(n_rows)), "p3d_live_plan")
        N, vae = int(n_rows.value), self.vae
        with self.torch.cuda.device(model.device):
            _p3d.check(lib.p3d_live_push(
                model._h, None if vae is None else vae._h, self.K, self.ctr if vae is not None else 0, self.emitted,
                P(self.state), _p3d.ptr(self.fstate), _p3d.ptr(self.fstarted), P(self.hin), P(self.hpush), P(self.hoff),
                P(self.hframe), P(self.hkind), S, N, P(self.m2), P(self.s2), P(self.u2), self.u2.numel(), P(self.m3),
                P(self.s3), P(self.u3), self.u3.numel(), 96, int(self.cache_on_fail), int(self.smooth), P(self.hxy),
                P(self.hout), P(self.hsrc), _p3d.ptr(self.hvar), self.work_ptr, self.work_bytes, model.stream()),
                "p3d_live_push")
            # the tick's last launch signals the model's completion word: wait on that, not on the stream
            _p3d.check(lib.p3d_host_signal(model._h, model.stream()), "p3d_host_signal")
            model._hsig = (model._hsig + 1) & 0xffffffff
            rc = lib.p3d_host_wait(model._h, model._hsig, model.stream())
            if rc:
                model.check_errors()
                _p3d.check(rc, "p3d_host_wait")
        self.emitted += N
        self.is_open[closing] = False
        return {s: d for s, d in enumerate(self._results(self.hoff.numpy().tolist(), self._views)) if d}

    def close(self, slot):
        """End the slot's stream: the rows that were still waiting for their window (the last four
        frames; a one-frame stream's frame), as push returns them for one slot (None: no rows)."""
        return self.push({}, close=(slot,)).get(int(slot))
