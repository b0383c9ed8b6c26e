"""A live OpenPose stream -> 3D poses, frame by frame (src/openpose_3dpose_sandbox_realtime.py), on
the MI355X.

    python openpose_3dpose_sandbox_realtime.py --pose_estimation_json <dir OpenPose writes into> \\
        --camera_frame --residual --batch_norm --dropout 0.5 --max_norm --evaluateActionWise \\
        --use_sh --epochs 200 --load 4874200 --idle_exit 5

Polls ``--pose_estimation_json DIR`` for new frame files and pushes them, IN FRAME-NUMBER ORDER and
every one of them, into one slot of an ``openpose_frontend.LiveLifter``: one ``p3d_live_push`` per
frame smooths the 2D tracks at a fixed delay of four frames, holds dropped joints, lifts the frame
that became final, optionally refines it with the temporal VAE filter (``--vae_filter W.npz``,
``--filter_samples K``) and post-processes it (axis swap, flip, spine offset, ``--cache_on_fail``).
The reference looks only at the NEWEST file of the directory at every turn of its loop and so
loses every frame that was written while it was busy; its poses are not smoothed and its cache rule
skips frame 0.  This driver follows the clip pipeline instead: the poses of the stream are those of
``openpose_3dpose_sandbox.py`` on the same directory.

After ``--idle_exit SECONDS`` without a new frame the stream is closed, the last four frames are
flushed and ``export_maya`` writes ``3d_data.json`` / ``2d_data.json`` into ``--out_dir``; with
``--export_bvh`` the stream's collected rows also go through ``skeleton_rows`` into ``skeleton.bvh``,
and with ``--root_trajectory --focal F --principal CX CY`` through ``trajectory_rows`` into
``trajectory.json`` (and the BVH's root): at export time, over the whole recorded stream -- its mean
window looks ahead, which is fine after the fact, and nothing is added to the per-frame push.
``--no_smooth`` lifts every frame at once.  A frame file that cannot be parsed yet (still being
written) is tried again at the next poll; a gap in the frame numbers is waited for and, if it is
still there at the idle exit, refused like the clip driver refuses it.

Not built: the pose plots and the ``cv2`` window of the reference (matplotlib / OpenCV, not hot
paths).  ``--interpolation`` and the clip driver's ``--spline_resample`` are refused: a smoothing spline
is fitted over the whole clip, every sample depends on frames that have not arrived yet, so it is not
causal and has no place in a stream.
"""
from __future__ import annotations

import logging
import os
import re
import sys
import time

import numpy as np

import data_utils
import openpose_3dpose_sandbox as sandbox
import openpose_frontend as of
import predict_3dpose as p3

logger = logging.getLogger(__name__)


def build_parser():
    p = sandbox.build_parser()
    p.add_argument("--idle_exit", type=float, default=5.0,
                   help="seconds without a new frame file after which the stream is closed and exported")
    p.add_argument("--poll", type=float, default=0.02, help="seconds between two looks at the directory")
    return p


def frame_files(directory):
    """{frame number: path} of the directory's *.json files (the number: the last run of digits)."""
    out = {}
    for name in os.listdir(directory):
        digits = re.findall(r"(\d+)", name)
        if name.endswith(".json") and digits:
            out[int(digits[-1])] = os.path.join(directory, name)
    return out


class Recorder:
    """The rows a stream has given so far, in frame order."""

    def __init__(self):
        self.poses, self.xy_s, self.src = [], [], []

    def add(self, rows):
        if rows is not None:
            self.poses += list(rows["poses"])
            self.xy_s += list(rows["xy_s"])
            self.src += list(rows["src"])

    def __len__(self):
        return len(self.poses)


def run_stream(flags, lifter, on_rows=None, clock=time.monotonic, sleep=time.sleep):
    """Poll flags.pose_estimation_json and push every frame in frame-number order until no new frame
    has come for flags.idle_exit seconds; close and flush.  Returns (frame_numbers, poses, xy_s, src)."""
    slot, rec, numbers = lifter.open(), Recorder(), []
    nxt, last_new = None, clock()
    while True:
        files = frame_files(flags.pose_estimation_json)
        if nxt is None and files:
            nxt = min(files)
        progressed = False
        while nxt is not None and nxt in files:
            try:
                xy = of.read_frame_file(files[nxt])
            except (ValueError, KeyError, IndexError) as e:   # (json.JSONDecodeError is a ValueError)
                if isinstance(e, ValueError) and "expected 18 joints" in str(e):
                    raise
                break                                         # still being written: the next poll
            rows = lifter.push({slot: xy}).get(slot)
            rec.add(rows)
            if on_rows is not None and rows is not None:
                on_rows(rows)
            numbers.append(nxt)
            nxt += 1
            progressed = True
        if progressed:
            last_new = clock()
        elif clock() - last_new >= flags.idle_exit:
            break
        else:
            sleep(flags.poll)
    if not numbers:
        raise SystemExit("no frame files appeared in %s within %g seconds" % (flags.pose_estimation_json, flags.idle_exit))
    later = [n for n in files if n >= nxt]
    if later and lifter.smooth:
        raise ValueError("frame numbers must be contiguous for smoothing (a gap after frame %d)" % (nxt - 1))
    rows = lifter.close(slot)
    rec.add(rows)
    if on_rows is not None and rows is not None:
        on_rows(rows)
    assert len(rec) == len(numbers)
    return np.array(numbers, np.int64), np.array(rec.poses), np.array(rec.xy_s), np.array(rec.src, np.int32)


def run(flags):
    if flags.interpolation or flags.spline_resample is not None:
        raise SystemExit("--interpolation / --spline_resample (UnivariateSpline resampling) fit a spline over the whole "
                         "clip, which is not causal: use openpose_3dpose_sandbox.py --spline_resample R on the recorded clip")
    if flags.write_gif:
        raise SystemExit("--write_gif (matplotlib pose plots) is not part of this build")
    if flags.clips_root or flags.export_unfiltered:
        raise SystemExit("--clips_root and --export_unfiltered belong to openpose_3dpose_sandbox.py")
    if flags.filter_samples is not None and not flags.vae_filter:
        raise SystemExit("--filter_samples needs --vae_filter")
    if flags.export_bvh and flags.predict_14:
        raise SystemExit("--export_bvh needs the 17-joint model: the skeleton's bones are not defined for --predict_14")
    p3.check_trajectory_flags(flags)
    logging.basicConfig(level={0: logging.ERROR, 1: logging.WARNING, 2: logging.INFO,
                               3: logging.DEBUG}.get(flags.verbose, logging.INFO))
    logger.info("the pose plots and the cv2 window are not part of this build")
    d = p3.load_data(flags)
    actions = data_utils.define_actions(flags.action)
    with p3.Session() as sess:
        model = p3.create_model(sess, actions, 128, flags)        # (batch_size = 128, :48)
        vae = sandbox.load_filter(flags, model) if flags.vae_filter else None
        lifter = of.LiveLifter(model, d["data_mean_2d"], d["data_std_2d"], d["dim_to_use_2d"], d["data_mean_3d"],
                               d["data_std_3d"], d["dim_to_ignore_3d"], slots=1, cache_on_fail=flags.cache_on_fail,
                               smooth=not flags.no_smooth, vae=vae, samples=flags.filter_samples)
        logger.info("polling %s (a frame is final %d frames after it arrives)", flags.pose_estimation_json,
                    lifter.latency())
        try:
            numbers, poses, xy_s, src = run_stream(
                flags, lifter, on_rows=lambda r: logger.debug("frames %s lifted", r["frames"].tolist()))
        finally:
            if vae is not None:
                vae.close()
            model.close()
    held = int((src != np.arange(len(src))).sum())
    if held:
        logger.info("%d failed frames replaced by the last good one", held)
    paths = of.export_maya(flags.out_dir, numbers, poses, xy_s)
    tr = None
    if flags.root_trajectory:
        tr = of.trajectory_rows(poses, xy_s, src, [0, len(numbers)], flags.focal, flags.principal,
                                flags.trajectory_smooth, device=model.device)[0]
    if flags.export_bvh:
        sk = of.skeleton_rows(poses, src, [0, len(numbers)], device=model.device)[0]
        paths += (sandbox.write_bvh(flags, flags.out_dir, numbers, sandbox.with_trajectory(sk, tr)),)
    if tr is not None:
        paths += (of.export_trajectory(flags.out_dir, numbers, tr),)
    for path in paths:
        logger.info("exported maya json to %s", path)
    logger.info("Done!")
    return paths


def main(argv=None):
    flags = build_parser().parse_args(argv)
    p3.FLAGS = flags
    return run(flags)


if __name__ == "__main__":
    main(sys.argv[1:])
