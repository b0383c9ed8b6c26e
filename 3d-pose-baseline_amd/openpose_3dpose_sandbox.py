"""OpenPose clip -> 3D poses and the Maya export (src/openpose_3dpose_sandbox.py), on the MI355X.

    python openpose_3dpose_sandbox.py --pose_estimation_json <dir of *_keypoints.json> \\
        --camera_frame --residual --batch_norm --dropout 0.5 --max_norm --evaluateActionWise \\
        --use_sh --epochs 200 --load 4874200

Reads the frame files (``read_openpose_json``, :39-127), then ONE ``p3d_clip_lift`` smooths the
2D tracks and holds dropped joints (:140-227), lifts every frame (:317-359), swaps / flips /
re-anchors the axes (:366-383) and replaces failed frames with the last good one
(``--cache_on_fail``, :389-417); ``export_maya`` writes ``maya/3d_data.json`` and
``maya/2d_data.json`` (:426-433).  The statistics come from the same loaders as training
(``predict_3dpose.load_data``; ``--use_sh`` for the Stacked Hourglass detections the reference's
sandbox normalises with).

Not built (they need matplotlib and are not hot paths): the curve and pose plots, ``--write_gif``.
The reference's ``--interpolation --multiplier 1/R`` (UnivariateSpline resampling, :240-291) is built
as ``--spline_resample R`` (build-specific, R a whole number 1..16: R output frames per input frame,
the reference's default multiplier 0.1 is R = 10): every smoothed 2D track is fitted with the
reference's cubic smoothing spline on the GPU and sampled R times per frame inside the same
``p3d_clips_lift_resampled`` call, and the export's frames are numbered 0 .. R m - 1 as the reference
renumbers them.  ``--interpolation`` itself still exits, pointing at
``--spline_resample`` (multipliers that are not 1/R garble the reference's own reshaping).
``--out_dir`` (build-specific) names the export directory.

Build-specific, all in ONE ``p3d_clips_lift``: ``--clips_root DIR`` lifts every clip under DIR (each
immediate subdirectory with frame files, exported to ``<out_dir>/<clip name>/``);
``--vae_filter W.npz`` refines the lifted poses with the temporal VAE filter whose weights
``3d_pose_vae_filter_kin.py`` saves (``--latent_dim`` / ``--enc_dim`` / ``--dec_dim`` as there),
between the forward and the post-processing, every clip a fresh sequence; ``--filter_samples K``
averages K posterior samples per frame; ``--export_unfiltered`` also writes
``3d_data_unfiltered.json``, the poses without the filter.  ``--export_bvh`` also writes
``skeleton.bvh`` beside ``3d_data.json`` (``ClipLifter.skeleton``: constant bone lengths per clip,
one rotation per bone and frame; ``--bvh_fps`` its frame rate; the 17-joint models only).
``--root_trajectory --focal F --principal CX CY`` also writes ``trajectory.json``
(``ClipLifter.trajectory``: the camera-frame root translation per frame that puts the lifted joints
onto their 2D tracks; ``--trajectory_smooth H`` its mean window's half width) and makes
it the root of ``skeleton.bvh``.  Without these flags the driver does what it did before them.
"""
from __future__ import annotations

import logging
import os
import sys

import numpy as np

import data_utils
import openpose_frontend as of
import predict_3dpose as p3

logger = logging.getLogger(__name__)


def build_parser():
    p = p3.build_parser()
    p.add_argument("--out_dir", type=str, default="maya", help="directory of 3d_data.json / 2d_data.json")
    p.add_argument("--no_smooth", action="store_true", default=False,
                   help="skip the median smoothing (read_openpose_json(smooth=False))")
    p.add_argument("--clips_root", type=str, default=None,
                   help="lift every clip under this directory (one subdirectory of frame files each) in one call")
    p.add_argument("--vae_filter", type=str, default=None,
                   help="weights (.npz) of the temporal VAE filter, run between the forward and the post-processing")
    p.add_argument("--filter_samples", type=int, default=None, help="average K posterior samples per frame (1 .. 64)")
    p.add_argument("--export_unfiltered", action="store_true", default=False,
                   help="also write 3d_data_unfiltered.json (needs --vae_filter)")
    p.add_argument("--spline_resample", type=int, default=None,
                   help="R output frames per input frame through the reference's smoothing spline "
                        "(its --interpolation --multiplier 1/R), 1..16; every clip needs 4 frames")
    p.add_argument("--latent_dim", type=int, default=24, help="VAE latent dimension")
    p.add_argument("--enc_dim", type=int, nargs="+", default=[40, 32], help="VAE encoder dimension")
    p.add_argument("--dec_dim", type=int, nargs="+", default=[32, 40], help="VAE decoder dimension")
    return p


def load_filter(flags, model):
    """The temporal filter of --vae_filter on the lifter's device: its input width (seq_len * 48) is
    the first encoder kernel's, read from the weights file."""
    from top_vae_3d_pose import models
    path = flags.vae_filter if flags.vae_filter.endswith(".npz") else flags.vae_filter + ".npz"
    key = "enc_h_%d/kernel" % flags.enc_dim[0]
    with np.load(path, allow_pickle=False) as z:
        if key not in z.files:
            raise SystemExit("--vae_filter %s has no %s: do --enc_dim / --dec_dim / --latent_dim match it?" % (path, key))
        in_size = int(z[key].shape[0])
    vae = models.VAE(in_size, latent_dim=flags.latent_dim, enc_dim=flags.enc_dim, dec_dim=flags.dec_dim,
                     device=model.device.index)
    vae.load_weights(path)
    return vae


def write_bvh(flags, out_dir, frame_numbers, sk):
    """--export_bvh of one clip: <out_dir>/skeleton.bvh from a ClipLifter.skeleton / skeleton_rows dict."""
    return of.export_bvh(os.path.join(out_dir, "skeleton.bvh"), frame_numbers, sk["lengths"], sk["euler"], sk["root"],
                         fps=flags.bvh_fps)


def with_trajectory(sk, tr):
    """A skeleton dict whose root is the trajectory (in the skeleton's coordinates), where there is one."""
    return sk if tr is None else dict(sk, root=tr["root_skel"])


def trajectory_of(flags, lifter):
    """--root_trajectory: ClipLifter.trajectory of the last lift under the flags' camera, else None."""
    if not flags.root_trajectory:
        return None
    return lifter.trajectory(flags.focal, flags.principal, flags.trajectory_smooth)


def run_clips(flags):
    """--clips_root / --vae_filter / --spline_resample: one p3d_clips_lift (p3d_clips_lift_resampled) over every clip."""
    if flags.clips_root:
        names, numbers, clips = of.read_clips(flags.clips_root)
    else:
        fn, xy = of.read_openpose_json(flags.pose_estimation_json)
        names, numbers, clips = None, [fn], [xy]
    smooth = not flags.no_smooth
    of.check_clips(numbers, smooth, names)
    d = p3.load_data(flags)
    actions = data_utils.define_actions(flags.action)
    with p3.Session() as sess:
        model = p3.create_model(sess, actions, 128, flags)
        lifter = of.ClipLifter(model, d["data_mean_2d"], d["data_std_2d"], d["dim_to_use_2d"], d["data_mean_3d"],
                               d["data_std_3d"], d["dim_to_ignore_3d"], max_frames=sum(len(c) for c in clips),
                               cache_on_fail=flags.cache_on_fail)
        vae = load_filter(flags, model) if flags.vae_filter else None
        logger.info("lifting %d clips, %d frames", len(clips), sum(len(c) for c in clips))
        results = lifter.lift_clips(clips, smooth=smooth, vae=vae, samples=flags.filter_samples,
                                    unfiltered=flags.export_unfiltered, resample=flags.spline_resample)
        if flags.spline_resample is not None:                 # the resampled frames, renumbered from 0 (:283-284)
            numbers = [np.arange(len(r["poses"]), dtype=np.int64) for r in results]
        skeletons = lifter.skeleton() if flags.export_bvh else None
        trajs = trajectory_of(flags, lifter)
        if skeletons and trajs:
            skeletons = [with_trajectory(sk, tr) for sk, tr in zip(skeletons, trajs)]
        if vae is not None:
            vae.close()
        model.close()
    if names is None:                                         # a single --pose_estimation_json clip
        r = results[0]
        paths = of.export_maya(flags.out_dir, numbers[0], r["poses"], r["xy_s"])
        if flags.export_unfiltered:
            paths += (of.export_unfiltered(flags.out_dir, numbers[0], r["poses_unfiltered"]),)
        if skeletons:
            paths += (write_bvh(flags, flags.out_dir, numbers[0], skeletons[0]),)
        if trajs:
            paths += (of.export_trajectory(flags.out_dir, numbers[0], trajs[0]),)
    else:
        paths = of.export_maya_clips(flags.out_dir, names, numbers, results, unfiltered=flags.export_unfiltered)
        if skeletons:
            bvh = of.export_bvh_clips(flags.out_dir, names, numbers, skeletons, fps=flags.bvh_fps)
            paths = [q + (b,) for q, b in zip(paths, bvh)]
        if trajs:
            paths = [q + (of.export_trajectory(os.path.join(flags.out_dir, name), fn, tr),)
                     for q, name, fn, tr in zip(paths, names, numbers, trajs)]
    logger.info("exported maya json under %s", flags.out_dir)
    logger.info("Done!")
    return paths


def run(flags):
    if flags.interpolation:
        raise SystemExit("--interpolation (UnivariateSpline resampling) is not part of this build: "
                         "--spline_resample R is its --multiplier 1/R")
    if flags.write_gif:
        raise SystemExit("--write_gif (matplotlib pose plots) is not part of this build")
    if flags.spline_resample is not None and not 1 <= flags.spline_resample <= 16:
        raise SystemExit("--spline_resample must be in 1..16")
    logging.basicConfig(level={0: logging.ERROR, 1: logging.WARNING, 2: logging.INFO,
                               3: logging.DEBUG}.get(flags.verbose, logging.INFO))
    if (flags.filter_samples is not None or flags.export_unfiltered) and not flags.vae_filter:
        raise SystemExit("--filter_samples and --export_unfiltered need --vae_filter")
    if flags.export_bvh and flags.predict_14:
        raise SystemExit("--export_bvh needs the 17-joint model: the skeleton's bones are not defined for --predict_14")
    p3.check_trajectory_flags(flags)
    if flags.clips_root or flags.vae_filter or flags.spline_resample is not None:
        return run_clips(flags)
    logger.info("start reading json files")
    frame_numbers, xy = of.read_openpose_json(flags.pose_estimation_json)
    smooth = not flags.no_smooth
    of.check_clip(frame_numbers, smooth)
    d = p3.load_data(flags)
    actions = data_utils.define_actions(flags.action)
    with p3.Session() as sess:
        batch_size = 128                                    # (:312)
        model = p3.create_model(sess, actions, batch_size, flags)
        lifter = of.ClipLifter(model, d["data_mean_2d"], d["data_std_2d"], d["dim_to_use_2d"], d["data_mean_3d"],
                               d["data_std_3d"], d["dim_to_ignore_3d"], max_frames=len(frame_numbers),
                               cache_on_fail=flags.cache_on_fail)
        logger.info("lifting %d frames", len(frame_numbers))
        poses, xy_s, src = lifter.lift_clip(xy, smooth=smooth)
        held = int((src != np.arange(len(src))).sum())
        if held:
            logger.info("%d failed frames replaced by the last good one", held)
        sk = lifter.skeleton()[0] if flags.export_bvh else None
        tr = trajectory_of(flags, lifter)
        tr = tr[0] if tr else None
        model.close()
    paths = of.export_maya(flags.out_dir, frame_numbers, poses, xy_s)
    if sk is not None:
        paths += (write_bvh(flags, flags.out_dir, frame_numbers, with_trajectory(sk, tr)),)
    if tr is not None:
        paths += (of.export_trajectory(flags.out_dir, frame_numbers, tr),)
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
