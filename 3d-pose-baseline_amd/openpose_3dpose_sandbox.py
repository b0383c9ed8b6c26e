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

Not built (they need scipy / matplotlib and are not hot paths): ``--interpolation``
(UnivariateSpline resampling, :240-291), the curve and pose plots, ``--write_gif``.  The driver
refuses those flags.  ``--out_dir`` (build-specific) names the export directory.
"""
from __future__ import annotations

import logging
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
    return p


def run(flags):
    if flags.interpolation:
        raise SystemExit("--interpolation (UnivariateSpline resampling) is not part of this build")
    if flags.write_gif:
        raise SystemExit("--write_gif (matplotlib pose plots) is not part of this build")
    logging.basicConfig(level={0: logging.ERROR, 1: logging.WARNING, 2: logging.INFO,
                               3: logging.DEBUG}.get(flags.verbose, logging.INFO))
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
        model.close()
    paths = of.export_maya(flags.out_dir, frame_numbers, poses, xy_s)
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
