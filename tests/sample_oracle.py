"""numpy restatement of sample()'s numbers for ONE key (src/predict_3dpose.py:474-546), for the
tests.  Built from oracle.ref_eval.unNormalizeData and oracle.ref_data.camera_to_world_frame,
both pinned to the reference's own goldens (tests/test_oracle.py, tests/test_oracle_data.py);
what is added here are exact elementwise float64 adds and subtracts."""
import numpy as np

from oracle import ref_data, ref_eval

N_JOINTS_H36M = 32
N_CAMERAS = 4


def key3d_of(key2d, camera_frame):
    """:480-481."""
    subj, b, fname = key2d
    key3d = key2d if camera_frame else (subj, b, '{0}.h5'.format(fname.split('.')[0]))
    return (subj, b, fname[:-3]) if fname.endswith('-sh') and camera_frame else key3d


def the_camera(rcams, key3d):
    """:529-536 -> the camera tuple of the sequence."""
    subj, _, sname = key3d
    cname = sname.split('.')[1]
    scams = {(subj, c + 1): rcams[(subj, c + 1)] for c in range(N_CAMERAS)}
    scam_idx = [scams[(subj, c + 1)][-1] for c in range(N_CAMERAS)].index(cname)
    the_cam = scams[(subj, scam_idx + 1)]
    assert the_cam[-1] == cname
    return the_cam


def cam2world_centered(data_3d_camframe, R, T):
    """:538-542."""
    w = ref_data.camera_to_world_frame(data_3d_camframe.reshape((-1, 3)), R, T)
    w = w.reshape((-1, N_JOINTS_H36M * 3))
    return w - np.tile(w[:, :3], (1, N_JOINTS_H36M))


def world_rows(yn, mean3, std3, ign3, R, T, root=None):
    """unNormalizeData (:513-514), + root (:526, when given), cam2world_centered (:545-546)."""
    x = ref_eval.unNormalizeData(yn, mean3, std3, ign3)
    if root is not None:
        x = x + np.tile(root, [1, N_JOINTS_H36M])
    return cam2world_centered(x, R, T)


def sample_key(enc_in_n, dec_out_n, poses3d_n, stats, camera_frame, cam=None, root=None):
    """(enc_in, dec_out, poses3d) of one key as :512-546 leaves them.  ``poses3d_n`` is the
    network's normalised output for the key's rows; ``stats`` holds data_mean_2d/std_2d,
    dim_to_ignore_2d and their 3D counterparts."""
    enc_in = ref_eval.unNormalizeData(enc_in_n, stats["data_mean_2d"], stats["data_std_2d"],
                                      stats["dim_to_ignore_2d"])
    m3, s3, i3 = stats["data_mean_3d"], stats["data_std_3d"], stats["dim_to_ignore_3d"]
    if not camera_frame:
        return enc_in, ref_eval.unNormalizeData(dec_out_n, m3, s3, i3), ref_eval.unNormalizeData(poses3d_n, m3, s3, i3)
    R, T = cam[0], cam[1]
    return (enc_in, world_rows(dec_out_n, m3, s3, i3, R, T, root=root),
            world_rows(poses3d_n, m3, s3, i3, R, T, root=None))


def picked_rows(n_last, nsamples=15):
    """:576-609 transcribed: the permutation of the last key's rows, and the entries the plot
    loop reads (exidx = 1, 2, ..., stopping where the reference's indexing would run out)."""
    idx = np.random.permutation(n_last)
    shown, exidx = [], 1
    for _ in np.arange(nsamples):
        if exidx >= n_last:
            break
        shown.append(idx[exidx])
        exidx = exidx + 1
    return np.array(shown, dtype=idx.dtype)
