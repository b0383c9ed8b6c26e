"""Host plumbing of the temporal VAE filter (src/top_vae_3d_pose/data_handler.py): the noise the
filter is trained to remove, the sliding windows over the 3D sequences, and the 2D -> 3D key map.
numpy only; nothing here touches the GPU."""
import numpy as np

from top_vae_3d_pose.args_def import ENVIRON as ENV

NOISE = 0.22108747          # data_handler.py:57
NOISE_OFFSET = 0.0011787938  # data_handler.py:60


def add_noise(data, noise_3d=None):
    """Noise on the 3D joints (data_handler.py:48-84): Gaussian noise on every coordinate of a
    sample and a larger one on the three coordinates of one randomly chosen joint.

    np.random is called in the reference's order -- randn(n, d), choice(arange(d), n), randn(n, 3),
    randn(n) -- so a seeded np.random gives what the reference would.  Its quirks are kept:

    * ``noise = 0.22108747`` is hard-coded and overrides ``noise_3d[0]``;
    * the Gaussian noise is offset by 0.0011787938;
    * ``probs`` is drawn with randn (not rand) and a sample is skipped when it is < 0.5, so about
      69 % of the samples stay clean;
    * the single joint's noise scale is ``noise + noise_3d[1]`` (a sum, not a product).

    ``noise_3d`` defaults to FLAGS.noise_3d.  Returns a noised copy in the dtype of `data`."""
    data_noised = np.array(data)
    nsamples, points_dim = data_noised.shape
    noise_3d = ENV.FLAGS.noise_3d if noise_3d is None else noise_3d
    joint_noise_factor = noise_3d[1]
    noise = NOISE
    noised_all = np.random.randn(nsamples, points_dim) * noise + NOISE_OFFSET
    joints_idx = np.random.choice(np.arange(points_dim), nsamples)
    noise_single_joint = np.random.randn(nsamples, 3) * (noise + joint_noise_factor)
    probs = np.random.randn(nsamples)
    rows = np.nonzero(~(probs < 0.5))[0]
    dt = data_noised.dtype
    # (sums formed in float64 and rounded to the data's type once per addition, as the reference's
    # in-place row and element updates are)
    data_noised[rows] = (data_noised[rows].astype(np.float64) + noised_all[rows]).astype(dt)
    jid = joints_idx[rows] - joints_idx[rows] % 3
    for k in range(3):
        data_noised[rows, jid + k] = (data_noised[rows, jid + k].astype(np.float64)
                                      + noise_single_joint[rows, k]).astype(dt)
    return data_noised


def get_key3d(key2d, camera_frame=None):
    """The key of the 3D set for a key of the 2D set (data_handler.py:218-225)."""
    camera_frame = ENV.FLAGS.camera_frame if camera_frame is None else camera_frame
    (subj, b, fname) = key2d
    key3d = key2d if camera_frame else (subj, b, '{0}.h5'.format(fname.split('.')[0]))
    key3d = (subj, b, fname[:-3]) if fname.endswith('-sh') and camera_frame else key3d
    return key3d


def _windows(poses, seq_len):
    keys = list(poses.keys())
    lens = [int(poses[k].shape[0]) for k in keys]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    width = poses[keys[0]].shape[1] if keys else 0
    frames = (np.concatenate([np.asarray(poses[k], np.float32) for k in keys], axis=0) if keys
              else np.zeros((0, width), np.float32))
    starts, wkey = [], []
    for i, n in enumerate(lens):
        nw = max(n - seq_len, 0)
        starts.append(off[i] + np.arange(nw, dtype=np.int64))
        wkey.append(np.full(nw, i, np.int64))
    starts = np.concatenate(starts) if starts else np.zeros(0, np.int64)
    wkey = np.concatenate(wkey) if wkey else np.zeros(0, np.int64)
    return {"frames": np.ascontiguousarray(frames), "starts": starts, "window_key": wkey, "keys": keys,
            "seq_off": off, "seq_len": int(seq_len)}


def load_dataset_3d_seq(data, seq_len=3):
    """The sliding windows of data_handler.py:506-574 in index form.  `data` is
    predict_3dpose.load_data's dict; returns (train, test), each a dict with

      frames      [N, 48] float32, the split's sequences concatenated in key order,
      starts      [W] int64, the first frame of every window,
      window_key  [W] int64, the index into `keys` of every window's sequence,
      keys, seq_off [len(keys) + 1], seq_len.

    Window i of a sequence of n frames covers frames i .. i + seq_len - 1 for i in
    range(n - seq_len): the reference drops the last possible window, and so does this.  Sequences
    shorter than seq_len + 1 give none.  A window's x is the seq_len * 48 contiguous floats of
    `frames` from its start (window_x) and its y its last frame (window_y)."""
    return _windows(data["train_set_3d"], seq_len), _windows(data["test_set_3d"], seq_len)


def window_x(split, idx=None):
    """[len(idx), seq_len * 48] inputs of the windows `idx` (all of them by default), host side."""
    starts = split["starts"] if idx is None else split["starts"][idx]
    w = split["frames"].shape[1]
    flat = split["frames"].reshape(-1)
    return flat[(starts * w)[:, None] + np.arange(split["seq_len"] * w)[None, :]]


def window_y(split, idx=None):
    """[len(idx), 48] targets: every window's last frame."""
    starts = split["starts"] if idx is None else split["starts"][idx]
    return split["frames"][starts + split["seq_len"] - 1]


def load_effnet_outputs(path, order_keys, sizes):
    """The precomputed EfficientNet features of the frames behind `order_keys`, concatenated in key
    order (load_effnet_h5py_outputs, data_handler.py:325-340): per key (subject, action, name) the
    dataset ``<subject>/<action>/<name without .h5>/data``, cut to the key's 2D frame count `size`
    (some frames have no 2D pose).  `path` is an ``.npz`` archive whose member names are those
    dataset paths (the archive convention of data_utils), or the reference's ``.hdf5`` file where
    h5py is installed.  A missing dataset or one shorter than `size` raises ValueError naming the key."""
    order_keys, sizes = list(order_keys), [int(n) for n in sizes]
    if len(order_keys) != len(sizes):
        raise ValueError("load_effnet_outputs: %d keys but %d sizes" % (len(order_keys), len(sizes)))
    if str(path).endswith(".npz"):
        src = np.load(path, allow_pickle=False)
        names = set(src.files)

        def read(rel):
            return np.asarray(src[rel]) if rel in names else None
    else:
        try:
            import h5py
        except ImportError:
            raise ImportError("reading %s needs h5py; pass the features as an .npz archive whose member names "
                              "are the dataset paths (<subject>/<action>/<name>/data)" % path)
        src = h5py.File(path, "r")

        def read(rel):
            return np.array(src[rel]) if rel in src else None
    try:
        data = []
        for key, size in zip(order_keys, sizes):
            subject, action, name = key[0], key[1], key[2]
            rel = "%s/%s/%s/data" % (subject, action, str(name).replace(".h5", ""))
            outs = read(rel)
            if outs is None:
                raise ValueError("load_effnet_outputs: no dataset %s for key %s in %s" % (rel, (subject, action, name), path))
            if outs.ndim != 2 or outs.shape[0] < size:
                raise ValueError("load_effnet_outputs: dataset %s of key %s has shape %s, fewer than %d rows"
                                 % (rel, (subject, action, name), tuple(outs.shape), size))
            data.append(outs[:size].astype(np.float32, copy=False))
    finally:
        src.close()
    if not data:
        raise ValueError("load_effnet_outputs: no keys")
    return np.concatenate(data, axis=0)
