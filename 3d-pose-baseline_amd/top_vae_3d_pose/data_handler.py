"""Data plumbing of the VAE filters (src/top_vae_3d_pose/data_handler.py): the noise the filters are
trained to remove -- the reference's numpy add_noise on the host, and add_noise_device, its
counter-based restatement drawn on the GPU by libp3d.so's p3d_vae_add_noise --, the stand-alone
denoiser's device-resident Dataset and load_3d_data, the sliding windows over the 3D sequences, and
the 2D -> 3D key map.  Everything but add_noise_device and Dataset is numpy only."""
from collections import namedtuple

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


NOISE_MAX_ROWS = 1 << 20    # p3d_vae_add_noise's B per call
Metadata = namedtuple("Metadata", "mean std dim_ignored dim_used")


def joint_scale(noise_3d=None):
    """The single joint's noise scale ``noise + noise_3d[1]``: the sum formed in double and rounded
    to float32 once."""
    noise_3d = ENV.FLAGS.noise_3d if noise_3d is None else noise_3d
    return np.float32(NOISE + noise_3d[1])


def add_noise_device(data, noise_3d=None, *, seed, ctr, row0=0, starts=None, width=None, out=None):
    """add_noise on the device (p3d_vae_add_noise, one k_vae_noise launch per 2^20 rows): `data` is a
    contiguous float32 device tensor [n, d]; returns the noised [B, width] device tensor.

    Without `starts`, B = n, width = d and output row r is row r of `data` (``out=data`` noises in
    place).  With `starts` (int64 device vector [B]) output row r is the `width` = k d contiguous
    floats of `data` from row starts[r] -- a window of k frames, read in place.

    The distribution is add_noise's; the bits are the library's Philox stream, keyed by (seed, ctr,
    row0 + r, column): the same seed, ctr and row give the same noise whatever the call's size, so
    splitting a call changes nothing.  ``noise_3d[0]`` stays ignored, as at add_noise."""
    import torch

    import _p3d
    if (not isinstance(data, torch.Tensor) or data.dim() != 2 or data.dtype != torch.float32 or not data.is_cuda
            or not data.is_contiguous()):
        raise ValueError("add_noise_device: data must be a contiguous float32 device tensor [n, d]")
    n, d = int(data.shape[0]), int(data.shape[1])
    if starts is None:
        if width not in (None, d):
            raise ValueError("add_noise_device: without starts width is d = %d, got %s" % (d, width))
        B, width = n, d
    else:
        if (not isinstance(starts, torch.Tensor) or starts.dim() != 1 or starts.dtype != torch.int64
                or starts.device != data.device or not starts.is_contiguous()):
            raise ValueError("add_noise_device: starts must be a contiguous int64 vector on %s" % data.device)
        B, width = int(starts.shape[0]), int(d if width is None else width)
    if out is None:
        out = torch.empty((B, width), dtype=torch.float32, device=data.device)
    elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, width) or out.dtype != torch.float32
          or out.device != data.device or not out.is_contiguous()):
        raise ValueError("add_noise_device: out must be a contiguous float32 tensor [%d, %d] on %s"
                         % (B, width, data.device))
    if B < 1:
        raise ValueError("add_noise_device: no rows")
    scale = float(joint_scale(noise_3d))
    with torch.cuda.device(data.device):
        stream = _p3d.stream_handle()
        for r0 in range(0, B, NOISE_MAX_ROWS):
            nb = min(NOISE_MAX_ROWS, B - r0)
            if starts is None:
                src, rows, st = data[r0:], n - r0, None
            else:
                src, rows, st = data, n, _p3d.ptr(starts[r0:])
            _p3d.check(_p3d.lib().p3d_vae_add_noise(_p3d.ptr(src), rows, d, st, width, nb, int(seed), int(ctr),
                                                    int(row0) + r0, NOISE, NOISE_OFFSET, scale, _p3d.ptr(out[r0:]),
                                                    stream), "p3d_vae_add_noise")
    return out


class Dataset(object):
    """The stand-alone denoiser's data (data_handler.py:167-214), resident on the device: `data`
    [n, d] and its noised copy, served in batches of (data_noised[idxs], data[idxs]).

    The indices are shuffled by np.random.shuffle on the host, as in the reference; the rows are
    gathered on the device.  Noise draw number k is add_noise_device(data, seed=seed,
    ctr=ctr0 + k * ctr_step): draw 0 at construction, one more per on_epoch_end(new_noise=True).
    The stream's row is the sample's position in `data`, so the noise belongs to the sample, not to
    its place in the epoch."""

    def __init__(self, data, batch_size=64, shuffle=True, metadata=None, *, seed=0, ctr0=0, ctr_step=1, device=None):
        import torch
        if not torch.cuda.is_available():
            import _p3d
            raise _p3d.P3DError("Dataset needs a ROCm GPU (torch.cuda.is_available() is False); the noise is "
                                "drawn by the HIP path, which has no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        if isinstance(data, torch.Tensor):
            self.data = data.to(device=dev, dtype=torch.float32).contiguous()
        else:
            self.data = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(dev)
        if self.data.dim() != 2:
            raise ValueError("Dataset: data must be [n, d], got %s" % (tuple(self.data.shape),))
        self.metadata = metadata
        self.shape = tuple(self.data.shape)
        self.batch_size = int(batch_size)
        self.batch_step = 0
        self.shuffle = shuffle
        self.indexes = np.arange(self.shape[0])
        self.seed, self.ctr0, self.ctr_step = int(seed), int(ctr0), int(ctr_step)
        self.draws = 0
        self.data_noised = torch.empty_like(self.data)
        self._idx_dev = None
        self._draw()

    def _draw(self):
        add_noise_device(self.data, seed=self.seed, ctr=self.ctr0 + self.draws * self.ctr_step, out=self.data_noised)
        self.draws += 1

    def __len__(self):
        """Batches per epoch (the floor: a short last batch is dropped)."""
        return int(self.shape[0] // self.batch_size)

    def __getitem__(self, index):
        if self._idx_dev is None:       # (the epoch's order on the device, copied once per shuffle)
            import torch
            self._idx_dev = torch.from_numpy(self.indexes).to(self.data.device)
        idxs = self._idx_dev[index * self.batch_size:(index + 1) * self.batch_size]
        return self.data_noised[idxs], self.data[idxs]

    def __iter__(self):
        return self

    def __next__(self):
        if self.batch_step == self.__len__():
            raise StopIteration()
        batch = self.__getitem__(self.batch_step)
        self.batch_step += 1
        return batch

    def on_epoch_end(self, new_noise=False):
        """Reset the iteration, reshuffle the indices and, with new_noise, draw the next noise."""
        self.batch_step = 0
        if self.shuffle is True:
            np.random.shuffle(self.indexes)
            self._idx_dev = None
        if new_noise:
            self._draw()


def join_data(train, test, order_keys_train, order_keys_test):
    """The sets joined in key order, train then test, as float32 (data_handler.py:115-122)."""
    train = np.concatenate([train[key] for key in order_keys_train], axis=0).astype('float32')
    test = np.concatenate([test[key] for key in order_keys_test], axis=0).astype('float32')
    return np.concatenate([train, test], axis=0)


def suffle_and_split(data, suffle_idx, train_size=0.8):
    """Permute the rows and split them train / test (data_handler.py:125-131)."""
    data = data[suffle_idx, :]
    tsize = int(data.shape[0] * train_size)
    return data[:tsize, :], data[tsize:, :]


def split_3d_data(d):
    """The host half of load_3d_data: all 3D poses of `d` (predict_3dpose.load_data's dict) joined in
    key order, permuted with np.random.choice(n, n, replace=False) and split 80/20.  Returns
    (train, test, metadata) with the halves numpy float32 arrays."""
    train_set_3d, test_set_3d = d["train_set_3d"], d["test_set_3d"]
    all_set = join_data(train_set_3d, test_set_3d, list(train_set_3d.keys()), list(test_set_3d.keys()))
    idx = np.random.choice(all_set.shape[0], all_set.shape[0], replace=False)
    train, test = suffle_and_split(all_set, idx)
    meta = Metadata(d["data_mean_3d"], d["data_std_3d"], d["dim_to_ignore_3d"], d["dim_to_use_3d"])
    return train, test, meta


def load_3d_data(d, device=None):
    """The stand-alone denoiser's (train, test) Datasets (data_handler.py:135-163) from
    predict_3dpose.load_data's dict `d`: split_3d_data, then the halves on the device.  The train
    half draws its noise at the even counters (ctr0 = 0), the test half at the odd ones (ctr0 = 1),
    both ctr_step = 2, seed FLAGS.seed."""
    train, test, meta = split_3d_data(d)
    f = ENV.FLAGS
    return (Dataset(train, batch_size=f.batch_size, shuffle=True, metadata=meta, seed=f.seed, ctr0=0, ctr_step=2,
                    device=device),
            Dataset(test, batch_size=f.batch_size, shuffle=True, metadata=meta, seed=f.seed, ctr0=1, ctr_step=2,
                    device=device))


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
