"""The VAE pose filter and the lifter + filter model (src/top_vae_3d_pose/models.py:12-91 VAE,
:485-540 Pose3DVae, :544-573 VAEBones) over libp3d.so's p3d_vae_* entry points (csrc/p3d_vae.h).

The reference's names are kept so that its scripts drop in.  Everything runs on the GPU; there is
no CPU fallback.  tf.random.normal's stream cannot be reproduced: eps comes from the library's
Philox stream (keyed by the model's seed, a call counter, the row and the column), or from the
caller (``eps=``).
"""
from __future__ import annotations

import ctypes

import numpy as np

import _p3d
from _p3d import check, lib, ptr
from top_vae_3d_pose import bones

HUMAN_3D_SIZE = 48
HUMAN_2D_SIZE = 32


class VAE(object):
    """Variational autoencoder input_size -> enc_dim -> {mean, log_varianze} -> dec_dim -> human_3d_size."""

    N_TERMS = 3          # entries of the loss vector and of a row of row_terms
    BONES = False        # VAEBones: the library's bones kind (p3d_vae_create_bones)

    def __init__(self, input_size, latent_dim, enc_dim, dec_dim, human_3d_size=HUMAN_3D_SIZE, *, max_batch=4096,
                 seed=None, device=None, init=True):
        import torch

        self.input_size = int(input_size)
        self.latent_dim = int(latent_dim)
        self.enc_dim = [int(u) for u in enc_dim]
        self.dec_dim = [int(u) for u in dec_dim]
        self.human_3d_size = int(human_3d_size)
        self.max_batch = int(max_batch)
        self.seed = int(seed if seed is not None else np.random.SeedSequence().entropy % (2 ** 63))
        self.torch = torch
        self._h = None
        enc = (ctypes.c_int32 * max(len(self.enc_dim), 1))(*self.enc_dim)
        dec = (ctypes.c_int32 * max(len(self.dec_dim), 1))(*self.dec_dim)
        h = ctypes.c_void_p()
        self.output_size = 64 if self.BONES else self.human_3d_size     # width of y and of a target row
        args = (self.input_size, len(self.enc_dim), enc, self.latent_dim, len(self.dec_dim), dec)
        args += (() if self.BONES else (self.human_3d_size,)) + (self.max_batch, self.seed, ctypes.byref(h))
        create, what = ((lib().p3d_vae_create_bones, "p3d_vae_create_bones") if self.BONES else
                        (lib().p3d_vae_create, "p3d_vae_create"))
        if torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
            with torch.cuda.device(self.device):
                check(create(*args), what)
        else:   # argument errors answer without a GPU; a valid shape then fails on the missing device
            rc = create(*args)
            if rc == _p3d.P3D_ERR_ARG:
                check(rc, what)
            raise _p3d.P3DError("VAE needs a ROCm GPU (torch.cuda.is_available() is False); "
                                "the HIP path has no CPU fallback")
        self._h = h
        n = ctypes.c_int32()
        check(lib().p3d_vae_param_count(self._h, ctypes.byref(n)), "p3d_vae_param_count")
        self.param_table = []   # (name, shape, offset) in keras order
        for i in range(n.value):
            name, numel, rows, cols, off = (ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32(),
                                            ctypes.c_int64())
            check(lib().p3d_vae_param_info(self._h, i, ctypes.byref(name), ctypes.byref(numel), ctypes.byref(rows),
                                           ctypes.byref(cols), ctypes.byref(off)), "p3d_vae_param_info")
            nm = name.value.decode()
            shape = (cols.value,) if nm.endswith("/bias") else (rows.value, cols.value)
            self.param_table.append((nm, shape, off.value))
        self._flat = {}
        self._loss = torch.zeros(self.N_TERMS, dtype=torch.float32, device=self.device)
        self._calls = 0     # eps counter of inference calls
        if init:
            self.initialize(self.seed)

    # ------------------------------------------------------------------ plumbing
    def stream(self):
        return _p3d.stream_handle()

    def flat(self, which):
        """Zero-copy view of a flat device buffer: 'params', 'grads', 'adam_m', 'adam_v',
        'workspace', 'packed'."""
        idx = ("params", "grads", "adam_m", "adam_v", "workspace", "packed").index(which)
        if idx not in self._flat:
            p, n = ctypes.c_void_p(), ctypes.c_int64()
            check(lib().p3d_vae_flat_ptr(self._h, idx, ctypes.byref(p), ctypes.byref(n)), "p3d_vae_flat_ptr")
            self._flat[idx] = _p3d.device_view(p.value, (n.value,), self.device.index)
        return self._flat[idx]

    def _tensors(self, which):
        f = self.flat(which)
        return {n: f[o:o + int(np.prod(s))].view(*s) for n, s, o in self.param_table}

    def variable(self, name):
        return self._tensors("params")[name]

    def grads(self):
        """{keras name: gradient} as numpy arrays (after compute_gradients / a training step)."""
        return {n: t.cpu().numpy() for n, t in self._tensors("grads").items()}

    def slots(self):
        """({name: adam m}, {name: adam v}) as numpy arrays."""
        return ({n: t.cpu().numpy() for n, t in self._tensors("adam_m").items()},
                {n: t.cpu().numpy() for n, t in self._tensors("adam_v").items()})

    def initialize(self, seed=0):
        """Glorot-uniform kernels, zero biases (keras.layers.Dense defaults, models.py:29-49)."""
        rng = np.random.default_rng(seed)
        w = []
        for name, shape, _ in self.param_table:
            if name.endswith("/kernel"):
                lim = np.sqrt(6.0 / (shape[0] + shape[1]))
                w.append(rng.uniform(-lim, lim, shape).astype(np.float32))
            else:
                w.append(np.zeros(shape, np.float32))
        self.set_weights(w)

    def get_weights(self):
        return [t.cpu().numpy() for t in self._tensors("params").values()]

    def set_weights(self, weights):
        if isinstance(weights, dict):
            weights = [weights[n] for n, _, _ in self.param_table]
        if len(weights) != len(self.param_table):
            raise ValueError("set_weights: expected %d arrays, got %d" % (len(self.param_table), len(weights)))
        views = self._tensors("params")
        for (name, shape, _), w in zip(self.param_table, weights):
            w = np.array(w, dtype=np.float32)      # (a writable copy: torch.from_numpy below)
            if tuple(w.shape) != tuple(shape):
                raise ValueError("set_weights: %s expects shape %s, got %s" % (name, shape, w.shape))
            views[name].copy_(self.torch.from_numpy(np.ascontiguousarray(w)))
        check(lib().p3d_vae_params_updated(self._h, self.stream()), "p3d_vae_params_updated")

    def save_weights(self, path):
        np.savez(path if str(path).endswith(".npz") else str(path) + ".npz",
                 **{n: w for (n, _, _), w in zip(self.param_table, self.get_weights())})

    def load_weights(self, path):
        with np.load(path if str(path).endswith(".npz") else str(path) + ".npz", allow_pickle=False) as z:
            self.set_weights({n: z[n] for n, _, _ in self.param_table})

    def get_step(self):
        s, b1, b2 = ctypes.c_int64(), ctypes.c_float(), ctypes.c_float()
        check(lib().p3d_vae_get_step(self._h, ctypes.byref(s), ctypes.byref(b1), ctypes.byref(b2)), "p3d_vae_get_step")
        return s.value, b1.value, b2.value

    def set_step(self, step, b1p=None, b2p=None):
        b1p = np.float32(0.9) ** (step + 1) if b1p is None else b1p
        b2p = np.float32(0.999) ** (step + 1) if b2p is None else b2p
        check(lib().p3d_vae_set_step(self._h, int(step), float(b1p), float(b2p)), "p3d_vae_set_step")

    def set_form(self, form):
        check(lib().p3d_vae_set_form(self._h, int(form)), "p3d_vae_set_form")

    def _dev(self, a, width, what):
        torch = self.torch
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float32, order="C"))
        if t.dim() != 2 or t.shape[1] != width:
            raise ValueError("%s: expected shape [None, %d], got %s" % (what, width, tuple(t.shape)))
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
        return t

    def _cat(self, segs):
        """A list of segments -- each a tensor [B, w] or a (table [rows, w], idx int64 [B]) pair -- as
        the library's p3d_vae_cat; returns (struct, B, the tensors it points into).  Nothing is
        copied: every segment must already be a contiguous float32 tensor on the model's device."""
        torch = self.torch
        if not 1 <= len(segs) <= 4:
            raise ValueError("vae input: 1 to 4 segments, got %d" % len(segs))
        cat, keep, B, total = _p3d.P3DVaeCat(), [], None, 0
        cat.n = len(segs)
        for s, seg in enumerate(segs):
            table, idx = seg if isinstance(seg, (tuple, list)) else (seg, None)
            if not isinstance(table, torch.Tensor) or table.dim() != 2:
                raise ValueError("vae input: segment %d must be a tensor [rows, width]" % s)
            if table.device != self.device or table.dtype != torch.float32 or not table.is_contiguous():
                raise ValueError("vae input: segment %d must be a contiguous float32 tensor on %s (got %s on %s)"
                                 % (s, self.device, table.dtype, table.device))
            rows, w = int(table.shape[0]), int(table.shape[1])
            if w < 8 or w % 8 != 0:
                raise ValueError("vae input: segment %d has width %d, not a multiple of 8" % (s, w))
            if rows < 1:
                raise ValueError("vae input: segment %d has no rows" % s)
            if idx is not None:
                if (not isinstance(idx, torch.Tensor) or idx.dim() != 1 or idx.dtype != torch.int64
                        or idx.device != self.device or not idx.is_contiguous()):
                    raise ValueError("vae input: the index of segment %d must be a contiguous int64 vector on %s"
                                     % (s, self.device))
                n = int(idx.shape[0])
            else:
                n = rows
            if B is None:
                B = n
            elif n != B:
                raise ValueError("vae input: segment %d gives %d rows, segment 0 gives %d" % (s, n, B))
            cat.p[s], cat.w[s], cat.idx[s], cat.rows[s] = ptr(table), w, ptr(idx) or None, rows
            keep += [table, idx]
            total += w
        if total != self.input_size:
            raise ValueError("vae input: the segments' widths sum to %d, the filter takes %d" % (total, self.input_size))
        if B < 1:
            raise ValueError("vae input: no rows")
        check(lib().p3d_vae_cat_check(ctypes.byref(cat), self.input_size, B), "p3d_vae_cat_check")
        return cat, B, keep

    def _factors(self, factors):
        if len(factors) != self.N_TERMS:
            raise ValueError("factors: expected %d values, got %d" % (self.N_TERMS, len(factors)))
        return (ctypes.c_float * self.N_TERMS)(*[float(f) for f in factors])

    # ------------------------------------------------------------------ device entry points
    MAX_SAMPLES = 64     # the library's bound on K

    def _samples(self, samples, what):
        if self.BONES:
            raise NotImplementedError("%s: a bones filter's outputs are lengths and direction cosines, and direction "
                                      "cosines do not average (samples is not served)" % what)
        K = int(samples)
        if K != samples or not 1 <= K <= self.MAX_SAMPLES:
            raise ValueError("%s: samples must be an integer in 1 .. %d, got %r" % (what, self.MAX_SAMPLES, samples))
        return K

    def _eps_k(self, eps, K, rows):
        """The caller's K draws as one contiguous [K, rows, latent] device tensor."""
        torch = self.torch
        t = eps if isinstance(eps, torch.Tensor) else torch.from_numpy(np.array(eps, dtype=np.float32, order="C"))
        if tuple(t.shape) != (K, rows, self.latent_dim):
            raise ValueError("eps: expected shape [%d, %d, %d], got %s" % (K, rows, self.latent_dim, tuple(t.shape)))
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
        return t

    def _forward_mc(self, x, K, eps, ctr, want):
        """One k_vae_fwd_mc launch: the mean ('y') and, if asked, the variance ('y_var') of K samples."""
        torch = self.torch
        widths = {"y": self.output_size, "y_var": self.output_size, "mean": self.latent_dim, "log_var": self.latent_dim}
        unknown = [k for k in want if k not in widths]
        if unknown:
            raise ValueError("forward_device: with samples the outputs are 'y', 'y_var', 'mean' and 'log_var', not %s"
                             % unknown)
        cat = None
        if isinstance(x, list):
            cat, B, _keep = self._cat(x)
        else:
            x = self._dev(x, self.input_size, "vae input")
            B = x.shape[0]
        eps = None if eps is None else self._eps_k(eps, K, B)
        out = {k: torch.empty((B, widths[k]), dtype=torch.float32, device=self.device) for k in want}
        y = out["y"] if "y" in out else torch.empty((B, self.output_size), dtype=torch.float32, device=self.device)
        fn, what, xin = ((lib().p3d_vae_forward_mc, "p3d_vae_forward_mc", ptr(x)) if cat is None else
                         (lib().p3d_vae_forward_mc_cat, "p3d_vae_forward_mc_cat", ctypes.byref(cat)))
        check(fn(self._h, xin, B, K, ptr(eps), int(ctr), ptr(y), ptr(out.get("y_var")), ptr(out.get("mean")),
                 ptr(out.get("log_var")), self.stream()), what)
        return out

    def forward_device(self, x, eps=None, ctr=0, target=None, want=("y",), samples=None):
        """One k_vae_fwd launch; returns a dict with the tensors named in `want` out of 'y',
        'mean', 'log_var', 'z' and, with a target, 'row_terms' [B, 3].

        samples=K (1 .. 64): one k_vae_fwd_mc launch that runs the encoder once and the decoder on K
        draws; 'y' is the mean of the K outputs and `want` may name 'y_var' (their variance),
        'mean' and 'log_var'.  eps is [K, B, latent]; without it draw k is the library's stream at
        counter ctr + k.  'z' and a target are not served with samples."""
        torch = self.torch
        if samples is not None:
            K = self._samples(samples, "forward_device")
            if target is not None or "z" in want:
                raise ValueError("forward_device: with samples there is no single z and no loss term "
                                 "('z' and target are not served)")
            return self._forward_mc(x, K, eps, ctr, want)
        cat = None
        if isinstance(x, list):     # [seg, ...]: the concatenation is formed inside the kernels
            cat, B, _keep = self._cat(x)
        else:
            x = self._dev(x, self.input_size, "vae input")
            B = x.shape[0]
        eps = None if eps is None else self._dev(eps, self.latent_dim, "eps")
        if eps is not None and eps.shape[0] != B:
            raise ValueError("eps: expected %d rows, got %d" % (B, eps.shape[0]))
        target = None if target is None else self._dev(target, self.output_size, "target")
        if target is not None and target.shape[0] != B:
            raise ValueError("target: expected %d rows, got %d" % (B, target.shape[0]))
        widths = {"y": self.output_size, "mean": self.latent_dim, "log_var": self.latent_dim, "z": self.latent_dim}
        out = {k: torch.empty((B, widths[k]), dtype=torch.float32, device=self.device) for k in want if k in widths}
        if target is not None:
            out["row_terms"] = torch.empty((B, self.N_TERMS), dtype=torch.float32, device=self.device)
        fn, what, xin = ((lib().p3d_vae_forward, "p3d_vae_forward", ptr(x)) if cat is None else
                         (lib().p3d_vae_forward_cat, "p3d_vae_forward_cat", ctypes.byref(cat)))
        check(fn(self._h, xin, B, ptr(eps), int(ctr), ptr(out.get("y")), ptr(out.get("mean")),
                 ptr(out.get("log_var")), ptr(out.get("z")), ptr(target), ptr(out.get("row_terms")),
                 self.stream()), what)
        return out

    def _step(self, fn, what, x, t, eps, middle, loss_out=None):
        """`middle`: the arguments between eps and loss3_dev (ctr, factors | factors, lr).  A list in
        place of x (segments, see _cat) goes to the call's _cat twin."""
        if isinstance(x, list):
            cat, B, _keep = self._cat(x)
            fn, what, xin = getattr(lib(), what + "_cat"), what + "_cat", ctypes.byref(cat)
        else:
            x = self._dev(x, self.input_size, "vae input")
            B, xin = x.shape[0], ptr(x)
        t = self._dev(t, self.output_size, "target")
        if t.shape[0] != B:
            raise ValueError("target: expected %d rows, got %d" % (B, t.shape[0]))
        eps = None if eps is None else self._dev(eps, self.latent_dim, "eps")
        if eps is not None and eps.shape[0] != B:
            raise ValueError("eps: expected %d rows, got %d" % (B, eps.shape[0]))
        loss = self._loss if loss_out is None else loss_out
        if loss_out is not None and int(loss_out.numel()) < self.N_TERMS:
            raise ValueError("loss_out: expected room for %d floats" % self.N_TERMS)
        check(fn(self._h, xin, ptr(t), B, ptr(eps), *middle, ptr(loss), self.stream()), what)
        return loss

    def loss_device(self, x, t, factors, eps=None, ctr=0, loss_out=None):
        """ELBO.compute_loss: the device 3-vector [like, kcs, dkl]."""
        return self._step(lib().p3d_vae_loss, "p3d_vae_loss", x, t, eps, (int(ctr), self._factors(factors)), loss_out)

    def compute_gradients(self, x, t, factors, eps=None, ctr=0, loss_out=None):
        """Loss and tape.gradient of the three terms' sum into the gradient buffer (no optimizer)."""
        return self._step(lib().p3d_vae_grad, "p3d_vae_grad", x, t, eps, (int(ctr), self._factors(factors)), loss_out)

    def train_step_device(self, x, t, factors, lr, eps=None, loss_out=None):
        """Loss, gradient and Keras Adam; one launch at B <= 64.  Capturable."""
        return self._step(lib().p3d_vae_train_step, "p3d_vae_train_step", x, t, eps,
                          (self._factors(factors), float(lr)), loss_out)

    def adam_apply(self, lr):
        check(lib().p3d_vae_adam_apply(self._h, float(lr), self.stream()), "p3d_vae_adam_apply")

    def eps_device(self, B, ctr=0, row0=0):
        out = self.torch.empty((B, self.latent_dim), dtype=self.torch.float32, device=self.device)
        check(lib().p3d_vae_eps(self.seed, int(ctr), int(row0), B, self.latent_dim, ptr(out), self.stream()),
              "p3d_vae_eps")
        return out

    # ------------------------------------------------------------------ the recurrence over sequences
    def _seq_len(self):
        if self.BONES:
            raise ValueError("filter_sequences: a bones filter has no sequence form")
        if self.input_size > 256:
            raise ValueError("filter_sequences: a wide filter (input_size %d > 256) has no sequence form"
                             % self.input_size)
        if self.input_size % self.human_3d_size != 0 or not 1 <= self.input_size // self.human_3d_size <= 5:
            raise ValueError("filter_sequences: input_size %d is not 1 .. 5 times human_3d_size %d"
                             % (self.input_size, self.human_3d_size))
        return self.input_size // self.human_3d_size

    SEQ_FORM_DEFAULT = 1   # the library's default, by measurement (MEASUREMENTS.md)

    def set_seq_form(self, form):
        """0: one wave per 16-sequence tile; 1 (the default): four waves per tile.  Same bits either way."""
        check(lib().p3d_vae_seq_set_form(self._h, int(form)), "p3d_vae_seq_set_form")

    def new_seq_state(self, S):
        """The zeroed (state [S, (seq_len - 1) * out], started [S]) pair that carries filter_sequences'
        buffer from one chunk of a stream to the next."""
        torch = self.torch
        w = (self._seq_len() - 1) * self.human_3d_size
        return (torch.zeros((int(S), w), dtype=torch.float32, device=self.device),
                torch.zeros((int(S),), dtype=torch.int32, device=self.device))

    def filter_sequences(self, pred, seq_off, eps=None, ctr=None, eps_row0=0, target=None, state=None,
                         want=("ref",), samples=None):
        """The temporal filter run as the reference's evaluate() recurrence over whole sequences in
        one k_vae_seq launch: frame f's refined pose feeds the windows of the next seq_len - 1.

        pred [N, out] holds the lifter's outputs with the sequences concatenated, seq_off [S + 1]
        their first frames (seq_off[0] = 0, seq_off[S] = N; empty sequences are legal).  A host
        seq_off (list, numpy, CPU tensor) is checked and uploaded; a device tensor is taken as it is,
        without a host round trip (the kernel clamps it into [0, N]), so the call stays capturable.
        eps [N, latent], or None for the library's Philox stream at (ctr, eps_row0 + frame index);
        ctr=None draws a fresh counter.  state is a new_seq_state() pair, updated in place.
        Returns a dict with the entries of `want` out of 'ref' [N, out], 'frame_err' [N, 2]
        {err_pred, err_ref} and 'seq_err' [S, 2] (float64); the last two need a target.

        samples=K (1 .. 64): one k_vae_seq4_mc launch in which frame f's refined pose is the mean of
        K samples (forward_device's samples) and that mean is what feeds the next windows; `want`
        may add 'ref_var' [N, out], eps is [K, N, latent], and without eps draw k uses counter
        ctr + k (a fresh ctr advances the call counter by K)."""
        torch = self.torch
        self._seq_len()
        K = None if samples is None else self._samples(samples, "filter_sequences")
        pred = self._dev(pred, self.human_3d_size, "pred")
        N = pred.shape[0]
        if isinstance(seq_off, torch.Tensor) and seq_off.is_cuda:
            off = seq_off
            if off.dim() != 1 or off.dtype != torch.int64 or off.shape[0] < 2 or not off.is_contiguous():
                raise ValueError("seq_off: expected a contiguous int64 vector [S + 1], got %s %s"
                                 % (off.dtype, tuple(off.shape)))
            if off.device != self.device:
                off = off.to(self.device)
        else:
            h = np.asarray(seq_off.numpy() if isinstance(seq_off, torch.Tensor) else seq_off)
            if h.ndim != 1 or h.shape[0] < 2 or not np.issubdtype(h.dtype, np.integer):
                raise ValueError("seq_off: expected an integer vector [S + 1], got %s %s" % (h.dtype, h.shape))
            h = h.astype(np.int64)
            if h[0] != 0 or h[-1] != N or (np.diff(h) < 0).any():
                raise ValueError("seq_off: offsets must start at 0, not decrease and end at N = %d (got %d .. %d)"
                                 % (N, h[0], h[-1]))
            off = torch.from_numpy(h).to(self.device)
        S = off.shape[0] - 1
        if K is not None:
            eps = None if eps is None else self._eps_k(eps, K, N)
        else:
            eps = None if eps is None else self._dev(eps, self.latent_dim, "eps")
        if K is None and eps is not None and eps.shape[0] != N:
            raise ValueError("eps: expected %d rows, got %d" % (N, eps.shape[0]))
        target = None if target is None else self._dev(target, self.human_3d_size, "target")
        if target is not None and target.shape[0] != N:
            raise ValueError("target: expected %d rows, got %d" % (N, target.shape[0]))
        unknown = [k for k in want if k not in ("ref", "frame_err", "seq_err") + (("ref_var",) if K else ())]
        if unknown:
            raise ValueError("filter_sequences: unknown outputs %s" % unknown)
        if target is None and ("frame_err" in want or "seq_err" in want):
            raise ValueError("filter_sequences: frame_err and seq_err need a target")
        st, started = (None, None) if state is None else state
        if state is not None:
            w = (self._seq_len() - 1) * self.human_3d_size
            if (tuple(st.shape) != (S, w) or tuple(started.shape) != (S,) or st.dtype != torch.float32
                    or started.dtype != torch.int32 or st.device != self.device or started.device != self.device
                    or not st.is_contiguous() or not started.is_contiguous()):
                raise ValueError("state: expected the (float32 [%d, %d], int32 [%d]) pair of new_seq_state" % (S, w, S))
        if ctr is None:
            ctr = self._calls + 1
            self._calls += K or 1
        out = {"ref": torch.empty((N, self.human_3d_size), dtype=torch.float32, device=self.device)}
        if "ref_var" in want:
            out["ref_var"] = torch.empty((N, self.human_3d_size), dtype=torch.float32, device=self.device)
        if "frame_err" in want:
            out["frame_err"] = torch.empty((N, 2), dtype=torch.float32, device=self.device)
        if "seq_err" in want:
            out["seq_err"] = torch.empty((S, 2), dtype=torch.float64, device=self.device)
        if N == 0:
            if "seq_err" in out:
                out["seq_err"].zero_()
        elif K is not None:
            check(lib().p3d_vae_seq_filter_mc(self._h, ptr(pred), ptr(off), S, N, K, ptr(eps), int(ctr), int(eps_row0),
                                              ptr(target), ptr(st), ptr(started), ptr(out["ref"]),
                                              ptr(out.get("ref_var")), ptr(out.get("frame_err")),
                                              ptr(out.get("seq_err")), self.stream()), "p3d_vae_seq_filter_mc")
        else:
            check(lib().p3d_vae_seq_filter(self._h, ptr(pred), ptr(off), S, N, ptr(eps), int(ctr), int(eps_row0),
                                           ptr(target), ptr(st), ptr(started), ptr(out["ref"]),
                                           ptr(out.get("frame_err")), ptr(out.get("seq_err")), self.stream()),
                  "p3d_vae_seq_filter")
        return {k: out[k] for k in want}

    # ------------------------------------------------------------------ the reference's interface
    def encode(self, x):
        """mean and log variance of Q(z|x) (models.py:62-65)."""
        o = self.forward_device(x, eps=self.torch.zeros((len(x), self.latent_dim), device=self.device),
                                want=("mean", "log_var"))
        return o["mean"], o["log_var"]

    def reparametrize(self, mean, log_var):
        """eps exp(0.5 log_var) + mean with eps from the library's stream (models.py:68-71)."""
        self._calls += 1
        eps = self.eps_device(mean.shape[0], ctr=self._calls)
        return eps * self.torch.exp(log_var * 0.5) + mean

    MAX_LAUNCH_ROWS = 1 << 20   # the library's bound on one call's rows

    def decode(self, z):
        """The decoder alone (models.py:74-76): y [B, out] from z [B, latent] in one k_vae_dec launch,
        bit-identical to the y forward_device gives for the same z."""
        z = self._dev(z, self.latent_dim, "z")
        B = z.shape[0]
        y = self.torch.empty((B, self.output_size), dtype=self.torch.float32, device=self.device)
        check(lib().p3d_vae_decode(self._h, ptr(z), B, 0, 0, ptr(y), None, self.stream()), "p3d_vae_decode")
        return y

    def sample(self, n, ctr=0, row0=0, want=("y",)):
        """n poses from the prior: z ~ N(0, I) drawn inside the decoder's launch from the library's
        prior stream (keyed by the model's seed, ctr, the global row row0 + r and the column) and
        decoded, with no input tensor.  Returns a dict with 'y' [n, out] and, if asked, 'z'
        [n, latent].  More than 2^20 rows go out as several launches with row0 advanced: the
        stream is keyed by the global row, so the split does not show."""
        torch = self.torch
        n, row0 = int(n), int(row0)
        if n < 1:
            raise ValueError("sample: n must be at least 1, got %d" % n)
        unknown = [k for k in want if k not in ("y", "z")]
        if unknown:
            raise ValueError("sample: unknown outputs %s" % unknown)
        y = torch.empty((n, self.output_size), dtype=torch.float32, device=self.device)
        z = torch.empty((n, self.latent_dim), dtype=torch.float32, device=self.device) if "z" in want else None
        for r in range(0, n, self.MAX_LAUNCH_ROWS):
            b = min(self.MAX_LAUNCH_ROWS, n - r)
            check(lib().p3d_vae_decode(self._h, None, b, int(ctr), row0 + r, ptr(y[r:r + b]),
                                       None if z is None else ptr(z[r:r + b]), self.stream()), "p3d_vae_decode")
        out = {"y": y}
        if z is not None:
            out["z"] = z
        return out

    def set_dec_grid(self, wgs_per_cu):
        """Workgroups of the decoder's launch per CU (0: the library's default).  Same bits either way."""
        check(lib().p3d_vae_dec_set_grid(self._h, int(wgs_per_cu)), "p3d_vae_dec_set_grid")

    def __call__(self, inputs, training=False, eps=None, samples=None):
        """samples=K: the mean of K posterior samples (forward_device); the call counter advances by K."""
        if samples is not None:
            K = self._samples(samples, type(self).__name__)
            ctr = self._calls + 1
            self._calls += K
            return self.forward_device(inputs, eps=eps, ctr=ctr, samples=K)["y"]
        self._calls += 1
        return self.forward_device(inputs, eps=eps, ctr=self._calls)["y"]

    def get_config(self):
        return {"input_size": self.input_size, "latent_dim": self.latent_dim, "enc_dim": self.enc_dim,
                "dec_dim": self.dec_dim, "human_3d_size": self.human_3d_size}

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._flat.clear()
            lib().p3d_vae_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VAEBones(VAE):
    """Variational autoencoder for bones (models.py:544-573): the decoder ends dec_dim -> mag1 (16,
    ReLU) -> {mag2 (16), cos2 (48)}.  The device output is one [B, 64] tensor [mag | cos]
    (forward_device's 'y', a target row, bones.convert_to_bones's result); calling the model returns
    the (mag, cos) views of it.  Loss vectors are [MAG, COS, DKL, ANG] under factors (mag, cos, dkl,
    ang) (losses.py:113-156).  The reference's layer 'cos1' feeds nothing and is not built."""

    N_TERMS = 4
    BONES = True

    def __init__(self, input_size, latent_dim, enc_dim, dec_dim, human_3d_size=HUMAN_3D_SIZE, **kw):
        if int(human_3d_size) != HUMAN_3D_SIZE:
            raise ValueError("VAEBones: human_3d_size must be %d (16 bones), got %s" % (HUMAN_3D_SIZE, human_3d_size))
        super(VAEBones, self).__init__(input_size, latent_dim, enc_dim, dec_dim, human_3d_size, **kw)

    def __call__(self, inputs, training=False, eps=None, samples=None):
        if samples is not None:
            self._samples(samples, "VAEBones")      # raises NotImplementedError
        self._calls += 1
        y = self.forward_device(inputs, eps=eps, ctr=self._calls)["y"]
        return y[:, :16], y[:, 16:]

    def decode(self, z):
        """(mag, cos) views of the decoder's [B, 64] output; bones.convert_to_joints turns them into joints."""
        y = super(VAEBones, self).decode(z)
        return y[:, :16], y[:, 16:]

    def sample(self, n, ctr=0, row0=0, want=("y",)):
        """VAE.sample with 'y' as the (mag, cos) views of one [n, 64] tensor."""
        out = super(VAEBones, self).sample(n, ctr=ctr, row0=row0, want=want)
        out["y"] = (out["y"][:, :16], out["y"][:, 16:])
        return out


class Pose3DVae(object):
    """The frozen lifter + the VAE filter (models.py:485-540): call(x2d) -> (out_3d, out_vae), both
    on the device with no host round trip between p3d_serve and p3d_vae_forward."""

    def __init__(self, latent_dim, enc_dim, dec_dim, use_effnet_ouptut=False, use_2d=False, pred_bones=False, *,
                 pose3d=None, max_batch=4096, seed=None):
        if use_2d:
            raise NotImplementedError("Pose3DVae(use_2d=True) is served by Pose3DVaeCat (the filter over [x2d, out_3d])")
        if use_effnet_ouptut:
            raise NotImplementedError("Pose3DVae(use_effnet_ouptut=True) is served by Pose3DVaeCat (precomputed "
                                      "EfficientNet features as a segment of the filter's input)")
        if pred_bones:
            raise NotImplementedError("Pose3DVae(pred_bones=True) is served by Pose3DVaeBones (VAEBones)")
        if pose3d is None:
            raise ValueError("Pose3DVae needs the lifter: pass pose3d=LinearModel(...) (the reference builds its "
                             "PoseBase here; this package's lifter is linear_model.LinearModel)")
        self.use_2d, self.use_effnet_ouptut, self.pred_bones = False, False, False
        self.human_3d_size, self.human_2d_size = HUMAN_3D_SIZE, HUMAN_2D_SIZE
        if pose3d.output_size != HUMAN_3D_SIZE:
            raise ValueError("Pose3DVae: the lifter must predict %d outputs, not %d" % (HUMAN_3D_SIZE, pose3d.output_size))
        self.pose3d = pose3d
        self.vae = VAE(HUMAN_3D_SIZE, latent_dim, enc_dim, dec_dim, max_batch=max_batch, seed=seed,
                       device=pose3d.device.index)

    def __call__(self, inputs, effnet_output=None, training=False, eps=None, samples=None):
        if effnet_output is not None:
            raise NotImplementedError("Pose3DVae: effnet_output is taken by Pose3DVaeCat")
        out_3d = self.pose3d.serve_device(inputs)      # raises ValueError on a bad shape
        if samples is not None:
            return out_3d, self.vae(out_3d, training=training, eps=eps, samples=samples)
        return out_3d, self.vae(out_3d, training=training, eps=eps)

    def save_weights(self, path):
        self.vae.save_weights(path)

    def load_weights(self, path):
        self.vae.load_weights(path)

    def close(self):
        self.vae.close()


class Pose3DVaeCat(object):
    """The frozen lifter + the VAE filter over a concatenated input (models.py:485-540 built with
    use_2d and / or use_effnet_ouptut): call(x2d, effnet_output) -> (out_3d, out_vae).  The filter's
    input is [inputs, out_3d] (use_2d), then effnet_output (models.py:532-536); the concatenation is
    formed inside the filter's kernels.  effnet_output is a [B, effnet_size] tensor or a (table,
    idx) pair: row r reads table[idx[r]] -- the precomputed features of data_handler.py:325-340."""

    def __init__(self, latent_dim, enc_dim, dec_dim, use_effnet_ouptut=False, use_2d=False, pred_bones=False, *,
                 pose3d=None, effnet_size=1280, max_batch=4096, seed=None):
        if pred_bones:
            raise NotImplementedError("Pose3DVaeCat(pred_bones=True) is served by Pose3DVaeBones (VAEBones)")
        if pose3d is None:
            raise ValueError("Pose3DVaeCat needs the lifter: pass pose3d=LinearModel(...)")
        if pose3d.output_size != HUMAN_3D_SIZE:
            raise ValueError("Pose3DVaeCat: the lifter must predict %d outputs, not %d"
                             % (HUMAN_3D_SIZE, pose3d.output_size))
        self.use_2d, self.use_effnet_ouptut, self.pred_bones = bool(use_2d), bool(use_effnet_ouptut), False
        self.human_3d_size, self.human_2d_size = HUMAN_3D_SIZE, HUMAN_2D_SIZE
        self.effnet_size = int(effnet_size)
        self.pose3d = pose3d
        self.input_size = (HUMAN_2D_SIZE if use_2d else 0) + HUMAN_3D_SIZE + (self.effnet_size if use_effnet_ouptut else 0)
        self.vae = VAE(self.input_size, latent_dim, enc_dim, dec_dim, max_batch=max_batch, seed=seed,
                       device=pose3d.device.index)

    def segments(self, inputs, out_3d, effnet_output=None):
        """The filter's input as the list of segments VAE's device entry points take."""
        torch = self.vae.torch
        B = int(out_3d.shape[0])
        segs = [inputs, out_3d] if self.use_2d else [out_3d]
        if self.use_effnet_ouptut:
            if effnet_output is None:
                raise ValueError("%s: this model was built with use_effnet_ouptut: pass effnet_output"
                                 % type(self).__name__)
            table, idx = effnet_output if isinstance(effnet_output, (tuple, list)) else (effnet_output, None)
            if not isinstance(table, torch.Tensor):
                table = torch.from_numpy(np.array(table, dtype=np.float32, order="C")).to(self.vae.device)
            if table.dim() != 2 or table.shape[1] != self.effnet_size:
                raise ValueError("effnet_output: expected shape [None, %d], got %s" % (self.effnet_size, tuple(table.shape)))
            n = int(table.shape[0]) if idx is None else int(idx.shape[0])
            if n != B:
                raise ValueError("effnet_output: expected %d rows, got %d" % (B, n))
            segs.append(table if idx is None else (table, idx))
        elif effnet_output is not None:
            raise ValueError("%s: effnet_output given to a model built without use_effnet_ouptut" % type(self).__name__)
        return segs

    def __call__(self, inputs, effnet_output=None, training=False, eps=None, samples=None):
        torch = self.vae.torch
        if not isinstance(inputs, torch.Tensor):
            inputs = torch.from_numpy(np.array(inputs, dtype=np.float32, order="C"))
        inputs = inputs.to(device=self.vae.device, dtype=torch.float32).contiguous()
        out_3d = self.pose3d.serve_device(inputs)      # raises ValueError on a bad shape
        if samples is not None:
            return out_3d, self.vae(self.segments(inputs, out_3d, effnet_output), training=training, eps=eps,
                                    samples=samples)
        self.vae._calls += 1
        y = self.vae.forward_device(self.segments(inputs, out_3d, effnet_output), eps=eps, ctr=self.vae._calls)["y"]
        return out_3d, y

    def save_weights(self, path):
        self.vae.save_weights(path)

    def load_weights(self, path):
        self.vae.load_weights(path)

    def close(self):
        self.vae.close()


class Pose3DVaeBones(object):
    """The frozen lifter + the bones filter (models.py:485-540 built with pred_bones):
    call(x2d, effnet_output) -> (out_3d, (mag, cos)).  The filter's input is
    [inputs?] | bones(out_3d) | [effnet_output?] (models.py:528-536), the bones 16 lengths and 48
    direction cosines (models.py:495-502); the concatenation is formed inside the filter's kernels.
    The call converts with the float64 arithmetic of bones.convert_to_bones (models.py:529);
    bones_tf() is the float32 form of the training step (pose_3d_bones.py:162-165)."""

    def __init__(self, latent_dim, enc_dim, dec_dim, use_effnet_ouptut=False, use_2d=False, *, pose3d=None,
                 effnet_size=1280, max_batch=4096, seed=None):
        if pose3d is None:
            raise ValueError("Pose3DVaeBones needs the lifter: pass pose3d=LinearModel(...)")
        if pose3d.output_size != HUMAN_3D_SIZE:
            raise ValueError("Pose3DVaeBones: the lifter must predict %d outputs, not %d"
                             % (HUMAN_3D_SIZE, pose3d.output_size))
        self.use_2d, self.use_effnet_ouptut, self.pred_bones = bool(use_2d), bool(use_effnet_ouptut), True
        self.human_3d_size, self.human_2d_size = HUMAN_3D_SIZE, HUMAN_2D_SIZE
        self.effnet_size = int(effnet_size)
        self.pose3d = pose3d
        self.bones_joints = bones.get_bones_joints()
        self.input_size = (HUMAN_2D_SIZE if use_2d else 0) + 64 + (self.effnet_size if use_effnet_ouptut else 0)
        self.vae = VAEBones(self.input_size, latent_dim, enc_dim, dec_dim, max_batch=max_batch, seed=seed,
                            device=pose3d.device.index)

    segments = Pose3DVaeCat.segments      # (the middle segment is the bones tensor)

    def bones_tf(self, out_3d, out=None):
        """The lifter's output as bones in float32 arithmetic (convert_to_bones_tf), one launch."""
        return bones.convert_to_bones(out_3d, precise=False, out=out)

    def __call__(self, inputs, effnet_output=None, training=False, eps=None, samples=None):
        torch = self.vae.torch
        if samples is not None:
            self.vae._samples(samples, "Pose3DVaeBones")      # raises NotImplementedError
        if not isinstance(inputs, torch.Tensor):
            inputs = torch.from_numpy(np.array(inputs, dtype=np.float32, order="C"))
        inputs = inputs.to(device=self.vae.device, dtype=torch.float32).contiguous()
        out_3d = self.pose3d.serve_device(inputs)      # raises ValueError on a bad shape
        b64 = bones.convert_to_bones(out_3d, self.bones_joints, precise=True)
        self.vae._calls += 1
        y = self.vae.forward_device(self.segments(inputs, b64, effnet_output), eps=eps, ctr=self.vae._calls)["y"]
        return out_3d, (y[:, :16], y[:, 16:])

    def save_weights(self, path):
        self.vae.save_weights(path)

    def load_weights(self, path):
        self.vae.load_weights(path)

    def close(self):
        self.vae.close()
