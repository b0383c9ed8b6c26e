"""Model shapes the create calls accept beyond the benchmark's: the shared tables, the integer cases
built on them, and the launch forms the library is expected to pick for each (no GPU needed).

The lifter (p3d_create) takes any linear_size % 64 == 0 and up to P3D_MAX_W = 40 layers; the VAE filter
(p3d_vae_create) 1-4 hidden layers per side, widths 8..256, latent and out 8..64, within 163,840 B of
LDS.  Every entry below sits on one side of a threshold at which csrc/p3d.hip selects another kernel
or launch form; tests/test_shape_cases_oracle.py proves on the CPU that the integer cases are exact
and that none of them is blind to a dropped k-group, tests/test_gpu_shapes.py and
tests/test_gpu_vae_shapes.py run them on the device.

expected_forward_tags / expected_backward_tags / serve_expected restate the dispatch conditions of
csrc/p3d.hip (forward_gemv, use_big, out_part_ok, use_xchg, p3d_backward's `multi`, serve_shape_error)
in the tags p3d_profile_start / p3d_profile_stop report.  vae_layout_bytes restates the size formula
of vae_layout (csrc/p3d_vae_layout.h), vae_layout_index vae_plan's three tries.
"""
import numpy as np

import exact_models
import vae_exact
from oracle import ref_mlp

# ---- the lifter -------------------------------------------------------------------------------
# name -> (L, N, residual, batch_norm, nnz, why).  nnz: non-zeros per weight column of the integer
# model; with 8 the 7- and 8-block models leave float32's exact range (5e8 and 5e9), with 2 they stay
# inside (3.9e5); five blocks at L = 256 reach 8.4e6 with 8 -- the limit itself -- and 3.5e5 with 4.
LIFTER_SHAPES = {
    "L64_N0": (64, 0, True, True, 8, "no hidden layer: training takes the fused-MSE output layer, not k_out_part; "
                                     "4 k-groups under 8 / 16 waves"),
    "L64_N1": (64, 1, True, True, 8, "smallest block; k_out_part with 4 k-groups over 8 K-splits"),
    "L128_N3": (128, 3, True, True, 8, "three blocks in training; smallest width p3d_serve takes"),
    "L192_N2": (192, 2, False, True, 8, "L % 128 != 0: serve refused, no large-M GEMM; 12 k-groups"),
    "L320_N1": (320, 1, True, False, 8, "L % 128 != 0; 20 column tiles (grid.x % 8 != 0: no sibling remap)"),
    "L256_N4": (256, 4, True, True, 8, "8 hidden layers: last shape of the batch <= 4 chain (P3D_GEMV_CHAIN_MAXH)"),
    "L256_N5": (256, 5, True, True, 4, "10 hidden layers: first shape past the chain"),
    "L128_N7": (128, 7, True, True, 2, "16 layers: last shape of wgrad_multi (P3D_WG_MULTI) and of p3d_serve"),
    "L128_N8": (128, 8, True, True, 2, "18 layers: per-layer k_wgrad, no fused tail, serve refused"),
    "L2112_N1": (2112, 1, True, True, 8, "past P3D_GEMV_CHAIN_MAXK = 2048; L % 128 != 0"),
    "L4160_N1": (4160, 1, True, True, 8, "past P3D_GEMV_FOLD_MAXK = 4096: plain k_gemv launches"),
}
GEMV_CHAIN_MAXH, GEMV_CHAIN_MAXK, GEMV_FOLD_MAXK = 8, 2048, 4096   # csrc/p3d_gemv.h
BIG_M, GEMV_MAXB, XCHG_MAXR, WG_MULTI, SERVE_MAXL = 256, 4, 16, 16, 16
REF_CUS = 256                                    # an MI355X's compute units

FORWARD_BATCHES = (1, 4, 5, 37, 64, 65, 300)     # k_gemv | per-layer k_fwd | k_gemm_f32 where L % 128 == 0
FORWARD_BATCHES_4160 = (1, 4, 64)
SERVE_BATCHES = (64, 64 * 20 + 5, 64 * 33 + 1)
ORACLE_BATCHES = (37, 300)
TRAIN_BATCHES = (17, 64)
XCHG_EDGE_BATCHES = (256, 257)                   # L64_N1: 16 row tiles (exchange) against 17 (split form)
ROW0_CASE = ("L128_N3", 64, 0.5, 192)            # a data-parallel rank's row offset in the mask key
TRAIN_KEEP = 0.5


def forward_batches(name):
    return FORWARD_BATCHES_4160 if LIFTER_SHAPES[name][0] == 4160 else FORWARD_BATCHES


def train_names():
    """The entries that train on the device (L = 2112 and 4160 are forward only)."""
    return [n for n, s in LIFTER_SHAPES.items() if s[0] <= 320]


def backward_nnz(name):
    """Non-zeros per column of the no-BN training twin: 8 up to three blocks, 2 beyond (with 8 the
    deeper twins' contractions leave float32's exact range; exact_backward asserts the pairing)."""
    return 8 if LIFTER_SHAPES[name][1] <= 3 else 2


def backward_runs():
    """Every (name, B, keep, row0) the bit-exact training test runs."""
    runs = [(n, B, TRAIN_KEEP, 0) for n in train_names() for B in TRAIN_BATCHES]
    runs += [("L64_N1", B, TRAIN_KEEP, 0) for B in XCHG_EDGE_BATCHES]
    runs.append(ROW0_CASE)
    return runs


def bn_runs():
    """Every (name, B) of the BN training test against the float64 oracle: up to three blocks at
    both batches, the deeper ones at 64, and both sides of the exchange's 16 row tiles."""
    runs = [(n, B) for n in train_names() for B in TRAIN_BATCHES if LIFTER_SHAPES[n][1] <= 3 or B == 64]
    return runs + [("L64_N1", B) for B in XCHG_EDGE_BATCHES]


def lifter_cfg(name, batch_norm=None):
    L, N, residual, bn, _, _ = LIFTER_SHAPES[name]
    return ref_mlp.Cfg(linear_size=L, num_layers=N, residual=residual, batch_norm=bn if batch_norm is None else batch_norm)


_exact, _backward = {}, {}


def lifter_exact_case(name, B):
    """(cfg, st, x, out) of the integer model of LIFTER_SHAPES[name] at batch B, proven exact by
    exact_models.exact_forward; computed once per process and shared (read-only arrays)."""
    if (name, B) not in _exact:
        L, N, residual, bn, nnz, _ = LIFTER_SHAPES[name]
        cfg, st = exact_models.integer_state(L, N, nnz=nnz, residual=residual, batch_norm=bn)
        x = exact_models.integer_inputs(B, seed=700 + B)
        out = exact_models.exact_forward(st, x)
        for a in (x, out):
            a.setflags(write=False)
        _exact[(name, B)] = (cfg, st, x, out)
    return _exact[(name, B)]


def lifter_backward_case(name, B, keep=TRAIN_KEEP, row0=0):
    """(cfg, st, x, dy, keep, row0, out, grads) of the entry's twin without BN, proven exact by
    exact_models.exact_backward (the layout of exact_models.backward_case); computed once."""
    key = (name, B, keep, row0)
    if key not in _backward:
        L, N, residual, _, _, _ = LIFTER_SHAPES[name]
        cfg, st = exact_models.integer_state(L, N, nnz=backward_nnz(name), residual=residual, batch_norm=False)
        x = exact_models.integer_inputs(B, seed=300 + B)
        dy = exact_models.integer_dy(B, cfg.output_size, seed=400 + B)
        out, grads = exact_models.exact_backward(st, x, dy, keep, exact_models.BACKWARD_SEED, exact_models.BACKWARD_CTR, row0)
        for a in [x, dy, out, *grads.values()]:
            a.setflags(write=False)
        _backward[key] = (cfg, st, x, dy, keep, row0, out, grads)
    return _backward[key]


def weight_names(cfg):
    """The weight matrix of every linear layer, input to output."""
    return [n for n, s in ref_mlp.param_names(cfg) if len(s) == 2]


def drop_kgroup(w, group=None):
    """A copy of the weight matrix w [K, N] with one 16-row k-group zeroed: by default the one
    holding the most non-zero weights (the first of them), since a sparse integer matrix of a wide
    layer has k-groups with none -- the 48 columns of w4 hold 384 non-zeros over 132 groups at L = 2112."""
    groups = (w.shape[0] + 15) // 16
    if group is None:
        nz = [int(np.count_nonzero(w[16 * g:16 * g + 16])) for g in range(groups)]
        group = int(np.argmax(nz))
    g = group
    w = np.array(w, copy=True)
    w[16 * g:16 * g + 16] = 0
    return w


# ---- expected launch forms ------------------------------------------------------------------------
def _use_xchg(L, B, cus):
    gx, gy = (L + 15) // 16, (B + 15) // 16
    return gy <= XCHG_MAXR and gx * gy <= cus


def _out_part_ok(cfg, B):
    return B <= 256 and cfg.output_size <= 64 and 2 * cfg.num_layers + 2 >= 3


def _put(tags, tag, n=1):
    if n > 0:
        tags[tag] = tags.get(tag, 0) + n


def expected_forward_tags(cfg, B, cus, training=None):
    """{tag: launches} of one forward of batch B on `cus` compute units, default environment.
    training None: inference (p3d_forward_ex).  "forward": the training forward alone
    (forward_device(training=True): the output layer carries no target).  "step": the forward inside
    p3d_train_fwd_bwd (the output layer as k_out_part where out_part_ok, else with the fused MSE)."""
    L, H = cfg.linear_size, 2 * cfg.num_layers
    tags = {}
    if training is None and B <= GEMV_MAXB:
        fold = H >= 2 and L <= GEMV_FOLD_MAXK and cfg.input_size == 32 and cfg.output_size <= 64
        if fold and H <= GEMV_CHAIN_MAXH and L <= GEMV_CHAIN_MAXK and H * (L // 16) <= cus:
            return {"gemv_chain": 1}
        if fold:
            _put(tags, "gemv_in_hidden")
            _put(tags, "gemv_hidden", H - 2)
            _put(tags, "gemv_hidden_out")
            return tags
        _put(tags, "gemv_in")
        _put(tags, "gemv_hidden", H)
        _put(tags, "gemv_out")
        return tags
    if training is None:
        _put(tags, "fwd_in_big" if B >= BIG_M else "fwd_in")
        _put(tags, "fwd_hidden_big" if B >= BIG_M and L % 128 == 0 else "fwd_hidden", H)
        _put(tags, "fwd_out")
        return tags
    if cfg.batch_norm:                       # the split BN-train kernels: one launch, or z + k_bn_fwd
        if _use_xchg(L, B, cus):
            _put(tags, "fwd_in_train_x")
            _put(tags, "fwd_hidden_train_x", H)
        else:
            _put(tags, "fwd_in_train_z")
            _put(tags, "fwd_hidden_train_z", H)
            _put(tags, "bn_fwd", H + 1)
    else:                                    # (a training layer saves z: never the large-M GEMM)
        _put(tags, "fwd_in_big" if B >= BIG_M else "fwd_in")
        _put(tags, "fwd_hidden", H)
    if training == "step":
        _put(tags, "fwd_out_part" if _out_part_ok(cfg, B) else "fwd_out_train")
    else:
        _put(tags, "fwd_out")
    return tags


def expected_backward_tags(cfg, B, cus):
    """{tag: launches} of p3d_backward, default environment: the data gradient of the output layer
    and of every hidden layer (each followed by k_bn_bwd where the BN exchange does not fit), then
    every layer's weight gradient in one launch while the layers fit P3D_WG_MULTI, else per layer."""
    L, H = cfg.linear_size, 2 * cfg.num_layers
    nl = H + 2
    tags = {}
    _put(tags, "dgrad_out")
    _put(tags, "dgrad_hidden", H)
    if cfg.batch_norm and not _use_xchg(L, B, cus):
        _put(tags, "bn_bwd", H + 1)
    if nl <= WG_MULTI:
        _put(tags, "wgrad_multi")
    else:
        _put(tags, "wgrad", nl)
    return tags


SERVE_REFUSAL = "p3d_serve: needs linear_size % 128 == 0, input/output size <= 64, <= 7 blocks"


def serve_expected(cfg, B):
    """"runs" or "refused": serve_shape_error of csrc/p3d.hip (float32 models)."""
    L = cfg.linear_size
    if B <= 0 or L <= 0 or L % 128 != 0 or cfg.input_size > 64 or cfg.output_size > 64 or \
            2 * cfg.num_layers + 2 > SERVE_MAXL:
        return "refused"
    return "runs"


# ---- the VAE filter ---------------------------------------------------------------------------
# name -> (in, enc, latent, dec, out); the layout index (0: weight-row stagger + staged input tile,
# 1: stagger alone, 2: neither) and the LDS bytes p3d_vae_lds_bytes answers are in VAE_LAYOUT.
VAE_SHAPES = {
    "nostagger_lat64": (144, (32,), 64, (32,), 48),        # ld = Np; 16 eps blocks per row, head of 128 columns
    "nostagger_w96": (144, (96,), 8, (64,), 48),           # ld = Np; width 96 / 64
    "deep44": (48, (40, 32, 24, 16), 8, (16, 24, 32, 40), 48),   # P3D_VAE_MAX_L = 10 layers, 22 tensors
    "deep44_small": (48, (32, 24, 16, 8), 8, (8, 16, 24, 32), 48),   # the same depth, input tile staged
    "w128": (48, (128,), 8, (64,), 48),                    # 8 column tiles in one layer
    "w136_edge": (48, (136,), 8, (64,), 48),               # 448 B under the limit; width 8 mod 16
    "w256": (48, (256,), 8, (8,), 8),                      # the widest layer; out 8, no KCS term
    "in256": (256, (24,), 8, (24,), 48),                   # the widest narrow input
    "out64": (48, (32,), 64, (32,), 64),                   # latent 64 and out 64
    "deep33_in96": (96, (32, 24, 16), 8, (16, 24, 32), 48),   # three layers per side on the two-frame input
    "wide_deep": (1360, (40, 32, 24), 16, (24, 32, 40), 48),  # the wide form with a deeper core
    "wide_edge": (264, (128, 64), 8, (64,), 48),           # the wide form 128 B under the limit, n0 = 128
}
VAE_LAYOUT = {
    "nostagger_lat64": (2, 161216), "nostagger_w96": (2, 159104), "deep44": (1, 156288),
    "deep44_small": (0, 136576), "w128": (0, 155520), "w136_edge": (0, 163392), "w256": (1, 163008),
    "in256": (1, 103296), "out64": (0, 157952), "deep33_in96": (0, 145152), "wide_deep": (0, 140544),
    "wide_edge": (0, 163712),
}
VAE_LDS_LIMIT = 163840
VAE_TRIES = ((4, 1), (4, 0), (0, 0))           # (wpad, stage_x) in the order vae_plan tries them
# the sequence filter serves the entries whose input is a whole number of 48-wide frames and whose
# layout leaves room for its state tile (p3d_vae_seq_lds_bytes > 0)
VAE_SEQ_NAMES = ("nostagger_lat64", "nostagger_w96", "deep33_in96", "deep44", "deep44_small", "w128", "w136_edge")
# w136_edge with one hidden width raised in the steps of 8 p3d_vae_create takes until no layout fits:
# the decoder's 64 -> 104 (five steps; the encoder's 136 needs six, to 184), found with
# p3d_vae_lds_bytes (tests/test_shape_cases_oracle.py repeats the search), and that shape's size
VAE_REFUSED = ((48, (136,), 8, (104,), 48), 168192)   # (shape, bytes of its smallest layout)


def _ceil16(n):
    return (n + 15) // 16 * 16


def vae_core(shape):
    """The shape whose layout sits in LDS: the shape itself, or behind layer 0 of a wide one (in > 256)."""
    n_in, enc, lat, dec, out = shape
    return shape if n_in <= 256 else (enc[0], tuple(enc[1:]), lat, dec, out)


def vae_layout_bytes(shape, wpad, stage_x):
    """Dynamic LDS bytes of vae_layout(shape, wpad, stage_x): the packed copy (rows of Np + wpad
    floats and a padded bias per layer, the head's two layers side by side), four waves' activation
    areas (a [16, Np + 2] tile per layer, the z and eps tiles, the bone tile of 48 outputs, the input
    tile where staged) and 64 x 4 floats of reduction scratch."""
    n_in, enc, lat, dec, out = vae_core(shape)
    dims, prev = [], n_in
    for u in list(enc) + [2 * lat]:
        dims.append((prev, u))
        prev = u
    prev = lat
    for u in list(dec) + [out]:
        dims.append((prev, u))
        prev = u
    pk = sum(K * (_ceil16(N) + wpad) + _ceil16(N) for K, N in dims)
    act = sum(16 * (_ceil16(N) + 2) for _, N in dims) + 2 * 16 * (_ceil16(lat) + 2)
    if out == 48:
        act += 16 * 50
    if stage_x:
        act += 16 * (_ceil16(n_in) + 2)
    return 4 * ((pk + 3) // 4 * 4 + 4 * ((act + 3) // 4 * 4) + 64 * 4)


def vae_layout_index(shape):
    """The first of vae_plan's three tries that fits the LDS limit (2 where none does)."""
    for i, (wpad, stage_x) in enumerate(VAE_TRIES):
        if vae_layout_bytes(shape, wpad, stage_x) <= VAE_LDS_LIMIT:
            return i
    return len(VAE_TRIES) - 1


def vae_best_bytes(shape):
    return vae_layout_bytes(shape, *VAE_TRIES[vae_layout_index(shape)])


def vae_exact_names():
    """The entries that carry the KCS term (48 outputs): tests/vae_exact.py's integer cases."""
    return [n for n, s in VAE_SHAPES.items() if s[4] == 48]


def vae_kernel_names(shape):
    """The kernel of every dense layer whose weights are not all zero in the integer model."""
    import vae_oracle as vo
    return [n + "/kernel" for n, _, _ in vo.layer_names(shape) if n != "log_varianze"]


VAE_EXACT_BATCHES = (16, 128)
assert set(VAE_EXACT_BATCHES) <= set(vae_exact.EXACT_BATCHES)
