"""The filter shapes the VAE planner's checks run over, and what is asked of the library for each --
through the ABI only, so the same questions can be put to any build.  tests/golden/vae_plan_parent.json
holds the answers of the build before the planner moved into csrc/p3d_vae_layout.h;
tests/test_vae_plan.py compares the current build with it."""
import ctypes
import json
import os

import _p3d
import shape_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "vae_plan_parent.json")
DEFAULT = (48, (40, 32), 24, (32, 40), 48)
MAX_BATCHES = (64, 200)
WORKSPACE_B = (1, 64, 65)


def cases():
    """[(name, kind, (in, enc, latent, dec, out))]: kind 1 is a bones filter (out = 64)."""
    out = [("table:" + n, 0, s) for n, s in sc.VAE_SHAPES.items()]
    out.append(("refused", 0, sc.VAE_REFUSED[0]))
    out.append(("default", 0, DEFAULT))
    with open(os.path.join(HERE, "golden", "vae_lds_parent.json")) as f:
        for i, rec in enumerate(json.load(f)):
            n_in, enc, lat, dec, n_out = rec["shape"]
            out.append(("lds_parent%d" % i, 0, (n_in, tuple(enc), lat, tuple(dec), n_out)))
    for n_in in (64, 96, 1376):
        out.append(("bones%d" % n_in, 1, (n_in, (40, 32), 24, (32, 40), 64)))
    # four layers a side: 11 layers and 26 tensors, the bounds of the descriptor's arrays
    out.append(("bones_deepest", 1, (64, (40, 32, 24, 16), 8, (16, 24, 32, 40), 64)))
    out.append(("dup_width", 0, (48, (40, 40), 24, (32, 40), 48)))
    return out


def _dims(v):
    return len(v), (ctypes.c_int32 * max(len(v), 1))(*v)


def host_answers(lib, shape):
    """The four *_lds_bytes calls on one shape (each for both of its variants): no GPU."""
    n_in, enc, lat, dec, out = shape
    (ne, e), (nd, d) = _dims(enc), _dims(dec)
    return {"lds": int(lib.p3d_vae_lds_bytes(n_in, ne, e, lat, nd, d, out)),
            "bones_lds": int(lib.p3d_vae_bones_lds_bytes(n_in, ne, e, lat, nd, d)),
            "dec_lds": [int(lib.p3d_vae_dec_lds_bytes(lat, nd, d, out, b)) for b in (0, 1)],
            "seq_lds": [int(lib.p3d_vae_seq_lds_bytes(n_in, ne, e, lat, nd, d, out, f)) for f in (0, 1)]}


A = 0x10000    # (a segment address: p3d_vae_cat_check never dereferences it)
# (widths, pointer offsets or None, rows, has index, in, B)
CAT_CASES = [
    ((32, 48, 1280), (0, 0, 0), (100, 100, 100), (0, 0, 0), 1360, 64),
    ((), (), (), (), 1360, 64),
    ((8, 8, 8, 8, 8), (0, 0, 0, 0, 0), (100,) * 5, (0,) * 5, 40, 64),
    ((4, 1356), (0, 0), (100, 100), (0, 0), 1360, 64),
    ((32, 48, 1272), (0, 0, 0), (100, 100, 100), (0, 0, 0), 1360, 64),
    ((32, 48, 1280), (0, None, 0), (100, 100, 100), (0, 0, 0), 1360, 64),
    ((32, 48, 1280), (0, 4, 0), (100, 100, 100), (0, 0, 0), 1360, 64),
    ((32, 48, 1280), (0, 0, 0), (100, 100, 10), (0, 0, 0), 1360, 64),
    ((32, 48, 1280), (0, 0, 0), (100, 100, 10), (0, 0, 1), 1360, 64),
    ((32, 48, 1280), (0, 0, 0), (100, 0, 100), (0, 0, 0), 1360, 64),
    ((1024, 1024, 8), (0, 0, 0), (100, 100, 100), (0, 0, 0), 2056, 64),
    ((32, 64), (0, 0), (100, 100), (0, 0), -1, 64),
    ((32, 64), (0, 0), (100, 100), (0, 0), 96, 0),
    ((32, 64), (0, 0), (100, 100), (0, 0), 96, (1 << 20) + 1),
]


def cat_answers(lib):
    """[code, message] of p3d_vae_cat_check on every CAT_CASES entry, and on a null struct."""
    out = []
    for widths, ptrs, rows, idx, n_in, B in CAT_CASES:
        c = _p3d.P3DVaeCat()
        c.n = len(widths)
        for s in range(min(len(widths), 4)):
            c.w[s], c.rows[s] = widths[s], rows[s]
            c.p[s] = None if ptrs[s] is None else A + ptrs[s]
            c.idx[s] = A if idx[s] else None
        rc = int(lib.p3d_vae_cat_check(ctypes.byref(c), n_in, B))
        out.append([rc, lib.p3d_last_error().decode() if rc else ""])
    rc = int(lib.p3d_vae_cat_check(None, 96, 64))
    out.append([rc, lib.p3d_last_error().decode()])
    return out


def gpu_answers(lib, kind, shape):
    """What a created filter reports without a launch: {"error": [code, text]} where create refuses,
    else its kind, parameter table and, per max_batch, the flat buffers' sizes and the workspace."""
    n_in, enc, lat, dec, out = shape
    (ne, e), (nd, d) = _dims(enc), _dims(dec)
    rec = {}
    for mb in MAX_BATCHES:
        h = ctypes.c_void_p()
        if kind:
            rc = lib.p3d_vae_create_bones(n_in, ne, e, lat, nd, d, mb, 1, ctypes.byref(h))
        else:
            rc = lib.p3d_vae_create(n_in, ne, e, lat, nd, d, out, mb, 1, ctypes.byref(h))
        if rc:
            return {"error": [int(rc), lib.p3d_last_error().decode()]}
        try:
            n = ctypes.c_int32()
            assert lib.p3d_vae_param_count(h, ctypes.byref(n)) == 0
            params = []
            for i in range(n.value):
                name, numel, rows = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int32()
                cols, off = ctypes.c_int32(), ctypes.c_int64()
                assert lib.p3d_vae_param_info(h, i, ctypes.byref(name), ctypes.byref(numel), ctypes.byref(rows),
                                              ctypes.byref(cols), ctypes.byref(off)) == 0
                params.append([name.value.decode(), numel.value, rows.value, cols.value, off.value])
            flat = []
            for which in (0, 4, 5):
                p, numel = ctypes.c_void_p(), ctypes.c_int64()
                assert lib.p3d_vae_flat_ptr(h, which, ctypes.byref(p), ctypes.byref(numel)) == 0
                flat.append(numel.value)
            got = {"kind": int(lib.p3d_vae_kind(h)), "params": params}
            assert rec.get("params", params) == params       # (the table does not depend on max_batch)
            rec.update(got)
            rec["mb%d" % mb] = {"flat_numel": flat,
                                "workspace": [int(lib.p3d_vae_workspace(h, B)) for B in WORKSPACE_B]}
        finally:
            lib.p3d_vae_destroy(h)
    return rec
