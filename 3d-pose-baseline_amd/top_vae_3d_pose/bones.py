"""Joints <-> bones (src/top_vae_3d_pose/bones.py) on the device: libp3d.so's p3d_bones_from_joints
and p3d_bones_to_joints (csrc/p3d_bones.h).

A pose is 48 floats, joints 1 .. 16 of a skeleton whose hip (joint 0) is the origin; its bones are
16 lengths and 16 direction-cosine triples, kept as one [B, 64] tensor [mag | cos] -- the layout of
``model.concat([mags, dir_cos])`` (models.py:528-530).  Bone b runs from joint BJA[b] to BJB[b].
"""
import numpy as np

import _p3d
from _p3d import check, lib, ptr

# bones.py:74-75, and what get_bones_joints yields on src/bones_mapping.yml
BJA = (0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 9, 14, 15, 9, 11, 12)
BJB = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13)


def get_bones_mapping(path=None):
    """The bones mapping file (bones.py:12-16); the path defaults to FLAGS.bones_mapping_dir."""
    import yaml
    if path is None:
        from top_vae_3d_pose.args_def import ENVIRON as ENV
        path = ENV.FLAGS.bones_mapping_dir
    with open(path) as fyml:
        return yaml.safe_load(fyml)


def get_bones_joints(bones_mapping=None):
    """(bja, bjb): the joints at the start and at the end of every bone, in the depth-first order of
    the mapping (bones.py:19-44); the hip is joint 0.  Without a mapping: the built-in table."""
    if bones_mapping is None:
        return np.array(BJA), np.array(BJB)
    pairs = []

    def bone_walk(mapping):
        for _, infop in mapping.items():
            if infop['next'] is None:
                continue
            for bmapn in infop['next']:
                for _, infoc in bmapn.items():
                    pairs.append((infop['joint_id_17'], infoc['joint_id_17']))
                bone_walk(bmapn)

    bone_walk(bones_mapping['bones_path'][0])
    bja, bjb = zip(*pairs)
    return np.array(bja) + 1, np.array(bjb) + 1


def _check_table(bones_joints):
    if bones_joints is None:
        return
    bja, bjb = bones_joints
    if tuple(int(v) for v in bja) != BJA or tuple(int(v) for v in bjb) != BJB:
        raise ValueError("bones: the kernels are built for the skeleton of src/bones_mapping.yml "
                         "(bja %s, bjb %s); got bja %s, bjb %s" % (BJA, BJB, tuple(bja), tuple(bjb)))


def _dev(a, width, what):
    import torch
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float32, order="C"))
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError("%s: expected shape [None, %d], got %s" % (what, width, tuple(t.shape)))
    if not torch.cuda.is_available():
        raise _p3d.P3DError("bones: the conversions need a ROCm GPU; the HIP path has no CPU fallback")
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(device=t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device()),
                 dtype=torch.float32).contiguous()
    if t.shape[0] < 1:
        raise ValueError("%s: no rows" % what)
    return t


def convert_to_bones(joints, bones_joints=None, precise=True, out=None):
    """joints [B, 48] -> the device tensor [B, 64] = [mag | cos].  precise=True is the reference's
    convert_to_bones (float64 arithmetic, bones.py:101-121), precise=False its convert_to_bones_tf
    (float32, bones.py:71-98).  Rows are converted 2^20 at a time."""
    import torch
    _check_table(bones_joints)
    j = _dev(joints, 48, "joints")
    B = j.shape[0]
    if out is None:
        out = torch.empty((B, 64), dtype=torch.float32, device=j.device)
    elif tuple(out.shape) != (B, 64) or out.dtype != torch.float32 or out.device != j.device or not out.is_contiguous():
        raise ValueError("convert_to_bones: out must be a contiguous float32 [%d, 64] tensor on %s" % (B, j.device))
    with torch.cuda.device(j.device):
        for r0 in range(0, B, 1 << 20):
            n = min(1 << 20, B - r0)
            check(lib().p3d_bones_from_joints(ptr(j[r0:]), n, 1 if precise else 0, ptr(out[r0:]), _p3d.stream_handle()),
                  "p3d_bones_from_joints")
    return out


def convert_to_joints(bones64, cos=None, bones_joints=None):
    """[B, 64] = [mag | cos] (or mag [B, 16] and cos [B, 48]) -> the float64 device tensor [B, 48] of
    joints, walked from the hip along the bones (bones.py:124-153)."""
    import torch
    _check_table(bones_joints)
    if cos is not None:
        bones64 = torch.cat([torch.as_tensor(bones64), torch.as_tensor(cos).reshape(len(cos), 48)], dim=1)
    b = _dev(bones64, 64, "bones")
    B = b.shape[0]
    out = torch.empty((B, 48), dtype=torch.float64, device=b.device)
    with torch.cuda.device(b.device):
        for r0 in range(0, B, 1 << 20):
            n = min(1 << 20, B - r0)
            check(lib().p3d_bones_to_joints(ptr(b[r0:]), n, ptr(out[r0:]), _p3d.stream_handle()), "p3d_bones_to_joints")
    return out
