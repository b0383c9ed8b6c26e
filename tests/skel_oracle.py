"""numpy float64 oracle of the rigid skeleton (csrc/p3d_skel.h states the same
operations in the same order): bone lengths of a clip, the shortest-arc rotation of every bone,
the local quaternions, Euler angles in BVH's Z X Y order, the rigid pose; the BVH writer's
hierarchy restated, and a small BVH reader with forward kinematics that knows nothing of either.

Rows are `poses` rows of the clip calls: [N, 96], 32 joints in exported coordinates.  src holds row
indices into the batch (-1: zeros), or None (every row its own)."""
import numpy as np

from top_vae_3d_pose.bones import BJA, BJB

H36M = np.array([0, 1, 2, 3, 6, 7, 8, 12, 13, 14, 15, 17, 18, 19, 25, 26, 27])
NAMES = ["Hip", "RHip", "RKnee", "RFoot", "LHip", "LKnee", "LFoot", "Spine", "Thorax", "NeckNose", "Head",
         "LShoulder", "LElbow", "LWrist", "RShoulder", "RElbow", "RWrist"]
JA, JB = np.array(BJA), np.array(BJB)
PB = np.array([list(BJB).index(a) if a else -1 for a in BJA])     # the bone that produces ja(b); -1: the hip
_REST = {"R": (-1.0, 0.0, 0.0), "L": (1.0, 0.0, 0.0), "down": (0.0, -1.0, 0.0), "up": (0.0, 1.0, 0.0)}
_KIND = {"RHip": "R", "RShoulder": "R", "RElbow": "R", "RWrist": "R", "LHip": "L", "LShoulder": "L", "LElbow": "L",
         "LWrist": "L", "RKnee": "down", "RFoot": "down", "LKnee": "down", "LFoot": "down", "Spine": "up",
         "Thorax": "up", "NeckNose": "up", "Head": "up"}
REST = np.array([_REST[_KIND[NAMES[j]]] for j in JB])               # [16, 3], by the bone's child joint
DEG = 57.29577951308232                                             # 180 / pi
TOL = 1e-9


def close(got, want, what=""):
    """|got - want| <= 1e-9 max(1, |want|) everywhere, NaN exactly where want has NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN in other places" % what
    err = np.abs(got - want)[~nan] / np.maximum(1.0, np.abs(want[~nan]))
    assert err.size == 0 or err.max() <= TOL, "%s: off by %.3e (relative to max(1, |value|))" % (what, err.max())


def to_skeleton(poses):
    """[N, 96] exported rows -> the 17 joints in skeleton coordinates (X, Y, Z) = (x, z, -y): [N, 17, 3]."""
    p = np.asarray(poses, np.float64).reshape(-1, 32, 3)[:, H36M]
    return np.stack([p[..., 0], p[..., 2], -p[..., 1]], axis=-1)


def from_skeleton(J, fill=np.nan):
    """The inverse: [N, 17, 3] -> [N, 96]; the 15 joints the skeleton does not use hold `fill`."""
    J = np.asarray(J, np.float64)
    out = np.full((J.shape[0], 32, 3), fill)
    out[:, H36M] = np.stack([J[..., 0], -J[..., 2], J[..., 1]], axis=-1)
    return out.reshape(-1, 96)


def bones(J):
    """v = J[jb] - J[ja] [N, 16, 3] and len = sqrt((vx^2 + vy^2) + vz^2) [N, 16]."""
    v = J[:, JB] - J[:, JA]
    return v, np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def _rows(poses, src):
    poses = np.asarray(poses, np.float64)
    n = poses.shape[0]
    src = np.arange(n) if src is None else np.asarray(src)
    return poses, src


def lengths(poses, src, off):
    """Per clip the mean bone lengths over the frames with src[n] == n whose 17 joints are finite
    -> (L [S, 16], n_used [S])."""
    poses, src = _rows(poses, src)
    J = to_skeleton(poses)
    _, ln = bones(J)
    counts = (src == np.arange(len(src))) & np.isfinite(J).all(axis=(1, 2))
    L, used = [], []
    for a, b in zip(off[:-1], off[1:]):
        m = counts[a:b]
        used.append(int(m.sum()))
        L.append(ln[a:b][m].mean(axis=0) if m.any() else np.zeros(16))
    return np.array(L), np.array(used, np.int64)


def directions(J):
    """d_b [N, 16, 3] (a zero-length bone: r_b) and the zero-length mask [N, 16]."""
    v, ln = bones(J)
    zero = ln == 0.0
    with np.errstate(all="ignore"):
        inv = 1.0 / ln
        d = np.where(zero[..., None], REST[None], v * inv[..., None])
    return d, zero


def arcs(d, zero):
    """g_b (w, x, y, z) [N, 16, 4]: normalize(1 + r.d, r x d) with r = (rx, ry, 0); 1 + r.d < 1e-12:
    (0, 0, 0, 1); a zero-length bone: the identity."""
    rx, ry = REST[None, :, 0], REST[None, :, 1]
    with np.errstate(all="ignore"):
        w = 1.0 + (rx * d[..., 0] + ry * d[..., 1])
        cx, cy, cz = ry * d[..., 2], -(rx * d[..., 2]), rx * d[..., 1] - ry * d[..., 0]
        inv = 1.0 / np.sqrt((w * w + cx * cx) + (cy * cy + cz * cz))
        g = np.stack([w * inv, cx * inv, cy * inv, cz * inv], axis=-1)
    g = np.where((w < 1e-12)[..., None], np.array([0.0, 0.0, 0.0, 1.0]), g)
    return np.where(zero[..., None], np.array([1.0, 0.0, 0.0, 0.0]), g)


def qmul(a, b):
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([((aw * bw - ax * bx) - ay * by) - az * bz,
                     ((aw * bx + ax * bw) + ay * bz) - az * by,
                     ((aw * by - ax * bz) + ay * bw) + az * bx,
                     ((aw * bz + ax * by) - ay * bx) + az * bw], axis=-1)


def qconj(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def quat_matrix(q):
    """The rotation matrix of a unit quaternion (w, x, y, z): [..., 3, 3]."""
    w, x, y, z = (q[..., k] for k in range(4))
    return np.stack([
        np.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)], axis=-1),
        np.stack([2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)], axis=-1),
        np.stack([2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)], axis=-1)], axis=-2)


def euler_zxy(q):
    """(Z, X, Y) degrees of q with R = Rz Rx Ry: [..., 3].  atan2 only."""
    R = quat_matrix(q)
    with np.errstate(all="ignore"):
        hx = np.hypot(R[..., 0, 1], R[..., 1, 1])
        gimbal = hx < 1e-12
        ex = np.arctan2(R[..., 2, 1], hx)
        ez = np.where(gimbal, np.arctan2(R[..., 1, 0], R[..., 0, 0]), np.arctan2(-R[..., 0, 1], R[..., 1, 1]))
        ey = np.where(gimbal, 0.0, np.arctan2(-R[..., 2, 0], R[..., 2, 2]))
    return np.stack([ez * DEG, ex * DEG, ey * DEG], axis=-1)


def euler_matrix(e):
    """Rz Rx Ry of (Z, X, Y) degrees: [..., 3, 3], from the plain axis rotations."""
    z, x, y = (np.radians(e[..., k]) for k in range(3))
    c, s, o, i = np.cos, np.sin, np.zeros_like(z), np.ones_like(z)
    m = lambda rows: np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)   # noqa: E731
    Rz = m([[c(z), -s(z), o], [s(z), c(z), o], [o, o, i]])
    Rx = m([[i, o, o], [o, c(x), -s(x)], [o, s(x), c(x)]])
    Ry = m([[c(y), o, s(y)], [o, i, o], [-s(y), o, c(y)]])
    return Rz @ Rx @ Ry


def pose(poses, src, off, L):
    """-> dict(quat [N, 16, 4], euler [N, 16, 3], rigid [N, 17, 3], root [N, 3]); L [S, 16]; a row
    with src < 0 counts as zeros."""
    poses, src = _rows(poses, src)
    poses = np.where((src < 0)[:, None], 0.0, poses)
    J = to_skeleton(poses)
    d, zero = directions(J)
    g = arcs(d, zero)
    quat = g.copy()
    has = PB >= 0
    quat[:, has] = qmul(qconj(g[:, PB[has]]), g[:, has])
    Lrow = np.repeat(np.asarray(L, np.float64), np.diff(off), axis=0)           # [N, 16]
    rigid = np.empty((poses.shape[0], 17, 3))
    rigid[:, 0] = J[:, 0]
    with np.errstate(all="ignore"):
        for b in range(16):                                                     # (a parent comes before its children)
            rigid[:, JB[b]] = rigid[:, JA[b]] + Lrow[:, b, None] * d[:, b]
        euler = euler_zxy(quat)
    return dict(quat=quat, euler=euler, rigid=rigid, root=J[:, 0].copy())


def composed(quat):
    """g_b again from the local rotations: the product along the bone's path from the hip."""
    g = np.array(quat, np.float64)
    for b in range(16):
        if PB[b] >= 0:
            g[:, b] = qmul(g[:, PB[b]], quat[:, b])
    return g


def rotate(q, v):
    return np.einsum("...ij,...j->...i", quat_matrix(q), v)


def fk(root, L, quat):
    """Forward kinematics from (root [N, 3], L [16], local quaternions [N, 16, 4]) -> [N, 17, 3]."""
    g = composed(quat)
    P = np.empty((root.shape[0], 17, 3))
    P[:, 0] = root
    for b in range(16):
        P[:, JB[b]] = P[:, JA[b]] + L[b] * rotate(g[:, b], REST[b])
    return P


# ---- inputs -------------------------------------------------------------------------------------
MARGIN = 1e-3   # every generated bone has 1 + r.d >= MARGIN: away from the antiparallel branch


def random_directions(rng, n):
    """[n, 16, 3] unit directions, redrawn until 1 + r.d >= MARGIN for every bone."""
    d = rng.standard_normal((n, 16, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    while True:
        bad = 1.0 + (d * REST[None]).sum(-1) < 10 * MARGIN
        if not bad.any():
            return d
        e = rng.standard_normal((int(bad.sum()), 3))
        d[bad] = e / np.linalg.norm(e, axis=-1, keepdims=True)


def rows_from(hip, d, ln, fill=np.nan):
    """`poses` rows from hips [n, 3], bone directions [n, 16, 3] and lengths [n, 16] (skeleton coordinates)."""
    J = np.empty((hip.shape[0], 17, 3))
    J[:, 0] = hip
    for b in range(16):
        J[:, JB[b]] = J[:, JA[b]] + ln[:, b, None] * d[:, b]
    return from_skeleton(J, fill)


def random_rows(rng, n, fill=np.nan):
    """n `poses` rows from random bone directions and lengths of 50-500 mm (drawn per frame, so the
    clip's mean is a real mean); the joints the skeleton does not use hold NaN."""
    return rows_from(rng.uniform(-1000.0, 1000.0, (n, 3)), random_directions(rng, n), rng.uniform(50.0, 500.0, (n, 16)),
                     fill)


def margins(poses):
    """1 + r.d of every bone of every row [N, 16] (what the oracle comparisons assert on)."""
    d, _ = directions(to_skeleton(poses))
    return 1.0 + (d * REST[None]).sum(-1)


# ---- BVH ----------------------------------------------------------------------------------------
def hierarchy(L):
    """The writer's hierarchy restated: [(name, parent name, offset [3])] for the 16 bone joints
    (a joint sits at its bone's START) and the End Sites of the leaves."""
    nodes = []
    for b in range(16):
        parent = "Hips" if PB[b] < 0 else "bone_" + NAMES[JB[PB[b]]]
        nodes.append(("bone_" + NAMES[JB[b]], parent, np.zeros(3) if PB[b] < 0 else L[PB[b]] * REST[PB[b]]))
    for b in range(16):
        if not (PB == b).any():
            nodes.append(("End_bone_" + NAMES[JB[b]], "bone_" + NAMES[JB[b]], L[b] * REST[b]))
    return nodes


def read_bvh(path):
    """A BVH file -> (nodes [(name, parent index, offset, channel names)], frame_time, motion [F, C]).
    End Sites are nodes named End_<parent> without channels."""
    tok = open(path).read().split()
    nodes, stack, i = [], [], 0
    assert tok[i] == "HIERARCHY"
    i += 1
    while tok[i] != "MOTION":
        t = tok[i]
        if t in ("ROOT", "JOINT"):
            name, i = tok[i + 1], i + 2
        elif t == "End":
            name, i = "End_" + nodes[stack[-1]][0], i + 2
        elif t == "}":
            stack.pop()
            i += 1
            continue
        else:
            raise ValueError("unexpected token %r" % t)
        assert tok[i] == "{" and tok[i + 1] == "OFFSET"
        offset = np.array([float(v) for v in tok[i + 2:i + 5]])
        i += 5
        ch = []
        if tok[i] == "CHANNELS":
            k = int(tok[i + 1])
            ch, i = tok[i + 2:i + 2 + k], i + 2 + k
        nodes.append((name, stack[-1] if stack else -1, offset, ch))
        stack.append(len(nodes) - 1)
    assert tok[i + 1] == "Frames:" and tok[i + 3:i + 5] == ["Frame", "Time:"]
    frames, frame_time = int(tok[i + 2]), float(tok[i + 5])
    motion = np.array([float(v) for v in tok[i + 6:]]).reshape(frames, -1)
    assert motion.shape[1] == sum(len(n[3]) for n in nodes)
    return nodes, frame_time, motion


def _axis(name, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return {"X": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "Y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "Z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[name]


def bvh_positions(nodes, motion):
    """World positions {node name: [F, 3]}: channels applied in the order the file lists them."""
    out = {n[0]: np.empty((motion.shape[0], 3)) for n in nodes}
    for f, row in enumerate(motion):
        world, c = [], 0
        for name, parent, offset, ch in nodes:
            R, t = np.eye(3), offset.copy()
            for k in ch:
                if k.endswith("position"):
                    t["XYZ".index(k[0])] += row[c]
                else:
                    R = R @ _axis(k[0], row[c])
                c += 1
            if parent >= 0:
                pR, pt = world[parent]
                R, t = pR @ R, pt + pR @ t
            world.append((R, t))
            out[name][f] = t
    return out


def bvh_rigid(positions):
    """The 17 joints [F, 17, 3] from a file's node positions: joint jb(b) is where bone b ENDS -- the
    start of a child bone's joint, or the leaf's End Site."""
    P = np.empty((positions["Hips"].shape[0], 17, 3))
    P[:, 0] = positions["Hips"]
    for b in range(16):
        kids = np.flatnonzero(PB == b)
        key = "bone_" + NAMES[JB[kids[0]]] if len(kids) else "End_bone_" + NAMES[JB[b]]
        P[:, JB[b]] = positions[key]
    return P
