"""A synthetic EfficientNet-feature archive for the H3.6M-shaped test data: per 2D key (subject,
action, name) the member ``<subject>/<action>/<name without .h5>/data`` of standard-normal rows
scaled by 0.1 -- the ``.npz`` form of the reference's human36m_effnet.hdf5 that
data_handler.load_effnet_outputs reads."""
import numpy as np


def write_effnet_archive(path, data_sets_2d, rng, width=1280, extra_rows=2):
    """One member per key of every dict in `data_sets_2d` ({(subject, action, name): [n, 32]}), with
    `extra_rows` rows more than the key has 2D frames (the reader cuts them).  Returns the member names."""
    members = {}
    for data in data_sets_2d:
        for (subj, action, name), poses in data.items():
            name = name[:-3] if name.endswith("-sh") else name
            rel = "%s/%s/%s/data" % (subj, action, name.replace(".h5", ""))
            if rel not in members:
                members[rel] = (0.1 * rng.standard_normal((poses.shape[0] + extra_rows, width))).astype(np.float32)
    np.savez(path, **members)
    return sorted(members)
