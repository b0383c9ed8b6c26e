"""numpy restatement of the VAE filters' decoder alone (float64 and float32): VAE.decode of
src/top_vae_3d_pose/models.py:74-76 and the bones filter's decoder (models.py:555-566) -- what
csrc/p3d_vae_dec.h is tested against.  The statements are written out here, not taken from
vae_oracle.forward / vae_bones_oracle.forward: tests/test_vae_dec_oracle.py pins them to those.

Shapes and parameter dicts are vae_oracle's (ELBO: (in, enc, latent, dec, out)) and
vae_bones_oracle's (bones: (in, enc, latent, dec)).  PRIOR_SITE is the Philox site of the prior
stream; its normals are vae_noise_oracle.normals4(rows, c4, PRIOR_SITE, seed, ctr).
"""
import numpy as np

PRIOR_SITE = 0x505249


def _hidden(p, dec, z, dt):
    h = z.astype(dt)
    for u in dec:
        h = np.maximum(h @ p["dec_f_%d/kernel" % u] + p["dec_f_%d/bias" % u], dt(0))
    return h


def decode(P, shape, z, dt=np.float64):
    """y [B, out] = dec_f_out(relu(dec_f_*( ... z)))."""
    dec = shape[3]
    p = {k: v.astype(dt) for k, v in P.items()}
    return _hidden(p, dec, z, dt) @ p["dec_f_out/kernel"] + p["dec_f_out/bias"]


def decode_bones(P, shape, z, dt=np.float64):
    """y [B, 64] = [mag2 | cos2] of relu(mag1(relu(dec_f_*( ... z))))."""
    dec = shape[3]
    p = {k: v.astype(dt) for k, v in P.items()}
    m1 = np.maximum(_hidden(p, dec, z, dt) @ p["mag1/kernel"] + p["mag1/bias"], dt(0))
    return np.concatenate([m1 @ p["mag2/kernel"] + p["mag2/bias"], m1 @ p["cos2/kernel"] + p["cos2/bias"]], axis=1)


def prior_stream(seed, ctr, row0, B, latent):
    """[B, latent] float32: rows row0 .. row0 + B - 1 of the prior stream as k_vae_dec draws them."""
    import vae_noise_oracle as no
    rows = (np.arange(B, dtype=np.int64) + row0).astype(np.uint32)[:, None]
    c4 = np.arange(latent // 4, dtype=np.uint32)[None, :]
    return no.normals4(rows, c4, PRIOR_SITE, seed, ctr).reshape(B, latent)
