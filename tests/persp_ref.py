"""VR_FLAG_PERSP restated in numpy float32 -- TEST INFRASTRUCTURE ONLY (the position law the GPU marches of
the six field modes are held to under the flag, bit for bit; include/vr_api.h VR_FLAG_PERSP).

Every float operation is one numpy float32 ufunc, so each is rounded on its own (no contraction).  With mc,
iv, tv the TEST chain's matrices (oracle.test_matrices; m[column][row], so the header's mc[4 c + r] is
mc[c, r] here):

  per frame   rS  = 1.0f / (float)S
  per ray     ax  = mc[0]*(float)x + mc[12],  ay = mc[5]*(float)y + mc[13]
              A_r = iv[r]*ax + iv[4+r]*ay
  per sample  t   = fs * rS,  qz = mc[10]*fs + mc[14]
              B_r = iv[8+r]*qz + iv[12+r]*1.0f
              q_r = A_r*t + B_r
              p_r = tv[5r]*q_r + tv[12+r]

Every restatement of a field mode (dvr_ref, sdvr_ref, cmap_ref, scdvr_ref, mip_ref, iso_ref, crop_ref) reaches
its positions through two names, dvr_ref.positions and iso_ref._positions_at.  `law()` puts this module's
functions in their place while a reference is computed, so a mode's perspective reference is the mode's own
restatement over these positions, and restores the originals on exit.
"""
import contextlib

import numpy as np

import dvr_ref
import iso_ref
import oracle

F = np.float32


def positions_at(mats, x, y, fs, S=None):
    """The law at float sample coordinates: three float32 arrays shaped like the broadcast of x, y, fs.
    S: samples per ray (rS = 1 / (float)S); `law()` binds it for iso_ref._positions_at's three-matrix call."""
    mc, iv, tv = mats
    x, y, fs = (np.asarray(c, F) for c in (x, y, fs))
    rS = F(1.0) / F(S)
    ax = mc[0, 0] * x + mc[3, 0]
    ay = mc[1, 1] * y + mc[3, 1]
    t = fs * rS
    qz = mc[2, 2] * fs + mc[3, 2]
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(3):
            A = iv[0, r] * ax + iv[1, r] * ay
            B = iv[2, r] * qz + iv[3, r] * F(1.0)
            q = A * t + B
            out.append((tv[r, r] * q + tv[3, r]).astype(F))
    return out


def positions(shape, p, cam, xs=None):
    """dvr_ref.positions under the flag: three float32 arrays [nx, H, S] (xs: the columns, default all)."""
    mats = oracle.test_matrices(shape, p, cam)
    xs = np.arange(p.width) if xs is None else np.asarray(xs)
    x = xs.astype(F)[:, None, None]
    y = np.arange(p.height, dtype=F)[None, :, None]
    s = np.arange(p.samples_per_ray, dtype=F)[None, None, :]
    full = (len(xs), p.height, p.samples_per_ray)
    return [np.ascontiguousarray(np.broadcast_to(c, full)) for c in positions_at(mats, x, y, s, p.samples_per_ray)]


@contextlib.contextmanager
def law(S):
    """While the block runs, dvr_ref.positions and iso_ref._positions_at are this module's (S: the frame's
    samples per ray, which iso_ref._positions_at's callers do not pass); the originals return on exit."""
    saved = dvr_ref.positions, iso_ref._positions_at
    dvr_ref.positions = positions
    iso_ref._positions_at = lambda mats, x, y, fs: positions_at(mats, x, y, fs, S)
    try:
        yield
    finally:
        dvr_ref.positions, iso_ref._positions_at = saved
