"""VR_MODE_MIP restated in numpy float32 -- TEST INFRASTRUCTURE ONLY (the definition the GPU march is
held to, bit for bit; include/vr_api.h VR_MODE_MIP).

Every float operation is one numpy float32 ufunc, so each is rounded on its own, like dvr_ref.

  position   dvr_ref.positions: the TEST chain, three glm mat * vec
  inside     0 <= p_a < d_a per axis
  value      corners (int)p and min((int)p + 1, d - 1), weights p - (int)p, a non-finite voxel reads as
             0, dvr_ref._lerp in y, then x, then z -- the block dvr_ref.sample_colors classifies,
             restated here for the scalar
  maximum    m from -inf, walking s upwards, replaced only when v > m (a NaN is never taken)
  pixel      no in-volume sample: the background's r, g, b, alpha 1; otherwise
             g = min(max((float)((double)m / cal_max), 0), 1) as (g, g, g, 1), the zero positive
"""
import numpy as np

import dvr_ref

F = np.float32


def sample_values(vol, p, cam, xs=None):
    """(v, inside): the trilinear value of every sample, float32 [nx, H, S] (0 where outside), and the
    in-volume mask."""
    vol = np.ascontiguousarray(vol, F)
    d = vol.shape
    px, py, pz = dvr_ref.positions(d, p, cam, xs)
    inside = ((px >= 0) & (px < F(d[0])) & (py >= 0) & (py < F(d[1])) & (pz >= 0) & (pz < F(d[2])))
    v = np.zeros(px.shape, F)
    P = [c[inside] for c in (px, py, pz)]
    if P[0].size == 0:
        return v, inside
    i0 = [c.astype(np.int32) for c in P]
    dx, dy, dz = [c - i.astype(F) for c, i in zip(P, i0)]
    clean = np.where(np.isfinite(vol), vol, F(0.0))
    i1 = [np.minimum(i + 1, n - 1) for i, n in zip(i0, d)]
    c = {}
    for k in range(8):
        ix = i1[0] if (k >> 2) & 1 else i0[0]
        iy = i1[1] if (k >> 1) & 1 else i0[1]
        iz = i1[2] if k & 1 else i0[2]
        c[k] = clean[ix, iy, iz]
    with np.errstate(over="ignore", invalid="ignore"):
        y1, y2 = dvr_ref._lerp(c[0], c[2], dy), dvr_ref._lerp(c[1], c[3], dy)
        y3, y4 = dvr_ref._lerp(c[4], c[6], dy), dvr_ref._lerp(c[5], c[7], dy)
        z1, z2 = dvr_ref._lerp(y1, y3, dx), dvr_ref._lerp(y2, y4, dx)
        v[inside] = dvr_ref._lerp(z1, z2, dz)
    return v, inside


def render(vol, cal_max, p, cam, xs=None):
    """(frame float32 [nx, H, 4], m float32 [nx, H], any bool [nx, H]) -- xs: the frame's columns."""
    v, inside = sample_values(vol, p, cam, xs)
    m = np.full(v.shape[:2], -np.inf, F)
    for s in range(v.shape[2]):
        take = inside[:, :, s] & (v[:, :, s] > m)
        m = np.where(take, v[:, :, s], m)
    hit = inside.any(axis=2)
    with np.errstate(over="ignore"):
        q = (m.astype(np.float64) / float(cal_max)).astype(F)
    g = np.where(q > 0, q, F(0.0)).astype(F)
    g = np.where(g < 1, g, F(1.0)).astype(F)
    f = np.empty(m.shape + (4,), F)
    f[..., :3] = np.where(hit[..., None], g[..., None], np.array(list(p.background), F)[:3])
    f[..., 3] = F(1.0)
    return f, m, hit
