"""VR_MODE_CDVR restated in numpy float32 -- TEST INFRASTRUCTURE ONLY (the definition the GPU march and
vr_colormap_eval are held to, bit for bit; include/vr_api.h VR_MODE_CDVR).

Every float operation is one numpy float32 ufunc, so each is rounded on its own (no contraction).

  samples    dvr_ref's: positions p (dvr_ref.positions), inside 0 <= p_a < d_a, corners (int)p and
             min((int)p + 1, d - 1), weights p - (int)p, a non-finite voxel reads as 0, dvr_ref._lerp in
             y, then x, then z.  No division by cal_max.
  colour     C(v) over the points (x_i, rgba_i): j = #{i : x_i <= v} (a NaN: 0); j == 0 -> rgba_0,
             j == n -> rgba_{n-1}; otherwise u = min((v - x_{j-1}) * inv_{j-1}, 1) with
             inv_i = 1 / (x_{i+1} - x_i), and a_k * (1 - u) + b_k * u per channel
  outside    C(0.0f)
  blend      dvr_ref.render's: back to front, f = f * (1 - a) + c * a, alpha 1
"""
import numpy as np

import dvr_ref

F = np.float32


def cmap_arrays(points):
    """points: [(x, (r, g, b, a)), ...] -> x float32 [n], rgba float32 [n, 4], inv float32 [n] (the last 0)."""
    x = np.array([p[0] for p in points], F)
    rgba = np.array([p[1] for p in points], F).reshape(len(points), 4)
    inv = np.zeros(len(points), F)
    with np.errstate(divide="ignore", over="ignore"):
        inv[:-1] = F(1.0) / (x[1:] - x[:-1])
    return x, rgba, inv


def C(points, v):
    """The colour map at the float32 values v: float32 v.shape + (4,)."""
    x, rgba, inv = cmap_arrays(points)
    n = len(x)
    v = np.asarray(v, F)
    j = np.zeros(v.shape, np.int32)
    for i in range(n):   # (a NaN compares false: j stays 0)
        j = j + (x[i] <= v).astype(np.int32)
    ja, jb = np.maximum(j - 1, 0), np.minimum(j, n - 1)
    a, b = rgba[ja], rgba[jb]
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.fmin((v - x[ja]) * inv[ja], F(1.0))
        u1 = F(1.0) - u
        mix = a * u1[..., None] + b * u[..., None]
    flat = ((j == 0) | (j == n))[..., None]
    return np.where(flat, a, mix).astype(F)


def sample_values(vol, p, cam, xs=None):
    """(inside bool [nx, H, S], v float32 [nx, H, S]; v is 0 where outside) -- DVR's samples."""
    vol = np.ascontiguousarray(vol, F)
    d = vol.shape
    px, py, pz = dvr_ref.positions(d, p, cam, xs)
    inside = ((px >= 0) & (px < F(d[0])) & (py >= 0) & (py < F(d[1])) & (pz >= 0) & (pz < F(d[2])))
    v = np.zeros(px.shape, F)
    P = [c[inside] for c in (px, py, pz)]
    if P[0].size == 0:
        return inside, v
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
    L = dvr_ref._lerp
    y1, y2 = L(c[0], c[2], dy), L(c[1], c[3], dy)
    y3, y4 = L(c[4], c[6], dy), L(c[5], c[7], dy)
    z1, z2 = L(y1, y3, dx), L(y2, y4, dx)
    v[inside] = L(z1, z2, dz)
    return inside, v


def sample_colors(vol, points, p, cam, xs=None, samples=None):
    """RGBA of every sample, float32 [nx, H, S, 4] (samples: sample_values' result, to share it)."""
    inside, v = sample_values(vol, p, cam, xs) if samples is None else samples
    out = np.empty(v.shape + (4,), F)
    out[...] = C(points, np.zeros(1, F))[0]
    if inside.any():
        out[inside] = C(points, v[inside])
    return out


def blend(col, p):
    """dvr_ref.render's blend of the samples' colours."""
    f = np.empty(col.shape[:2] + (4,), F)
    f[...] = np.array(list(p.background), F)
    for s in range(p.samples_per_ray - 1, -1, -1):
        a = col[:, :, s, 3:4]
        f[..., :3] = f[..., :3] * (F(1.0) - a) + col[:, :, s, :3] * a
    f[..., 3] = F(1.0)
    return f


def render(vol, points, p, cam, xs=None, samples=None):
    """The frame (xs: its columns), float32 [nx, H, 4]."""
    return blend(sample_colors(vol, points, p, cam, xs, samples), p)
