"""VR_MODE_DVR restated in numpy float32 -- TEST INFRASTRUCTURE ONLY (the definition the GPU march is
held to, bit for bit; include/vr_api.h VR_MODE_DVR).

Every float operation is one numpy float32 ufunc, so each is rounded on its own (no contraction),
like the oracle's C.  Vectorised over (x, y, s); the blend walks s.

  position   p = toVolume * (inverse(lookAt) * (modelCam * (x, y, s, 1))), three glm mat * vec
             (the oracle's matrices: oracle.test_matrices), the TEST chain
  inside     0 <= p_a < d_a per axis; outside -> TF((float)(0.0f / cal_max))
  corners    i0 = (int)p, i1 = min(i0 + 1, d - 1), w = p - (float)i0; a non-finite voxel reads as 0
  value      lerp(a, b, w) = a * (1 - w) + b * w in y, then x, then z, on the scalar values
  class      TF((float)((double)v / cal_max)): the last closed interval containing it, default 0
  blend      back to front, f = f * (1 - a) + c * a, alpha 1

test_rule=True evaluates the reference's TEST colour rule instead (getColorFromNF, kernel.cu:124-175:
corners (int)(p + {0, 1}) through the flat index with only the idx < total guard, each corner
classified, the colours lerped) on the same positions and weights: that variant must equal
oracle.render_test bit for bit, which pins the position chain and weights the two modes share.
"""
import numpy as np

import oracle

F = np.float32


def tf_arrays(tf):
    """tf: [(lo, hi, (r, g, b, a)), ...] -> lo, hi float32 [n], rgba float32 [n, 4]."""
    lo = np.array([t[0] for t in tf], F)
    hi = np.array([t[1] for t in tf], F)
    rgba = np.array([t[2] for t in tf], F).reshape(len(tf), 4)
    return lo, hi, rgba


def classify(v, cal_max, lo, hi):
    """The literal scan on (float)((double)v / cal_max), vectorised: int32 classes."""
    n = (np.asarray(v, F).astype(np.float64) / float(cal_max)).astype(F)
    r = np.zeros(n.shape, np.int32)
    for i in range(len(lo)):
        r = np.where((n >= lo[i]) & (n <= hi[i]), np.int32(i), r)
    return r


def _mulv(m, vx, vy, vz):
    """glm mat4 * vec4(x, y, z, 1), w dropped: (m0 x + m1 y) + (m2 z + m3 1); m[column][row]."""
    out = []
    for r in range(3):
        a0 = m[0, r] * vx + m[1, r] * vy
        a1 = m[2, r] * vz + m[3, r] * F(1.0)
        out.append(a0 + a1)
    return out


def positions(shape, p, cam, xs=None):
    """Sample positions in voxel units, three float32 arrays [nx, H, S] (xs: the columns, default all)."""
    mc, iv, tv = oracle.test_matrices(shape, p, cam)
    xs = np.arange(p.width) if xs is None else np.asarray(xs)
    x = xs.astype(F)[:, None, None]
    y = np.arange(p.height, dtype=F)[None, :, None]
    s = np.arange(p.samples_per_ray, dtype=F)[None, None, :]
    q = _mulv(mc, x, y, s)
    q = _mulv(iv, *q)
    q = _mulv(tv, *q)
    full = (len(xs), p.height, p.samples_per_ray)
    return [np.broadcast_to(c, full).astype(F) for c in q]


def _lerp(a, b, w):
    return a * (F(1.0) - w) + b * w


def sample_colors(vol, cal_max, tf, p, cam, xs=None, test_rule=False):
    """RGBA of every sample, float32 [nx, H, S, 4]."""
    vol = np.ascontiguousarray(vol, F)
    d = vol.shape
    lo, hi, rgba = tf_arrays(tf)
    px, py, pz = positions(d, p, cam, xs)
    inside = ((px >= 0) & (px < F(d[0])) & (py >= 0) & (py < F(d[1])) & (pz >= 0) & (pz < F(d[2])))
    col0 = rgba[classify(F(0.0), cal_max, lo, hi)]
    out = np.empty(px.shape + (4,), F)
    out[...] = col0
    P = [c[inside] for c in (px, py, pz)]   # only the in-volume samples go on
    if P[0].size == 0:
        return out
    i0 = [c.astype(np.int32) for c in P]
    w = [c - i.astype(F) for c, i in zip(P, i0)]
    dx, dy, dz = w
    if test_rule:
        flat = vol.reshape(-1)
        total = flat.size
        i1 = [(c + F(1.0)).astype(np.int32) for c in P]
        cc = []
        for k in range(8):   # corner order kernel.cu:124-158: (0,0,0), (0,0,1), (0,1,0), ...
            ix = i1[0] if (k >> 2) & 1 else i0[0]
            iy = i1[1] if (k >> 1) & 1 else i0[1]
            iz = i1[2] if k & 1 else i0[2]
            idx = ix.astype(np.int64) * d[1] * d[2] + iy.astype(np.int64) * d[2] + iz
            ok = idx < total
            v = np.where(ok, flat[np.where(ok, idx, 0)], F(0.0))
            cc.append(rgba[classify(v, cal_max, lo, hi)])
        wy, wx, wz = dy[:, None], dx[:, None], dz[:, None]
        y1, y2 = _lerp(cc[0], cc[2], wy), _lerp(cc[1], cc[3], wy)
        y3, y4 = _lerp(cc[4], cc[6], wy), _lerp(cc[5], cc[7], wy)
        z1, z2 = _lerp(y1, y3, wx), _lerp(y2, y4, wx)
        out[inside] = _lerp(z1, z2, wz)
        return out
    clean = np.where(np.isfinite(vol), vol, F(0.0))
    i1 = [np.minimum(i + 1, n - 1) for i, n in zip(i0, d)]
    c = {}
    for k in range(8):
        ix = i1[0] if (k >> 2) & 1 else i0[0]
        iy = i1[1] if (k >> 1) & 1 else i0[1]
        iz = i1[2] if k & 1 else i0[2]
        c[k] = clean[ix, iy, iz]
    y1, y2 = _lerp(c[0], c[2], dy), _lerp(c[1], c[3], dy)
    y3, y4 = _lerp(c[4], c[6], dy), _lerp(c[5], c[7], dy)
    z1, z2 = _lerp(y1, y3, dx), _lerp(y2, y4, dx)
    v = _lerp(z1, z2, dz)
    out[inside] = rgba[classify(v, cal_max, lo, hi)]
    return out


def render(vol, cal_max, tf, p, cam, xs=None, test_rule=False):
    """The frame (xs: its columns), float32 [nx, H, 4], blended back to front like blendSampleColors."""
    col = sample_colors(vol, cal_max, tf, p, cam, xs, test_rule)
    f = np.empty(col.shape[:2] + (4,), F)
    f[...] = np.array(list(p.background), F)
    for s in range(p.samples_per_ray - 1, -1, -1):
        a = col[:, :, s, 3:4]
        f[..., :3] = f[..., :3] * (F(1.0) - a) + col[:, :, s, :3] * a
    f[..., 3] = F(1.0)
    return f
