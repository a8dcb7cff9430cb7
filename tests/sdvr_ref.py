"""VR_MODE_SDVR restated in numpy float32 -- TEST INFRASTRUCTURE ONLY (the definition the GPU march is
held to, bit for bit; include/vr_api.h VR_MODE_SDVR).

Every float operation is one numpy float32 ufunc, so each is rounded on its own, like dvr_ref, mip_ref
and iso_ref, whose functions it is built from (imported, not copied): the sample, value, tap and
position arithmetic is the pinned one by construction.

  samples    dvr_ref.sample_colors (position, in-volume test, value, class, colour) and
             mip_ref.sample_values' in-volume mask
  shaded     the samples in the volume with alpha != 0; every other sample keeps its DVR colour
  gradient   at the sample's own position p (dvr_ref.positions), per axis a: q+ = min(p_a + 1, d_a - 1),
             q- = max(p_a - 1, 0), g_a = (v+ - v-) / (q+ - q-) (0 when the span is 0), the taps by
             iso_ref._value; N = -g / |g| when |g|^2 > 0
  light      once per ray, iso_ref._positions_at: e = p(S > 1 ? S - 1 : 0) - p(0); L = -e / |e| when |e|^2 > 0
  two-sided  ndl = N.L; ndl < 0 negates N before the law
  colour     shade_normal: d = max(N.L, 0), spec = d > 0 ? ks exp2(n log2 d) : (n == 0 ? ks : 0); without N
             or L: d = 1, spec = 0; channel = c * (ka + kd d) + spec, alpha unchanged
  blend      dvr_ref.render's: back to front, f = f * (1 - a) + c' * a, alpha 1
"""
import numpy as np

import dvr_ref
import iso_ref
import mip_ref
import oracle

F = np.float32


def shade_samples(vol, cal_max, tf, p, cam, shade, xs=None):
    """(col, record): the colours of every sample after shading, float32 [nx, H, S, 4], and per sample
    [nx, H, S]: shaded, has_normal (bool), ndl (float32, N.L before the flip; 0 without a normal or a
    light), d (float32; 1 where unshaded or without a normal or a light) and N [nx, H, S, 3] (before the
    flip; 0 without a normal)."""
    vol = np.ascontiguousarray(vol, F)
    dims = vol.shape
    ka, kd, ks, shin = (F(c) for c in shade)
    S = p.samples_per_ray
    col = dvr_ref.sample_colors(vol, cal_max, tf, p, cam, xs).copy()
    inside = mip_ref.sample_values(vol, p, cam, xs)[1]
    shaded = inside & (col[..., 3] != 0)
    rec = {"shaded": shaded, "has_normal": np.zeros(shaded.shape, bool), "ndl": np.zeros(shaded.shape, F),
           "d": np.ones(shaded.shape, F), "N": np.zeros(shaded.shape + (3,), F)}
    ix, iy, is_ = np.nonzero(shaded)
    if ix.size == 0:
        return col, rec
    pos = dvr_ref.positions(dims, p, cam, xs)
    ps = [c[ix, iy, is_] for c in pos]
    clean = np.where(np.isfinite(vol), vol, F(0.0))
    xs_all = np.arange(p.width) if xs is None else np.asarray(xs)
    mats = oracle.test_matrices(dims, p, cam)

    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        # gradient of the trilinear field at p
        g = []
        for a in range(3):
            qp = np.minimum(ps[a] + F(1.0), F(dims[a] - 1))
            qm = np.maximum(ps[a] - F(1.0), F(0.0))
            vp = iso_ref._value(clean, [qp if c == a else ps[c] for c in range(3)])
            vm = iso_ref._value(clean, [qm if c == a else ps[c] for c in range(3)])
            span = qp - qm
            g.append(np.where(span > 0, (vp - vm) / span, F(0.0)).astype(F))
        len2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        has_n = len2 > 0
        inv = F(1.0) / np.sqrt(np.where(has_n, len2, F(1.0)))
        N = [np.where(has_n, -c * inv, F(0.0)).astype(F) for c in g]

        # headlight along the ray, once per ray
        x = np.broadcast_to(xs_all.astype(F)[:, None], shaded.shape[:2]).astype(F)
        y = np.broadcast_to(np.arange(p.height, dtype=F)[None, :], shaded.shape[:2]).astype(F)
        zero = np.zeros(x.shape, F)
        pb = iso_ref._positions_at(mats, x, y, zero + F(S - 1 if S > 1 else 0))
        pa = iso_ref._positions_at(mats, x, y, zero)
        e = [b - a for a, b in zip(pa, pb)]
        n2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        has_l_ray = n2 > 0
        il = F(1.0) / np.sqrt(np.where(has_l_ray, n2, F(1.0)))
        L = [(-c * il)[ix, iy] for c in e]
        has_l = has_l_ray[ix, iy]

        # two-sided: a normal facing away from the light is negated (exact) before the law
        lit = has_n & has_l
        ndl0 = (N[0] * L[0] + N[1] * L[1]) + N[2] * L[2]
        flip = lit & (ndl0 < 0)
        Nf = [np.where(flip, -c, c).astype(F) for c in N]

        # shade_normal
        ndl = (Nf[0] * L[0] + Nf[1] * L[1]) + Nf[2] * L[2]
        d = np.where(lit, np.where(ndl > 0, ndl, F(0.0)), F(1.0)).astype(F)
        pw = np.exp2(shin * np.log2(np.where(d > 0, d, F(1.0)))).astype(F)
        spec = np.where(d > 0, ks * pw, ks if shin == 0 else F(0.0)).astype(F)
        spec = np.where(lit, spec, F(0.0)).astype(F)
        k = ka + kd * d
        for c in range(3):
            col[ix, iy, is_, c] = col[ix, iy, is_, c] * k + spec

    rec["has_normal"][ix, iy, is_] = has_n
    rec["ndl"][ix, iy, is_] = np.where(lit, ndl0, F(0.0))
    rec["d"][ix, iy, is_] = d
    for c in range(3):
        rec["N"][ix, iy, is_, c] = N[c]
    return col, rec


def render(vol, cal_max, tf, p, cam, shade, xs=None):
    """(frame float32 [nx, H, 4], record) -- xs: the frame's columns; shade = (ka, kd, ks, shininess)."""
    col, rec = shade_samples(vol, cal_max, tf, p, cam, shade, xs)
    f = np.empty(col.shape[:2] + (4,), F)
    f[...] = np.array(list(p.background), F)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(p.samples_per_ray - 1, -1, -1):
            a = col[:, :, s, 3:4]
            f[..., :3] = f[..., :3] * (F(1.0) - a) + col[:, :, s, :3] * a
    f[..., 3] = F(1.0)
    return f, rec
