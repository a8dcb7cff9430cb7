"""VR_MODE_SCDVR restated in numpy float32 -- TEST INFRASTRUCTURE ONLY (the definition the GPU march and
vr_gradient_opacity_eval are held to, bit for bit; include/vr_api.h VR_MODE_SCDVR).

Every float operation is one numpy float32 ufunc, so each is rounded on its own.  Built from the other
restatements (imported, not copied): the samples, the colour map and the blend are cmap_ref's, the
positions dvr_ref's, the taps iso_ref._value, the ray's end points iso_ref._positions_at; the lighting
steps follow sdvr_ref.shade_samples operation for operation, and tests/test_scdvr_ref.py holds the two to
each other bit for bit through colour maps that equal an interval TF.

  samples    cmap_ref.sample_values (position, in-volume test, value) and cmap_ref.sample_colors (C(v);
             C(0) outside the volume)
  lit        the samples in the volume with alpha != 0; every other sample keeps its CDVR colour and alpha
  gradient   at the sample's own position p, per axis a: q+ = min(p_a + 1, d_a - 1), q- = max(p_a - 1, 0),
             g_a = (v+ - v-) / (q+ - q-) (0 when the span is 0); len2 = (g_x^2 + g_y^2) + g_z^2;
             mag = sqrt(len2); N = -g * (1 / mag) when len2 > 0
  opacity    a' = a * G(mag): G is cmap_ref.C with one channel over the points (m_i, w_i)
  light      once per ray: e = p(S > 1 ? S - 1 : 0) - p(0); L = -e / |e| when |e|^2 > 0
  two-sided  ndl = N.L; ndl < 0 negates N before the law
  colour     d = max(N.L, 0), spec = d > 0 ? ks exp2(n log2 d) : (n == 0 ? ks : 0); without N or L: d = 1,
             spec = 0; channel = c * (ka + kd d) + spec
  blend      cmap_ref.blend: back to front, f = f * (1 - a') + c' * a', alpha 1
"""
import numpy as np

import cmap_ref
import dvr_ref
import iso_ref
import oracle

F = np.float32

UNIT = [(0.0, 1.0)]   # a context's first gradient-opacity map


def G(gopa, mag):
    """The gradient-opacity map at the float32 magnitudes mag: the colour map's law with one channel."""
    return cmap_ref.C([(m, (w, w, w, w)) for m, w in gopa], mag)[..., 3]


def lit_samples(vol, points, gopa, p, cam, shade, xs=None, samples=None):
    """(col, record): the colours and alphas of every sample after lighting and gradient opacity, float32
    [nx, H, S, 4], and per sample [nx, H, S]: lit, has_normal (bool), mag (float32; 0 where not lit),
    g (float32, the weight G(mag); 1 where not lit), d (float32; 1 where not lit or without a normal or a
    light) and ndl (float32, N.L before the flip; 0 without a normal or a light)."""
    vol = np.ascontiguousarray(vol, F)
    dims = vol.shape
    ka, kd, ks, shin = (F(c) for c in shade)
    S = p.samples_per_ray
    if samples is None:
        samples = cmap_ref.sample_values(vol, p, cam, xs)
    inside = samples[0]
    col = cmap_ref.sample_colors(vol, points, p, cam, xs, samples).copy()
    lit = inside & (col[..., 3] != 0)
    rec = {"lit": lit, "has_normal": np.zeros(lit.shape, bool), "mag": np.zeros(lit.shape, F),
           "g": np.ones(lit.shape, F), "d": np.ones(lit.shape, F), "ndl": np.zeros(lit.shape, F)}
    ix, iy, is_ = np.nonzero(lit)
    if ix.size == 0:
        return col, rec
    pos = dvr_ref.positions(dims, p, cam, xs)
    ps = [c[ix, iy, is_] for c in pos]
    clean = np.where(np.isfinite(vol), vol, F(0.0))
    xs_all = np.arange(p.width) if xs is None else np.asarray(xs)
    mats = oracle.test_matrices(dims, p, cam)

    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        g = []
        for a in range(3):
            qp = np.minimum(ps[a] + F(1.0), F(dims[a] - 1))
            qm = np.maximum(ps[a] - F(1.0), F(0.0))
            vp = iso_ref._value(clean, [qp if c == a else ps[c] for c in range(3)])
            vm = iso_ref._value(clean, [qm if c == a else ps[c] for c in range(3)])
            span = qp - qm
            g.append(np.where(span > 0, (vp - vm) / span, F(0.0)).astype(F))
        len2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        mag = np.sqrt(len2).astype(F)
        has_n = len2 > 0
        inv = F(1.0) / np.where(has_n, mag, F(1.0))
        N = [np.where(has_n, -c * inv, F(0.0)).astype(F) for c in g]

        # gradient opacity, with or without a normal
        gw = G(gopa, mag)
        col[ix, iy, is_, 3] = col[ix, iy, is_, 3] * gw

        # headlight along the ray, once per ray
        x = np.broadcast_to(xs_all.astype(F)[:, None], lit.shape[:2]).astype(F)
        y = np.broadcast_to(np.arange(p.height, dtype=F)[None, :], lit.shape[:2]).astype(F)
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
        both = has_n & has_l
        ndl0 = (N[0] * L[0] + N[1] * L[1]) + N[2] * L[2]
        flip = both & (ndl0 < 0)
        Nf = [np.where(flip, -c, c).astype(F) for c in N]

        ndl = (Nf[0] * L[0] + Nf[1] * L[1]) + Nf[2] * L[2]
        d = np.where(both, np.where(ndl > 0, ndl, F(0.0)), F(1.0)).astype(F)
        pw = np.exp2(shin * np.log2(np.where(d > 0, d, F(1.0)))).astype(F)
        spec = np.where(d > 0, ks * pw, ks if shin == 0 else F(0.0)).astype(F)
        spec = np.where(both, spec, F(0.0)).astype(F)
        k = ka + kd * d
        for c in range(3):
            col[ix, iy, is_, c] = col[ix, iy, is_, c] * k + spec

    rec["has_normal"][ix, iy, is_] = has_n
    rec["mag"][ix, iy, is_] = mag
    rec["g"][ix, iy, is_] = gw
    rec["d"][ix, iy, is_] = d
    rec["ndl"][ix, iy, is_] = np.where(both, ndl0, F(0.0))
    return col, rec


def render(vol, points, gopa, p, cam, shade, xs=None, samples=None):
    """(frame float32 [nx, H, 4], record) -- xs: the frame's columns; shade = (ka, kd, ks, shininess)."""
    col, rec = lit_samples(vol, points, gopa, p, cam, shade, xs, samples)
    with np.errstate(over="ignore", invalid="ignore"):
        return cmap_ref.blend(col, p), rec
