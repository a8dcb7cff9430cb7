"""VR_MODE_ISO restated in numpy float32 -- TEST INFRASTRUCTURE ONLY (the definition the GPU march is
held to, bit for bit; include/vr_api.h VR_MODE_ISO).

Every float operation is one numpy float32 ufunc, so each is rounded on its own, like dvr_ref and
mip_ref.  The march is mip_ref.sample_values (all samples of the frame); everything after the hit is
vectorised over the hit rays.

  samples    mip_ref.sample_values: DVR's positions, in-volume test and value
  hit        s_h = the smallest s whose sample is in the volume with v >= iso (a NaN never hits)
  refine     only when s_h > 0 and sample s_h - 1 is in the volume: lo = s_h - 1, hi = s_h, VR_ISO_REFINE
             rounds of mid = (lo + hi) * 0.5; in the volume with v(mid) >= iso -> hi = mid, else lo = mid
  gradient   per axis a: q+ = min(p*_a + 1, d_a - 1), q- = max(p*_a - 1, 0), g_a = (v+ - v-) / (q+ - q-)
             (0 when the span is 0) at p* = p(hi); N = -g / |g| when |g|^2 > 0
  light      e = p(S > 1 ? S - 1 : 0) - p(0); L = -e / |e| when |e|^2 > 0
  colour     shade_normal: d = max(N.L, 0), spec = d > 0 ? ks exp2(n log2 d) : (n == 0 ? ks : 0); without N
             or L: d = 1, spec = 0; channel = rgb_c * (ka + kd d) + spec, alpha 1; no hit: the background
"""
import numpy as np

import dvr_ref
import mip_ref
import oracle

F = np.float32
REFINE = 6   # vr_api.h VR_ISO_REFINE


def _positions_at(mats, x, y, fs):
    """The position chain at float sample coordinates: three float32 arrays shaped like x, y, fs."""
    mc, iv, tv = mats
    q = dvr_ref._mulv(mc, x, y, fs)
    q = dvr_ref._mulv(iv, *q)
    return dvr_ref._mulv(tv, *q)


def _inside(P, d):
    return ((P[0] >= 0) & (P[0] < F(d[0])) & (P[1] >= 0) & (P[1] < F(d[1])) & (P[2] >= 0) & (P[2] < F(d[2])))


def _value(clean, P):
    """The trilinear value at in-volume points P (three float32 arrays): mip_ref.sample_values' block."""
    d = clean.shape
    i0 = [c.astype(np.int32) for c in P]
    dx, dy, dz = [c - i.astype(F) for c, i in zip(P, i0)]
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
        return dvr_ref._lerp(z1, z2, dz)


def _value_where(clean, P, ok):
    """_value at the points where ok, 0 elsewhere."""
    v = np.zeros(P[0].shape, F)
    if ok.any():
        v[ok] = _value(clean, [c[ok] for c in P])
    return v


def render(vol, p, cam, iso, rgb, shade, xs=None):
    """(frame float32 [nx, H, 4], record) -- xs: the frame's columns; shade = (ka, kd, ks, shininess).

    record: per ray [nx, H]: hit, s_h (int32, 0 without a hit), refinable, lo, hi (float32), has_normal,
    d (float32; 1 without a normal or a light), and N [nx, H, 3] (0 without a normal)."""
    vol = np.ascontiguousarray(vol, F)
    dims = vol.shape
    iso = F(iso)
    ka, kd, ks, shin = (F(c) for c in shade)
    S = p.samples_per_ray
    v, inside = mip_ref.sample_values(vol, p, cam, xs)
    with np.errstate(invalid="ignore"):
        ge = inside & (v >= iso)
    hit = ge.any(axis=2)
    s_h = np.where(hit, ge.argmax(axis=2), 0).astype(np.int32)
    nx, H = hit.shape
    rec = {"hit": hit, "s_h": s_h, "refinable": np.zeros(hit.shape, bool), "lo": np.zeros(hit.shape, F),
           "hi": np.zeros(hit.shape, F), "has_normal": np.zeros(hit.shape, bool), "d": np.ones(hit.shape, F),
           "N": np.zeros(hit.shape + (3,), F)}
    frame = np.empty(hit.shape + (4,), F)
    frame[..., :3] = np.array(list(p.background), F)[:3]
    frame[..., 3] = F(1.0)
    ix, iy = np.nonzero(hit)
    if ix.size == 0:
        return frame, rec
    xs_all = np.arange(p.width) if xs is None else np.asarray(xs)
    mats = oracle.test_matrices(dims, p, cam)
    clean = np.where(np.isfinite(vol), vol, F(0.0))
    x, y = xs_all[ix].astype(F), iy.astype(F)
    sh = s_h[ix, iy]

    # refinement
    prev = np.maximum(sh - 1, 0)
    refinable = (sh > 0) & inside[ix, iy, prev]
    hi = sh.astype(F)
    lo = np.where(refinable, (sh - 1).astype(F), hi)
    for _ in range(REFINE):
        mid = (lo + hi) * F(0.5)
        P = _positions_at(mats, x, y, mid)
        ok = _inside(P, dims)
        with np.errstate(invalid="ignore"):
            take = ok & (_value_where(clean, P, ok) >= iso)
        hi = np.where(refinable & take, mid, hi)
        lo = np.where(refinable & ~take, mid, lo)
    ps = _positions_at(mats, x, y, hi)

    # gradient of the trilinear field at p*
    g = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for a in range(3):
            qp = np.minimum(ps[a] + F(1.0), F(dims[a] - 1))
            qm = np.maximum(ps[a] - F(1.0), F(0.0))
            vp = _value(clean, [qp if c == a else ps[c] for c in range(3)])
            vm = _value(clean, [qm if c == a else ps[c] for c in range(3)])
            span = qp - qm
            g.append(np.where(span > 0, (vp - vm) / span, F(0.0)).astype(F))
        len2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        has_n = len2 > 0
        inv = F(1.0) / np.sqrt(np.where(has_n, len2, F(1.0)))
        N = [np.where(has_n, -c * inv, F(0.0)).astype(F) for c in g]

        # headlight along the ray
        zero = np.zeros(x.shape, F)
        pb = _positions_at(mats, x, y, zero + F(S - 1 if S > 1 else 0))
        pa = _positions_at(mats, x, y, zero)
        e = [b - a for a, b in zip(pa, pb)]
        n2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        has_l = n2 > 0
        il = F(1.0) / np.sqrt(np.where(has_l, n2, F(1.0)))
        L = [-c * il for c in e]

        # shade_normal
        lit = has_n & has_l
        ndl = (N[0] * L[0] + N[1] * L[1]) + N[2] * L[2]
        d = np.where(lit, np.where(ndl > 0, ndl, F(0.0)), F(1.0)).astype(F)
        pw = np.exp2(shin * np.log2(np.where(d > 0, d, F(1.0)))).astype(F)
        spec = np.where(d > 0, ks * pw, ks if shin == 0 else F(0.0)).astype(F)
        spec = np.where(lit, spec, F(0.0)).astype(F)
        k = ka + kd * d
        for c in range(3):
            frame[ix, iy, c] = F(rgb[c]) * k + spec

    rec["refinable"][ix, iy] = refinable
    rec["lo"][ix, iy] = lo
    rec["hi"][ix, iy] = hi
    rec["has_normal"][ix, iy] = has_n
    rec["d"][ix, iy] = d
    for c in range(3):
        rec["N"][ix, iy, c] = N[c]
    return frame, rec
