"""vr_set_crop_box restated in numpy float32 -- TEST INFRASTRUCTURE ONLY (the definition the GPU marches
are held to, bit for bit; include/vr_api.h vr_set_crop_box).

Built from the six modes' restatements by composition (imported, not copied; none of them changes):

  in the box   lo[a] <= p_a < hi[a] on every axis: float32 compares of dvr_ref.positions against the box's
               float32 bounds, no arithmetic
  DVR, CDVR    dvr_ref.sample_colors / cmap_ref.sample_colors, the samples not in the box replaced by the
               mode's outside colour (TF((float)(0.0f / cal_max)), C(0.0f)), then the mode's blend
  SDVR, SCDVR  sdvr_ref.shade_samples / scdvr_ref.lit_samples likewise: every sample is lit on its own, from
               the whole volume, so replacing the samples not in the box leaves exactly the in-box ones lit
  MIP          mip_ref.sample_values with inside &= in_box, then mip_ref.render's maximum and pixel
  ISO          iso_ref.render's steps with the box in all three in-volume tests (the hit, sample s_h - 1, every
               bisection midpoint), on iso_ref._positions_at, _value and _value_where; the gradient taps
               and the light read the whole volume

box = (lo, hi), or None for the box off (the mode's own restatement).

Each function takes what does not depend on the box ready-made (colors / samples: the mode's per-sample
colours or values, P: the frame's positions), so that the samples of one frame are evaluated once for all
its boxes (tests/crop_cases.py); the frames are the same bit for bit either way.
"""
import numpy as np

import cmap_ref
import dvr_ref
import iso_ref
import mip_ref
import oracle
import scdvr_ref
import sdvr_ref

F = np.float32


def box_arrays(box):
    return np.array(box[0], F), np.array(box[1], F)


def points_in_box(P, box):
    """The rule itself on three float32 arrays of positions."""
    lo, hi = box_arrays(box)
    with np.errstate(invalid="ignore"):
        return ((P[0] >= lo[0]) & (P[0] < hi[0]) & (P[1] >= lo[1]) & (P[1] < hi[1]) &
                (P[2] >= lo[2]) & (P[2] < hi[2]))


def in_box(shape, p, cam, box, xs=None, P=None):
    """The in-box mask of every sample of the frame, bool [nx, H, S] (all True with the box off).  P: the
    frame's dvr_ref.positions, to share them among the boxes of one frame."""
    if P is None:
        P = dvr_ref.positions(shape, p, cam, xs)
    if box is None:
        return np.ones(P[0].shape, bool)
    return points_in_box(P, box)


def _replace(col, keep, outside):
    col = col.copy()
    col[~keep] = outside
    return col


def tf_outside(cal_max, tf):
    lo, hi, rgba = dvr_ref.tf_arrays(tf)
    return rgba[dvr_ref.classify(F(0.0), cal_max, lo, hi)]


def cmap_outside(points):
    return cmap_ref.C(points, np.zeros(1, F))[0]


def dvr(vol, cal_max, tf, p, cam, box, xs=None, colors=None, P=None):
    """The VR_MODE_DVR frame under the box, float32 [nx, H, 4] (colors: dvr_ref.sample_colors' result, to
    share one frame's samples among its boxes)."""
    col = dvr_ref.sample_colors(vol, cal_max, tf, p, cam, xs) if colors is None else colors
    col = _replace(col, in_box(np.shape(vol), p, cam, box, xs, P), tf_outside(cal_max, tf))
    return cmap_ref.blend(col, p)   # (dvr_ref.render's blend, as a function of the colours)


def sdvr(vol, cal_max, tf, p, cam, shade, box, xs=None, colors=None, P=None):
    """(frame, lit bool [nx, H, S]): VR_MODE_SDVR under the box and its shaded samples (colors:
    sdvr_ref.shade_samples' (col, record), to share one frame's samples among its boxes)."""
    col, rec = sdvr_ref.shade_samples(vol, cal_max, tf, p, cam, shade, xs) if colors is None else colors
    keep = in_box(np.shape(vol), p, cam, box, xs, P)
    col = _replace(col, keep, tf_outside(cal_max, tf))
    with np.errstate(over="ignore", invalid="ignore"):
        return cmap_ref.blend(col, p), rec["shaded"] & keep


def cdvr(vol, points, p, cam, box, xs=None, samples=None, colors=None, P=None):
    """The VR_MODE_CDVR frame under the box (colors: cmap_ref.sample_colors' result under these points)."""
    col = cmap_ref.sample_colors(vol, points, p, cam, xs, samples) if colors is None else colors
    col = _replace(col, in_box(np.shape(vol), p, cam, box, xs, P), cmap_outside(points))
    return cmap_ref.blend(col, p)


def scdvr(vol, points, gopa, p, cam, shade, box, xs=None, samples=None, colors=None, P=None):
    """(frame, lit bool [nx, H, S]): VR_MODE_SCDVR under the box and its lit samples (colors:
    scdvr_ref.lit_samples' (col, record) under these ingredients)."""
    col, rec = scdvr_ref.lit_samples(vol, points, gopa, p, cam, shade, xs, samples) if colors is None else colors
    keep = in_box(np.shape(vol), p, cam, box, xs, P)
    col = _replace(col, keep, cmap_outside(points))
    with np.errstate(over="ignore", invalid="ignore"):
        return cmap_ref.blend(col, p), rec["lit"] & keep


def mip(vol, cal_max, p, cam, box, xs=None, samples=None, P=None):
    """(frame, hit bool [nx, H]): VR_MODE_MIP under the box -- mip_ref.render with inside &= in_box
    (samples: mip_ref.sample_values' (v, inside))."""
    v, inside = mip_ref.sample_values(vol, p, cam, xs) if samples is None else samples
    inside = inside & in_box(np.shape(vol), p, cam, box, xs, P)
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
    return f, hit


def iso(vol, p, cam, iso_value, rgb, shade, box, xs=None, samples=None, P=None):
    """(frame, record {hit, s_h, refinable}): VR_MODE_ISO under the box -- iso_ref.render's steps, the box in
    the hit test, in the test of sample s_h - 1 and in the test of every bisection midpoint (samples:
    mip_ref.sample_values' (v, inside))."""
    vol = np.ascontiguousarray(vol, F)
    dims = vol.shape
    iso_value = F(iso_value)
    ka, kd, ks, shin = (F(c) for c in shade)
    S = p.samples_per_ray
    v, inside = mip_ref.sample_values(vol, p, cam, xs) if samples is None else samples
    inside = inside & in_box(dims, p, cam, box, xs, P)
    with np.errstate(invalid="ignore"):
        ge = inside & (v >= iso_value)
    hit = ge.any(axis=2)
    s_h = np.where(hit, ge.argmax(axis=2), 0).astype(np.int32)
    rec = {"hit": hit, "s_h": s_h, "refinable": np.zeros(hit.shape, bool)}
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

    def ok_at(P):
        ok = iso_ref._inside(P, dims)
        return ok if box is None else ok & points_in_box(P, box)

    prev = np.maximum(sh - 1, 0)
    refinable = (sh > 0) & inside[ix, iy, prev]
    hi = sh.astype(F)
    lo = np.where(refinable, (sh - 1).astype(F), hi)
    for _ in range(iso_ref.REFINE):
        mid = (lo + hi) * F(0.5)
        P = iso_ref._positions_at(mats, x, y, mid)
        ok = ok_at(P)
        with np.errstate(invalid="ignore"):
            take = ok & (iso_ref._value_where(clean, P, ok) >= iso_value)
        hi = np.where(refinable & take, mid, hi)
        lo = np.where(refinable & ~take, mid, lo)
    ps = iso_ref._positions_at(mats, x, y, hi)

    g = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for a in range(3):   # the taps read the whole volume
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
        zero = np.zeros(x.shape, F)
        pb = iso_ref._positions_at(mats, x, y, zero + F(S - 1 if S > 1 else 0))
        pa = iso_ref._positions_at(mats, x, y, zero)
        e = [b - a for a, b in zip(pa, pb)]
        n2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        has_l = n2 > 0
        il = F(1.0) / np.sqrt(np.where(has_l, n2, F(1.0)))
        L = [-c * il for c in e]
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
    return frame, rec
