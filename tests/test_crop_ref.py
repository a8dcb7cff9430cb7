"""tests/crop_ref.py (the numpy restatement of vr_set_crop_box) held to the six modes' own restatements,
and the boxes, ingredients and cached references tests/test_gpu_crop.py shares (no GPU).

A box containing the volume gives each mode's own reference bit for bit; a box disjoint from the volume
gives the background (MIP, ISO) or the all-TF(0) blend; the `faces` box takes its bounds from actual
sample coordinates of the frame, so samples sit exactly on its faces: those with p_a == lo[a] are kept,
those with p_a == hi[a] dropped.
"""
import ctypes as C

import numpy as np
import pytest

import cmap_cases as cc
import cmap_ref
import crop_ref
import dvr_ref
import iso_ref
import mip_ref
import oracle
import param_cases as pc
import scdvr_cases as xc
import scdvr_ref
import sdvr_ref
import volumerenderingproject_amd as vr
from test_gpu_dvr import camera_pair

F = np.float32
MODES = ("dvr", "sdvr", "cdvr", "scdvr", "mip", "iso")
FRAMES = [(64, 48, 64), (37, 91, 50)]
VIEWS = ["default", "reset", "inside"]

# ---- the ingredients of every mode (zero transparent, and the two fog variants) -----------------------
SHADE = pc.SH_N0                 # SDVR, SCDVR: a coefficient set of param_cases.SHADE_BITWISE
ISO_VALUE, ISO_RGB, ISO_SHADE = 100.0, pc.ISO_RGB, pc.SH_KS0
GOPA = "edges"


def tf_of(variant):
    """The default TF, or ("fog") the same with the class of the value 0 at alpha 0.3: interval 0 of the
    default TF holds 0, and the fog TF repeats it with alpha 0.3 as its last interval (the scan keeps the
    last interval containing the value)."""
    tf = pc.default_tf()
    if variant == "fog":
        lo, hi, rgba = tf[0]
        assert lo <= 0.0 <= hi
        tf = tf + [(0.0, 0.0, (0.3, 0.6, 0.9, 0.3))]
    return tf


FOG_MAP = [(-10.0, (0.1, 0.2, 0.3, 0.3)), (0.0, (0.1, 0.2, 0.3, 0.3)), (60.0, (0.9, 0.5, 0.1, 0.4)),
           (200.0, (0.2, 0.9, 0.6, 0.1))]


def map_of(variant, cal):
    return FOG_MAP if variant == "fog" else cc.map_of("smooth5", cal)


# ---- the boxes ----------------------------------------------------------------------------------------
AVG_BOXES = {
    "cut": ((0.0, 0.0, 0.0), (45.5, 109.0, 91.0)),
    "roi": ((20.25, 30.5, 17.75), (70.5, 80.25, 60.0)),     # no face on an 8-voxel cell boundary
    "whole": ((-5.0, -5.0, -5.0), (200.0, 200.0, 200.0)),
    "out": ((200.0, 200.0, 200.0), (300.0, 300.0, 300.0)),
    "empty": ((10.0, 50.0, 10.0), (80.0, 50.0, 80.0)),      # lo[1] == hi[1]
}
BOX_NAMES = ("cut", "roi", "slab", "faces", "whole", "out", "empty")
DRAWS_NOTHING = ("out", "empty")


def _ray_positions(shape, p, cam, x, y):
    P = dvr_ref.positions(shape, p, cam, xs=[x])
    return [c[0, y, :] for c in P]


def _in_volume(P, shape, margin=(0.0, 0.0, 0.0)):
    ok = np.ones(P[0].shape, bool)
    for a in range(3):
        ok &= (P[a] >= margin[a]) & (P[a] < shape[a] - margin[a])
    return ok


def box_of(name, shape, p, cam, where=None, axis=2):
    """The named box for a frame: the fixed ones, and the two taken from the frame's own samples.
    slab   a z range thinner than one sample step, around the z of a sample of the centre ray in the volume
           (10 voxels from its z faces, a quarter of the depth where the volume is shallower); the other two
           axes reach past the volume.  axis: the slab's axis where it is not z
    faces  lo and hi are the positions of two samples, a third and two thirds of the way along the rays of
           the pixels a quarter and three quarters into the frame (sorted per axis)
    where (bool [W, H, S]; the frames off the default parameters, tests/crop_cases.py): the samples the boxes
    are taken from -- those of the frame that lie in the volume and show.  slab takes the middle one of the
    centre ray's, away from the z faces as above; failing that the middle one of the whole frame's, away from
    the faces and then anywhere; and the volume's middle z when `where` is empty.  faces takes the pixels a
    quarter and three quarters into the bounding rectangle of the rays with such samples, and on the two rays
    the sample a third and two thirds of the way along their run of them.  An axis on which the two positions
    coincide (a single sample per ray, a zero viewplane distance) is widened by a quarter voxel either side."""
    if name in AVG_BOXES:
        return AVG_BOXES[name]
    W, H, S = p.width, p.height, p.samples_per_ray
    if name == "slab":
        def slab(z, half):
            lo, hi = [-5.0] * 3, [max(200.0, d + 5.0) for d in shape]
            lo[axis], hi[axis] = z - half, z + half
            return (tuple(lo), tuple(hi))

        P = _ray_positions(shape, p, cam, W // 2, H // 2)
        m = [0.0, 0.0, 0.0]
        m[axis] = min(10.0, shape[axis] / 4.0)
        ok = _in_volume(P, shape, m)
        if where is not None:
            ok = np.nonzero(ok & where[W // 2, H // 2])[0]
            Q = dvr_ref.positions(shape, p, cam)
            for margin in (m, (0.0, 0.0, 0.0)):
                if len(ok):
                    break
                ix, iy, js = np.nonzero(_in_volume(Q, shape, margin) & where)
                if len(js):
                    j = len(js) // 2
                    P, ok = [c[ix[j], iy[j], :] for c in Q], js[j:j + 1]
            if len(ok) == 0:
                return slab(shape[axis] / 2.0, 0.25)
        else:
            ok = np.nonzero(ok)[0]
        s = int(ok[len(ok) // 2])
        z = float(P[axis][s])
        step = abs(float(P[axis][min(s + 1, S - 1)]) - float(P[axis][max(s - 1, 0)])) / 2.0
        half = 0.2 * step if step > 0 else 0.25      # (a view along which z does not move: a quarter voxel)
        return slab(z, half)
    if name == "faces":
        xa, ya, xb, yb = W // 4, H // 4, (3 * W) // 4, (3 * H) // 4
        sa, sb = S // 3, (2 * S) // 3
        if where is not None and where.any():
            met = where.any(axis=2)
            xs, ys = np.nonzero(met.any(axis=1))[0], np.nonzero(met.any(axis=0))[0]
            x0, x1, y0, y1 = int(xs[0]), int(xs[-1]) + 1, int(ys[0]), int(ys[-1]) + 1
            xa, ya = x0 + (x1 - x0) // 4, y0 + (y1 - y0) // 4
            xb, yb = x0 + (3 * (x1 - x0)) // 4, y0 + (3 * (y1 - y0)) // 4
            ia, ib = np.nonzero(where[xa, ya])[0], np.nonzero(where[xb, yb])[0]
            if len(ia):
                sa = int(ia[len(ia) // 3])
            if len(ib):
                sb = int(ib[(2 * len(ib)) // 3])
        A = _ray_positions(shape, p, cam, xa, ya)
        B = _ray_positions(shape, p, cam, xb, yb)
        a = [float(c[sa]) for c in A]
        b = [float(c[sb]) for c in B]
        lo, hi = [min(u, v) for u, v in zip(a, b)], [max(u, v) for u, v in zip(a, b)]
        if where is not None:
            for c in range(3):
                if lo[c] == hi[c]:
                    lo[c], hi[c] = lo[c] - 0.25, hi[c] + 0.25
        return (tuple(lo), tuple(hi))
    raise KeyError(name)


# ---- the references, one per (mode, volume, frame, view, box, variant), shared read-only ---------------
_REFS, _SAMPLES = {}, {}


def oracle_view(view, W, H, S):
    return oracle.params(W, H, S), camera_pair(oracle, view, W, H)[1]


def reference(mode, key, vol, cal, W, H, S, view, box, variant="zt", xs=None):
    """(frame, aux) of crop_ref under `box` (None: off).  aux: lit samples (SDVR, SCDVR), hit rays (MIP, ISO)."""
    k = (mode, key, W, H, S, view, box, variant, None if xs is None else tuple(xs))
    if k not in _REFS:
        p, cam = oracle_view(view, W, H, S)
        aux = None
        if mode == "dvr":
            f = crop_ref.dvr(vol, cal, tf_of(variant), p, cam, box, xs)
        elif mode == "sdvr":
            f, aux = crop_ref.sdvr(vol, cal, tf_of(variant), p, cam, SHADE, box, xs)
        elif mode in ("cdvr", "scdvr"):
            sk = (key, W, H, S, view, None if xs is None else tuple(xs))
            if sk not in _SAMPLES:
                _SAMPLES.clear()   # (one frame's samples at a time)
                _SAMPLES[sk] = cmap_ref.sample_values(vol, p, cam, xs)
            if mode == "cdvr":
                f = crop_ref.cdvr(vol, map_of(variant, cal), p, cam, box, xs, _SAMPLES[sk])
            else:
                f, aux = crop_ref.scdvr(vol, map_of(variant, cal), xc.gopa_of(GOPA), p, cam, SHADE, box, xs,
                                        _SAMPLES[sk])
        elif mode == "mip":
            f, aux = crop_ref.mip(vol, cal, p, cam, box, xs)
        else:
            f, rec = crop_ref.iso(vol, p, cam, ISO_VALUE, ISO_RGB, ISO_SHADE, box, xs)
            aux = rec["hit"]
        f.setflags(write=False)
        _REFS[k] = (f, None if aux is None else int(aux.sum()))
    return _REFS[k]


def own_reference(mode, vol, cal, W, H, S, view):
    """The mode's own restatement, without crop_ref."""
    p, cam = oracle_view(view, W, H, S)
    if mode == "dvr":
        return dvr_ref.render(vol, cal, tf_of("zt"), p, cam)
    if mode == "sdvr":
        return sdvr_ref.render(vol, cal, tf_of("zt"), p, cam, SHADE)[0]
    if mode == "cdvr":
        return cmap_ref.render(vol, map_of("zt", cal), p, cam)
    if mode == "scdvr":
        return scdvr_ref.render(vol, map_of("zt", cal), xc.gopa_of(GOPA), p, cam, SHADE)[0]
    if mode == "mip":
        return mip_ref.render(vol, cal, p, cam)[0]
    return iso_ref.render(vol, p, cam, ISO_VALUE, ISO_RGB, ISO_SHADE)[0]


def bits_equal(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def background(W, H, S):
    return np.array(list(oracle.params(W, H, S).background), F)[:3]


# ---- the CPU tests ------------------------------------------------------------------------------------
CPU_FRAME = (37, 91, 50)


@pytest.mark.parametrize("mode", MODES)
def test_box_containing_the_volume_is_the_mode(avg152, mode):
    vol, cal = avg152
    W, H, S = CPU_FRAME
    for view in ("default", "reset"):
        own = own_reference(mode, vol, cal, W, H, S, view)
        for box in (AVG_BOXES["whole"], ((0.0, 0.0, 0.0), tuple(float(d) for d in vol.shape)), None):
            assert bits_equal(reference(mode, "avg", vol, cal, W, H, S, view, box)[0], own), (mode, view, box)
        assert np.any(own[..., :3] != background(W, H, S)), (mode, view)


@pytest.mark.parametrize("mode", MODES)
def test_disjoint_and_empty_boxes(avg152, mode):
    vol, cal = avg152
    W, H, S = CPU_FRAME
    p, cam = oracle_view("reset", W, H, S)
    bg = background(W, H, S)
    for name in DRAWS_NOTHING:
        f, aux = reference(mode, "avg", vol, cal, W, H, S, "reset", AVG_BOXES[name])
        assert np.all(f[..., :3] == bg) and np.all(f[..., 3] == 1.0), (mode, name)
        assert not aux
    if mode in ("dvr", "cdvr"):   # fog: every sample is the outside colour -- the all-TF(0) blend
        outside = crop_ref.tf_outside(cal, tf_of("fog")) if mode == "dvr" else crop_ref.cmap_outside(map_of("fog", cal))
        assert outside[3] == F(0.3)
        col = np.empty((W, H, S, 4), F)
        col[...] = outside
        fog = cmap_ref.blend(col, p)
        f, _ = reference(mode, "avg", vol, cal, W, H, S, "reset", AVG_BOXES["out"], "fog")
        assert bits_equal(f, fog) and np.all(np.any(f[..., :3] != bg, axis=-1))


def test_faces_keep_lo_and_drop_hi(avg152):
    vol, cal = avg152
    W, H, S = CPU_FRAME
    p, cam = oracle_view("default", W, H, S)
    box = box_of("faces", vol.shape, p, cam)
    lo, hi = crop_ref.box_arrays(box)
    assert np.all(lo < hi)
    P = dvr_ref.positions(vol.shape, p, cam)
    keep = crop_ref.in_box(vol.shape, p, cam, box)
    inside = mip_ref.sample_values(vol, p, cam)[1]
    on_lo = np.zeros(keep.shape, bool)
    on_hi = np.zeros(keep.shape, bool)
    for a in range(3):
        others = np.ones(keep.shape, bool)
        for b in range(3):
            if b != a:
                others &= (P[b] >= lo[b]) & (P[b] < hi[b])
        on_lo |= (P[a] == lo[a]) & others
        on_hi |= (P[a] == hi[a]) & others
    # samples exactly on each kind of face, in the volume, on every axis the default view fixes per pixel
    assert (on_lo & inside).sum() >= 20 and (on_hi & inside).sum() >= 20
    assert keep[on_lo & ~on_hi].all() and not keep[on_hi].any()
    # and they count: MIP over the box moved by one ulp on either kind of face differs in its sample set
    v, _ = mip_ref.sample_values(vol, p, cam)
    grown = (tuple(np.nextafter(lo, F(-np.inf))), tuple(np.nextafter(hi, F(np.inf))))
    assert crop_ref.in_box(vol.shape, p, cam, grown).sum() >= keep.sum() + on_hi.sum()
    shrunk = (tuple(np.nextafter(lo, F(np.inf))), box[1])
    assert crop_ref.in_box(vol.shape, p, cam, shrunk).sum() <= keep.sum() - (on_lo & ~on_hi).sum()
    for mode in MODES:
        f, _ = reference(mode, "avg", vol, cal, W, H, S, "default", box)
        assert np.any(f[..., :3] != background(W, H, S)), mode


def test_boxes_bite(avg152):
    """cut, roi and slab change every mode's frame and still draw something."""
    vol, cal = avg152
    W, H, S = CPU_FRAME
    p, cam = oracle_view("reset", W, H, S)
    for mode in MODES:
        own = reference(mode, "avg", vol, cal, W, H, S, "reset", None)[0]
        for name in ("cut", "roi", "slab"):
            f, _ = reference(mode, "avg", vol, cal, W, H, S, "reset", box_of(name, vol.shape, p, cam))
            assert not bits_equal(f, own), (mode, name)
            assert np.any(f[..., :3] != background(W, H, S)), (mode, name)


def test_null_context_is_einval():
    lo, hi, on = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), C.c_int32()
    assert vr.lib().vr_set_crop_box(None, lo, hi) == -1
    assert vr.lib().vr_set_crop_box(None, None, None) == -1
    assert vr.lib().vr_get_crop_box(None, lo, hi, C.byref(on)) == -1
