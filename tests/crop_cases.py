"""vr_set_crop_box off the default parameters, volume and views -- TEST INFRASTRUCTURE ONLY.  Shared by
tests/test_crop_cases.py (CPU: the table bites) and tests/test_gpu_crop_params.py / tests/test_gpu_random.py
(GPU: the library against tests/crop_ref.py), so they cannot drift apart.  Importing this module needs neither
a GPU nor libvr.so beyond what test_crop_ref needs.

A row is a volume by name (sdvr_cases.volume), an unshaded VR_MODE_DVR param_cases.Case for the view -- the
rows of field_param_cases, reused -- and the isovalues ISO runs at.  Every mode has one zero-transparent
ingredient set (k = 0), SDVR and CDVR a second one under which the value 0 is visible (k = 1: the clip must
not narrow the range and no tile may be culled).  The boxes of a row are the fixed ones of its volume's shape
and the two test_crop_ref.box_of derives from the row's own samples.

The samples of one row (positions, values, and each mode's per-sample colours) are evaluated once and
shared by all its boxes; the frames are cached, computed once per (mode, set, row, isovalue, box).
"""
import numpy as np

import cmap_cases as cc
import cmap_ref
import crop_ref
import dvr_ref
import field_param_cases as fp
import mip_ref
import param_cases as pc
import scdvr_cases as xc
import scdvr_ref
import sdvr_cases as sc
import sdvr_ref
import test_crop_ref as tc

F = np.float32
MODES = tc.MODES                      # dvr, sdvr, cdvr, scdvr, mip, iso
MODE_ID = {"dvr": pc.DVR, "sdvr": fp.SDVR, "cdvr": fp.CDVR, "scdvr": fp.SCDVR, "mip": pc.MIP, "iso": pc.ISO}
N_SETS = {"dvr": 1, "sdvr": 2, "cdvr": 2, "scdvr": 1, "mip": 1, "iso": 1}
BLOB_SHAPE, CUBE_SHAPE = (33, 40, 29), (32, 17, 32)
AWKWARD_VIEWS = ("z", "obl")
CUBE_VPD_VIEWS = ("z", "obl", "x_back")
CUBE_VIEWS = CUBE_VPD_VIEWS + ("y", "z_back")
ISO_CUBE = 200.0


class Row:
    def __init__(self, label, vol, view, isos=None):
        self.label, self.vol, self.view = (vol,) + tuple(label), vol, view
        self.isos = (view.iso,) if isos is None else tuple(float(v) for v in isos)
        self.frame = (view.W, view.H, view.S)

    @property
    def boxes(self):
        """The names of the boxes the row is paired with."""
        if self.vol in pc.DEEP:
            return DEEP_BOXES
        if self.vol in AWKWARD:
            return AWKWARD_BOXES + DERIVED
        return FIXED + DERIVED

    @property
    def shape(self):
        return sc.volume(self.vol)[0].shape


def _rows(vol, labelled, isos=None):
    return [Row(label, vol, view, isos) for label, view in labelled]


def vpd_rows():
    return _rows("blob", fp.vpd_rows())


def view_rows():
    """fp.vpd_rows(), fp.screen_rows() and fp.s1_rows() on the blob."""
    return _rows("blob", fp.view_rows())


def deep_rows(name):
    return _rows(name, fp.deep_rows(), (pc.ISO_DEEP,))


def cal_rows(name):
    return _rows(name, fp.cal_rows())


AWKWARD_ISOS = {"special": pc.ISO_SPECIAL, "subnormal": (pc.ISO_SUBNORMAL,), "small": (pc.ISO_SMALL,)}
AWKWARD = ("special", "subnormal", "small") + tuple(sc.BLOB_CALS)


def awkward_rows(name):
    if name in sc.BLOB_CALS:
        return cal_rows(name)
    return _rows(name, [(("awkward", v), pc.Case(v, pc.DVR)) for v in AWKWARD_VIEWS], AWKWARD_ISOS[name])


def cube_rows():
    """The cube through param_cases.VPD along z, obl and x_back, and along the two views that look at its other
    cut faces at the default parameters."""
    rows = [(label, view) for label, view in fp.vpd_rows() if view.view in CUBE_VPD_VIEWS]
    rows += [(("faces", v), pc.Case(v, pc.DVR)) for v in CUBE_VIEWS if v not in CUBE_VPD_VIEWS]
    return _rows("cube", rows, (ISO_CUBE,))


def blob_face_rows():
    """The blob along the views of cube_rows() (test_cells_and_last_layer)."""
    return _rows("blob", [(("faces", v), pc.Case(v, pc.DVR)) for v in CUBE_VIEWS])


def all_rows():
    out = view_rows() + blob_face_rows() + cube_rows()
    for name in pc.DEEP:
        out += deep_rows(name)
    for name in AWKWARD:
        out += awkward_rows(name)
    return out


# ---- the ingredients ----------------------------------------------------------------------------------
# blob_small's voxels are k * 2^-72: SMOOTH5 in those units.  blob_subnormal's are k * 2^-140 <= 1.8e-40,
# below the narrowest span a colour map can hold (cmap_cases.OPAQUE0_SUBNORMAL): one span with a transparent
# foot, so C(0) is transparent and the voxels take alphas up to 0.4 * 1.8e-40 / 4e-39.
SMOOTH5_SMALL = [(x * pc.SMALL_SCALE, c) for x, c in cc.SMOOTH5]
ZT_SUBNORMAL = [(0.0, (0.0, 0.0, 0.0, 0.0)), (4e-39, (0.9, 0.5, 0.1, 0.4))]
GOPA = tc.GOPA
ISO_RGB, ISO_SHADE = pc.ISO_RGB, pc.SH_KS0
assert (fp.SDVR_SETS[0], fp.CDVR_SETS[0], fp.SCDVR_SETS[0]) == (("default", tc.SHADE), "smooth5", ("smooth5", GOPA, tc.SHADE))


def tf_of(mode, k):
    return sc.tf_of(fp.SDVR_SETS[k][0]) if mode == "sdvr" else pc.default_tf()


def shade_of(mode, k):
    if mode == "iso":
        return ISO_SHADE
    return fp.SDVR_SETS[k][1] if mode == "sdvr" else tc.SHADE


def map_of(vol, k):
    if k == 1:
        return cc.map_of(fp.CDVR_SETS[1])
    if vol == "small":
        return SMOOTH5_SMALL
    if vol == "subnormal":
        return ZT_SUBNORMAL
    return cc.map_of(fp.CDVR_SETS[0])


def ert_tolerance(mode, k, row, flat):
    """The ERT bound of a (mode, set) on a row: `flat` (TOL = 1e-4; S <= 64 here) under the first sets, whose
    colours are the modes' own, and field_param_cases.ert_bound per channel under the second ones."""
    assert row.view.S <= 64
    if k == 0:
        return flat
    return fp.ert_bound(*fp.mode_colours(MODE_ID[mode], k), row.view.bg, 1e-5, row.view.S)


# ---- the boxes ----------------------------------------------------------------------------------------
FIXED = ("cells", "roi", "last_z", "last_x", "thin", "poke")
DERIVED = ("faces", "slab")
AWKWARD_BOXES = ("roi", "cells")
EMPTY = ((10.0, 20.0, 10.0), (30.0, 20.0, 25.0))           # lo[1] == hi[1]
DISJOINT = ((200.0, 200.0, 200.0), (300.0, 300.0, 300.0))
# every lo face past the volume, hi cut on x and z: a cull that projected the box's lo corner with the
# volume's hi corner would see the whole dataset box (test_gpu_crop_params.test_cull_levels_agree)
HI_CUT = ((-3.0, -3.0, -3.0), (12.5, 50.0, 6.5))


def cell_edge(shape):
    """The edge of the marches' ESS cells on a volume of this shape: 8 voxels, doubled until there are at most
    2^18 cells (the rule by which the library sets its dvr_tcb)."""
    tcb = 3
    while np.prod([(d + (1 << tcb) - 1) >> tcb for d in shape], dtype=np.int64) > (1 << 18):
        tcb += 1
    return 1 << tcb


def fixed_box(name, shape):
    """The fixed boxes of the blob's shape (33, 40, 29) and the cube's (32, 17, 32), voxel coordinates."""
    d = tuple(float(n) for n in shape)
    blob = tuple(shape) == BLOB_SHAPE
    assert blob or tuple(shape) == CUBE_SHAPE
    assert cell_edge(shape) == 8
    if name == "cells":      # every face on a multiple of the cell edge
        return ((8.0, 8.0, 8.0), (24.0, 32.0, 24.0) if blob else (24.0, 16.0, 24.0))
    if name == "roi":        # fractional faces off every cell boundary
        return ((6.25, 9.5, 4.75), (20.5, 30.25, 19.0)) if blob else ((6.25, 3.5, 4.75), (20.5, 12.25, 19.0))
    if name == "last_z":     # only the layer [d - 1, d), where the upper corner is clamped
        return ((0.0, 0.0, d[2] - 1.0), d)
    if name == "last_x":
        return ((d[0] - 1.0, 0.0, 0.0), d)
    if name == "thin":       # a quarter voxel strictly between two voxel planes
        return ((-3.0, -3.0, 13.25), (50.0, 50.0, 13.5))
    if name == "poke":       # x: a negative lo and a real hi; y: lo = -0.0 and hi past d; z: a real cut
        return ((-3.5, -0.0, 6.5), (20.75, d[1] + 7.0, 22.0))
    raise KeyError(name)


DEEP_BOXES = ("deep_cells", "deep_off", "slab")


def deep_box(name, shape):
    """A box that cuts a needle of param_cases.DEEP along its length: at cell boundaries (cells 88 to 100 of
    188) and off them; the two short axes reach past the volume."""
    a = int(np.argmax(shape))
    edge = float(cell_edge(shape))
    lo, hi = {"deep_cells": (88.0 * edge, 101.0 * edge), "deep_off": (701.3, 811.6)}[name]
    return (tuple(lo if c == a else -2.0 for c in range(3)), tuple(hi if c == a else 9.0 for c in range(3)))


def derived_box(name, row):
    """test_crop_ref.box_of on the row's own samples: those in the volume that DVR shows under the default TF
    (a non-zero alpha).  The slab of a needle lies across its length, and where every sample of the frame in
    the volume has one z (a view along z at a zero viewplane distance or with one sample per ray) the slab
    lies across x."""
    s = samples(row)
    where = s.inside & (s.colours("dvr", 0)[..., 3] != 0)
    axis = 2
    if row.vol in pc.DEEP:
        axis = int(np.argmax(row.shape))
    elif s.inside.any() and np.ptp(s.P[2][s.inside]) == 0:
        axis = 0
    return tc.box_of(name, row.shape, s.p, s.cam, where=where, axis=axis)


_DERIVED = {}


def box(name, row):
    if name in DERIVED:
        if (row.label, name) not in _DERIVED:
            _DERIVED[(row.label, name)] = derived_box(name, row)
        return _DERIVED[(row.label, name)]
    if name in ("deep_cells", "deep_off"):
        return deep_box(name, row.shape)
    if name == "empty":
        return EMPTY
    if name == "disjoint":
        return DISJOINT
    if name == "hi_cut":
        return HI_CUT
    return fixed_box(name, row.shape)


# ---- one row's samples, evaluated once ----------------------------------------------------------------

class Samples:
    def __init__(self, row):
        self.row = row
        self.vol, self.cal = sc.volume(row.vol)
        self.p, self.cam = row.view.oracle_params(), row.view.oracle_camera()
        self.P = dvr_ref.positions(self.vol.shape, self.p, self.cam)
        self.v, self.inside = mip_ref.sample_values(self.vol, self.p, self.cam)
        self._col = {}

    def colours(self, mode, k):
        """The per-sample colours of a blending mode under ingredient set k (and the record beside them)."""
        if (mode, k) not in self._col:
            vol, cal, p, cam = self.vol, self.cal, self.p, self.cam
            if mode == "dvr":
                c = dvr_ref.sample_colors(vol, cal, tf_of(mode, k), p, cam)
            elif mode == "sdvr":
                c = sdvr_ref.shade_samples(vol, cal, tf_of(mode, k), p, cam, shade_of(mode, k))
            elif mode == "cdvr":
                c = cmap_ref.sample_colors(vol, map_of(self.row.vol, k), p, cam, None, (self.inside, self.v))
            else:
                c = scdvr_ref.lit_samples(vol, map_of(self.row.vol, k), xc.gopa_of(GOPA), p, cam, shade_of(mode, k),
                                          None, (self.inside, self.v))
            self._col[(mode, k)] = c
        return self._col[(mode, k)]

    def caught(self, bx):
        """The samples in the volume and in the box, bool [W, H, S]."""
        return self.inside & crop_ref.points_in_box(self.P, bx)

    def frame(self, mode, k, bx, iso=None):
        """(frame, aux) of crop_ref under the box (None: off)."""
        vol, cal, p, cam = self.vol, self.cal, self.p, self.cam
        aux = None
        if mode == "dvr":
            f = crop_ref.dvr(vol, cal, tf_of(mode, k), p, cam, bx, colors=self.colours(mode, k), P=self.P)
        elif mode == "sdvr":
            f, aux = crop_ref.sdvr(vol, cal, tf_of(mode, k), p, cam, shade_of(mode, k), bx,
                                   colors=self.colours(mode, k), P=self.P)
        elif mode == "cdvr":
            f = crop_ref.cdvr(vol, map_of(self.row.vol, k), p, cam, bx, colors=self.colours(mode, k), P=self.P)
        elif mode == "scdvr":
            f, aux = crop_ref.scdvr(vol, map_of(self.row.vol, k), xc.gopa_of(GOPA), p, cam, shade_of(mode, k), bx,
                                    colors=self.colours(mode, k), P=self.P)
        elif mode == "mip":
            f, aux = crop_ref.mip(vol, cal, p, cam, bx, samples=(self.v, self.inside), P=self.P)
        else:
            f, rec = crop_ref.iso(vol, p, cam, iso, ISO_RGB, ISO_SHADE, bx, samples=(self.v, self.inside), P=self.P)
            aux = rec["hit"]
        return f, aux


_SAMPLES, _FRAMES = {}, {}


def samples(row):
    """The row's samples; one row at a time is kept."""
    if row.label not in _SAMPLES:
        _SAMPLES.clear()
        _SAMPLES[row.label] = Samples(row)
    return _SAMPLES[row.label]


def reference(mode, k, row, bx, iso=None):
    """(frame, number of lit samples / hit rays or None) under the box, cached and read-only."""
    iso = row.isos[0] if mode == "iso" and iso is None else (iso if mode == "iso" else None)
    key = (mode, k, row.label, iso, bx)
    if key not in _FRAMES:
        f, aux = samples(row).frame(mode, k, bx, iso)
        f.setflags(write=False)
        _FRAMES[key] = (f, None if aux is None else int(aux.sum()))
    return _FRAMES[key]


def draws(frame, row):
    return bool(fp.drawn(frame, row.view.bg).any())


# ---- the table: what the restatement measures, as literals ------------------------------------------------
# row label -> (samples in the volume, then per box of Row.boxes the samples in the volume and in the box).
# A fixed box with 0 is a draws-nothing pair: the frame is all background and the pair tests the empty side
# of the culls.  The derived boxes' counts are held as floors (half of them), the fixed ones' exactly where 0.
CAUGHT = {
    ('blob', 'vpd', 2.0, 1.0, 'z'): (10488, 1950, 1287, 456, 0, 456, 3456, 448, 456),
    ('blob', 'vpd', 2.0, 1.0, 'z_back'): (10488, 1950, 1287, 456, 0, 456, 3456, 448, 456),
    ('blob', 'vpd', 2.0, 1.0, 'x'): (11016, 1620, 1248, 0, 408, 0, 3672, 448, 648),
    ('blob', 'vpd', 2.0, 1.0, 'y_back'): (10336, 1710, 1224, 0, 0, 0, 3456, 392, 608),
    ('blob', 'vpd', 2.0, 1.0, 'obl'): (11020, 1764, 1210, 382, 335, 97, 3697, 782, 130),
    ('blob', 'vpd', 2.0, 1.0, 'x_back'): (11016, 1620, 1248, 0, 408, 0, 3672, 336, 648),
    ('blob', 'vpd', 2.0, 1.0, 'y'): (10336, 1710, 1224, 0, 0, 0, 3456, 280, 608),
    ('blob', 'vpd', 0.9, 1.0, 'z'): (8208, 1350, 0, 912, 0, 0, 1728, 256, 456),
    ('blob', 'vpd', 0.9, 1.0, 'z_back'): (8208, 600, 1170, 0, 0, 0, 2016, 320, 456),
    ('blob', 'vpd', 0.9, 1.0, 'x'): (8976, 810, 0, 0, 816, 0, 0, 336, 528),
    ('blob', 'vpd', 0.9, 1.0, 'y_back'): (9044, 1260, 792, 0, 0, 0, 3024, 448, 532),
    ('blob', 'vpd', 0.9, 1.0, 'obl'): (6531, 603, 36, 555, 482, 37, 730, 45, 52),
    ('blob', 'vpd', 0.9, 1.0, 'x_back'): (8976, 945, 1144, 0, 0, 0, 4752, 112, 528),
    ('blob', 'vpd', 0.9, 1.0, 'y'): (9044, 1260, 792, 0, 0, 0, 3024, 56, 532),
    ('blob', 'vpd', 3.5, 1.0, 'z'): (5928, 1200, 702, 456, 0, 0, 2016, 192, 456),
    ('blob', 'vpd', 3.5, 1.0, 'z_back'): (5928, 1050, 819, 0, 0, 0, 2016, 448, 456),
    ('blob', 'vpd', 3.5, 1.0, 'x'): (6120, 1080, 624, 0, 408, 0, 1944, 280, 360),
    ('blob', 'vpd', 3.5, 1.0, 'y_back'): (5814, 990, 648, 0, 0, 0, 1944, 504, 342),
    ('blob', 'vpd', 3.5, 1.0, 'obl'): (6287, 1006, 699, 216, 191, 55, 2115, 382, 125),
    ('blob', 'vpd', 3.5, 1.0, 'x_back'): (6120, 945, 728, 0, 0, 0, 2160, 392, 360),
    ('blob', 'vpd', 3.5, 1.0, 'y'): (5814, 990, 720, 0, 0, 0, 1944, 280, 342),
    ('blob', 'vpd', 0.6, 0.3, 'z'): (29184, 6450, 4329, 0, 0, 456, 11808, 1152, 456),
    ('blob', 'vpd', 0.6, 0.3, 'z_back'): (29184, 6450, 4446, 0, 0, 456, 11808, 1280, 456),
    ('blob', 'vpd', 0.6, 0.3, 'x'): (26112, 5670, 3952, 0, 0, 0, 9288, 1120, 1536),
    ('blob', 'vpd', 0.6, 0.3, 'y_back'): (20672, 5760, 3960, 0, 0, 0, 6912, 392, 1216),
    ('blob', 'vpd', 0.6, 0.3, 'obl'): (28593, 5814, 3858, 840, 745, 269, 10347, 2232, 107),
    ('blob', 'vpd', 0.6, 0.3, 'x_back'): (26112, 5670, 3952, 0, 0, 0, 9504, 1400, 1536),
    ('blob', 'vpd', 0.6, 0.3, 'y'): (20672, 5670, 4032, 0, 0, 0, 6912, 1232, 1216),
    ('blob', 'vpd', -0.5, -0.2, 'z'): (9576, 0, 702, 0, 0, 0, 288, 128, 456),
    ('blob', 'vpd', -0.5, -0.2, 'z_back'): (9576, 750, 0, 1368, 0, 0, 0, 64, 456),
    ('blob', 'vpd', -0.5, -0.2, 'x'): (11424, 270, 832, 0, 0, 0, 6048, 336, 672),
    ('blob', 'vpd', -0.5, -0.2, 'y_back'): (12597, 1170, 576, 0, 0, 0, 4212, 392, 741),
    ('blob', 'vpd', -0.5, -0.2, 'obl'): (8958, 317, 816, 2, 5, 77, 4093, 445, 38),
    ('blob', 'vpd', -0.5, -0.2, 'x_back'): (11424, 0, 0, 0, 1632, 0, 0, 56, 672),
    ('blob', 'vpd', -0.5, -0.2, 'y'): (12597, 1170, 648, 0, 0, 0, 4212, 56, 741),
    ('blob', 'vpd', 0.0, 0.2, 'z'): (29184, 9600, 0, 0, 0, 0, 0, 4096, 1536),
    ('blob', 'vpd', 0.0, 0.2, 'z_back'): (29184, 0, 7488, 0, 0, 0, 18432, 4096, 1536),
    ('blob', 'vpd', 0.0, 0.2, 'x'): (26112, 0, 0, 0, 0, 0, 0, 3584, 1536),
    ('blob', 'vpd', 0.0, 0.2, 'y_back'): (20672, 5760, 4608, 0, 0, 0, 6912, 3584, 1216),
    ('blob', 'vpd', 0.0, 0.2, 'obl'): (24960, 4032, 320, 1472, 1280, 128, 4352, 2368, 704),
    ('blob', 'vpd', 0.0, 0.2, 'x_back'): (26112, 8640, 6656, 0, 0, 0, 13824, 3584, 1536),
    ('blob', 'vpd', 0.0, 0.2, 'y'): (20672, 5760, 4608, 0, 0, 0, 6912, 3584, 1216),
    ('blob', 'screen', 2.0, 0.7, 'z'): (15732, 4030, 2673, 684, 0, 684, 5184, 144, 684),
    ('blob', 'screen', 2.0, 0.7, 'z_back'): (15732, 4030, 2673, 684, 0, 684, 5184, 720, 684),
    ('blob', 'screen', 2.0, 0.7, 'x'): (16524, 3348, 2592, 0, 612, 0, 5508, 1008, 972),
    ('blob', 'screen', 2.0, 0.7, 'y_back'): (21888, 3990, 2754, 0, 0, 0, 7680, 784, 608),
    ('blob', 'screen', 2.0, 0.7, 'obl'): (18149, 3779, 2600, 608, 536, 163, 6209, 1077, 229),
    ('blob', 'screen', 2.0, 0.7, 'x_back'): (16524, 3348, 2592, 0, 612, 0, 5508, 504, 972),
    ('blob', 'screen', 2.0, 0.7, 'y'): (21888, 3990, 2754, 0, 0, 0, 7680, 896, 608),
    ('blob', 'screen', 0.8, 2.6, 'z'): (14352, 2808, 1617, 624, 0, 624, 4836, 855, 624),
    ('blob', 'screen', 0.8, 2.6, 'z_back'): (14352, 2808, 1617, 624, 299, 624, 4680, 285, 624),
    ('blob', 'screen', 0.8, 2.6, 'x'): (15093, 2592, 1764, 351, 559, 0, 5083, 850, 351),
    ('blob', 'screen', 0.8, 2.6, 'y_back'): (16896, 2736, 1785, 1536, 0, 0, 4960, 608, 1536),
    ('blob', 'screen', 0.8, 2.6, 'obl'): (14705, 2535, 1741, 439, 325, 133, 5333, 946, 184),
    ('blob', 'screen', 0.8, 2.6, 'x_back'): (15093, 2592, 1764, 351, 559, 0, 5304, 510, 351),
    ('blob', 'screen', 0.8, 2.6, 'y'): (16896, 2736, 1785, 1536, 352, 0, 4800, 532, 1536),
    ('blob', 'screen', 3.1, 2.325, 'z'): (4485, 702, 440, 195, 345, 195, 1440, 250, 195),
    ('blob', 'screen', 3.1, 2.325, 'z_back'): (4485, 702, 440, 195, 345, 195, 1440, 200, 195),
    ('blob', 'screen', 3.1, 2.325, 'x'): (4455, 648, 480, 0, 165, 0, 1530, 100, 405),
    ('blob', 'screen', 3.1, 2.325, 'y_back'): (4576, 684, 425, 0, 352, 0, 1536, 40, 416),
    ('blob', 'screen', 3.1, 2.325, 'obl'): (4602, 737, 503, 166, 136, 31, 1548, 227, 45),
    ('blob', 'screen', 3.1, 2.325, 'x_back'): (4455, 648, 480, 0, 165, 0, 1530, 20, 405),
    ('blob', 'screen', 3.1, 2.325, 'y'): (4576, 684, 425, 0, 352, 0, 1536, 20, 416),
    ('blob', 's1', 2.0, 0.2, 'z'): (456, 150, 0, 0, 0, 0, 0, 64, 24),
    ('blob', 's1', 2.0, 0.2, 'obl'): (390, 63, 5, 23, 20, 2, 68, 37, 11),
    ('blob', 's1', 0.6, 0.2, 'z'): (456, 150, 0, 0, 0, 0, 0, 64, 24),
    ('blob', 's1', 0.6, 0.2, 'obl'): (390, 63, 5, 23, 20, 2, 68, 37, 11),
    ('blob', 'faces', 'z'): (10488, 1950, 1287, 456, 0, 456, 3456, 448, 456),
    ('blob', 'faces', 'obl'): (11020, 1764, 1210, 382, 335, 97, 3697, 782, 130),
    ('blob', 'faces', 'x_back'): (11016, 1620, 1248, 0, 408, 0, 3672, 336, 648),
    ('blob', 'faces', 'y'): (10336, 1710, 1224, 0, 0, 0, 3456, 280, 608),
    ('blob', 'faces', 'z_back'): (10488, 1950, 1287, 456, 0, 456, 3456, 448, 456),
    ('cube', 'vpd', 2.0, 1.0, 'z'): (9984, 1152, 924, 312, 0, 0, 3120, 1080, 312),
    ('cube', 'vpd', 2.0, 1.0, 'obl'): (9796, 1148, 1009, 303, 304, 75, 3090, 831, 79),
    ('cube', 'vpd', 2.0, 1.0, 'x_back'): (9984, 1152, 924, 0, 312, 416, 3276, 576, 416),
    ('cube', 'vpd', 0.9, 1.0, 'z'): (8736, 720, 0, 624, 0, 0, 1248, 720, 312),
    ('cube', 'vpd', 0.9, 1.0, 'obl'): (6292, 581, 4, 536, 463, 22, 222, 2602, 37),
    ('cube', 'vpd', 0.9, 1.0, 'x_back'): (8736, 720, 924, 0, 0, 364, 4368, 576, 364),
    ('cube', 'vpd', 3.5, 1.0, 'z'): (5616, 648, 528, 0, 0, 0, 1872, 144, 312),
    ('cube', 'vpd', 3.5, 1.0, 'obl'): (5571, 651, 573, 173, 173, 46, 1742, 323, 77),
    ('cube', 'vpd', 3.5, 1.0, 'x_back'): (5616, 648, 528, 0, 312, 234, 1716, 72, 234),
    ('cube', 'vpd', 0.6, 0.3, 'z'): (19968, 3816, 2706, 0, 0, 312, 10608, 2232, 312),
    ('cube', 'vpd', 0.6, 0.3, 'obl'): (23419, 3781, 2875, 494, 568, 225, 8250, 2646, 71),
    ('cube', 'vpd', 0.6, 0.3, 'x_back'): (19968, 3816, 3102, 0, 0, 832, 7488, 1512, 832),
    ('cube', 'vpd', -0.5, -0.2, 'z'): (12168, 504, 1320, 0, 0, 0, 2704, 648, 312),
    ('cube', 'vpd', -0.5, -0.2, 'obl'): (9060, 91, 1246, 0, 0, 68, 4199, 2260, 29),
    ('cube', 'vpd', -0.5, -0.2, 'x_back'): (12168, 504, 0, 0, 1248, 507, 0, 936, 507),
    ('cube', 'vpd', 0.0, 0.2, 'z'): (19968, 4608, 0, 0, 0, 0, 0, 4608, 832),
    ('cube', 'vpd', 0.0, 0.2, 'obl'): (20480, 3648, 0, 960, 896, 192, 1600, 4928, 512),
    ('cube', 'vpd', 0.0, 0.2, 'x_back'): (19968, 4608, 4224, 0, 0, 832, 9984, 4608, 832),
    ('cube', 'faces', 'y'): (9792, 1152, 1089, 0, 0, 408, 3264, 864, 408),
    ('cube', 'faces', 'z_back'): (9984, 1152, 924, 312, 0, 0, 3120, 1008, 312),
    ('deep_x', 'deep', 'z', 1.2): (33, 3, 3, 1),
    ('deep_x', 'deep', 'x', 1.2): (24, 1, 1, 1),
    ('deep_x', 'deep', 'y_back', 1.2): (33, 3, 3, 1),
    ('deep_x', 'deep', 'obl', 1.2): (0, 0, 0, 0),
    ('deep_x', 'deep', 'obl', 0.02): (12, 12, 12, 12),
    ('deep_z', 'deep', 'z', 1.2): (24, 1, 1, 1),
    ('deep_z', 'deep', 'x', 1.2): (33, 3, 3, 1),
    ('deep_z', 'deep', 'y_back', 1.2): (30, 3, 3, 1),
    ('deep_z', 'deep', 'obl', 1.2): (0, 0, 0, 0),
    ('deep_z', 'deep', 'obl', 0.02): (17, 17, 17, 17),
    ('special', 'awkward', 'z'): (10488, 1287, 1950, 448, 456),
    ('special', 'awkward', 'obl'): (11020, 1210, 1764, 782, 130),
    ('subnormal', 'awkward', 'z'): (10488, 1287, 1950, 448, 456),
    ('subnormal', 'awkward', 'obl'): (11020, 1210, 1764, 782, 130),
    ('small', 'awkward', 'z'): (10488, 1287, 1950, 448, 456),
    ('small', 'awkward', 'obl'): (11020, 1210, 1764, 782, 130),
    ('blob200', 'cal', 'z'): (10488, 1287, 1950, 512, 456),
    ('blob200', 'cal', 'obl'): (11020, 1210, 1764, 886, 125),
    ('blob1000', 'cal', 'z'): (10488, 1287, 1950, 224, 456),
    ('blob1000', 'cal', 'obl'): (11020, 1210, 1764, 656, 125),
}

# the derived boxes under which ISO finds no sample at its isovalue although it draws with the box off (a box
# between the last data layer and the empty one, a quarter-voxel slab of the cube at 200, the one sample a
# needle's slab catches): the frame still changes and the other five modes draw
ISO_MISSES = {
    (("blob", "vpd", -0.5, -0.2, "z_back"), "faces"), (("cube", "vpd", 0.0, 0.2, "z"), "slab"),
    (("cube", "vpd", 0.0, 0.2, "obl"), "slab"), (("cube", "vpd", 0.0, 0.2, "x_back"), "faces"),
    (("cube", "vpd", 0.0, 0.2, "x_back"), "slab"),
} | {((n, "deep", v, 1.2), "slab") for n in pc.DEEP for v in ("z", "x", "y_back")}
# the 0.02 screen sees 15 voxels of a needle: every box of the row holds all its samples (the frame is the
# box-off one, through the CROP marches)
DEEP_WHOLE = {(n, "deep", "obl", 0.02) for n in pc.DEEP}


def caught(row, name):
    """The table's count of a row's box."""
    return CAUGHT[row.label][1 + row.boxes.index(name)]



# ---- the random views ---------------------------------------------------------------------------------
RANDOM_STREAM = 7


def random_boxes(seed, shape, n=fp.RANDOM_VIEWS):
    """One box per view of field_param_cases.random_view_cases(seed): per axis, with probability 1/4 the whole
    axis (past the volume on both sides), otherwise lo < hi uniform in [-2, d + 2] with at least 3 voxels
    between them."""
    rng = np.random.default_rng([seed, RANDOM_STREAM])
    out = []
    for _ in range(n):
        lo, hi = [], []
        for d in shape:
            if rng.random() < 0.25:
                a, b = -5.0, d + 5.0
            else:
                while True:
                    a, b = np.sort(rng.uniform(-2.0, d + 2.0, 2))
                    if b - a >= 3.0:
                        break
            lo.append(float(F(a)))
            hi.append(float(F(b)))
        out.append((tuple(lo), tuple(hi)))
    return out


def random_references(view, bx):
    """{mode: frame} of one random view on avg152 under a box, the six modes from one evaluation of the view's
    samples (the first ingredient sets; ISO at test_crop_ref.ISO_VALUE).  Not cached."""
    s = Samples(Row(("random",), "avg152", view, (tc.ISO_VALUE,)))
    return {m: s.frame(m, 0, bx, tc.ISO_VALUE)[0] for m in MODES}, int(s.caught(bx).sum())


# ---- the library's side -------------------------------------------------------------------------------

def gpu_params(mode, k, view, flags=0):
    """The library's parameters of a view case in a mode under ingredient set k."""
    p = view.gpu_params(flags=flags)
    p.mode = MODE_ID[mode]
    p.shade_ambient, p.shade_diffuse, p.shade_specular, p.shade_shininess = shade_of(mode, k)
    return p


def apply_set(ctx, mode, k, vol):
    """A mode's ingredient set k on a context holding the named volume (ISO's isovalue apart)."""
    if mode in ("dvr", "sdvr"):
        ctx.set_transfer_function(tf_of(mode, k))
    elif mode in ("cdvr", "scdvr"):
        ctx.set_colormap(map_of(vol, k))
        if mode == "scdvr":
            ctx.set_gradient_opacity(xc.gopa_of(GOPA))
