"""Volumes, views, parameter cases and reference calls off the defaults -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_param_cases.py (CPU: the cases are not vacuous) and tests/test_gpu_params.py /
tests/test_gpu_volumes.py / tests/test_gpu_shade.py (GPU: the library against the references), so
they cannot drift apart.
Importing this module needs neither a GPU nor libvr.so: the library's cameras and parameters are
built on first use (gpu_camera, gpu_params).

References: VRC is the oracle's octree march (OracleOctree.render_vrc; render_vrc_shaded for a case
with shading coefficients), TEST oracle.render_test, DVR
tests/dvr_ref.py, MIP tests/mip_ref.py, ISO tests/iso_ref.py (the case carries the isovalue, the surface
colour and the shading coefficients the context is given).  A volume with non-finite voxels takes the closed-form octree (implicit=True): the
literal tree's search recurses past its leaves when max == min is false (NaN), the closed form
returns x > 0 ? x : 0 -- what the library's classify kernel states -- and equals the literal tree bit
for bit on finite volumes (tests/test_param_cases.py, tests/test_oracle_pin.py).
"""
import numpy as np

import dvr_ref
import iso_ref
import mip_ref
import oracle

F = np.float32
VRC, TEST, DVR, MIP, ISO = 1, 5, 6, 7, 8  # vr_api.h VR_MODE_*
SHADE, CONIC = 8, 16              # vr_api.h VR_FLAG_SHADE, VR_FLAG_CONIC
MODES = {"vrc": VRC, "test": TEST, "dvr": DVR, "mip": MIP, "iso": ISO}

W, H, S = 48, 36, 64              # the frame of every case but the tiny shapes
RSW = 2.0
DEFAULT_BG = (0.2, 0.2, 0.2, 1.0)

# name -> (position, up): derive_camera / camera_derive at scale * position
VIEWS = {
    "z": ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0)),
    "z_back": ((0.0, 0.0, -1.0), (0.0, 1.0, 0.0)),
    "x": ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
    "y_back": ((0.0, -1.0, 0.0), (0.0, 0.0, 1.0)),
    "obl": ((0.6, 0.5, 0.7), (0.0, 1.0, 0.0)),
    "x_back": ((-1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
    "y": ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0)),
}
AXIS_VIEWS = ("z", "z_back", "x", "y_back", "x_back", "y")   # with these every face of the volume is looked at

# VRC march cases: name -> (sample_distance, front_clip_plane); None = the default 2 / S
SD_FC = {
    "default": (None, 0.0),
    "fc_in": (None, 0.9),          # the first sample lies inside the data
    "fc_neg": (None, -0.7),
    "sd_big": (0.11, 0.0),         # rays leave the unit cube, more than 7 leaves per step, pad off
    "sd_small": (0.004, 0.8),      # the whole ray stays within a few leaves
    "sd_neg": (-2.0 / 64, 2.0),    # the march direction flips
    "sd_zero": (0.0, 1.0),         # S copies of one point
}

# TEST / DVR cases: (viewplane_distance, camera scale)
VPD = [(2.0, 1.0), (0.9, 1.0), (3.5, 1.0),
       (0.6, 0.3),                 # the camera sits inside the box
       (-0.5, -0.2),               # mc[10] = -vpd / S is positive: the march axis runs the other way
       (0.0, 0.2)]                 # every sample in the camera plane

# (real_screen_width, real_screen_height): anamorphic, anamorphic the other way, far
SCREENS = [(2.0, 0.7), (0.8, 2.6), (3.1, 3.1 * H / W)]

# tiny volumes: frame 40 x 30 x 48; shape -> real_screen_width (height = width * H / W).  Every shape
# draws at least one pixel in VRC and in TEST along z, x and obl at 1.2 (tests/test_param_cases.py), so
# no shape needed a narrower screen.
TW, TH, TS = 40, 30, 48
TINY = {
    (1, 1, 1): 1.2, (2, 3, 5): 1.2, (5, 4, 3): 1.2, (1, 9, 4): 1.2, (7, 1, 2): 1.2, (3, 3, 1): 1.2,
    (9, 8, 7): 1.2, (17, 5, 33): 1.2, (65, 3, 2): 1.2,
}
TINY_VALUES = (0.0, 50.0, 112.0, 150.0, 255.0)   # default TF: class 0, each coloured class, above every interval

# the deep shapes: depth 11, 2048 leaves a side for 9,000 voxels -- the largest LDS carve-up of the shaded
# march (leaf maps + three raw maps + sample table).  Tiny frame, see deep_cases().
DEEP = {"deep_x": (1500, 3, 2), "deep_z": (2, 3, 1500)}

# shading coefficient sets (ka, kd, ks, shininess), VR_FLAG_SHADE.  The device evaluates d^shininess
# with its hardware exp2 / log2, the oracle with exp2f / log2f; everything else of the stage is the
# same IEEE operations in the same order.  So the frame is the oracle's bit for bit where the specular
# term is exact: ks = 0 (spec = 0 * finite = +0 and x + 0 = x) and shininess = 0 (spec = ks *
# exp2(0 * log2 d) = ks).  (1, 0, 0, n) is the identity: k = 1 + 0 * d = 1, rgb * 1 + 0 = rgb.
SH_KS0 = (0.3, 0.7, 0.0, 16.0)
SH_N0 = (0.2, 0.5, 0.4, 0.0)
SH_ID = (1.0, 0.0, 0.0, 7.0)
SH_GEN = (0.3, 0.7, 0.2, 16.0)
SH_SHARP = (0.1, 0.6, 0.9, 96.0)
SHADE_SETS = {"ks0": SH_KS0, "n0": SH_N0, "id": SH_ID, "gen": SH_GEN, "sharp": SH_SHARP}
SHADE_BITWISE = ("ks0", "n0", "id")
ISO_RGB = (0.9, 0.8, 0.7)         # the surface colour of an ISO case unless it names another

SPECIAL = (np.nan, np.inf, -np.inf, -1.0, -0.0, 255.5, 256.0, 1e30, -1e30, 1e-40, 3.4e38, 127.49999)


def _blob_rng():
    rng = np.random.default_rng(3)
    vol = np.zeros((33, 40, 29), F)
    vol[4:28, 6:33, 3:25] = rng.integers(0, 256, (24, 27, 22)).astype(F)
    return vol, rng


def blob():
    """(33, 40, 29), integers 0..255 in a box strictly inside the volume, zeros around it."""
    return _blob_rng()[0]


def blob_special():
    """blob() with 600 of its non-zero voxels replaced by the SPECIAL values in turn."""
    vol, rng = _blob_rng()
    flat = vol.reshape(-1)
    nz = np.flatnonzero(flat)
    pick = rng.choice(nz, 600, replace=False)
    with np.errstate(over="ignore"):
        flat[pick] = np.array([SPECIAL[i % len(SPECIAL)] for i in range(600)], np.float64).astype(F)
    return vol


SUBNORMAL_SCALE = 2.0 ** -140
SUBNORMAL_CAL = 255.0 * 2.0 ** -140   # (a double: the value is below float32's normal range)


def blob_subnormal():
    """blob() * 2^-140: every voxel an exact subnormal float32 (k * 2^-140, k = 0..255), so a march that
    flushes subnormals -- on a load, in a lerp or in a compare -- renders the all-zero volume instead.
    With cal_max = SUBNORMAL_CAL the normalised values are blob()'s k / 255."""
    vol = blob() * F(SUBNORMAL_SCALE)
    assert vol.dtype == F
    return vol


SMALL_SCALE = 2.0 ** -72
SMALL_CAL = 255.0 * 2.0 ** -72


def blob_small():
    """blob() * 2^-72: every voxel a normal float32, every gradient component of the trilinear field
    about 2^-72 times an integer ratio -- so ISO's len2 = (gx gx + gy gy) + gz gz is a subnormal (down to
    2^-149) or underflows to 0, and 1 / sqrt(len2) is the correctly rounded square root of a subnormal.
    With cal_max = SMALL_CAL the normalised values are blob()'s k / 255."""
    vol = blob() * F(SMALL_SCALE)
    assert vol.dtype == F
    return vol


# ISO's isovalues off the blob's 128: on blob_special() from below every voxel to above every one, the
# blob's 128 on the two scaled volumes, and the needles' median
ISO_SPECIAL = (-1e30, -0.5, 1e-40, 100.0, 255.5, 1e30, 3.4e38)
ISO_SUBNORMAL = float(F(128) * F(SUBNORMAL_SCALE))
ISO_SMALL = float(F(128) * F(SMALL_SCALE))
ISO_DEEP = 112.0


def cube():
    """(32, 17, 32): integers 0..255, those below 120 zeroed.  x and z fill the octree cube and no face
    is empty, so the one-sided differences of the shading stage at the six faces are visible."""
    v = np.random.default_rng(11).integers(0, 256, (32, 17, 32)).astype(F)
    v[v < 120] = 0
    return v


def tiny_volume(shape):
    """Seeded by the shape (seed word 3: with it the single voxel of (1, 1, 1) draws a coloured class)."""
    return np.random.default_rng([3, *shape]).choice(np.array(TINY_VALUES, F), size=shape).astype(F)


def deep_cases(view, **kw):
    """The frames of a deep shape along a view.  The data is a needle 1500 voxels long and 3 x 2 / 2048
    of the cube across.  "wide" sees its whole length (axis views only: the oblique rays of a 1.2
    screen step over it); "narrow" is a 0.02 screen around the centre with 48 samples of 0.002 about
    it, where every view, obl included, draws (tests/test_param_cases.py)."""
    centre = float(np.sqrt(np.sum(np.square(VIEWS[view][0]))))
    narrow = Case(view, VRC, rsw=0.02, sd=0.002, fc=centre - 0.048, frame=(TW, TH, TS), **kw)
    wide = Case(view, VRC, rsw=1.2, frame=(TW, TH, TS), **kw)
    return [narrow] if view == "obl" else [wide, narrow]


def deep_volume_cases(mode, **kw):
    """The frames of a deep shape in DVR, MIP and ISO (no sample distance or front clip there: the ray is the
    viewplane distance long).  The 1.2 screen sees the needle along z, x and y_back and steps over it
    along obl -- a frame of background through the whole march, kept as a case -- and the 0.02 screen
    draws along obl (tests/test_param_cases.py)."""
    frame = (TW, TH, TS)
    return [Case(view, mode, rsw=1.2, frame=frame, **kw) for view in ("z", "x", "y_back", "obl")] + \
        [Case("obl", mode, rsw=0.02, frame=frame, **kw)]


def default_tf():
    """The default transfer function as [(lo, hi, rgba)] from the oracle (no libvr.so needed)."""
    arr, n = oracle.default_tf()
    return [(arr[i].lo, arr[i].hi, tuple(arr[i].rgba)) for i in range(n)]


def tf_zero_visible():
    """The default TF plus a last interval [0, 0] with alpha 0.1: the class of the value 0 is a visible
    one, so a voxel that must read as 0 (negative, -0.0, NaN in VRC and DVR) shows when it does not."""
    return default_tf() + [(0.0, 0.0, (0.3, 0.6, 0.9, 0.1))]


class Case:
    """One frame's runtime inputs: the numbers both sides are built from."""

    def __init__(self, view, mode=VRC, sd=None, fc=0.0, vpd=2.0, scale=1.0, rsw=RSW, rsh=None, bg=DEFAULT_BG,
                 conic=False, frame=(W, H, S), shade=None, iso=128.0, rgb=ISO_RGB):
        self.view, self.mode, self.fc, self.vpd, self.scale = view, mode, float(fc), float(vpd), float(scale)
        self.W, self.H, self.S = frame
        self.sd = 2.0 / self.S if sd is None else float(sd)
        self.rsw = float(rsw)
        self.rsh = self.rsw * self.H / self.W if rsh is None else float(rsh)
        self.bg = tuple(float(b) for b in bg)
        self.conic = bool(conic)
        if shade is None and mode == ISO:   # (the mode is always shaded: its coefficients, not VR_FLAG_SHADE)
            shade = SH_KS0
        self.shade = None if shade is None else tuple(float(c) for c in shade)   # (ka, kd, ks, shininess)
        if self.shade is not None and mode not in (VRC, ISO):
            raise ValueError("shading is defined for VRC and ISO only")
        self.iso = float(iso)                      # ISO: the context's isovalue and surface colour
        self.rgb = tuple(float(c) for c in rgb)

    def plain(self):
        """The same case without shading."""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.shade = None
        return c

    def key(self):
        return (self.view, self.mode, self.sd, self.fc, self.vpd, self.scale, self.rsw, self.rsh, self.bg,
                self.conic, self.W, self.H, self.S, self.shade, self.iso, self.rgb)

    def pos_up(self):
        pos, up = VIEWS[self.view]
        return tuple(self.scale * c for c in pos), up

    def oracle_camera(self):
        pos, up = self.pos_up()
        if self.conic:
            return oracle.camera_derive_conic(pos, up, self.rsw, self.rsh, self.vpd)
        return oracle.camera_derive(pos, up, self.rsw, self.rsh)

    def oracle_params(self):
        p = oracle.params(self.W, self.H, self.S)
        p.real_screen_width, p.real_screen_height = self.rsw, self.rsh
        p.viewplane_distance, p.front_clip_plane, p.sample_distance = self.vpd, self.fc, self.sd
        for i in range(4):
            p.background[i] = self.bg[i]
        p.conic = 1 if self.conic else 0
        return p

    def gpu_camera(self):
        import volumerenderingproject_amd as vr
        pos, up = self.pos_up()
        if self.conic:
            return vr.derive_camera_conic(pos, up, self.rsw, self.rsh, self.vpd)
        return vr.derive_camera(pos, up, self.rsw, self.rsh)

    def gpu_params(self, flags=0, ert_epsilon=1e-5):
        import volumerenderingproject_amd as vr
        # (VR_MODE_ISO reads the shade_* fields without VR_FLAG_SHADE, which it refuses)
        flags |= (CONIC if self.conic else 0) | (SHADE if self.shade is not None and self.mode != ISO else 0)
        p = vr.default_params(self.W, self.H, self.S, mode=self.mode, flags=flags, ert_epsilon=ert_epsilon)
        if self.shade is not None:
            p.shade_ambient, p.shade_diffuse, p.shade_specular, p.shade_shininess = self.shade
        p.real_screen_width, p.real_screen_height = self.rsw, self.rsh
        p.viewplane_distance, p.front_clip_plane, p.sample_distance = self.vpd, self.fc, self.sd
        for i in range(4):
            p.background[i] = self.bg[i]
        return p


def sd_fc_case(name, view, **kw):
    sd, fc = SD_FC[name]
    return Case(view, VRC, sd=sd, fc=fc, **kw)


class Reference:
    """The references of one volume, each frame computed once and shared read-only.

    literal=False takes the closed-form octree for VRC (required when a voxel is not finite)."""

    def __init__(self, vol, cal_max, tf=None, literal=True):
        self.vol = np.ascontiguousarray(vol, F)
        self.cal = float(cal_max)
        self.tf = tf if tf is not None else default_tf()
        self.otf = oracle.tf_array(self.tf)
        self.literal = literal
        if literal and not np.all(np.isfinite(self.vol)):
            raise ValueError("the literal octree's search does not terminate on non-finite voxels")
        self._octree = None
        self._frames = {}
        self._mips = {}
        self._isos = {}

    @property
    def octree(self):
        if self._octree is None:
            self._octree = oracle.OracleOctree(self.vol, implicit=not self.literal)
        return self._octree

    def frame(self, case):
        k = case.key()
        if k not in self._frames:
            p, cam = case.oracle_params(), case.oracle_camera()
            if case.mode == ISO:
                f = self.iso(case)[0]
            elif case.shade is not None:
                f = self.octree.render_vrc_shaded(self.cal, self.otf, p, cam, case.shade)
            elif case.mode == VRC:
                f = self.octree.render_vrc(self.cal, self.otf, p, cam)
            elif case.mode == TEST:
                f = oracle.render_test(self.vol, self.cal, self.otf, p, cam)
            elif case.mode == MIP:
                f = self.mip(case)[0]
            else:
                f = dvr_ref.render(self.vol, self.cal, self.tf, p, cam)
            f.setflags(write=False)
            self._frames[k] = f
        return self._frames[k]

    def mip(self, case):
        """mip_ref.render's (frame, m, hit) of a MIP case: the running maximum and the in-volume mask too."""
        k = case.key()
        if k not in self._mips:
            out = mip_ref.render(self.vol, self.cal, case.oracle_params(), case.oracle_camera())
            for a in out:
                a.setflags(write=False)
            self._mips[k] = out
        return self._mips[k]

    def iso(self, case):
        """iso_ref.render's (frame, record) of an ISO case: s_h, refinable, lo, hi, has_normal, d and N too."""
        k = case.key()
        if k not in self._isos:
            frame, rec = iso_ref.render(self.vol, case.oracle_params(), case.oracle_camera(), case.iso, case.rgb,
                                        case.shade)
            frame.setflags(write=False)
            for a in rec.values():
                a.setflags(write=False)
            self._isos[k] = (frame, rec)
        return self._isos[k]

    def inside(self, case):
        """The in-volume mask [W, H, S] of a case's samples (mip_ref.sample_values'), not cached."""
        return mip_ref.sample_values(self.vol, case.oracle_params(), case.oracle_camera())[1]

    def count_in_samples(self, case):
        return self.octree.count_in_samples(case.oracle_params(), case.oracle_camera())


_SHARED = {}


def shared_reference(name):
    """The Reference of a named volume, one per process: "blob", "avg152", "special" / "special200"
    (blob_special at cal_max 255 / 200.7, closed-form octree), "special_tf0" (blob_special under
    tf_zero_visible), "cube", "subnormal" (blob_subnormal at SUBNORMAL_CAL; DVR, MIP and ISO only), "small"
    (blob_small at SMALL_CAL; ISO), "deep_x" / "deep_z" (closed-form octree)."""
    if name not in _SHARED:
        if name == "blob":
            _SHARED[name] = Reference(blob(), 255.0)
        elif name == "special":
            _SHARED[name] = Reference(blob_special(), 255.0, literal=False)
        elif name == "special200":
            _SHARED[name] = Reference(blob_special(), 200.7, literal=False)
        elif name == "special_tf0":
            _SHARED[name] = Reference(blob_special(), 255.0, tf=tf_zero_visible(), literal=False)
        elif name == "cube":
            _SHARED[name] = Reference(cube(), 255.0)
        elif name == "subnormal":
            _SHARED[name] = Reference(blob_subnormal(), SUBNORMAL_CAL, literal=False)
        elif name == "small":
            _SHARED[name] = Reference(blob_small(), SMALL_CAL, literal=False)
        elif name in DEEP:   # (a literal octree of depth 11 is out of reach: closed form)
            _SHARED[name] = Reference(tiny_volume(DEEP[name]), 255.0, literal=False)
        elif name == "avg152":
            from volumerenderingproject_amd import volumes
            vol, hdr = volumes.avg152()
            _SHARED[name] = Reference(vol, hdr["cal_max"])
        else:
            raise KeyError(name)
    return _SHARED[name]


def non_background(frame, bg=DEFAULT_BG):
    """Pixels with a colour channel off the background."""
    return int(np.any(frame[..., :3] != np.array(bg[:3], F), axis=-1).sum())
