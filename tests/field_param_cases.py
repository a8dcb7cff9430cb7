"""VR_MODE_SDVR, VR_MODE_CDVR and VR_MODE_SCDVR off the default parameters -- TEST INFRASTRUCTURE ONLY.
Shared by tests/test_field_param_cases.py (CPU: the cases bite) and tests/test_gpu_field_params.py /
tests/test_gpu_random.py (GPU: the library against tests/sdvr_ref.py, cmap_ref.py and scdvr_ref.py), so they
cannot drift apart.  Importing this module needs neither a GPU nor libvr.so beyond what sdvr_cases needs.

Every frame is an unshaded param_cases.Case of VR_MODE_DVR -- param_cases' viewplane distances, screens,
backgrounds and deep shapes -- wrapped in an sdvr_cases.SCase, with one of two ingredient sets per mode:

  SDVR    (default TF, SH_N0) and (tf_zero_visible, SH_KS0): under the second TF(0) is visible, so the
          out-of-volume samples of a camera inside the box show
  CDVR    SMOOTH5 and OPAQUE0
  SCDVR   (SMOOTH5, EDGES, SH_N0) and (OPAQUE0, sixteen, SH_KS0)

The coefficient sets are of param_cases.SHADE_BITWISE: the frames are the restatements' bit for bit.
"""
import numpy as np

import cmap_cases as cc
import param_cases as pc
import scdvr_cases as xc
import sdvr_cases as sc

F = np.float32
SDVR, CDVR, SCDVR = sc.SDVR, cc.CDVR, xc.SCDVR
MODES = (SDVR, CDVR, SCDVR)
FRAME = (pc.W, pc.H, pc.S)
DEEP_FRAME = (pc.TW, pc.TH, pc.TS)

SDVR_SETS = [("default", pc.SH_N0), ("zero_visible", pc.SH_KS0)]              # (TF, coefficients)
CDVR_SETS = ["smooth5", "opaque0"]                                            # colour map
SCDVR_SETS = [("smooth5", "edges", pc.SH_N0), ("opaque0", "sixteen", pc.SH_KS0)]   # (colour map, G, coefficients)
assert all(s[-1] in [pc.SHADE_SETS[n] for n in pc.SHADE_BITWISE] for s in SDVR_SETS + SCDVR_SETS)
N_SETS = 2

# S = 1: p(S - 1) = p(0), so the ray has no light direction.  The camera sits inside the blob (scale 0.2),
# and the one sample of every ray lies in the viewplane: (viewplane distance, camera scale), views
S1_FRAME = (pc.W, pc.H, 1)
S1_VPD = [(2.0, 0.2), (0.6, 0.2)]
S1_VIEWS = ("z", "obl")
NO_LIGHT_VPD = (0.0, 0.2)   # the row of param_cases.VPD with every sample in the camera plane: |e|^2 = 0
BG_VIEWS = ("z", "obl")
CAL_VIEWS = ("z", "obl")


def vpd_rows():
    """(label, view case) over param_cases.VPD x VIEWS."""
    return [(("vpd", vpd, scale, view), pc.Case(view, pc.DVR, vpd=vpd, scale=scale))
            for vpd, scale in pc.VPD for view in pc.VIEWS]


def screen_rows():
    """(label, view case) over param_cases.SCREENS x VIEWS."""
    return [(("screen", rsw, rsh, view), pc.Case(view, pc.DVR, rsw=rsw, rsh=rsh))
            for rsw, rsh in pc.SCREENS for view in pc.VIEWS]


def s1_rows():
    """(label, view case): the single-sample frames."""
    return [(("s1", vpd, scale, view), pc.Case(view, pc.DVR, vpd=vpd, scale=scale, frame=S1_FRAME))
            for vpd, scale in S1_VPD for view in S1_VIEWS]


def view_rows():
    return vpd_rows() + screen_rows() + s1_rows()


def has_light(label):
    """A row whose rays have a light direction (S > 1 and a non-zero viewplane distance)."""
    return label[0] == "screen" or (label[0] == "vpd" and (label[1], label[2]) != NO_LIGHT_VPD)


def background_rows(bg):
    """(label, view case) under a background: the default screen, and the far screen of param_cases.SCREENS,
    where the volume leaves a row of 16 x 16 tiles to the visible-tile cull."""
    far = pc.SCREENS[2]
    return [(("bg", view), pc.Case(view, pc.DVR, bg=bg)) for view in BG_VIEWS] + \
        [(("bg", view, "far"), pc.Case(view, pc.DVR, bg=bg, rsw=far[0], rsh=far[1])) for view in BG_VIEWS]


def cal_rows():
    return [(("cal", view), pc.Case(view, pc.DVR)) for view in CAL_VIEWS]


def deep_rows():
    """param_cases.deep_volume_cases: z, x, y_back and obl at the 1.2 screen, obl at the 0.02 screen."""
    return [(("deep", c.view, c.rsw), c) for c in pc.deep_volume_cases(pc.DVR)]


def _frame(view):
    return (view.W, view.H, view.S)


def sdvr_case(view, k=0, vol="blob"):
    """The SDVR case of a view under ingredient set k."""
    tf, shade = SDVR_SETS[k]
    return sc.SCase(vol, view, _frame(view), shade, tf)


def cdvr_case(view, vol="blob"):
    """The CDVR case of a view (the colour map is named beside it: CDVR_SETS[k], or "grey")."""
    return cc.case(vol, view, _frame(view))


def scdvr_case(view, k=0, vol="blob"):
    """The SCDVR case of a view under ingredient set k."""
    cmap, gopa, shade = SCDVR_SETS[k]
    return xc.case(vol, view, _frame(view), cmap, gopa, shade)


def background(c):
    """The background of an sdvr_cases.SCase (its rgb, float32)."""
    return np.array(list(c.oracle_params().background)[:3], F)


def drawn(frame, bg):
    """The pixels [W, H] with a colour channel off the background."""
    return np.any(frame[..., :3] != np.asarray(bg, F)[:3], axis=-1)


# ---- the ERT bound with lit samples and any background ------------------------------------------------

def sample_colour_range(colours, shade=None):
    """(lo, hi) per channel of the colours a sample can take: `colours` are the TF's interval colours or the
    colour map's point colours (rgb, all >= 0).  A colour-map sample is a convex mix of two neighbouring point
    colours, so it lies between the points' extremes.  A lit sample is c * (ka + kd d) + spec with d in [0, 1]
    and spec in [0, ks]: between c * ka and c * (ka + kd) + ks.  A sample outside the volume, or one without a
    normal or a light (d = 1, spec = 0: c * (ka + kd)), keeps c or lies inside that interval; c itself is kept
    in the range."""
    c = np.array([col[:3] for col in colours], np.float64)
    assert np.all(c >= 0)
    lo, hi = c.min(axis=0), c.max(axis=0)
    if shade is not None:
        ka, kd, ks, _ = shade
        lo, hi = np.minimum(lo, lo * ka), np.maximum(hi, hi * (ka + kd) + ks)
    return lo, hi


def ert_bound(colours, shade, bg, eps, S):
    """test_gpu_params.ert_bound (test_ert_epsilon's docstring: eps * R + 6 * S * 2^-24 * M per channel) with
    the TF colours replaced by the extremes of sample_colour_range: R is the spread of [lo, hi] and the
    background, M the largest magnitude among them.  Both of the argument's steps hold as they stand: what
    the early stop leaves out and what it puts in its place are T times convex mixes of sample colours and the
    background -- whatever alpha a sample has, G's weight included -- and every blend step rounds three times
    on values of magnitude at most M."""
    lo, hi = sample_colour_range(colours, shade)
    b = np.array(bg[:3], np.float64)
    cols = np.stack([lo, hi, b])
    R = cols.max(axis=0) - cols.min(axis=0)
    M = np.abs(cols).max(axis=0)
    return eps * R + 6.0 * S * 2.0 ** -24 * M


def mode_colours(mode, k):
    """(colours, coefficients) of a mode's ingredient set k, for ert_bound."""
    if mode == SDVR:
        tf, shade = SDVR_SETS[k]
        return [t[2] for t in sc.tf_of(tf)], shade
    if mode == CDVR:
        return [p[1] for p in cc.map_of(CDVR_SETS[k])], None
    cmap, _, shade = SCDVR_SETS[k]
    return [p[1] for p in xc.map_of(cmap)], shade


# ---- the random views ---------------------------------------------------------------------------------

RANDOM_SEEDS = (1, 2, 3)
RANDOM_VIEWS = 16
RANDOM_M = 1.1   # SH_N0 on colours in [0, 1]: c * 0.7 + 0.4 <= 1.1


class FreeView(pc.Case):
    """An unshaded VR_MODE_DVR param_cases.Case whose camera position and up vector are given, not named."""

    def __init__(self, pos, up, frame):
        pc.Case.__init__(self, "free", pc.DVR, frame=frame)
        self.pos, self.up = tuple(float(c) for c in pos), tuple(float(c) for c in up)

    def key(self):
        return pc.Case.key(self) + (self.pos, self.up)

    def pos_up(self):
        return self.pos, self.up


def random_view_cases(seed):
    """test_gpu_random.random_views(16, seed) as view cases on avg152 (default screen: 2 x 2 H / W)."""
    from test_gpu_random import random_views
    return [FreeView(pos, up, (W, H, S)) for W, H, S, pos, up in random_views(RANDOM_VIEWS, seed)]


def random_references(view):
    """({mode: frame}, shaded samples of SDVR, lit samples of SCDVR) of one random view on avg152: SDVR
    under (default TF, SH_N0), CDVR under SMOOTH5, SCDVR under (SMOOTH5, EDGES, SH_N0).  Not cached: the
    records of a 96 x 80 x 319 frame are large and each view is rendered once per process and test."""
    import cmap_ref
    import scdvr_ref
    import sdvr_ref
    vol, cal = sc.volume("avg152")
    p, cam = view.oracle_params(), view.oracle_camera()
    tf, shade = SDVR_SETS[0]
    cmap, gopa, xshade = SCDVR_SETS[0]
    assert CDVR_SETS[0] == cmap
    fs, rec = sdvr_ref.render(vol, cal, sc.tf_of(tf), p, cam, shade)
    samples = cmap_ref.sample_values(vol, p, cam)
    fc = cmap_ref.render(vol, cc.map_of(cmap, cal), p, cam, samples=samples)
    fx, xrec = scdvr_ref.render(vol, xc.map_of(cmap, cal), xc.gopa_of(gopa), p, cam, xshade, samples=samples)
    return {SDVR: fs, CDVR: fc, SCDVR: fx}, int(rec["shaded"].sum()), int(xrec["lit"].sum())


def random_ert_bound(S):
    """The project's bound at eps = 1e-5 with R = M = RANDOM_M over S samples, and never under TOL_ERT = 1e-4
    (the rule of the modes' own tests, which the derived bound exceeds past S of about 250)."""
    return max(1e-4, 1e-5 * RANDOM_M + 6.0 * S * 2.0 ** -24 * RANDOM_M)
