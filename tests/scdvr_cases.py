"""The VR_MODE_SCDVR cases -- TEST INFRASTRUCTURE ONLY.  Shared by tests/test_scdvr_ref.py (CPU: the law,
the pins to the CDVR and SDVR restatements, the cases shown to bite) and tests/test_gpu_scdvr.py (GPU: the
library against tests/scdvr_ref.py), so the two cannot drift apart.  A case is an sdvr_cases.SCase (volume,
view, frame, coefficients) with the name of a colour map of cmap_cases and the name of a gradient-opacity
map G; cmap_cases' samples are shared, and the restatement's frame is computed once per case.
"""
import numpy as np

import cmap_cases as cc
import param_cases as pc
import scdvr_ref
import sdvr_cases as sc

F = np.float32
SCDVR = 11       # vr_api.h VR_MODE_SCDVR
GOPA_MAX = 16    # vr_api.h VR_GOPA_MAX_POINTS

# ---- the gradient-opacity maps (m in voxel units per voxel) ------------------------------------------
# avg152's lit samples under cmap_cases.SKIN_BONE (reset view, 64 x 48 x 64) have magnitudes from 0 to 136
# with a median of 15 and a tenth of them at 0; the points below were chosen against that spread so that
# every tail and span is met (tests/test_scdvr_ref.py::test_gpu_cases_are_not_vacuous)
UNIT = scdvr_ref.UNIT
# flat tissue transparent (weight 0 below 1.5: the lower tail, met by every constant region), a ramp to
# full weight at the strongest boundaries (80: past most of the steps between the tiny volumes' seeded values too)
EDGES = [(1.5, 0.0), (8.0, 0.25), (80.0, 1.0)]
ONE = [(3.0, 0.5)]


def sixteen():
    """16 seeded points over [0.25, 60]: ascending m, weights in [0, 1], every fourth one 0."""
    rng = np.random.default_rng(16)
    m = np.sort(np.concatenate(([0.25], rng.random(14) * 40.0 + 0.5, [60.0]))).astype(F)
    assert np.all(np.diff(m) > F(0.05))
    w = rng.random(16)
    w[::4] = 0.0
    return [(float(a), float(F(b))) for a, b in zip(m, w)]


GOPAS = {"unit": UNIT, "edges": EDGES, "one": ONE, "sixteen": sixteen()}

# blob_small's voxels are k * 2^-72: OPAQUE0's shape in those units
SMALL_MAP = [(0.0, (0.1, 0.2, 0.3, 0.05)), (60.0 * pc.SMALL_SCALE, (0.9, 0.5, 0.1, 0.4)),
             (200.0 * pc.SMALL_SCALE, (0.2, 0.9, 0.6, 0.1))]
# block01: transparent air, the block of float32(0.1) visible (inside it the field is constant: mag = 0)
BLOCK_MAP = [(0.0, (0.0, 0.0, 0.0, 0.0)), (0.02, (0.0, 0.0, 0.0, 0.0)), (0.08, (1.0, 0.5, 0.25, 0.5))]


# cmap_cases.seeded_map(8, 8) -- the threshold size of search_maps() -- is transparent at every point (its
# rule clears the first run of 8), so nothing is lit under it; the same size with a visible ramp beside it
EIGHT = [(float(x), (0.1 * i, 1.0 - 0.1 * i, 0.5, 0.04 * i)) for i, x in enumerate((0.0, 25.0, 50.0, 85.0, 120.0, 160.0, 200.0, 250.0))]
ALL_TRANSPARENT = [("seeded", cc.SMALL, 8)]


def map_of(name, cal=255.0):
    if name == "small":
        return SMALL_MAP
    if name == "eight":
        return EIGHT
    if name == "block":
        return BLOCK_MAP
    return cc.map_of(name, cal)


def gopa_of(name):
    return GOPAS[name]


class Case:
    """One SCDVR frame: an sdvr_cases.SCase (its interval TF unused), a colour map and a G, by name."""

    def __init__(self, base, cmap, gopa="unit"):
        self.base, self.cmap, self.gopa = base, cmap, gopa

    def key(self):
        return (self.base.key()[:5], self.cmap, self.gopa, self.base.shade)

    def what(self):
        b = self.base
        return (b.vol, self.cmap, self.gopa, getattr(b.view, "view", b.view), b.W, b.H, b.S, b.shade)

    def with_(self, gopa=None, shade=None, cmap=None):
        return Case(self.base if shade is None else self.base.with_shade(shade),
                    self.cmap if cmap is None else cmap, self.gopa if gopa is None else gopa)

    def gpu_params(self, flags=0, mode=SCDVR):
        return self.base.gpu_params(flags=flags, mode=mode)

    def gpu_camera(self):
        return self.base.gpu_camera()


def case(vol, view, frame, cmap, gopa="unit", shade=pc.SH_N0):
    return Case(sc.SCase(vol, view, frame, shade), cmap, gopa)


_FRAMES = {}


def reference(c):
    """scdvr_ref.render's (frame, record) of a case, computed once and shared read-only."""
    k = c.key()
    if k not in _FRAMES:
        vol, cal = cc.volume(c.base.vol)
        frame, rec = scdvr_ref.render(vol, map_of(c.cmap, cal), gopa_of(c.gopa), c.base.oracle_params(),
                                      c.base.oracle_camera(), c.base.shade, samples=cc.samples(c.base))
        frame.setflags(write=False)
        for a in rec.values():
            a.setflags(write=False)
        _FRAMES[k] = (frame, rec)
    return _FRAMES[k]


# ---- the GPU cases --------------------------------------------------------------------------------------

# (G, coefficients) pairs of the byte / float path test: every G and every coefficient set once
PATH_SETS = [("unit", "ks0"), ("edges", "n0"), ("sixteen", "gen"), ("one", "id"), ("edges", "sharp")]
FRAC_SETS = [("edges", "n0"), ("sixteen", "gen")]
BUDGET_MAP = ("seeded", 256, 256)
BUDGET_S = (3000, 3800)
BLOCK_FRAME = (32, 32, 64)
CULL_FRAME = (160, 96, 64)


def paths_cases(W, H, S, vol="avg152", sets=PATH_SETS, cmap="skin_bone"):
    return [case(vol, v, (W, H, S), cmap, g, pc.SHADE_SETS[s]) for v in sc.VIEWS for g, s in sets]


def face_cases():
    return [Case(b.with_shade(pc.SH_KS0), "opaque0", "edges") for b in sc.face_cases()]


def special_cases():
    maps = {"special": "opaque0", "small": "small", "subnormal": "opaque0_subnormal"}
    return [Case(b.with_shade(pc.SH_N0), maps[b.vol], "edges") for b in sc.special_cases()]


def tiny_cases(shape):
    return [Case(b, m, g) for b in sc.tiny_cases(shape) for m, g in (("opaque0", "edges"), ("smooth5", "sixteen"))]


def long_case():
    return Case(sc.long_case(), "smooth5", "edges")


def search_maps():
    """cmap_cases.search_maps() (1, 2, threshold, threshold + 1 and 256 points) and a visible map of the threshold size."""
    return cc.search_maps() + ["eight"]


def search_cases():
    return [case("avg152", v, sc.FRAMES[0], m, "edges", pc.SH_KS0) for m in search_maps() for v in ("default", "reset")]


def margin_cases():
    return [case("margin", cc.MARGIN_VIEW, cc.MARGIN_FRAME, "margin_zt", g, pc.SH_N0) for g in ("edges", "one")]


def budget_cases():
    return [case("avg152", "reset", (20, 14, S), BUDGET_MAP, "sixteen", pc.SH_KS0) for S in BUDGET_S]


def block_cases():
    return [case("block01", "reset", BLOCK_FRAME, "block", g, pc.SH_N0) for g in ("edges", "one")]


def plumbing_cases():
    return [case("avg152", v, sc.PLUMB_FRAME, "skin_bone", "edges", pc.SH_KS0) for v in sc.VIEWS]


def state_cases():
    """The state test's frames: reset view, the four maps G in turn, and the first-batch views."""
    out = [case("avg152", "reset", sc.FRAMES[0], "smooth5", g, pc.SH_KS0) for g in GOPAS]
    return out + [case("avg152", v, sc.FRAMES[0], "smooth5", "edges", pc.SH_KS0) for v in sc.VIEWS]


def cull_cases():
    return [case("avg152", v, CULL_FRAME, m, "edges", pc.SH_KS0) for m in ("smooth5", "opaque0") for v in ("reset", "default")]


def all_gpu_cases():
    """Every case the GPU tests hold to the restatement, each once."""
    out = []
    for fr in sc.FRAMES:
        out += paths_cases(*fr) + paths_cases(*fr, vol="frac", sets=FRAC_SETS, cmap="smooth5")
    out += face_cases() + special_cases()
    for shape in sc.TINY_SHAPES:
        out += tiny_cases(shape)
    out += [long_case()] + search_cases() + margin_cases() + budget_cases() + block_cases() + plumbing_cases()
    out += state_cases() + cull_cases()
    seen, uniq = set(), []
    for c in out:
        if c.key() not in seen:
            seen.add(c.key())
            uniq.append(c)
    return uniq
