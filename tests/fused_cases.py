"""The fused column march's cases: the documented tile rule restated, the volumes and the frames --
TEST INFRASTRUCTURE ONLY.

Shared by tests/test_fused_cases.py (CPU: the cases are not vacuous -- every claimed tile shape, rectangle
position, full tile and rolled footprint holds for the references alone) and tests/test_gpu_fused_params.py
(GPU: the library against the references), so they cannot drift apart.  Builds on tests/param_cases.py;
importing this module needs neither a GPU nor libvr.so.

A case is an FCase: a param_cases.Case with its own position and up vector (the rolled views are not among
param_cases.VIEWS) and a window shift, applied alike to the oracle's camera and the library's as multiples
of the camera's right and up.  An Entry names the case, its volume and what the tests may claim of it.
"""
import math
from collections import namedtuple

import numpy as np

import param_cases as pc
from param_cases import VRC, Case

F = np.float32

LADDER = [(64, 48), (48, 48), (48, 32), (32, 32), (32, 16), (16, 16)]
FUSE_COLS = 256
BACKGROUNDS = [(0.7, -0.25, 1.5, 0.3), (0.0, 0.0, 0.0, 0.0), (1e6, 1e-30, 0.5, 9.0)]   # test_gpu_params.BACKGROUNDS
EPSILONS = (0.0, 1e-7, 1e-3, 0.5)
SAMPLES = (1, 2, 7, 9, 15, 17, 33, 250, 1100)
FRAME = (96, 72, 64)


# ---- the documented rule, restated ----

def shape_rule(W, H, rsw, rsh, right, up, front, nleaf):
    """The documented rule (vr_api.h, vr_column_fused_plan): the largest ladder shape P x Q under which no
    tile can have more than 256 leaf columns -- per fixed axis floor(d) + 2 leaves for d = (P - 1) |rsw / W
    right_a| nleaf + (Q - 1) |rsh / H up_a| nleaf (with the library's rounding allowance), the product over
    the two axes.  None: no shape fits."""
    ma = int(np.flatnonzero(np.array(front, np.float32))[0])
    fixed = [a for a in range(3) if a != ma]
    for P, Q in LADDER:
        cols = 1
        for a in fixed:
            dx = abs(float(np.float32(rsw)) / W * float(right[a])) * nleaf
            dy = abs(float(np.float32(rsh)) / H * float(up[a])) * nleaf
            cols *= math.floor(((P - 1) * dx + (Q - 1) * dy) * (1.0 + 1e-6) + 1e-3) + 2
        if cols <= FUSE_COLS:
            return (P, Q)
    return None


def shape_bound(case, nleaf, P, Q):
    """The rule's bound on the leaf columns under a P x Q tile of the case."""
    cam = case.oracle_camera()
    ma = int(np.flatnonzero(np.array(cam.front, np.float32))[0])
    cols = 1
    for a in range(3):
        if a != ma:
            dx = abs(float(np.float32(case.rsw)) / case.W * float(cam.right[a])) * nleaf
            dy = abs(float(np.float32(case.rsh)) / case.H * float(cam.up[a])) * nleaf
            cols *= math.floor(((P - 1) * dx + (Q - 1) * dy) * (1.0 + 1e-6) + 1e-3) + 2
    return cols


def expected_shape(case, nleaf):
    """shape_rule of a case's frame and (oracle) camera."""
    cam = case.oracle_camera()
    return shape_rule(case.W, case.H, case.rsw, case.rsh, cam.right, cam.up, cam.front, nleaf)


TileColumns = namedtuple("TileColumns", "n0 n1 distinct pixels")


def tile_columns(case, nleaf, P, Q):
    """The pixel-to-leaf-column formula in float32, operation for operation: q = ((tlc_a + A right_a) +
    B (-up_a)) + 0.5 with A = (float)x rsw / W and B = (float)y rsh / H, v = q leaves, the column (int)v.
    Per P x Q tile (arrays [ntx, nty]): the sides n0, n1 of the bounding column rectangle of the tile's
    in-cube pixels (0 <= q < 1 on both fixed axes; 0 x 0 where there is none), the number of distinct
    columns among them and the number of those pixels."""
    cam = case.oracle_camera()
    W, H = case.W, case.H
    ma = int(np.flatnonzero(np.array(cam.front, F))[0])
    a0, a1 = (1 if ma == 0 else 0), (1 if ma == 2 else 2)
    A = (np.arange(W, dtype=F) * F(case.rsw) / F(W))[:, None]
    B = (np.arange(H, dtype=F) * F(case.rsh) / F(H))[None, :]
    idx, inside = [], np.ones((W, H), bool)
    for a in (a0, a1):
        q = ((F(cam.top_left[a]) + A * F(cam.right[a])) + B * (-F(cam.up[a]))) + F(0.5)
        assert q.dtype == F
        inside &= (q >= 0) & (q < 1)
        v = q * F(nleaf)
        idx.append(np.where((q >= 0) & (q < 1), v, 0).astype(np.int64))
    ntx, nty = -(-W // P), -(-H // Q)
    out = TileColumns(*(np.zeros((ntx, nty), np.int64) for _ in range(4)))
    for tx in range(ntx):
        for ty in range(nty):
            sl = (slice(tx * P, (tx + 1) * P), slice(ty * Q, (ty + 1) * Q))
            m = inside[sl]
            if not m.any():
                continue
            i0, i1 = idx[0][sl][m], idx[1][sl][m]
            out.n0[tx, ty] = i0.max() - i0.min() + 1
            out.n1[tx, ty] = i1.max() - i1.min() + 1
            out.distinct[tx, ty] = len(np.unique(i0 * nleaf + i1))
            out.pixels[tx, ty] = int(m.sum())
    return out


# ---- the cases ----

class FCase(Case):
    """A VRC Case seen from `pos` with `up` (default: param_cases.VIEWS[view]), its window moved by
    shift = (sx, sy): top_left += sx right + sy up, on the oracle's camera and the library's alike."""

    def __init__(self, view, pos=None, up=None, shift=(0.0, 0.0), **kw):
        super().__init__(view, VRC, **kw)
        vp, vu = pc.VIEWS.get(view, (None, None))
        self.pos = tuple(float(c) for c in (vp if pos is None else pos))
        self.up = tuple(float(c) for c in (vu if up is None else up))
        self.shift = (float(shift[0]), float(shift[1]))

    def key(self):
        return super().key() + (self.pos, self.up, self.shift)

    def pos_up(self):
        return tuple(self.scale * c for c in self.pos), self.up

    def _shifted(self, cam):
        sx, sy = self.shift
        if sx != 0.0 or sy != 0.0:
            for a in range(3):
                cam.top_left[a] = cam.top_left[a] + sx * cam.right[a] + sy * cam.up[a]
        return cam

    def oracle_camera(self):
        return self._shifted(super().oracle_camera())

    def gpu_camera(self):
        return self._shifted(super().gpu_camera())


def sd_fc(name, view, **kw):
    sd, fc = pc.SD_FC[name]
    return FCase(view, sd=sd, fc=fc, **kw)


def roll(axis, degrees):
    """(position, up) of the view along `axis` rolled by `degrees`: up = (sin t, cos t, 0) along z."""
    t = math.radians(degrees)
    s, c = math.sin(t), math.cos(t)
    return {"z": ((0.0, 0.0, 1.0), (s, c, 0.0)), "x": ((1.0, 0.0, 0.0), (0.0, c, s)),
            "y": ((0.0, 1.0, 0.0), (s, 0.0, c))}[axis]


# An Entry: id, the volume's name (reference()), the case, the group (a test function's share), `fused`
# (True: the rule gives a shape and the frame is fused; False: a gate case, with the reason in `gate`),
# `touch` (rectangle-position cases: the frame edges the drawn rectangle touches, a frozenset of "left",
# "right", "top", "bottom"; the other sides have a whole tile of background; None elsewhere), `eps` (the
# ERT epsilon; None = the default) and `min_drawn` (the floor on the reference frame's non-background pixels).
Entry = namedtuple("Entry", "id volume case group fused gate touch eps min_drawn")


def _entry(id, volume, case, group, fused=True, gate=None, touch=None, eps=None, min_drawn=40):
    return Entry(id, volume, case, group, fused, gate, touch, eps, min_drawn)


# ---- the volumes: param_cases' by name (reference()), and two of this module's own ----
BOX16_SHAPE = (13, 16, 11)
TINY2 = (2, 2, 1)   # two leaves a side: param_cases.TINY has no such shape
# tiny shape -> real_screen_width on the 40 x 30 frame: param_cases.TINY's 1.2 where a tile shape fits it (at
# most 16 leaves), else the widest round screen that 16 x 16 fits
TINY_RSW = {s: (w if max(s) <= 16 else (0.4 if max(s) <= 64 else 0.2)) for s, w in pc.TINY.items()}
TINY_RSW[TINY2] = 1.2


def box16():
    """(13, 16, 11), 16 leaves a side: seeded integers 0..255 in a box strictly inside, zeros around it."""
    vol = np.zeros(BOX16_SHAPE, F)
    vol[3:10, 3:13, 2:9] = np.random.default_rng(16).integers(0, 256, (7, 10, 7)).astype(F)
    return vol


def tiny_name(shape):
    return "tiny_" + "x".join(map(str, shape))


_REFS = {}


def reference(name):
    """The Reference of a volume of the cases, one per process: param_cases.shared_reference's names, "box16",
    and tiny_<d1>x<d2>x<d3>."""
    if name not in _REFS:
        if name == "box16":
            _REFS[name] = pc.Reference(box16(), 255.0)
        elif name.startswith("tiny_"):
            _REFS[name] = pc.Reference(pc.tiny_volume(tuple(int(d) for d in name[5:].split("x"))), 255.0)
        else:
            _REFS[name] = pc.shared_reference(name)
    return _REFS[name]


def nleaf_of(name):
    """Leaves a side of the volume's octree: the power of two that holds its longest dimension
    (tests/test_fused_cases.py holds it to the oracle's depth)."""
    L = max(reference(name).vol.shape)
    n = 1
    while n < L:
        n *= 2
    return n


def window_shift(frame, rsw, centre):
    """The shift that puts the projection of the cube's centre at pixel `centre` of a frame with square
    pixels: unshifted it is the frame's centre.  (A shift along right moves the picture left, one along up
    moves it down.)"""
    W, H, _ = frame
    cx, cy = centre
    return (-(cx - W / 2.0) * rsw / W, (cy - H / 2.0) * (rsw * H / W) / H)


# rectangle positions: name -> (the edges touched, where the drawn box sits on x and on y: -1 at the low
# edge, 0 in the middle, 1 at the high edge)
POSITIONS = {
    "top_left": (("left", "top"), -1, -1), "top": (("top",), 0, -1), "top_right": (("right", "top"), 1, -1),
    "left": (("left",), -1, 0), "centre": ((), 0, 0), "right": (("right",), 1, 0),
    "bottom_left": (("left", "bottom"), -1, 1), "bottom": (("bottom",), 0, 1),
    "bottom_right": (("right", "bottom"), 1, 1),
}
# the rectangle cases' frames: cube() along z -- 32 x 17 leaves of 32 on the screen, drawn to its faces --
# (name, frame, real_screen_width, the tile shape claimed)
RECT_FRAMES = [("s16", (96, 72, 64), 2.4, (16, 16)), ("s32x16", (128, 96, 64), 2.5, (32, 16))]
EDGE_GAP = 4   # pixels between a touched frame edge and the dataset box's projection


def position_shift(frame, rsw, pname):
    """The window shift that puts cube()'s projection along z at a position of POSITIONS."""
    W, H, _ = frame
    ex, ey = 1.0 * W / rsw, (17.0 / 32.0) * W / rsw   # the box's projection in pixels (square pixels)
    _, px, py = POSITIONS[pname]
    cx = {-1: EDGE_GAP + ex / 2, 0: W / 2.0, 1: W - EDGE_GAP - ex / 2}[px]
    cy = {-1: EDGE_GAP + ey / 2, 0: H / 2.0, 1: H - EDGE_GAP - ey / 2}[py]
    return window_shift(frame, rsw, (cx, cy))


def rect_cases():
    out = []
    for fname, frame, rsw, shape in RECT_FRAMES:
        kw = dict(frame=frame, rsw=rsw)
        for pname, (touch, px, py) in POSITIONS.items():
            case = FCase("z", shift=position_shift(frame, rsw, pname), **kw)
            out.append(_entry(f"rect-{fname}-{pname}", "cube", case, "rect-" + fname, touch=frozenset(touch)))
        # a window that misses the dataset: nothing is visible, the frame is the cull's background and
        # takes no column path (axis_columns_plan: no visible rectangle)
        out.append(_entry(f"rect-{fname}-empty", "cube", FCase("z", shift=(3.0, 0.0), **kw), "rect-" + fname,
                          fused=False, gate="nothing visible", min_drawn=0))
    # a frame of a single tile, the dataset to all four edges
    out.append(_entry("rect-one-tile-16", "cube", FCase("z", frame=(16, 16, 64), rsw=0.4), "rect-s16",
                      touch=frozenset(("left", "right", "top", "bottom"))))
    out.append(_entry("rect-one-tile-64x48", "cube", FCase("z", frame=(64, 48, 64), rsw=0.4), "rect-s32x16",
                      touch=frozenset(("left", "right", "top", "bottom"))))
    return out


MARCH_SCREENS = {"s16": 1.2, "s64": 0.36}   # blob at 96 x 72: 16 x 16, and the narrow screen that selects 64 x 48
ROLLS = (30.0, -120.0)
ROLL_SCREENS = (0.6, 0.3, 1.2)              # 32 x 16, 48 x 48, and none
ANAMORPHIC = ((0.9, 0.45), (0.4, 1.0))      # rsh != rsw H / W, both ways
DEGENERATE = {(1, 1): (0.01, 0.01), (5, 3): (0.05, 0.03), (1, 130): (0.01, 1.0), (257, 3): (1.0, 0.02)}
BOX16_PPC = (4.0, 3.3, 2.8, 2.3, 1.6, 1.1)  # pixels per leaf column -> the six ladder shapes in turn


# The march cases' camera stands a quarter of a leaf further back than param_cases' unit distance.  At the unit
# distance the default row's samples along the view axis fall on leaf faces, q * 64 = 96 - 2 s exactly, and
# fc_neg's 0.8 of a leaf off them, 140.8 - 2 s: both read the even leaves, and along z the two frames are
# the same frame.  A quarter leaf back the default row reads the even leaves and fc_neg the odd ones.
MARCH_DIST = 1.0 + 1.0 / 256.0


def march_case(name, scr, view):
    return sd_fc(name, view, frame=FRAME, rsw=MARCH_SCREENS[scr], scale=MARCH_DIST)


def march_cases(screens=tuple(MARCH_SCREENS), views=pc.AXIS_VIEWS):
    """Every SD_FC row x views x screens on blob at FRAME.  sd_zero is a case of the gate."""
    out = []
    for name in pc.SD_FC:
        for scr in screens:
            for view in views:
                zero = name == "sd_zero"
                out.append(_entry(f"march-{name}-{scr}-{view}", "blob", march_case(name, scr, view),
                                  "march-" + name, fused=not zero, gate="a zero step has no column path" if zero else None))
    return out


def full_tile_case(view="z"):
    return _entry(f"full-{view}", "blob", FCase(view, frame=FRAME, rsw=1.45), "full")


def build_entries():
    out = march_cases()
    out += [full_tile_case(v) for v in ("z", "x", "y_back")]
    for axis in ("z", "x", "y"):
        for deg in ROLLS:
            pos, up = roll(axis, deg)
            for rsw in ROLL_SCREENS:
                fits = rsw != 1.2
                out.append(_entry(f"roll-{axis}-{deg:g}-{rsw}", "blob", FCase(f"roll_{axis}_{deg:g}", pos, up, frame=FRAME, rsw=rsw),
                                  "roll-" + axis, fused=fits, gate=None if fits else "no tile shape fits"))
    for rsw, rsh in ANAMORPHIC:
        for view in ("z", "x"):
            out.append(_entry(f"anam-{view}-{rsw}-{rsh}", "blob", FCase(view, frame=FRAME, rsw=rsw, rsh=rsh), "anamorphic"))
        pos, up = roll("z", 30.0)
        out.append(_entry(f"anam-roll-{rsw}-{rsh}", "blob", FCase("roll_z_30", pos, up, frame=FRAME, rsw=rsw, rsh=rsh),
                          "anamorphic"))
    out += rect_cases()
    for i, bg in enumerate(BACKGROUNDS):
        for view in ("z", "x"):
            out.append(_entry(f"bg{i}-{view}", "blob", FCase(view, frame=FRAME, rsw=1.2, bg=bg), "background"))
    for eps in EPSILONS:
        for view in ("z", "x_back"):
            out.append(_entry(f"eps-{eps:g}-{view}", "blob", FCase(view, frame=FRAME, rsw=1.2), "epsilon", eps=eps))
    for S in SAMPLES:
        for view in ("z", "y"):
            # (one sample: inside the data, not in the camera plane; S = 2 has its second at the cube's centre)
            out.append(_entry(f"S{S}-{view}", "blob", FCase(view, frame=(96, 72, S), rsw=1.2, fc=0.9 if S == 1 else 0.0),
                              "samples"))
    for (W, H), (rsw, rsh) in DEGENERATE.items():
        out.append(_entry(f"frame-{W}x{H}", "blob", FCase("z", frame=(W, H, 64), rsw=rsw, rsh=rsh), "degenerate",
                          min_drawn=min(40, W * H)))
    for shape in list(pc.TINY) + [TINY2]:
        for view in ("z", "x", "y_back"):
            out.append(_entry(f"{tiny_name(shape)}-{view}", tiny_name(shape),
                              FCase(view, frame=(pc.TW, pc.TH, pc.TS), rsw=TINY_RSW[shape]), "tiny"))
    for view in pc.AXIS_VIEWS:
        out.append(_entry(f"cube-{view}", "cube", FCase(view, frame=FRAME, rsw=1.2), "cube"))
    for view in ("z", "x", "y_back"):
        out.append(_entry(f"special-{view}", "special", FCase(view, frame=FRAME, rsw=1.2), "special"))
        out.append(_entry(f"special_tf0-{view}", "special_tf0", FCase(view, frame=FRAME, rsw=1.2), "special",
                          fused=False, gate="TF(0) is visible: no column path"))
    for name in pc.DEEP:
        for view in ("z", "x", "y_back"):
            centre = 1.0
            out.append(_entry(f"{name}-{view}", name,
                              FCase(view, frame=(64, 48, 48), rsw=0.02, sd=0.002, fc=centre - 0.048), "deep"))
    for ppc in BOX16_PPC:
        for view in ("z", "x_back"):
            out.append(_entry(f"box16-{ppc}-{view}", "box16", FCase(view, frame=FRAME, rsw=96 / (ppc * 16)), "box16"))
    for name, view, rsw in (("sd_neg", "z", 0.68), ("fc_in", "x", 0.33)):
        sd, fc = pc.SD_FC[name]
        out.append(_entry(f"avg152-{name}-{view}", "avg152", FCase(view, sd=sd, fc=fc, frame=FRAME, rsw=rsw), "avg152"))
    assert len({e.id for e in out}) == len(out)
    return out


ENTRIES = build_entries()
GROUPS = sorted({e.group for e in ENTRIES})


def group(name):
    return [e for e in ENTRIES if e.group == name]


def claimed_shape(e):
    """What the fused context's plan must be for an entry: the rule's shape, None for a gate case."""
    return expected_shape(e.case, nleaf_of(e.volume)) if e.fused else None


# ---- the batch and the living context (tests/test_gpu_fused_params.py) ----

BATCH_BG = BACKGROUNDS[0]


def batch_entries(n):
    """n frames of one vr_render_batch call on cube(): the camera dollies back three quarters of a leaf a
    frame and the window moves over the nine rectangle positions in turn; sd_neg's parameters (the march
    runs towards the camera) and a non-default background.  One vr_params serves them all.  The dolly
    starts where sd_neg's last sample (t = 2) just reaches the cube's far face: its steps are one leaf of
    the cube's 32 long, so nearer than that every frame of a position is the same frame, and from there on
    each frame loses leaves at the far end -- 33 different frames, each with its own sample range."""
    fname, frame, rsw, shape = RECT_FRAMES[0]
    sd, fc = pc.SD_FC["sd_neg"]
    names = list(POSITIONS)
    out = []
    for i in range(n):
        pname = names[i % len(names)]
        case = FCase("z", shift=position_shift(frame, rsw, pname), frame=frame, rsw=rsw, sd=sd, fc=fc, bg=BATCH_BG,
                     scale=1.5 + 3.0 * i / 128.0)
        out.append(_entry(f"batch-{i}-{pname}", "cube", case, "batch", touch=frozenset(POSITIONS[pname][0])))
    return out


LIVING_RSW = 0.6   # blob at FRAME: 32 x 32 upright, 32 x 16 rolled by 30 degrees


def living_entries():
    """The frames of the living context on blob at FRAME and one screen, so one vr_params serves a batch
    of them: two tile shapes (upright and rolled views) and an oblique view, which is off the column path."""
    out = []
    for name in ("z", "roll_z_30", "x", "obl", "roll_z_-120", "y", "z_back"):
        if name.startswith("roll"):
            pos, up = roll("z", float(name.split("_")[2]))
            case = FCase(name, pos, up, frame=FRAME, rsw=LIVING_RSW)
        else:
            case = FCase(name, frame=FRAME, rsw=LIVING_RSW)
        obl = name == "obl"
        out.append(_entry("living-" + name, "blob", case, "living", fused=not obl,
                          gate="an oblique view has no column path" if obl else None))
    return out
