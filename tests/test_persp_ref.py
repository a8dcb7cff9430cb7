"""tests/persp_ref.py (the numpy restatement of VR_FLAG_PERSP's position law) held to the law's stated
properties and to the orthographic restatement, vr_persp_screen held to its formula, and the views, frames
and cached references tests/test_gpu_persp.py shares (no GPU).

A mode's perspective reference is the mode's own restatement (through tests/crop_ref.py, which is that
restatement with the crop box off) computed while persp_ref.law() stands in for dvr_ref.positions and
iso_ref._positions_at.
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
import persp_ref
import scdvr_cases as xc
import scdvr_ref
import sdvr_ref
import test_crop_ref as tc
import volumerenderingproject_amd as vr
from test_dvr_ref import seeded_tf
from test_gpu_dvr import camera_pair

F = np.float32
MODES = tc.MODES
FRAMES = [(64, 48, 64), (37, 91, 50)]
VIEWS = ["default", "reset", "inside", "near", "within"]
# near: the eye beside the volume's (+, +, +) corner, which then lies behind the eye plane; within: the eye in
# the volume (camera_pair's `inside` is inside the unit cube, 3.55 voxels off avg152's upper z face)
OWN_POS = {"near": (0.3, 0.2, 0.5), "within": (0.0, 0.0, 0.35)}
BOXES = ("cut", "roi", "out", "empty")
# the long rays: the last S whose B table fits (kMaxTestTab - 8) and the first whose does not
LONG_W, LONG_H, LONG_S = 16, 16, (4088, 4089)
SMALL_S = (1, 2)
# the cull frame: ten by six 16 x 16 tiles under a 100-degree vertical field of view, where the volume leaves
# the outer tiles of the default view empty
CULL_FRAME, CULL_FOV = (160, 96, 64), 100.0
# the ingredients: test_crop_ref's ("zt": at most 9 TF segments and 8 map points, the marches' compare chains),
# or ("search") a TF of 17 intervals and a map of 9 points, past both thresholds: the marches' LDS searches
SEARCH_FRAME, SEARCH_VIEWS = (37, 91, 50), ("reset", "within")


def tf_of(variant):
    return seeded_tf(17, 17) if variant == "search" else tc.tf_of("zt")


def map_of(variant, cal):
    return cc.map_of(("seeded", cc.SMALL + 1, 9)) if variant == "search" else tc.map_of("zt", cal)


def screen_of(fov_y, W, H, vpd):
    return vr.persp_screen(fov_y, W, H, vpd)


def view_pair(O, name, W, H):
    """(the library's camera, the oracle's) of a named view: test_gpu_dvr.camera_pair's, and `near`."""
    if name not in OWN_POS:
        return camera_pair(O, name, W, H)
    up = tuple(vr.default_camera(W, H).up)
    return vr.derive_camera(OWN_POS[name], up, 2.0, 2.0 * H / W), O.camera_derive(OWN_POS[name], up, 2.0, 2.0 * H / W)


def oracle_view(view, W, H, S, fov=None):
    """(oracle parameters, oracle camera); fov: the screen is vr_persp_screen's at that vertical field of view."""
    p = oracle.params(W, H, S)
    if fov is not None:
        p.real_screen_width, p.real_screen_height = screen_of(fov, W, H, p.viewplane_distance)
    return p, view_pair(oracle, view, W, H)[1]


# ---- the references, one per (mode, frame, view, box, fov), shared read-only ---------------------------
_REFS, _ING = {}, {}


def _ingredients(mode, vol, cal, p, cam, key, variant):
    """What does not depend on the box: the frame's positions and the mode's per-sample colours or values
    (one frame's at a time)."""
    if key not in _ING:
        _ING.clear()
        P = persp_ref.positions(vol.shape, p, cam)
        if mode == "dvr":
            c = dvr_ref.sample_colors(vol, cal, tf_of(variant), p, cam)
        elif mode == "sdvr":
            c = sdvr_ref.shade_samples(vol, cal, tf_of(variant), p, cam, tc.SHADE)
        elif mode == "cdvr":
            c = cmap_ref.sample_colors(vol, map_of(variant, cal), p, cam)
        elif mode == "scdvr":
            c = scdvr_ref.lit_samples(vol, map_of(variant, cal), xc.gopa_of(tc.GOPA), p, cam, tc.SHADE)
        else:
            c = mip_ref.sample_values(vol, p, cam)
        _ING[key] = (P, c)
    return _ING[key]


def reference(mode, vol, cal, W, H, S, view, box=None, fov=None, variant="zt"):
    """The perspective frame of `mode` under `box` (None: off): crop_ref over persp_ref's positions."""
    k = (mode, W, H, S, view, box, fov, variant)
    if k not in _REFS:
        p, cam = oracle_view(view, W, H, S, fov)
        with persp_ref.law(S):
            P, c = _ingredients(mode, vol, cal, p, cam, k[:5] + (fov, variant), variant)
            if mode == "dvr":
                f = crop_ref.dvr(vol, cal, tf_of(variant), p, cam, box, None, c, P)
            elif mode == "sdvr":
                f = crop_ref.sdvr(vol, cal, tf_of(variant), p, cam, tc.SHADE, box, None, c, P)[0]
            elif mode == "cdvr":
                f = crop_ref.cdvr(vol, map_of(variant, cal), p, cam, box, None, None, c, P)
            elif mode == "scdvr":
                f = crop_ref.scdvr(vol, map_of(variant, cal), xc.gopa_of(tc.GOPA), p, cam, tc.SHADE, box, None, None,
                                   c, P)[0]
            elif mode == "mip":
                f = crop_ref.mip(vol, cal, p, cam, box, None, c, P)[0]
            else:
                f = crop_ref.iso(vol, p, cam, tc.ISO_VALUE, tc.ISO_RGB, tc.ISO_SHADE, box, None, c, P)[0]
        f.setflags(write=False)
        _REFS[k] = f
    return _REFS[k]


def gpu_cases():
    """(W, H, S, view, fov) of every frame tests/test_gpu_persp.py renders against a reference."""
    cases = [(W, H, S, v, None) for (W, H, S) in FRAMES for v in VIEWS]
    cases += [(LONG_W, LONG_H, S, v, None) for S in LONG_S for v in ("reset", "default")]
    cases += [(64, 48, S, "within", None) for S in SMALL_S]
    cases += [CULL_FRAME + (v, CULL_FOV) for v in ("default", "reset", "inside", "within")]
    cases += [SEARCH_FRAME + (v, None) for v in SEARCH_VIEWS]
    return cases


def draws(frame, W, H, S):
    return np.any(frame[..., :3] != tc.background(W, H, S), axis=-1)


# ---- the CPU tests ------------------------------------------------------------------------------------

def test_python_surface():
    assert vr.VR_FLAG_PERSP == 32
    assert callable(vr.persp_screen)
    assert "vr_persp_screen" in vr.renderer.EXPORTED
    assert "VR_FLAG_PERSP" in vr.default_params.__doc__


def test_persp_screen():
    """Within 1 ulp of numpy's double formula, and the refusals."""
    for fov, W, H, vpd in ((45.0, 64, 48, 2.0), (100.0, 160, 96, 2.0), (1.0, 37, 91, 0.125), (179.0, 1920, 1080, 3.5),
                           (60.0, 1, 1, 1e-3)):
        rsw, rsh = vr.persp_screen(fov, W, H, vpd)
        h = 2.0 * float(F(vpd)) * np.tan(float(F(fov)) * np.pi / 360.0)
        w = float(F(h)) * W / H
        assert abs(rsh - h) <= np.spacing(F(h)), (fov, rsh, h)
        assert abs(rsw - w) <= np.spacing(F(w)), (fov, rsw, w)
    L = vr.lib()
    a, b = C.c_float(), C.c_float()
    nan, inf = float("nan"), float("inf")
    assert L.vr_persp_screen(45.0, 64, 48, 2.0, C.byref(a), C.byref(b)) == 0
    assert L.vr_persp_screen(45.0, 64, 48, 2.0, None, C.byref(b)) == -1
    assert L.vr_persp_screen(45.0, 64, 48, 2.0, C.byref(a), None) == -1
    for fov in (0.0, -1.0, 180.0, 200.0, nan, inf):
        assert L.vr_persp_screen(fov, 64, 48, 2.0, C.byref(a), C.byref(b)) == -1, fov
    for vpd in (nan, inf, -inf):
        assert L.vr_persp_screen(45.0, 64, 48, vpd, C.byref(a), C.byref(b)) == -1, vpd
    for W, H in ((0, 48), (64, 0), (-1, 48), (64, -3)):
        assert L.vr_persp_screen(45.0, W, H, 2.0, C.byref(a), C.byref(b)) == -1, (W, H)


@pytest.mark.parametrize("W,H,S", FRAMES + [(64, 48, 1), (64, 48, 2)])
def test_law_properties(avg152, W, H, S):
    """One eye; the centre ray is the orthographic one bit for bit; the cross-section at fs = S is the
    orthographic one within 2 ulps; away from the centre the rays differ."""
    vol, _ = avg152
    for view in VIEWS:
        p, cam = oracle_view(view, W, H, S)
        P = persp_ref.positions(vol.shape, p, cam)
        O = dvr_ref.positions(vol.shape, p, cam)
        for a in range(3):
            assert P[a].dtype == F and P[a].shape == (W, H, S)
            assert np.all(P[a][:, :, 0].view(np.uint32) == P[a][0, 0, 0].view(np.uint32)), (view, a)   # the eye
            if W % 2 == 0 and H % 2 == 0:
                assert np.array_equal(P[a][W // 2, H // 2].view(np.uint32), O[a][W // 2, H // 2].view(np.uint32)), (view, a)
        mats = oracle.test_matrices(vol.shape, p, cam)
        x = np.arange(W, dtype=F)[:, None]
        y = np.arange(H, dtype=F)[None, :]
        end_p = persp_ref.positions_at(mats, x, y, F(S), S)
        end_o = iso_ref._positions_at(mats, x, y, F(S))
        for a in range(3):
            big = np.maximum(np.abs(end_o[a]), F(vol.shape[a]))   # (ulps of the scale of |p|: a coordinate may pass 0)
            assert np.all(np.abs(end_p[a] - end_o[a]) <= 2 * np.spacing(big)), (view, a)
        if S > 1:
            assert any(not np.array_equal(P[a], O[a]) for a in range(3)), view


def test_law_manager_restores(avg152):
    vol, _ = avg152
    W, H, S = 37, 91, 50
    p, cam = oracle_view("reset", W, H, S)
    before = dvr_ref.positions, iso_ref._positions_at
    ortho = mip_ref.sample_values(vol, p, cam)[1]
    with persp_ref.law(S):
        assert dvr_ref.positions is persp_ref.positions
        persp = mip_ref.sample_values(vol, p, cam)[1]
    assert (dvr_ref.positions, iso_ref._positions_at) == before
    assert not np.array_equal(ortho, persp)
    with pytest.raises(RuntimeError):
        with persp_ref.law(S):
            raise RuntimeError("inside")
    assert (dvr_ref.positions, iso_ref._positions_at) == before


@pytest.mark.parametrize("case", gpu_cases(), ids=str)
def test_linear_model_margin(avg152, case):
    """The restated positions depart from test_clip's linear model -- pa = p(0), pb = p(S - 1),
    dp = (pb - pa) / (S - 1) in float, p ~= pa + s dp -- by less than half its 0.01-voxel margin."""
    vol, _ = avg152
    W, H, S, view, fov = case
    p, cam = oracle_view(view, W, H, S, fov)
    P = persp_ref.positions(vol.shape, p, cam)
    s = np.arange(S, dtype=F)
    for a in range(3):
        pa, pb = P[a][:, :, :1], P[a][:, :, S - 1:]
        dp = (pb - pa) / F(S - 1) if S > 1 else np.zeros_like(pa)
        model = pa.astype(np.float64) + s.astype(np.float64) * dp.astype(np.float64)
        assert float(np.abs(model - P[a]).max()) < 0.005, (case, a)


@pytest.mark.parametrize("case", gpu_cases(), ids=str)
def test_gpu_cases_draw_and_differ(avg152, case):
    """Every frame the GPU file holds to a reference has a ray that draws, and a drawing pixel that differs
    from the orthographic frame (S = 1: the one sample is the eye, which every ray shares with its
    orthographic ray only at the centre -- the frames differ all the same)."""
    vol, cal = avg152
    W, H, S, view, fov = case
    f = reference("mip", vol, cal, W, H, S, view, None, fov)
    d = draws(f, W, H, S)
    assert d.any(), case
    p, cam = oracle_view(view, W, H, S, fov)
    ortho = mip_ref.render(vol, cal, p, cam)[0]
    assert np.any(f[d] != ortho[d]), case


def test_views_are_what_they_are_named(avg152):
    """within: the eye is in the volume; near: it is outside, with a corner of the dataset box behind the eye
    plane and one in front; default, reset: every corner at or beyond sample 1 (the culls make a claim);
    inside: the eye is off the volume with the nearest corners between samples 1 and 2 at S = 64."""
    vol, _ = avg152
    W, H, S = 64, 48, 64
    d = np.array(vol.shape, np.float64)
    for view in VIEWS:
        p, cam = oracle_view(view, W, H, S)
        mc, iv, tv = (m.astype(np.float64) for m in oracle.test_matrices(vol.shape, p, cam))
        eye = np.array([float(c[0, 0, 0]) for c in persp_ref.positions(vol.shape, p, cam, xs=[0])])
        R = np.array([[iv[c, r] for c in range(3)] for r in range(3)])
        ts = []
        for k in range(8):
            corner = np.array([d[a] if (k >> a) & 1 else 0.0 for a in range(3)])
            q = np.array([(corner[a] - tv[3, a]) / tv[a, a] - iv[3, a] for a in range(3)])
            ts.append(np.linalg.solve(R, q)[2] / -float(p.viewplane_distance))
        in_vol = bool(np.all(eye >= 0) and np.all(eye < d))
        assert in_vol == (view == "within"), (view, eye)
        if view == "within":
            assert min(ts) < 0 < max(ts), ts
        if view == "inside":
            assert 1.0 / S <= min(ts) < 2.0 / S, ts
        if view == "near":
            assert min(ts) < 0 < max(ts), ts
        if view in ("default", "reset"):
            assert min(ts) >= 1.0 / S, ts


def test_search_ingredients_pass_the_thresholds():
    """The `search` TF has more than 1 + kDvrSeg8 = 9 segments and the `search` map more than kCmapSmall = 8
    points, the `zt` ones at most that many; both leave the value 0 transparent (ESS applies)."""
    cal = 255.0
    assert len(vr.tf_segments(tf_of("search"), cal)[0]) > 9 >= len(vr.tf_segments(tf_of("zt"), cal)[0])
    assert len(map_of("search", cal)) > cc.SMALL >= len(map_of("zt", cal))
    assert crop_ref.tf_outside(cal, tf_of("search"))[3] == 0.0
    assert crop_ref.cmap_outside(map_of("search", cal))[3] == 0.0
