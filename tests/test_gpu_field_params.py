"""VR_MODE_SDVR, VR_MODE_CDVR and VR_MODE_SCDVR off the default parameters on the GPU: viewplane distances
(negative, zero, a camera inside the box), anamorphic and far screens, a single sample per ray, backgrounds, a
fractional cal_max and the deep shapes, against the numpy restatements through the rows of
tests/field_param_cases.py (which tests/test_field_param_cases.py keeps from being vacuous).

The rule of comparison is that of the modes' own tests, whose check_all_flags helpers are imported: the exact
frame is bitwise the restatement's, the ESS frame bitwise the exact one, ERT and ESS | ERT within 1e-4 of the
exact frame with alpha 1 -- the project's bound eps R + 6 S 2^-24 M (test_gpu_params.test_ert_epsilon) with
margin: 3.6e-5 at S = 64, eps = 1e-5 and sample colours of magnitude at most 1.1.  Only the backgrounds,
where the colours are not within [0, 1.1], take the bound itself (field_param_cases.ert_bound).

Every test prints the number of frames it compared and the largest ERT deviation it saw.
"""
import numpy as np
import pytest

import cmap_cases as cc
import field_param_cases as fp
import param_cases as pc
import scdvr_cases as xc
import sdvr_cases as sc
import volumerenderingproject_amd as vr
from test_gpu_cmap import check_all_flags as cdvr_check
from test_gpu_dvr import assert_bits
from test_gpu_params import BACKGROUNDS
from test_gpu_scdvr import check_all_flags as scdvr_check
from test_gpu_sdvr import check_all_flags as sdvr_check

pytestmark = pytest.mark.gpu

E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
SDVR, CDVR, SCDVR = fp.SDVR, fp.CDVR, fp.SCDVR
MODE_IDS = ["sdvr", "cdvr", "scdvr"]
F = np.float32
_EXACT = {}   # (test, mode, set, volume name, label) -> the exact frame of the first context that rendered it


class Recorder:
    """A context seen through its render call: counts the frames and, case by case, takes the largest
    deviation of an ERT frame from the exact frame of the same case."""

    def __init__(self, ctx):
        self.ctx, self.frames, self.count, self.worst = ctx, [], 0, 0.0

    def render(self, p, cam):
        f = self.ctx.render(p, cam)
        self.count += 1
        self.frames.append((int(p.flags), f))
        return f

    def case_done(self):
        exact = [f for fl, f in self.frames if fl == 0]
        assert len(exact) == 1 and len(self.frames) == 4
        for fl, f in self.frames:
            if fl & T:
                self.worst = max(self.worst, float(np.abs(f - exact[0]).max()))
        self.frames = []


def report(name, recorders):
    print(name, "frames compared", sum(r.count for r in recorders), "largest ERT deviation",
          max(r.worst for r in recorders))


def apply_set(ctx, mode, k, cal):
    """A mode's ingredient set k on a context."""
    if mode == SDVR:
        ctx.set_transfer_function(sc.tf_of(fp.SDVR_SETS[k][0]))
    elif mode == CDVR:
        ctx.set_colormap(cc.map_of(fp.CDVR_SETS[k], cal))
    else:
        ctx.set_colormap(xc.map_of(fp.SCDVR_SETS[k][0], cal))
        ctx.set_gradient_opacity(xc.gopa_of(fp.SCDVR_SETS[k][1]))


def check(r, mode, k, view, vol, what, cmap=None):
    """One view in one mode under ingredient set k (already on the context; cmap: CDVR's map when it is not
    the set's) in the four flag combinations, by the mode's own rule.  Returns the exact frame."""
    if mode == SDVR:
        exact = sdvr_check(r, fp.sdvr_case(view, k, vol), what)
    elif mode == CDVR:
        exact = cdvr_check(r, fp.cdvr_case(view, vol), cmap or fp.CDVR_SETS[k], what)
    else:
        exact = scdvr_check(r, fp.scdvr_case(view, k, vol), what)
    r.case_done()
    return exact


def same_as_first(key, exact):
    """The exact frame is bitwise the one the first context that rendered this row gave (the byte-copy
    context and the float-volume one are separate cases of a test)."""
    assert_bits(exact, _EXACT.setdefault(key, exact), key)


def parts(mode, k, view, vol="blob"):
    """(reference frame, flags -> params, camera) of one view in one mode under ingredient set k."""
    if mode == SDVR:
        c = fp.sdvr_case(view, k, vol)
        return sc.reference(c)[0], c.gpu_params, c.gpu_camera()
    if mode == CDVR:
        c = fp.cdvr_case(view, vol)
        return cc.reference(c, fp.CDVR_SETS[k]), lambda fl: cc.gpu_params(c, fl), c.gpu_camera()
    c = fp.scdvr_case(view, k, vol)
    return xc.reference(c)[0], c.gpu_params, c.gpu_camera()


@pytest.mark.parametrize("volume", [0, 1], ids=["byte", "float"])
@pytest.mark.parametrize("mode", fp.MODES, ids=MODE_IDS)
def test_viewplane_and_screen(mode, volume):
    """Every row of param_cases.VPD and SCREENS in the seven views, and the single-sample rows, under both
    ingredient sets of the mode: the headlight, the two-sided flip and the gradient taps follow the view where
    the march axis flips (a negative distance), where the first samples are already in the volume (a camera
    inside the box) and where L differs per pixel in voxel space (anamorphic screens); and the ray without a
    light direction (vpd = 0, S = 1: e = p(S - 1) - p(0) = 0) is d = 1, spec = 0 although the sample has a
    normal."""
    vol, cal = sc.volume("blob")
    with vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=volume)) as ctx:
        r = Recorder(ctx)
        for k in range(fp.N_SETS):
            apply_set(ctx, mode, k, cal)
            for label, view in fp.view_rows():
                exact = check(r, mode, k, view, "blob", (label, "set", k, "dvr_volume", volume))
                same_as_first(("view", mode, k, label), exact)
        assert r.count == 4 * fp.N_SETS * len(fp.view_rows())
        report("viewplane and screen", [r])


@pytest.mark.parametrize("bg", BACKGROUNDS, ids=["mixed", "zero", "huge"])
def test_background(bg):
    """Modes 9 to 11 under both ingredient sets on contexts at cull 0, 1 and 2, views z and obl on the default
    screen and on the far one (where the visible-tile list leaves tiles out): the back-to-front start value,
    the front-to-back T * bg, culled tiles (the first sets) and frames without a background pixel (the second
    ones).  Exact frames are bitwise the restatement's and ESS frames bitwise the exact ones.

    ERT and ESS | ERT are held per channel to field_param_cases.ert_bound, test_gpu_params.ert_bound
    generalised: eps * R + 6 * S * 2^-24 * M, where R is the spread and M the largest magnitude of that channel
    over the background and the extremes a sample colour can take.  Those extremes: a colour-map sample is a
    convex mix of two point colours, a TF sample an interval colour c; lit, it is c * (ka + kd d) + spec with
    d in [0, 1] and spec in [0, ks], so it lies in [c ka, c (ka + kd) + ks]; unlit (outside the volume, or
    transparent) it is c itself, which is kept in the range.  The argument of test_ert_epsilon then holds
    unchanged: what the early stop leaves out, and what it puts in its place, are T < eps times convex mixes
    of such colours and the background, and each blend step rounds three times on values of magnitude at most
    M.  At the huge background the bound is loose (eps * R is 10 in red), as in test_background_is_honoured:
    the bitwise exact and ESS frames carry that case.

    At cull 2 the tile path as well: all tiles, and the visible tiles alone assembled with the background,
    equal the reference."""
    import torch
    vol, cal = sc.volume("blob")
    tw = th = 16
    nt = (-(-pc.W // tw)) * (-(-pc.H // th))
    rs = {cull: vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(cull=cull)) for cull in (0, 1, 2)}
    frames, worst, dropped = 0, (0.0, 0.0, 0.0), 0   # worst: (error / bound, error, bound) of the channel nearest its bound
    try:
        for mode in fp.MODES:
            for k in range(fp.N_SETS):
                for r in rs.values():
                    apply_set(r, mode, k, cal)
                bound = fp.ert_bound(*fp.mode_colours(mode, k), bg, 1e-5, pc.S)
                for label, view in fp.background_rows(bg):
                    want, params, cam = parts(mode, k, view)
                    what = (mode, k, label)
                    assert np.all(want[..., 3] == 1.0)
                    for cull, r in rs.items():
                        exact = r.render(params(0), cam)
                        assert_bits(exact, want, (what, "cull", cull))
                        assert_bits(r.render(params(E), cam), exact, (what, "cull", cull, "ess"))
                        for fl in (T, E | T):
                            fast = r.render(params(fl), cam)
                            err = np.abs(fast[..., :3].astype(np.float64) - want[..., :3]).max(axis=(0, 1))
                            j = int(np.argmax(err / bound))
                            if err[j] / bound[j] > worst[0]:
                                worst = (float(err[j] / bound[j]), float(err[j]), float(bound[j]))
                            assert np.all(err <= bound), (what, cull, fl, err, bound)
                            assert np.all(fast[..., 3] == 1.0)
                        frames += 4
                    r = rs[2]
                    p = params(0)
                    vis = r.visible_tiles(p, cam, tw, th)
                    dropped += nt - len(vis)
                    for ids in (np.arange(nt, dtype=np.int32), vis):
                        tiles = torch.zeros((max(1, len(ids)), tw * th, 3), dtype=torch.float32, device="cuda:0")
                        frame = torch.full((pc.W, pc.H, 4), -7.0, dtype=torch.float32, device="cuda:0")
                        torch.cuda.current_stream().synchronize()   # (the fills run on torch's stream, the context's is non-blocking)
                        if len(ids) == nt:
                            assert r.render_tiles(p, cam, tw, th, 0, 1, tiles.data_ptr(), rgb=True) == nt
                        else:
                            assert r.render_tile_list(p, cam, tw, th, ids, 0, 1, tiles.data_ptr(), rgb=True) == len(ids)
                        r.assemble_tile_list(pc.W, pc.H, tw, th, ids, 1, max(1, len(ids)), tiles.data_ptr(), list(bg),
                                             frame.data_ptr(), rgb=True)
                        assert_bits(frame.cpu().numpy(), want, (what, "tiles", len(ids)))
                        frames += 1
    finally:
        for r in rs.values():
            r.close()
    assert dropped > 0   # (the far screen's visible-tile lists leave tiles to the assembly's background)
    print("background", bg, "frames compared", frames, "tiles left to the background", dropped,
          "ERT deviation nearest its bound (ratio, deviation, bound)", worst)


@pytest.mark.parametrize("name", list(sc.BLOB_CALS), ids=[str(c) for c in sc.BLOB_CALS.values()])
def test_cal_max_not_an_integer(name):
    """The blob at cal_max 200.7 and 1000.25, from the byte copy and from the float volume: CDVR under a
    context's first map, the never-set grey ramp to float32(cal_max); SDVR under the default TF, which
    classifies v / cal_max by the double as DVR does; then CDVR under SMOOTH5 and SCDVR under SMOOTH5 / EDGES."""
    vol, cal = sc.volume(name)
    assert cal == sc.BLOB_CALS[name] and cal != int(cal)
    recorders = []
    exact = {}
    for volume in (0, 1):
        with vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=volume)) as ctx:
            r = Recorder(ctx)
            recorders.append(r)
            assert ctx.colormap == [(0.0, (0.0, 0.0, 0.0, 0.0)), (float(F(cal)), (1.0, 1.0, 1.0, 1.0))]
            steps = [(CDVR, "grey"), (SDVR, None), (CDVR, fp.CDVR_SETS[0]), (SCDVR, None)]
            for mode, cmap in steps:
                if cmap != "grey":
                    apply_set(ctx, mode, 0, cal)
                for label, view in fp.cal_rows():
                    got = check(r, mode, 0, view, name, (cal, mode, cmap, label, "dvr_volume", volume), cmap=cmap)
                    assert pc.non_background(got) >= 40
                    assert_bits(got, exact.setdefault((mode, cmap, label), got), (cal, mode, cmap, label, "both volumes"))
    report("cal_max %s" % cal, recorders)


@pytest.mark.parametrize("volume", [0, 1], ids=["byte", "float"])
@pytest.mark.parametrize("name", list(pc.DEEP))
def test_deep_shapes(name, volume):
    """The needles of param_cases.DEEP (1500 voxels, 188 cells along one axis) through
    param_cases.deep_volume_cases in modes 9 to 11 under the first ingredient set of each: the shaded marches'
    own batch state and test_cell_jump calls, and CDVR's and SCDVR's own cell bits, under ESS.  The obl frame
    of the 1.2 screen is background through the whole march."""
    vol, cal = sc.volume(name)
    with vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=volume)) as ctx:
        r = Recorder(ctx)
        for mode in fp.MODES:
            apply_set(ctx, mode, 0, cal)
            for label, view in fp.deep_rows():
                exact = check(r, mode, 0, view, name, (name, mode, label, "dvr_volume", volume))
                same_as_first(("deep", name, mode, label), exact)
                if view.view == "obl" and view.rsw == 1.2:
                    assert pc.non_background(exact) == 0
                else:
                    assert pc.non_background(exact) >= 1
        report("deep shapes %s" % name, [r])
