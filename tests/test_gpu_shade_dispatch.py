"""The SHADE dimension of launch_dvr_march and launch_cmap_march: VR_MODE_DVR and VR_MODE_SDVR are one kernel
text (dvr_march_kernel, SHADE off / on), VR_MODE_CDVR and VR_MODE_SCDVR another (cmap_march_kernel), and the
launchers pick the instantiation from (F2B, ESS, U8, SEG8 or SMALL, SEP, SHADE).  Here every value of each
of those that a frame can reach is rendered in all four modes, interleaved on one context and one stream
with nothing synchronised between the frames of a state, and held to the modes' own restatements
(tests/dvr_ref.py, sdvr_ref.py, cmap_ref.py, scdvr_ref.py) by the rule of the modes' own tests: exact and ESS
frames bitwise (the coefficients are param_cases.SH_KS0 = (0.3, 0.7, 0, 16): no specular term, so nothing
goes through the hardware exp2 / log2), ERT and ESS | ERT within test_gpu_shade.TOL_ERT = 1e-4 of the exact
frame.

  F2B, ESS   flags 0, ESS, ERT, ESS | ERT
  U8         a 9 x 7 x 5 volume of integers 0 .. 255 (the byte copy) and the same plus seeded fractions
             (the float volume)
  SEG8       the default TF (7 segments) and test_dvr_ref.seeded_tf(17, 17) (past 1 + kDvrSeg8 = 9)
  SMALL      cmap_cases.SMOOTH5 (5 points) and cmap_cases.seeded_map(9, 9) (kCmapSmall + 1)
  view       "default" (axis-aligned) and "reset" (oblique), test_gpu_dvr.camera_pair's.  SEP itself is on
             for every matrix vr_render builds (modelCam and toVolume are scale + translation, DESIGN.md
             "ISO"): the SEP-off instantiations cannot be reached through the API, by these modes' own tests
             either

A swapped SHADE dispatch cannot pass: for every (volume, TF or map) the shaded and the unshaded restatement
differ (asserted below), and each frame is held to its own.
"""
import numpy as np
import pytest

import cmap_cases as cc
import cmap_ref
import dvr_ref
import param_cases as pc
import scdvr_cases as xc
import scdvr_ref
import sdvr_ref
import volumerenderingproject_amd as vr
from test_dvr_ref import seeded_tf
from test_gpu_dvr import assert_bits, camera_pair
from test_gpu_shade import TOL_ERT

pytestmark = pytest.mark.gpu

E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
DVR, SDVR, CDVR, SCDVR = vr.VR_MODE_DVR, vr.VR_MODE_SDVR, vr.VR_MODE_CDVR, vr.VR_MODE_SCDVR
F = np.float32
SHAPE, CAL = (9, 7, 5), 255.0
W, H, S = 33, 21, 24
SHADE = pc.SH_KS0
GOPA = xc.EDGES
VIEWS = ("default", "reset")
FLAGS = (0, E, T, E | T)
ORDER = (SDVR, CDVR, DVR, SCDVR)   # the modes of one (view, flags), interleaved
# the states of a context: (interval TF, colour map), one side of each threshold per state
STATES = {"seg8_small": (vr.default_transfer_function, lambda: cc.SMOOTH5),
          "search_lds": (lambda: seeded_tf(17, 17), lambda: cc.seeded_map(cc.SMALL + 1, 9))}
_REFS = {}


def volume(kind):
    vol = np.random.default_rng(975).integers(0, 256, size=SHAPE).astype(F)
    if kind == "frac":
        vol = (vol + np.random.default_rng(3).random(SHAPE, dtype=F)).astype(F)
    return vol


def references(O, kind, state):
    """{(view, mode): the restatement's frame} of a volume under a state, computed once and shared read-only."""
    if (kind, state) not in _REFS:
        vol, tf, points = volume(kind), STATES[state][0](), STATES[state][1]()
        out = {}
        for view in VIEWS:
            p, cam = O.params(W, H, S), camera_pair(O, view, W, H)[1]
            samples = cmap_ref.sample_values(vol, p, cam)
            out[view, DVR] = dvr_ref.render(vol, CAL, tf, p, cam)
            out[view, SDVR] = sdvr_ref.render(vol, CAL, tf, p, cam, SHADE)[0]
            out[view, CDVR] = cmap_ref.render(vol, points, p, cam, samples=samples)
            out[view, SCDVR] = scdvr_ref.render(vol, points, GOPA, p, cam, SHADE, samples=samples)[0]
        for a in out.values():
            a.setflags(write=False)
        _REFS[kind, state] = out
    return _REFS[kind, state]


def params(mode, flags):
    p = vr.default_params(W, H, S, mode=mode, flags=flags)
    p.shade_ambient, p.shade_diffuse, p.shade_specular, p.shade_shininess = SHADE
    return p


@pytest.mark.parametrize("kind", ["byte", "frac"])
def test_every_dispatch_point_in_four_modes(oracle_mod, kind):
    import torch
    # the states sit on both sides of the SEG8 (1 + kDvrSeg8 = 9 segments) and SMALL (kCmapSmall points) thresholds
    nseg = {s: len(vr.tf_segments(STATES[s][0](), CAL)[0]) for s in STATES}
    assert nseg["seg8_small"] <= 9 < nseg["search_lds"], nseg
    assert len(STATES["seg8_small"][1]()) <= cc.SMALL < len(STATES["search_lds"][1]())
    vol = volume(kind)
    with vr.VolumeRenderer(vol, CAL, device=0) as r:
        r.set_gradient_opacity(GOPA)
        jobs = [(view, flags, mode) for view in VIEWS for flags in FLAGS for mode in ORDER]
        t = torch.empty((len(jobs), W, H, 4), dtype=torch.float32, device="cuda:0")
        for state, (tf, points) in STATES.items():
            refs = references(oracle_mod, kind, state)
            for view in VIEWS:   # (a swapped SHADE dispatch cannot pass)
                assert np.any(refs[view, DVR] != refs[view, SDVR]), (kind, state, view, "dvr == sdvr")
                assert np.any(refs[view, CDVR] != refs[view, SCDVR]), (kind, state, view, "cdvr == scdvr")
            r.set_transfer_function(tf())
            r.set_colormap(points())
            for k, (view, flags, mode) in enumerate(jobs):
                r.render_device(params(mode, flags), camera_pair(oracle_mod, view, W, H)[0], t[k].data_ptr(),
                                asynchronous=True)
            r.synchronize()
            got = {job: frame for job, frame in zip(jobs, t.cpu().numpy())}
            for view in VIEWS:
                for mode in ORDER:
                    what = (kind, state, view, mode)
                    exact = got[view, 0, mode]
                    assert_bits(exact, refs[view, mode], what + ("exact",))
                    assert_bits(got[view, E, mode], exact, what + ("ess",))
                    for flags in (T, E | T):
                        fast = got[view, flags, mode]
                        err = float(np.abs(fast - exact).max())
                        assert err <= TOL_ERT, what + (flags, err)
                        assert np.all(fast[..., 3] == 1.0)
