"""The off-default cases of tests/param_cases.py on the CPU (oracle and dvr_ref only, no GPU): every
case draws something and leaves background, the tiny shapes are visible, the special voxels change
the frame, the closed-form octree equals the literal one where both exist, and the DVR restatement
stays pinned to the oracle off the default viewplane distance."""
import numpy as np
import pytest

import dvr_ref
import oracle
import param_cases as pc
from param_cases import DVR, TEST, VRC, Case

MIN_PIXELS = 40


def check_content(frame, what):
    assert np.all(np.isfinite(frame)), what
    n = pc.non_background(frame)
    total = frame.shape[0] * frame.shape[1]
    assert n >= MIN_PIXELS, (what, n)
    assert total - n >= MIN_PIXELS, (what, total - n)


@pytest.mark.parametrize("name", list(pc.SD_FC))
def test_sd_fc_cases_draw_and_literal_equals_closed_form(name):
    ref = pc.shared_reference("blob")
    closed = pc.Reference(pc.blob(), 255.0, literal=False)
    for view in pc.VIEWS:
        case = pc.sd_fc_case(name, view)
        f = ref.frame(case)
        check_content(f, (name, view))
        g = closed.frame(case)
        assert np.array_equal(f.view(np.uint32), g.view(np.uint32)), (name, view)
        assert ref.count_in_samples(case) == closed.count_in_samples(case), (name, view)


def test_conic_rows_draw():
    ref = pc.shared_reference("blob")
    for name in ("fc_in", "sd_big"):
        for view in ("z", "obl"):
            check_content(ref.frame(pc.sd_fc_case(name, view, conic=True)), (name, view, "conic"))


@pytest.mark.parametrize("vpd,scale", pc.VPD)
def test_vpd_cases_draw_and_dvr_ref_mirrors_oracle(vpd, scale):
    ref = pc.shared_reference("blob")
    for view in pc.VIEWS:
        for mode in (TEST, DVR):
            check_content(ref.frame(Case(view, mode, vpd=vpd, scale=scale)), (vpd, scale, view, mode))
        case = Case(view, TEST, vpd=vpd, scale=scale)
        got = dvr_ref.render(ref.vol, ref.cal, ref.tf, case.oracle_params(), case.oracle_camera(), test_rule=True)
        want = ref.frame(case)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (vpd, scale, view)


@pytest.mark.parametrize("rsw,rsh", pc.SCREENS)
def test_screen_cases_draw(rsw, rsh):
    ref = pc.shared_reference("blob")
    for view in pc.VIEWS:
        for mode in (VRC, TEST, DVR):
            check_content(ref.frame(Case(view, mode, rsw=rsw, rsh=rsh)), (rsw, rsh, view, mode))


@pytest.mark.parametrize("shape", list(pc.TINY))
def test_tiny_shapes_are_visible(shape):
    ref = pc.Reference(pc.tiny_volume(shape), 255.0)
    for view in ("z", "x", "obl"):
        for mode in (VRC, TEST):
            f = ref.frame(Case(view, mode, rsw=pc.TINY[shape], frame=(pc.TW, pc.TH, pc.TS)))
            assert np.all(np.isfinite(f))
            assert pc.non_background(f) >= 1, (shape, view, mode)


@pytest.mark.parametrize("name", ["special", "special200"])
def test_special_voxels_change_the_frame(name):
    """Closed-form octree only: the literal tree is never built on blob_special()."""
    ref = pc.shared_reference(name)
    assert not ref.literal and ref.octree.o.number_of_nodes == 0
    assert int((~np.isfinite(ref.vol)).sum()) >= 100
    plain = pc.Reference(pc.blob(), ref.cal, literal=False)
    for mode in (VRC, TEST, DVR):
        for view in pc.VIEWS:
            a, b = ref.frame(Case(view, mode)), plain.frame(Case(view, mode))
            assert np.all(np.isfinite(a)), (name, mode, view)
            changed = int(np.any(a != b, axis=-1).sum())
            assert changed >= 20, (name, mode, view, changed)


def test_zero_visible_tf_tells_nan_from_zero():
    """Under tf_zero_visible the VRC frame of blob_special() changes when its NaN voxels are given a
    value of class 0 instead of the 0 they read as (1e30: above every interval): the case that pins
    max(0, v) on NaN.  Under the default TF the two frames are the same."""
    vol = pc.blob_special()
    other = np.where(np.isnan(vol), np.float32(1e30), vol)
    for tf, differ in ((pc.tf_zero_visible(), True), (None, False)):
        a = pc.Reference(vol, 255.0, tf=tf, literal=False)
        b = pc.Reference(other, 255.0, tf=tf, literal=False)
        for view in ("z", "obl"):
            fa, fb = a.frame(Case(view, VRC)), b.frame(Case(view, VRC))
            assert np.all(np.isfinite(fa))
            n = int(np.any(fa != fb, axis=-1).sum())
            assert (n >= 5) if differ else (n == 0), (differ, view, n)   # (50 NaN voxels; a few pixels suffice)
