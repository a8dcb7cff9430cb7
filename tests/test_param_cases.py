"""The off-default cases of tests/param_cases.py on the CPU (oracle and dvr_ref only, no GPU): every
case draws something and leaves background, the tiny shapes are visible, the special voxels change
the frame, the closed-form octree equals the literal one where both exist, the DVR restatement
stays pinned to the oracle off the default viewplane distance, and the same cases draw in VR_MODE_MIP
(mip_ref): enough in-volume pixels and different maxima, clamped and unclamped pixels at a fractional
cal_max, the deep shapes, and a volume of subnormals that is not the zero volume."""
import numpy as np
import pytest

import dvr_ref
import oracle
import param_cases as pc
from param_cases import DVR, MIP, TEST, VRC, Case

MIN_PIXELS = 40
F32 = np.float32


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


# ---- VR_MODE_MIP and the DVR / MIP volumes: the cases of tests/test_gpu_params.py and
# tests/test_gpu_volumes.py are not vacuous.  The floors are round numbers under what mip_ref /
# dvr_ref give (>= 1 where that is 1).

def check_mip_content(ref, case, what):
    """At least 140 in-volume pixels with at least 90 different maxima among them."""
    f, m, hit = ref.mip(case)
    assert f is ref.frame(case) and np.all(np.isfinite(f)) and np.all(f[..., 3] == 1.0), what
    assert int(hit.sum()) >= 140, (what, int(hit.sum()))
    assert len(np.unique(m[hit])) >= 90, (what, len(np.unique(m[hit])))
    return f, m, hit


@pytest.mark.parametrize("vpd,scale", pc.VPD)
def test_mip_vpd_cases_draw(vpd, scale):
    ref = pc.shared_reference("blob")
    for view in pc.VIEWS:
        check_mip_content(ref, Case(view, MIP, vpd=vpd, scale=scale), (vpd, scale, view))


@pytest.mark.parametrize("rsw,rsh", pc.SCREENS)
def test_mip_screen_cases_draw(rsw, rsh):
    ref = pc.shared_reference("blob")
    for view in pc.VIEWS:
        check_mip_content(ref, Case(view, MIP, rsw=rsw, rsh=rsh), (rsw, rsh, view))


def test_mip_fractional_cal_max_clamps_some_pixels_only():
    """cal_max = 200.7: min(max(m / cal_max, 0), 1) is hit from above on some in-volume pixels and
    not on others (z: 149 inside (0, 1) and 91 at 1; obl: 298 and 93)."""
    ref = pc.Reference(pc.blob(), 200.7)
    for view, inner, clamped in (("z", 140, 90), ("obl", 290, 90)):
        f, m, hit = ref.mip(Case(view, MIP))
        g = f[..., 0][hit]
        assert int(((g > 0) & (g < 1)).sum()) >= inner, (view, int(((g > 0) & (g < 1)).sum()))
        assert int((g == 1).sum()) >= clamped, (view, int((g == 1).sum()))
        assert np.all(m[hit][g == 1] >= F32(200.7))


@pytest.mark.parametrize("shape", list(pc.TINY))
def test_tiny_shapes_are_visible_in_mip(shape):
    """(the minimum is one pixel, (65, 3, 2) along x)"""
    ref = pc.Reference(pc.tiny_volume(shape), 255.0)
    for view in ("z", "x", "y_back", "obl"):
        f, m, hit = ref.mip(Case(view, MIP, rsw=pc.TINY[shape], frame=(pc.TW, pc.TH, pc.TS)))
        assert np.all(np.isfinite(f))
        assert int(hit.sum()) >= 1, (shape, view)


@pytest.mark.parametrize("name", ["special", "special200"])
def test_special_voxels_reach_mip(name):
    ref = pc.shared_reference(name)
    for view in pc.VIEWS:
        f, m, hit = ref.mip(Case(view, MIP))
        assert np.all(np.isfinite(f)), (name, view)
        assert len(np.unique(m[hit])) >= 180, (name, view, len(np.unique(m[hit])))
        assert int((f[..., 0][hit] == 1).sum()) >= 90, (name, view)   # (1e30, 3.4e38, 255.5, 256: clamped)


@pytest.mark.parametrize("name", list(pc.DEEP))
def test_deep_shapes_in_dvr_and_mip(name):
    """The 1.2 screen draws along z, x and y_back in both modes (MIP: 1 to 33 pixels) and nothing along
    obl; the 0.02 screen draws along obl (MIP: 12 pixels on deep_x, 17 on deep_z; DVR: 7 and 9)."""
    ref = pc.shared_reference(name)
    for mode in (DVR, MIP):
        for case in pc.deep_volume_cases(mode):
            f = ref.frame(case)
            assert np.all(np.isfinite(f))
            n = int(ref.mip(case)[2].sum()) if mode == MIP else pc.non_background(f)
            if case.view == "obl" and case.rsw == 1.2:
                assert n == 0, (name, mode, n)
            elif case.view == "obl":
                assert n >= (10 if mode == MIP else 5), (name, mode, n)
            else:
                assert n >= 1, (name, mode, case.view, n)


def test_subnormal_volume_is_not_the_zero_volume():
    """blob_subnormal(): every voxel k * 2^-140, an exact subnormal.  Its DVR and MIP frames draw, and
    they are not the frames of the all-zero volume -- what a march that flushes subnormals to zero
    renders.  The byte copy is not taken (no voxel but 0 is an integer), so the float gathers are the
    path under test."""
    ref = pc.shared_reference("subnormal")
    v = ref.vol
    nz = v[v != 0]
    assert nz.size >= 10000 and np.all(nz > 0) and np.all(nz < F32(2.0 ** -126))
    assert np.array_equal(v.astype(np.float64) * 2.0 ** 140, pc.blob().astype(np.float64))   # exact multiples
    # the gate of dvr_bytes_kernel: every voxel an integer in 0..255
    with np.errstate(invalid="ignore"):
        lossless = (v >= 0) & (v <= 255) & (v.astype(np.int32).astype(F32) == v)
    assert not np.all(lossless)
    zero = pc.Reference(np.zeros_like(v), pc.SUBNORMAL_CAL, literal=False)
    for view in ("z", "x", "obl"):
        for mode in (DVR, MIP):
            case = Case(view, mode)
            f = ref.frame(case)
            assert np.all(np.isfinite(f)), (view, mode)
            assert pc.non_background(f) >= MIN_PIXELS, (view, mode, pc.non_background(f))
            changed = int(np.any(f != zero.frame(case), axis=-1).sum())
            assert changed >= MIN_PIXELS, (view, mode, changed)
        f, m, hit = ref.mip(Case(view, MIP))
        assert len(np.unique(m[hit])) >= 90 and np.all(m[hit] < F32(2.0 ** -126)), view


# ---- the shading stage (VR_FLAG_SHADE): the cases of tests/test_gpu_shade.py are not vacuous ----

SHADE_ROWS = [(v, False) for v in pc.VIEWS] + [("z", True), ("obl", True)]   # (view, conic)
TINY_SHADED = [(1, 1, 1), (1, 9, 4), (7, 1, 2), (3, 3, 1), (9, 8, 7), (65, 3, 2)]


def shade_changes(ref, case, what, expect=True):
    """The shaded reference differs from the plain one by more than 1e-2 somewhere."""
    a, b = ref.frame(case), ref.frame(case.plain())
    assert np.all(np.isfinite(a)), what
    d = float(np.abs(a.astype(np.float64) - b).max())
    assert (d > 1e-2) == expect, (what, d)


@pytest.mark.parametrize("name", ["blob", "cube"])
def test_shading_changes_every_view(name):
    ref = pc.shared_reference(name)
    for view, conic in SHADE_ROWS:
        for sname, sh in pc.SHADE_SETS.items():
            case = Case(view, VRC, conic=conic, shade=sh)
            check_content(ref.frame(case), (name, view, conic, sname))
            if sname == "id":   # the identity coefficients: the plain frame bit for bit
                assert np.array_equal(ref.frame(case).view(np.uint32), ref.frame(case.plain()).view(np.uint32))
            else:
                shade_changes(ref, case, (name, view, conic, sname))


def test_shaded_reference_follows_conic_and_march_params():
    """render_vrc_shaded goes through or_vrc_sample_point like the plain march: with the identity
    coefficients it is the plain frame at every sample distance, front clip and projection, on the
    literal and on the closed-form octree, and the two octrees agree on a general coefficient set."""
    ref = pc.shared_reference("blob")
    closed = pc.Reference(pc.blob(), 255.0, literal=False)
    rows = [(n, v, False) for n in pc.SD_FC for v in ("z", "x", "obl")] + [(n, v, True) for n in ("default", "fc_in")
                                                                            for v in ("z", "obl")]
    for name, view, conic in rows:
        ident = pc.sd_fc_case(name, view, conic=conic, shade=pc.SH_ID)
        plain = ref.frame(ident.plain())
        assert np.array_equal(ref.frame(ident).view(np.uint32), plain.view(np.uint32)), (name, view, conic)
        case = pc.sd_fc_case(name, view, conic=conic, shade=pc.SH_KS0)
        shade_changes(ref, case, (name, view, conic))
        assert np.array_equal(ref.frame(case).view(np.uint32), closed.frame(case).view(np.uint32)), (name, view, conic)
    # sd, fc and conic are honoured: a shaded frame changes with each of them
    for view in ("z", "obl"):
        base = ref.frame(Case(view, VRC, shade=pc.SH_KS0))
        for other in (pc.sd_fc_case("fc_in", view, shade=pc.SH_KS0), pc.sd_fc_case("sd_big", view, shade=pc.SH_KS0),
                      Case(view, VRC, conic=True, shade=pc.SH_KS0)):
            assert int(np.any(ref.frame(other) != base, axis=-1).sum()) >= MIN_PIXELS, (view, other.key())


def test_cube_has_a_visible_voxel_in_every_face():
    ref = pc.shared_reference("cube")
    v = ref.vol
    cls = np.array([oracle.tf_class(ref.otf[0], ref.otf[1], float(np.float32(x) / np.float32(255))) for x in range(256)])
    visible = np.array([ref.tf[k][2][3] != 0.0 for k in cls])[v.astype(int)]
    for a in range(3):
        for side in (0, -1):
            assert visible.take(side, axis=a).any(), (a, side)
    # and the one-sided difference is not the central one there: some face voxel's gradient changes
    # when the volume is padded with zeros
    assert v[0].any() and v[-1].any() and v[:, 0].any() and v[:, -1].any() and v[..., 0].any() and v[..., -1].any()


@pytest.mark.parametrize("shape", TINY_SHADED + list(pc.DEEP))
def test_shaded_small_and_deep_shapes_are_visible(shape):
    deep = isinstance(shape, str)
    ref = pc.shared_reference(shape) if deep else pc.Reference(pc.tiny_volume(shape), 255.0)
    if deep:
        assert ref.octree.depth == 11 and ref.vol.shape == pc.DEEP[shape]
    for view in ("z", "x", "obl"):
        for sh in (pc.SH_KS0, pc.SH_N0):
            cases = pc.deep_cases(view, shade=sh) if deep else [Case(view, VRC, rsw=pc.TINY[shape],
                                                                     frame=(pc.TW, pc.TH, pc.TS), shade=sh)]
            for case in cases:
                f = ref.frame(case)
                assert np.all(np.isfinite(f))
                assert pc.non_background(f) >= 1, (shape, view, case.rsw)
                if shape != (1, 1, 1):   # (one flat voxel: d = 1, and ka + kd = 1 in SH_KS0)
                    shade_changes(ref, case, (shape, view, sh, case.rsw))


def test_shaded_non_finite_gradients_are_reached():
    """blob_special under tf_zero_visible: the shaded frame changes when the non-finite voxels are
    zeroed.  And with NaN and -inf alone zeroed -- voxels that read as 0 either way, so the plain
    frame stays the same bit for bit -- the shaded frame still changes: that difference can only
    come from the gradients of their neighbours."""
    vol = pc.blob_special()
    a = pc.shared_reference("special_tf0")
    zeroed = pc.Reference(np.where(np.isfinite(vol), vol, np.float32(0.0)), 255.0, tf=pc.tf_zero_visible(),
                          literal=False)
    same_class = pc.Reference(np.where(np.isnan(vol) | (vol == -np.inf), np.float32(0.0), vol), 255.0,
                              tf=pc.tf_zero_visible(), literal=False)
    for view in ("z", "obl"):
        plain = Case(view, VRC)
        assert np.array_equal(a.frame(plain).view(np.uint32), same_class.frame(plain).view(np.uint32)), view
        for sh in (pc.SH_KS0, pc.SH_N0):
            case = Case(view, VRC, shade=sh)
            fa = a.frame(case)
            assert np.all(np.isfinite(fa)), (view, sh)
            for b in (zeroed, same_class):
                n = int(np.any(fa != b.frame(case), axis=-1).sum())
                assert n >= 20, (view, sh, n)
    for name in ("special", "special_tf0"):
        ref = pc.shared_reference(name)
        for view in ("z", "obl"):
            shade_changes(ref, Case(view, VRC, shade=pc.SH_KS0), (name, view))


def test_special_volume_holds_a_denormal_headlight_cosine():
    """blob_special has a voxel whose N.L along z is a positive denormal (its z neighbours are 1e-40
    and a zero): the device's hardware log2 reads such a d as 0, and d^0 must still be 1 (SH_N0)."""
    v = pc.blob_special()

    def grad(ax):
        lo = np.concatenate([np.take(v, [0], ax), np.take(v, range(v.shape[ax] - 1), ax)], ax)
        hi = np.concatenate([np.take(v, range(1, v.shape[ax]), ax), np.take(v, [-1], ax)], ax)
        return (hi - lo) * np.float32(0.5)

    with np.errstate(all="ignore"):
        gx, gy, gz = grad(0), grad(1), grad(2)
        len2 = (gx * gx + gy * gy) + gz * gz
        d = -gz * (np.float32(1.0) / np.sqrt(len2))   # view "z": the headlight is (0, 0, 1)
        tiny = (len2 > 0) & (d > 0) & (d < np.float32(2.0 ** -126)) & (v > 0) & np.isfinite(v)
    assert int(tiny.sum()) >= 1
    ref = pc.shared_reference("special")
    for x in v[tiny]:   # and it is drawn: its class is a visible one
        assert ref.tf[oracle.tf_class(ref.otf[0], ref.otf[1], float(np.float32(x) / np.float32(255)))][2][3] != 0.0
