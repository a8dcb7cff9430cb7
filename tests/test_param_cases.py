"""The off-default cases of tests/param_cases.py on the CPU (oracle and dvr_ref only, no GPU): every
case draws something and leaves background, the tiny shapes are visible, the special voxels change
the frame, the closed-form octree equals the literal one where both exist, the DVR restatement
stays pinned to the oracle off the default viewplane distance, and the same cases draw in VR_MODE_MIP
(mip_ref): enough in-volume pixels and different maxima, clamped and unclamped pixels at a fractional
cal_max, the deep shapes, and a volume of subnormals that is not the zero volume.  VR_MODE_ISO
(iso_ref's record): enough hit rays on every row, refinable and non-refinable hits, the first
in-volume sample at iso = -1, the thresholds of blob_special(), and the three ranges of len2."""
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


# ---- VR_MODE_ISO: the cases of tests/test_gpu_params.py, tests/test_gpu_volumes.py are not vacuous.
# Conditions on iso_ref's record; the floors are round numbers under what the restatement gives.

ISO_SPECIAL, ISO_SUBNORMAL, ISO_SMALL, ISO_DEEP = pc.ISO_SPECIAL, pc.ISO_SUBNORMAL, pc.ISO_SMALL, pc.ISO_DEEP


def iso_record(ref, case):
    frame, rec = ref.iso(case)
    assert frame is ref.frame(case) and np.all(np.isfinite(frame)) and np.all(frame[..., 3] == 1.0), case.key()
    return frame, rec


def check_iso_hits_first_inside(ref, case, what):
    """Every in-volume ray hits at its first in-volume sample, and none is refinable (that sample's
    predecessor is outside the volume): the linear-model clip may not drop it."""
    frame, rec = iso_record(ref, case)
    inside = ref.inside(case)
    hit = rec["hit"]
    assert np.array_equal(hit, inside.any(axis=2)) and hit.any(), what
    assert np.array_equal(rec["s_h"][hit], inside.argmax(axis=2)[hit]), what
    assert not rec["refinable"].any(), what
    return frame, rec


@pytest.mark.parametrize("vpd,scale", pc.VPD)
def test_iso_vpd_cases_draw(vpd, scale):
    """iso = 128 on the blob: at least 50 hit rays (52 at (0.0, 0.2) along obl).  With every sample in the
    camera plane there is no light direction and nothing to refine; with the camera inside the box
    some view has hits whose predecessor is outside beside hits that are refined."""
    ref = pc.shared_reference("blob")
    mixed = False
    for view in pc.VIEWS:
        _, rec = iso_record(ref, Case(view, pc.ISO, vpd=vpd, scale=scale))
        hit = rec["hit"]
        n, nr = int(hit.sum()), int(rec["refinable"].sum())
        assert n >= 50, (vpd, scale, view, n)
        if vpd == 0.0:
            assert nr == 0 and np.all(rec["d"][hit] == 1.0), (view, nr)
        mixed |= 0 < nr < n
        # and at iso = -1: the clip check
        check_iso_hits_first_inside(ref, Case(view, pc.ISO, vpd=vpd, scale=scale, iso=-1.0), (vpd, scale, view))
    if (vpd, scale) in ((0.6, 0.3), (-0.5, -0.2)):
        assert mixed, (vpd, scale)


@pytest.mark.parametrize("rsw,rsh", pc.SCREENS)
def test_iso_screen_cases_draw(rsw, rsh):
    """At least 70 hits (76 the smallest), all refinable: the blob lies strictly inside the volume."""
    ref = pc.shared_reference("blob")
    for view in pc.VIEWS:
        _, rec = iso_record(ref, Case(view, pc.ISO, rsw=rsw, rsh=rsh))
        n = int(rec["hit"].sum())
        assert n >= 70 and np.array_equal(rec["refinable"], rec["hit"]), (rsw, rsh, view, n)
        check_iso_hits_first_inside(ref, Case(view, pc.ISO, rsw=rsw, rsh=rsh, iso=-1.0), (rsw, rsh, view))


@pytest.mark.parametrize("iso", ISO_SPECIAL)
def test_iso_special_voxels_thresholds(iso):
    """blob_special() under thresholds from below every voxel to above every one: the cell bounds' margin
    (max + 2^-20 max(|min|, |max|)) is tried at each, and from 255.5 up a hit lies beside a voxel of 1e30
    or 3.4e38 -- len2 overflows to +inf, inv = 0, N = (-0, -0, -0), d = 0 on a ray that has a normal."""
    ref = pc.shared_reference("special")
    bg = np.array(pc.DEFAULT_BG[:3], F32)
    for view in ("z", "x", "obl"):
        case = Case(view, pc.ISO, iso=iso)
        if iso < 0:
            check_iso_hits_first_inside(ref, case, (iso, view))
            continue
        frame, rec = iso_record(ref, case)
        hit = rec["hit"]
        n = int(hit.sum())
        if iso in (1e-40, 100.0):   # (224 and 220 at the least)
            assert n >= 200 and np.array_equal(rec["refinable"], hit), (iso, view, n)
        elif iso in (255.5, 1e30):  # (51 at the least, at 1e30)
            assert n >= 50, (iso, view, n)
            assert np.all(rec["has_normal"][hit]) and np.all(rec["d"][hit] == 0.0), (iso, view)
            assert np.all(rec["N"][hit] == 0.0), (iso, view)
        else:
            assert n == 0 and np.all(frame[..., :3] == bg), (iso, view, n)


def test_iso_subnormal_volume_has_a_surface_and_no_normal():
    """blob_subnormal() at 128 * 2^-140: the blob's surface at 128 (hit, s_h and hi are equal: scaling by
    a power of two commutes with every lerp down there, no product rounds), but len2 -- squares of
    gradients below 2^-132 -- underflows to 0 on every hit: no normal, d = 1.  Not the zero volume's frame."""
    ref, blob = pc.shared_reference("subnormal"), pc.shared_reference("blob")
    zero = pc.Reference(np.zeros_like(ref.vol), pc.SUBNORMAL_CAL, literal=False)
    for view in ("z", "x", "obl"):
        case = Case(view, pc.ISO, iso=ISO_SUBNORMAL)
        frame, rec = iso_record(ref, case)
        _, want = iso_record(blob, Case(view, pc.ISO))
        hit = rec["hit"]
        assert int(hit.sum()) >= 200, view
        for k in ("hit", "s_h", "hi"):
            assert np.array_equal(rec[k], want[k]), (view, k)
        assert not rec["has_normal"][hit].any() and np.all(rec["d"][hit] == 1.0), view
        changed = int(np.any(frame != zero.frame(case), axis=-1).sum())
        assert changed >= MIN_PIXELS, (view, changed)


def test_iso_small_volume_normals_come_from_subnormal_len2():
    """blob_small() at 128 * 2^-72: the blob's surface again, and every hit has a normal although len2 is
    a subnormal: few bits are left of it, so N = -g / sqrt(len2) is not the blob's N on most rays (equal
    on 5 of 224 along z, 10 of 322 along obl).  A device that flushed len2 (no normal, d = 1) or took
    the square root as if its input were normal cannot produce this frame."""
    ref, blob = pc.shared_reference("small"), pc.shared_reference("blob")
    v = ref.vol
    nz = v[v != 0]
    assert np.all(nz >= F32(2.0 ** -126)) and np.array_equal(v.astype(np.float64) * 2.0 ** 72, pc.blob())
    for view in ("z", "x", "obl"):
        case = Case(view, pc.ISO, iso=ISO_SMALL)
        frame, rec = iso_record(ref, case)
        plain_frame, want = iso_record(blob, Case(view, pc.ISO))
        hit = rec["hit"]
        n = int(hit.sum())
        assert n >= 200, (view, n)
        for k in ("hit", "s_h", "hi"):
            assert np.array_equal(rec[k], want[k]), (view, k)
        assert np.all(rec["has_normal"][hit]), view
        differ = int(np.any(rec["N"][hit] != want["N"][hit], axis=-1).sum())
        assert 2 * differ > n, (view, differ, n)
        assert pc.non_background(frame) >= MIN_PIXELS and not np.array_equal(frame, plain_frame), view


@pytest.mark.parametrize("name", list(pc.DEEP))
def test_deep_shapes_in_iso(name):
    """iso = 112 on the needles over deep_volume_cases: deep_x 17 / 1 / 17 / 0 / 8 hits, deep_z 1 / 16 /
    14 / 0 / 6 (z, x, y_back, obl at 1.2, obl at 0.02)."""
    ref = pc.shared_reference(name)
    assert float(np.median(ref.vol)) == ISO_DEEP
    for case in pc.deep_volume_cases(pc.ISO, iso=ISO_DEEP):
        _, rec = iso_record(ref, case)
        n = int(rec["hit"].sum())
        if case.view == "obl" and case.rsw == 1.2:
            assert n == 0, (name, n)
        else:
            assert n > 0, (name, case.view, case.rsw, n)


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
