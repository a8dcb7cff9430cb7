"""Seeded random views against the oracle: cameras on a sphere around the volume (re-derived with
processInput's formulas, myApp.cu:1105-1112, on both sides), odd frame sizes and sample counts,
every compositing mode.  Exact and ESS-only frames are bitwise the oracle's (the reference's
back-to-front blend, kernel.cu:194-225); ESS + ERT and ERT alone within 1e-4; TEST exact bitwise
(kernel.cu:72-187).  Covers the general-view paths (padded leaf maps, lazy empty-space tests,
empty-cell skipping of exact frames) on views no other test picks.  The same views in DVR, MIP and ISO
against tests/dvr_ref.py, mip_ref.py and iso_ref.py (test_random_views_field_modes), and in SDVR, CDVR and
SCDVR against tests/sdvr_ref.py, cmap_ref.py and scdvr_ref.py (test_random_views_lit_field_modes), and in all
six field modes under a seeded crop box per view against tests/crop_ref.py (test_random_views_crop)."""
import math

import numpy as np
import pytest

import volumerenderingproject_amd as vr
from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu

TOL = 1e-4
E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT


def random_views(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        W, H = int(rng.integers(17, 97)), int(rng.integers(13, 81))
        S = int(rng.integers(20, 320))
        th, ph = rng.uniform(0, 2 * math.pi), rng.uniform(-1.2, 1.2)
        dist = rng.uniform(0.7, 1.3)
        pos = (dist * math.cos(ph) * math.sin(th), dist * math.sin(ph), dist * math.cos(ph) * math.cos(th))
        up = (0.0, 1.0, 0.0) if abs(ph) < 1.0 else (1.0, 0.0, 0.0)
        out.append((W, H, S, pos, up))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_views_match_oracle(avg152, avg152_octree, oracle_mod, seed):
    vol, cal = avg152
    O = oracle_mod
    r = vr.VolumeRenderer(vol, cal, device=0)
    try:
        for i, (W, H, S, pos, up) in enumerate(random_views(16, seed)):
            p = vr.default_params(W, H, S)
            cam = vr.derive_camera(pos, up, p.real_screen_width, p.real_screen_height)
            op = O.params(W, H, S)
            ocam = O.camera_derive(pos, up, op.real_screen_width, op.real_screen_height)
            ref = avg152_octree.render_vrc(cal, O.default_tf(), op, ocam)
            for flags in (0, E):
                assert_bitwise(r.render(vr.default_params(W, H, S, flags=flags), cam), ref)
            for flags in (E | T, T):
                got = r.render(vr.default_params(W, H, S, flags=flags), cam)
                assert np.abs(got - ref).max() <= TOL, (i, flags)
            if i % 3 == 0:
                tref = O.render_test(vol, cal, O.default_tf(), op, ocam)
                assert_bitwise(r.render(vr.default_params(W, H, S, mode=vr.VR_MODE_TEST), cam), tref)
    finally:
        r.close()


ISO_RGB, ISO_SHADE = (0.9, 0.8, 0.7), (0.3, 0.7, 0.0, 16.0)   # (ks = 0: the specular term is exact)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_views_field_modes(avg152, oracle_mod, seed):
    """The three modes of the trilinear field on the same views, against their numpy restatements.  DVR:
    exact and ESS bitwise, ERT and ESS | ERT within TOL.  MIP and ISO: all four flag combinations
    bitwise; ISO at iso = 100 (refined surfaces) and at iso = -1 (the first in-volume sample of every
    ray: the clip).  Every third view again from the float volume (dvr_volume = 1)."""
    import dvr_ref
    import iso_ref
    import mip_ref
    from test_gpu_params import assert_same
    vol, cal = avg152
    O = oracle_mod
    tf = vr.default_transfer_function()
    DVR, MIP, ISO = vr.VR_MODE_DVR, vr.VR_MODE_MIP, vr.VR_MODE_ISO

    def params(mode, W, H, S, flags):
        p = vr.default_params(W, H, S, mode=mode, flags=flags)
        if mode == ISO:
            p.shade_ambient, p.shade_diffuse, p.shade_specular, p.shade_shininess = ISO_SHADE
        return p

    hits = refinable = 0
    with vr.VolumeRenderer(vol, cal, device=0) as a, \
            vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for i, (W, H, S, pos, up) in enumerate(random_views(16, seed)):
            op = O.params(W, H, S)
            cam = vr.derive_camera(pos, up, op.real_screen_width, op.real_screen_height)
            ocam = O.camera_derive(pos, up, op.real_screen_width, op.real_screen_height)
            dref = dvr_ref.render(vol, cal, tf, op, ocam)
            mref = mip_ref.render(vol, cal, op, ocam)[0]
            irefs = {}
            for iso in (100.0, -1.0):
                irefs[iso], rec = iso_ref.render(vol, op, ocam, iso, ISO_RGB, ISO_SHADE)
                hits += int(rec["hit"].sum())
                refinable += int(rec["refinable"].sum())
            for r in ((a, b) if i % 3 == 0 else (a,)):
                for flags in (0, E):
                    assert_same(r.render(params(DVR, W, H, S, flags), cam), dref, (i, "dvr", flags))
                for flags in (T, E | T):
                    got = r.render(params(DVR, W, H, S, flags), cam)
                    assert np.abs(got - dref).max() <= TOL, (i, flags)
                for flags in (0, E, T, E | T):
                    assert_same(r.render(params(MIP, W, H, S, flags), cam), mref, (i, "mip", flags))
                for iso, iref in irefs.items():
                    r.set_isosurface(iso, ISO_RGB)
                    for flags in (0, E, T, E | T):
                        assert_same(r.render(params(ISO, W, H, S, flags), cam), iref, (i, "iso", iso, flags))
    # the views bite (iso_ref's records over both isovalues: 21223 hit rays and 6403 refinable ones at the least)
    assert hits >= 2000 and refinable >= 1500, (seed, hits, refinable)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_views_lit_field_modes(seed):
    """The same views in the three modes added after ISO, against their numpy restatements
    (tests/field_param_cases.py builds them): SDVR under the default TF with (0.2, 0.5, 0.4, 0), CDVR under
    cmap_cases.SMOOTH5, SCDVR under SMOOTH5 with scdvr_cases.EDGES and the same coefficients.  Exact and ESS
    frames are bitwise the restatement's, on the byte-copy context for every view and on the float-volume one
    (dvr_volume = 1) for every third.

    ERT and ESS | ERT against the exact frame: S reaches 319 here, and the project's bound 1e-5 R + 6 S 2^-24 M
    (test_gpu_params.test_ert_epsilon; R = M = 1.1, the largest lit colour c * 0.7 + 0.4) passes 1e-4 for S
    above about 250, so each view is held to the larger of the two (field_param_cases.random_ert_bound).
    Largest error seen on the MI355X: 8.3e-6, 8.2e-6 and 8.2e-6 for seeds 1, 2 and 3 (264 frames each),
    against bounds of 1e-4 to 1.37e-4; it is printed."""
    import cmap_cases as cc
    import field_param_cases as fp
    import scdvr_cases as xc
    import sdvr_cases as sc
    from test_gpu_dvr import assert_bits
    vol, cal = sc.volume("avg152")
    worst = frames = 0
    with vr.VolumeRenderer(vol, cal, device=0) as a, \
            vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for r in (a, b):
            r.set_colormap(cc.map_of(fp.SCDVR_SETS[0][0], cal))
            r.set_gradient_opacity(xc.gopa_of(fp.SCDVR_SETS[0][1]))
        for i, view in enumerate(fp.random_view_cases(seed)):
            refs = fp.random_references(view)[0]
            bound = fp.random_ert_bound(view.S)
            cam = view.gpu_camera()
            cases = {fp.SDVR: fp.sdvr_case(view, 0, "avg152"), fp.CDVR: fp.cdvr_case(view, "avg152"),
                     fp.SCDVR: fp.scdvr_case(view, 0, "avg152")}
            for r in ((a, b) if i % 3 == 0 else (a,)):
                for mode, case in cases.items():
                    exact = r.render(case.gpu_params(0, mode=mode), cam)
                    assert_bits(exact, refs[mode], (seed, i, mode, "exact"))
                    assert_bits(r.render(case.gpu_params(E, mode=mode), cam), exact, (seed, i, mode, "ess"))
                    for flags in (T, E | T):
                        got = r.render(case.gpu_params(flags, mode=mode), cam)
                        err = float(np.abs(got - exact).max())
                        worst = max(worst, err)
                        assert err <= bound, (seed, i, mode, flags, view.S, err, bound)
                        assert np.all(got[..., 3] == 1.0)
                    frames += 4
    print("random views, lit field modes: seed", seed, "frames compared", frames, "largest ERT error", worst)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_views_crop(seed):
    """The same views under a crop box each (crop_cases.random_boxes: per axis whole with probability 1/4,
    otherwise lo < hi uniform in [-2, d + 2] at least 3 voxels apart), in the six field modes against
    tests/crop_ref.py, one evaluation of a view's samples shared by the modes.  The rule is
    test_gpu_crop.check_all_flags: exact and ESS bitwise, MIP and ISO bitwise in all four flag combinations, ERT
    and ESS | ERT within field_param_cases.random_ert_bound(S); on the byte-copy context for every view and on
    the float-volume one for every third.  At least half of a seed's views draw under their box."""
    import crop_cases as cx
    import field_param_cases as fp
    import sdvr_cases as sc
    import test_crop_ref as tc
    from test_gpu_crop import check_all_flags, set_box
    vol, cal = sc.volume("avg152")
    seen, frames, drawing = [], 0, 0
    boxes = cx.random_boxes(seed, vol.shape)
    with vr.VolumeRenderer(vol, cal, device=0) as a, \
            vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for r in (a, b):
            for mode in ("dvr", "scdvr"):
                cx.apply_set(r, mode, 0, "avg152")
            r.set_isosurface(tc.ISO_VALUE, cx.ISO_RGB)
        for i, (view, bx) in enumerate(zip(fp.random_view_cases(seed), boxes)):
            refs, caught = cx.random_references(view, bx)
            drew = bool(fp.drawn(refs["dvr"], view.bg).any())
            assert caught > 0 or not drew
            drawing += drew
            bound = fp.random_ert_bound(view.S)
            cam = view.gpu_camera()
            for r in ((a, b) if i % 3 == 0 else (a,)):
                set_box(r, bx)
                for mode in cx.MODES:
                    check_all_flags(r, mode, refs[mode], view.W, view.H, view.S, cam, (seed, i, mode, bx), bound,
                                    make=lambda fl: cx.gpu_params(mode, 0, view, fl), seen=seen)
                    frames += 4
    print("random views under a crop box: seed", seed, "frames compared", frames, "views drawing", drawing,
          "largest ERT error", max(seen))
    assert 2 * drawing >= len(boxes), (seed, drawing)
