"""Non-default render parameters on the GPU: sample distance and front clip (VRC), viewplane distance
(TEST, DVR, MIP, ISO), anamorphic and far screens, backgrounds, ERT epsilons and a fractional cal_max, on
every specialised march, against the references of tests/param_cases.py (which
tests/test_param_cases.py keeps from being vacuous).

The project's rules: exact frames (flags 0) are the reference's values bit for bit, ESS alone equals
the exact frame, ERT and ESS | ERT at the default epsilon, background and TF are within TOL = 1e-4.
VR_MODE_MIP and VR_MODE_ISO have no tolerance: all four flag combinations give the exact frame
(check_flags_bitwise; ISO with the coefficient sets whose specular term is exact, SH_KS0 and SH_N0).
Values are compared with np.array_equal, not bit patterns: a background of -0.0 legitimately comes
back as +0.0 from a marched pixel.
"""
import numpy as np
import pytest

import param_cases as pc
import volumerenderingproject_amd as vr
from param_cases import DVR, ISO, MIP, TEST, VRC, Case

pytestmark = pytest.mark.gpu

E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
TOL = 1e-4
F = np.float32


def assert_same(got, ref, what):
    assert got.shape == ref.shape, what
    if not np.array_equal(got, ref):
        d = np.abs(got.astype(np.float64) - ref)
        raise AssertionError((what, "values differ:", int((got != ref).sum()), "max |diff|", float(d.max()),
                              "at", np.unravel_index(d.argmax(), d.shape)))


def check_flags(r, ref, case, what):
    """flags 0 == ref, ESS == exact, ERT and ESS | ERT within TOL, alpha 1.  Returns the exact frame."""
    cam = case.gpu_camera()
    exact = r.render(case.gpu_params(0), cam)
    assert_same(exact, ref, (what, "exact"))
    assert_same(r.render(case.gpu_params(E), cam), exact, (what, "ess"))
    for fl in (T, E | T):
        fast = r.render(case.gpu_params(fl), cam)
        err = float(np.abs(fast - ref).max())
        assert err <= TOL, (what, "flags", fl, err)
        assert np.all(fast[..., 3] == 1.0), (what, fl)
    return exact


def check_flags_bitwise(r, ref, case, what):
    """VR_MODE_MIP and VR_MODE_ISO: flags 0 == ref, and ESS, ERT and ESS | ERT == the flags-0 frame -- a
    skipped sample is one that could not have replaced the maximum (MIP) or lies below the isovalue
    (ISO), so there is no tolerance -- alpha 1.  Returns the exact frame."""
    assert case.mode in (MIP, ISO)
    cam = case.gpu_camera()
    exact = r.render(case.gpu_params(0), cam)
    assert_same(exact, ref, (what, "exact"))
    assert np.all(exact[..., 3] == 1.0), what
    for fl in (E, T, E | T):
        assert_same(r.render(case.gpu_params(fl), cam), exact, (what, "flags", fl))
    return exact


def check_flags_mip(r, ref, case, what):
    """check_flags_bitwise for a MIP case."""
    assert case.mode == MIP
    return check_flags_bitwise(r, ref, case, what)


def check_mode(r, ref, case, what):
    """check_flags_bitwise for a MIP or an ISO case (ISO: after giving the context the case's isovalue
    and surface colour), check_flags for every other mode."""
    if case.mode == ISO:
        r.set_isosurface(case.iso, case.rgb)
    return (check_flags_bitwise if case.mode in (MIP, ISO) else check_flags)(r, ref, case, what)


def ert_bound(tf, bg, eps, S):
    """Per channel: eps * R + 6 * S * 2^-24 * M (test_ert_epsilon's docstring)."""
    cols = np.array([t[2][:3] for t in tf] + [tuple(bg[:3])], np.float64)
    R = cols.max(axis=0) - cols.min(axis=0)
    M = np.abs(cols).max(axis=0)
    return eps * R + 6.0 * S * 2.0 ** -24 * M


OPTION_SETS = {
    "defaults": {},
    "columns": {"axis_columns": 2},
    "no_table": {"axis_columns": 0, "axis_table": 0},
    "no_pad": {"leaf_map_pad": 0},
    "run_words": {"run_words": 2, "table_split": 0},
    "cell_columns": {"leaf_columns": 0},
    "idx64": {"force_idx64": 1},
    "no_exact_skip": {"exact_skip": 0},
    "no_cull": {"cull": 0},
}


def check_vrc_cases(r, ref, views, frame, columns_forced, what):
    for name in pc.SD_FC:
        for view in views:
            case = pc.sd_fc_case(name, view, frame=frame)
            if columns_forced and view in pc.AXIS_VIEWS:
                cam = case.gpu_camera()
                for fl in (0, E, T, E | T):
                    plan = r.axis_columns_plan(case.gpu_params(fl), cam)
                    # the column path's gate: every axis view with a non-zero step, never a zero one
                    assert plan["columns"] == (case.sd != 0.0), (what, name, view, fl, plan)
            check_flags(r, ref.frame(case), case, (what, name, view))


@pytest.mark.parametrize("opts", list(OPTION_SETS))
def test_vrc_march_params(opts):
    ref = pc.shared_reference("blob")
    with vr.VolumeRenderer(ref.vol, ref.cal, device=0, options=vr.default_options(**OPTION_SETS[opts])) as r:
        check_vrc_cases(r, ref, list(pc.VIEWS), (pc.W, pc.H, pc.S), opts == "columns", opts)
        if opts == "defaults":   # perspective rays: the same clip and step through the conic march
            for name in ("fc_in", "sd_big"):
                for view in ("z", "obl"):
                    case = pc.sd_fc_case(name, view, conic=True)
                    assert not r.axis_columns_plan(case.gpu_params(0), case.gpu_camera())["columns"]
                    check_flags(r, ref.frame(case), case, ("conic", name, view))


@pytest.mark.parametrize("opts", ["defaults", "columns"])
def test_vrc_march_params_avg152(opts):
    """The same cases on avg152: 128 leaves, 2-bit classes, the real TF."""
    ref = pc.shared_reference("avg152")
    with vr.VolumeRenderer(ref.vol, ref.cal, device=0, options=vr.default_options(**OPTION_SETS[opts])) as r:
        check_vrc_cases(r, ref, ("z", "x", "obl"), (64, 48, 64), opts == "columns", ("avg152", opts))


def test_count_and_cull_follow_params():
    ref = pc.shared_reference("blob")
    tw = th = 16
    ntx, nty = -(-pc.W // tw), -(-pc.H // th)
    with vr.VolumeRenderer(ref.vol, ref.cal, device=0) as r:
        for name in pc.SD_FC:
            for view in pc.VIEWS:
                case = pc.sd_fc_case(name, view)
                p, cam = case.gpu_params(0), case.gpu_camera()
                assert r.count_samples(p, cam) == ref.count_in_samples(case), (name, view)
                frame = ref.frame(case)
                bg = np.array(case.bg, F)
                ids = set(r.visible_tiles(p, cam, tw, th).tolist())
                assert ids <= set(range(ntx * nty)), (name, view)
                for t in set(range(ntx * nty)) - ids:
                    tx, ty = divmod(t, nty)
                    blk = frame[tx * tw:(tx + 1) * tw, ty * th:(ty + 1) * th]
                    assert np.all(blk[..., :3] == bg[:3]), (name, view, t)


TEST_DVR_CONTEXTS = {
    "test_plane_march": (TEST, {"test_plane_march": 1}),
    "test_no_plane_march": (TEST, {"test_plane_march": 0}),
    "test_corners0": (TEST, {"test_corners": 0}),
    "test_corners1": (TEST, {"test_corners": 1}),
    "test_corners2": (TEST, {"test_corners": 2}),
    "test_corners3": (TEST, {"test_corners": 3}),
    "dvr_auto": (DVR, {"dvr_volume": 0}),
    "dvr_float": (DVR, {"dvr_volume": 1}),
    "mip_auto": (MIP, {"dvr_volume": 0}),
    "mip_float": (MIP, {"dvr_volume": 1}),
    "iso_auto": (ISO, {"dvr_volume": 0}),
    "iso_float": (ISO, {"dvr_volume": 1}),
    "vrc_screens": (VRC, {}),
}

# ISO runs every row twice: at iso = 128 (refined surfaces; camera inside the box: hits whose
# predecessor is outside) and at iso = -1 (every in-volume ray hits at its first in-volume sample, the
# clip check), and the viewplane rows once more with the other bitwise coefficient set
ISO_PASSES = [{"iso": 128.0}, {"iso": -1.0}]


@pytest.mark.parametrize("ctx", list(TEST_DVR_CONTEXTS))
def test_test_and_dvr_viewplane_and_screen(ctx):
    mode, opts = TEST_DVR_CONTEXTS[ctx]
    ref = pc.shared_reference("blob")
    with vr.VolumeRenderer(ref.vol, ref.cal, device=0, options=vr.default_options(**opts)) as r:
        for kw in (ISO_PASSES if mode == ISO else [{}]):
            if mode != VRC:   # (VRC reads no viewplane distance; its sd and fc are test_vrc_march_params')
                for vpd, scale in pc.VPD:
                    for view in pc.VIEWS:
                        case = Case(view, mode, vpd=vpd, scale=scale, **kw)
                        check_mode(r, ref.frame(case), case, (ctx, kw, "vpd", vpd, scale, view))
            for rsw, rsh in pc.SCREENS:
                for view in pc.VIEWS:
                    case = Case(view, mode, rsw=rsw, rsh=rsh, **kw)
                    check_mode(r, ref.frame(case), case, (ctx, kw, "screen", rsw, rsh, view))
        if mode == ISO:   # shininess 0: the specular term is ks where d > 0 and where d = 0 alike
            for vpd, scale in pc.VPD:
                for view in pc.VIEWS:
                    case = Case(view, mode, vpd=vpd, scale=scale, shade=pc.SH_N0)
                    check_mode(r, ref.frame(case), case, (ctx, "n0", "vpd", vpd, scale, view))


BACKGROUNDS = [(0.7, -0.25, 1.5, 0.3), (0.0, 0.0, 0.0, 0.0), (1e6, 1e-30, 0.5, 9.0)]


@pytest.mark.parametrize("bg", BACKGROUNDS, ids=["mixed", "zero", "huge"])
def test_background_is_honoured(bg):
    """Every mode, culled tiles included, and the tile path: the frame's rgb starts from the given
    background, its alpha is 1 whatever the background's."""
    import torch
    ref = pc.shared_reference("blob")
    tw = th = 16
    nt = (-(-pc.W // tw)) * (-(-pc.H // th))
    rs = {cull: vr.VolumeRenderer(ref.vol, ref.cal, device=0, options=vr.default_options(cull=cull))
          for cull in (0, 1, 2)}
    try:
        for mode in (VRC, TEST, DVR, MIP, ISO):
            for view in ("z", "obl"):
                case = Case(view, mode, bg=bg)
                want = ref.frame(case)
                assert np.all(want[..., 3] == 1.0)
                cam = case.gpu_camera()
                for cull, r in rs.items():
                    if mode == MIP:   # every flag combination bitwise: the background is a pixel's whole value or no part of it
                        check_flags_mip(r, want, case, (mode, view, "cull", cull))
                        continue
                    if mode == ISO:   # the same: a ray without a hit is the background, one with a hit holds none of it
                        r.set_isosurface(case.iso, case.rgb)
                        check_flags_bitwise(r, want, case, (mode, view, "cull", cull))
                        continue
                    exact = r.render(case.gpu_params(0), cam)
                    assert_same(exact, want, (mode, view, "cull", cull))
                    assert_same(r.render(case.gpu_params(E), cam), exact, (mode, view, "cull", cull, "ess"))
                    bound = ert_bound(ref.tf, bg, 1e-5, pc.S)
                    for fl in (T, E | T):
                        fast = r.render(case.gpu_params(fl), cam)
                        err = np.abs(fast[..., :3].astype(np.float64) - want[..., :3]).max(axis=(0, 1))
                        assert np.all(err <= bound), (mode, view, cull, fl, err, bound)
                        assert np.all(fast[..., 3] == 1.0)
                # the tile output: every tile rendered as rgb blocks and assembled, and the visible
                # tiles alone with the assembly filling the culled ones with the background
                r = rs[2]
                p = case.gpu_params(0)
                for ids in (np.arange(nt, dtype=np.int32), r.visible_tiles(p, cam, tw, th)):
                    tiles = torch.zeros((max(1, len(ids)), tw * th, 3), dtype=torch.float32, device="cuda:0")
                    frame = torch.full((pc.W, pc.H, 4), -7.0, dtype=torch.float32, device="cuda:0")
                    torch.cuda.current_stream().synchronize()   # (the fills run on torch's stream, the context's is non-blocking)
                    if len(ids) == nt:
                        assert r.render_tiles(p, cam, tw, th, 0, 1, tiles.data_ptr(), rgb=True) == nt
                    else:
                        assert r.render_tile_list(p, cam, tw, th, ids, 0, 1, tiles.data_ptr(), rgb=True) == len(ids)
                    r.assemble_tile_list(pc.W, pc.H, tw, th, ids, 1, max(1, len(ids)), tiles.data_ptr(), list(bg),
                                         frame.data_ptr(), rgb=True)
                    assert_same(frame.cpu().numpy(), want, (mode, view, "tiles", len(ids)))
    finally:
        for r in rs.values():
            r.close()


@pytest.mark.parametrize("mode", [VRC, TEST], ids=["vrc", "test"])
def test_ert_epsilon(mode):
    """Front to back with early termination at transmittance T < eps, against the exact frame.

    Bound, per channel: |got - exact| <= eps * R + 6 * S * 2^-24 * M, with R the spread (max - min) of
    that channel over the TF colours and the background and M the largest absolute value among them.
    First term: when the march stops at transmittance T < eps, what it leaves out is T times a convex
    mix of TF colours and the background, and what it puts in its place (T times the background) is
    one too; two convex mixes differ by at most R.  Second term: the two blend orders evaluate the
    same sum in different orders, each makes at most three roundings per step (multiply, multiply,
    add) on values of magnitude at most M, over S steps: 2 * 3 * S * 2^-24 * M.

    And epsilon steers the march: the samples evaluated do not grow with eps and are strictly fewer
    at 0.5 than at 0."""
    ref = pc.shared_reference("blob")
    epsilons = (0.0, 1e-7, 1e-5, 1e-3, 0.05, 0.5)
    with vr.VolumeRenderer(ref.vol, ref.cal, device=0) as r:
        for view in ("z", "obl"):
            case = Case(view, mode)
            cam = case.gpu_camera()
            exact = ref.frame(case)
            assert_same(r.render(case.gpu_params(0), cam), exact, (mode, view))
            for fl in (T, E | T):
                marched = []
                for eps in epsilons:
                    got = r.render(case.gpu_params(fl, ert_epsilon=eps), cam)
                    err = np.abs(got[..., :3].astype(np.float64) - exact[..., :3]).max(axis=(0, 1))
                    bound = ert_bound(ref.tf, case.bg, eps, pc.S)
                    assert np.all(err <= bound), (mode, view, fl, eps, err, bound)
                    assert np.all(got[..., 3] == 1.0)
                    if mode == VRC:
                        marched.append(r.count_marched(case.gpu_params(fl, ert_epsilon=eps), cam)[1])   # samples
                if mode == VRC:
                    assert all(a >= b for a, b in zip(marched, marched[1:])), (view, fl, marched)
                    assert marched[-1] < marched[0], (view, fl, marched)


@pytest.mark.parametrize("cal", [200.7, 1000.25])
def test_cal_max_not_an_integer(cal):
    """VRC divides by (float)(int)cal_max, TEST, DVR and MIP by the double.  MIP at 200.7: the clamp
    min(max(m / cal_max, 0), 1) is hit from above on some in-volume pixels and not on others (the
    blob's voxels reach 255)."""
    ref = pc.Reference(pc.blob(), cal)
    with vr.VolumeRenderer(ref.vol, cal, device=0) as r:
        for mode in (VRC, TEST, DVR):
            for view in ("z", "obl"):
                case = Case(view, mode)
                got = r.render(case.gpu_params(0), case.gpu_camera())
                assert_same(got, ref.frame(case), (cal, mode, view))
                assert pc.non_background(got) >= 40
        for view in ("z", "obl"):
            case = Case(view, MIP)
            got = check_flags_mip(r, ref.frame(case), case, (cal, "mip", view))
            g = got[..., 0][ref.mip(case)[2]]   # the in-volume pixels
            assert g.size >= 140
            if cal == 200.7:
                assert int((g == 1.0).sum()) >= 90 and int(((g > 0.0) & (g < 1.0)).sum()) >= 140, (view, g.size)
            else:
                assert np.all(g < 1.0), view
    # and the two divisors differ: at 200.7 some voxel changes class between them
    if cal == 200.7:
        v = np.arange(256, dtype=F)
        a = [pc.oracle.tf_class(ref.otf[0], ref.otf[1], float(x / F(int(cal)))) for x in v]
        b = [pc.oracle.tf_class(ref.otf[0], ref.otf[1], float(F(float(x) / cal))) for x in v]
        assert a != b
