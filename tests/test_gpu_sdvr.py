"""VR_MODE_SDVR on the GPU (dvr_march_kernel, SHADE): VR_MODE_DVR with every non-transparent in-volume sample
lit by the gradient of the trilinear field, held to the numpy restatement tests/sdvr_ref.py (itself held
to the DVR and ISO restatements and to a closed form by tests/test_sdvr_ref.py, which also shows that the
cases of tests/sdvr_cases.py bite).

Rule of comparison, as tests/test_gpu_shade.py and tests/test_gpu_iso.py state it: exact and ESS frames
are bitwise the restatement's for the coefficient sets of param_cases.SHADE_BITWISE, and within
test_gpu_shade.TOL_EXACT for the two whose specular term goes through the hardware exp2 / log2 (SH_GEN,
SH_SHARP; the largest deviation is printed); ESS equals exact bit for bit, always; ERT and ESS | ERT are
within test_gpu_shade.TOL_ERT of the exact frame, with frame alpha 1.
"""
import ctypes as C

import numpy as np
import pytest

import param_cases as pc
import sdvr_cases as sc
import volumerenderingproject_amd as vr
from test_gpu_dvr import assert_bits
from test_gpu_shade import TOL_ERT, TOL_EXACT

pytestmark = pytest.mark.gpu

E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
SDVR, DVR = vr.VR_MODE_SDVR, vr.VR_MODE_DVR
F = np.float32


def check_all_flags(r, case, what=None, bitwise=None):
    """One case on one context in the four flag combinations, by the rule above.  Returns the exact frame."""
    what = what or (case.vol, case.tf, getattr(case.view, "view", case.view), case.shade)
    ref = sc.reference(case)[0]
    cam = case.gpu_camera()
    exact = r.render(case.gpu_params(0), cam)
    if bitwise is None:
        bitwise = case.shade in [pc.SHADE_SETS[n] for n in pc.SHADE_BITWISE]
    if bitwise:
        assert_bits(exact, ref, (what, "exact"))
    else:
        err = float(np.abs(exact - ref).max())
        print(what, "largest deviation", err)
        assert err <= TOL_EXACT, (what, err)
    assert_bits(r.render(case.gpu_params(E), cam), exact, (what, "ess"))
    for fl in (T, E | T):
        fast = r.render(case.gpu_params(fl), cam)
        err = float(np.abs(fast - exact).max())
        assert err <= TOL_ERT, (what, fl, err)
        assert np.all(fast[..., 3] == 1.0)
    return exact


def contexts(vol, cal, **kw):
    """The byte-copy context and the float-volume one."""
    return (vr.VolumeRenderer(vol, cal, device=0, **kw),
            vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1), **kw))


@pytest.mark.parametrize("W,H,S", sc.FRAMES)
def test_byte_and_float_paths(W, H, S):
    vol, cal = sc.volume("avg152")
    a, b = contexts(vol, cal)
    with a, b:
        for base in sc.paths_cases(W, H, S):
            for name, shade in pc.SHADE_SETS.items():
                case = base.with_shade(shade)
                fa = check_all_flags(a, case, ("byte", base.view, name))
                fb = check_all_flags(b, case, ("float", base.view, name))
                assert_bits(fa, fb, (base.view, name))
        assert a.info.device_bytes - b.info.device_bytes == vol.size + 64   # (the byte copy was taken)


@pytest.mark.parametrize("W,H,S", sc.FRAMES)
def test_fractional_volume_takes_float_path(W, H, S):
    vol, cal = sc.volume("frac")
    a, b = contexts(vol, cal)
    with a, b:
        for base in sc.paths_cases(W, H, S, vol="frac"):
            for name in ("n0", "gen"):
                case = base.with_shade(pc.SHADE_SETS[name])
                fa = check_all_flags(a, case, ("auto", base.view, name))
                assert_bits(fa, b.render(case.gpu_params(0), case.gpu_camera()), (base.view, name))
        assert a.info.device_bytes == b.info.device_bytes   # no byte copy kept: both read the float volume


@pytest.mark.parametrize("volume", ["random", "cube"])
def test_faces(volume):
    """Data up to every face of the volume: the one-sided spans of the gradient and the clamped corner reads
    of the taps in the last voxel layer of every axis."""
    vol, cal = sc.volume(volume)
    a, b = contexts(vol, cal)
    with a, b:
        for base in sc.face_cases():
            if base.vol != volume:
                continue
            for name in ("ks0", "n0"):
                case = base.with_shade(pc.SHADE_SETS[name])
                for r in (a, b):
                    check_all_flags(r, case)


@pytest.mark.parametrize("volume", ["special", "small", "subnormal"])
def test_special_values(volume):
    """NaN and +-inf voxels read as 0 in the taps too (under a TF whose class of 0 is visible); gradients whose
    len2 is a subnormal or underflows (blob_small); subnormal voxels (blob_subnormal: no normal anywhere)."""
    vol, cal = sc.volume(volume)
    for base in sc.special_cases():
        if base.vol != volume:
            continue
        a, b = contexts(vol, cal, tf=sc.tf_of(base.tf))
        with a, b:
            for name in ("ks0", "n0"):
                case = base.with_shade(pc.SHADE_SETS[name])
                ref = sc.reference(case)[0]
                assert np.all(np.isfinite(ref))
                for r in (a, b):
                    check_all_flags(r, case)


@pytest.mark.parametrize("shape", sc.TINY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tiny_volumes(shape):
    """d_a = 1 (the gradient's span is 0 on that axis), cells larger than the volume; (1, 1, 1) has no normal
    at all and SH_N0 shows it as c * 0.7."""
    vol, cal = sc.volume(shape)
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        for case in sc.tiny_cases(shape):
            assert case.shade == pc.SH_N0
            check_all_flags(r, case)


def test_tf_paths():
    """17 seeded intervals (the LDS search, not SEG8); an opaque TF(0) (no clip, no skipping, the out-of-volume
    samples visible and unshaded); a TF set on a live context against a fresh one."""
    vol, cal = sc.volume("avg152")
    with vr.VolumeRenderer(vol, cal, device=0) as live:
        for tf in ("seeded17", "opaque0"):
            live.set_transfer_function(sc.tf_of(tf))
            if tf == "seeded17":
                assert len(vr.tf_segments(sc.tf_of(tf), cal)[0]) > 9
            with vr.VolumeRenderer(vol, cal, tf=sc.tf_of(tf), device=0) as fresh:
                for base in sc.tf_cases(tf):
                    for name in ("ks0", "gen"):
                        case = base.with_shade(pc.SHADE_SETS[name])
                        got = check_all_flags(fresh, case)
                        cam = case.gpu_camera()
                        assert_bits(live.render(case.gpu_params(0), cam), got, (tf, base.view, name, "live"))
                        assert_bits(live.render(case.gpu_params(E), cam), got, (tf, base.view, name, "live ess"))


def test_long_ray():
    """20 x 14 x 4089, the first S without the B table in LDS (every position computed per sample), from the
    byte copy and from the float volume: exact is bitwise, ESS equals exact, and ERT is held to
    test_gpu_params.ert_bound over the operative samples, with the TF's colours replaced by the largest a
    shaded sample can take, c * (ka + kd) + ks.  Measured on the MI355X, largest ERT error over both contexts
    and both ERT flag combinations: 7.3e-6 (red; S_op = 999, the bound's tightest channel 3.5e-4) -- under the
    project's 1e-4 the way DVR's 6.9e-6 is, so TOL_ERT is asserted as well."""
    from test_gpu_params import ert_bound
    case = sc.long_case()
    assert (case.W, case.H, case.S) == (20, 14, 4089) and case.shade == pc.SH_N0
    vol, cal = sc.volume("avg152")
    ref, rec = sc.reference(case)
    ka, kd, ks, _ = case.shade
    tf_max = [(lo, hi, tuple(c * (ka + kd) + ks for c in rgba[:3]) + (rgba[3],)) for lo, hi, rgba in sc.tf_of(case.tf)]
    import dvr_ref
    col = dvr_ref.sample_colors(vol, cal, sc.tf_of(case.tf), case.oracle_params(), case.oracle_camera())
    s_op = int((col[..., 3] != 0.0).sum(axis=2).max())
    assert 0 < s_op <= case.S
    bound = ert_bound(tf_max, (0.2, 0.2, 0.2), 1e-5, s_op)
    cam = case.gpu_camera()
    worst = 0.0
    a, b = contexts(vol, cal)
    with a, b:
        for r in (a, b):
            exact = r.render(case.gpu_params(0), cam)
            assert_bits(exact, ref, "exact")
            assert_bits(r.render(case.gpu_params(E), cam), exact, "ess")
            for fl in (T, E | T):
                fast = r.render(case.gpu_params(fl), cam)
                err = np.abs(fast[..., :3].astype(np.float64) - ref[..., :3]).max(axis=(0, 1))
                worst = max(worst, float(err.max()))
                print("long ray flags", fl, "ERT error per channel", err, "bound", bound, "S_op", s_op)
                assert np.all(err <= bound), (fl, s_op, err, bound)
                assert np.all(fast[..., 3] == 1.0)
                assert err.max() <= TOL_ERT, (fl, err)
    print("long ray largest ERT error", worst)


def test_identity_is_dvr():
    """With (1, 0, 0, n) the exact and ESS frames are bitwise the same context's VR_MODE_DVR frames."""
    vol, cal = sc.volume("avg152")
    a, b = contexts(vol, cal)
    with a, b:
        for base in sc.paths_cases(*sc.FRAMES[0]):
            case = base.with_shade(pc.SH_ID)
            cam = case.gpu_camera()
            for r in (a, b):
                for fl in (0, E):
                    dvr = r.render(case.gpu_params(fl, mode=DVR), cam)
                    assert_bits(r.render(case.gpu_params(fl), cam), dvr, (base.view, fl))
                other = r.render(base.with_shade(pc.SH_N0).gpu_params(0), cam)
                assert np.any(other != dvr)   # (the coefficients are read)


def test_tiles_group_and_batch(tmp_path):
    import torch
    vol, cal = sc.volume("avg152")
    cases = sc.plumbing_cases()
    W, H, S = sc.PLUMB_FRAME
    p = cases[0].gpu_params(E | T)
    cams = [c.gpu_camera() for c in cases]
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        frames = [r.render(p, c) for c in cams]
        exact = r.render(cases[1].gpu_params(0), cams[1])
        assert_bits(exact, sc.reference(cases[1])[0], "reset exact")
        assert np.abs(frames[1] - exact).max() <= TOL_ERT
        # tile buffers (farming): blocks equal the frame
        tiles = torch.zeros((8, 64 * 64, 3), dtype=torch.float32, device="cuda:0")
        n = r.render_tiles(p, cams[1], 64, 64, 3, 5, tiles.data_ptr(), rgb=True)
        nty = (H + 63) // 64
        got = tiles.cpu().numpy()
        assert n == 2
        for k in range(n):
            tx, ty = divmod(3 + 5 * k, nty)
            blk = got[k].reshape(64, 64, 3)
            x1, y1 = min(W, tx * 64 + 64), min(H, ty * 64 + 64)
            assert np.array_equal(blk[:x1 - tx * 64, :y1 - ty * 64], frames[1][tx * 64:x1, ty * 64:y1, :3])
        # a tile list: the visible tiles of the view (DVR's cull), each block equal to the frame
        ids = [int(t) for t in r.visible_tiles(p, cams[1], 64, 64)]
        pd = cases[1].gpu_params(E | T, mode=DVR)
        assert ids == [int(t) for t in r.visible_tiles(pd, cams[1], 64, 64)] and 0 < len(ids)
        tl = torch.zeros((len(ids), 64 * 64, 3), dtype=torch.float32, device="cuda:0")
        assert r.render_tile_list(p, cams[1], 64, 64, ids, 0, 1, tl.data_ptr(), rgb=True) == len(ids)
        got = tl.cpu().numpy()
        culled = np.ones((W, H), bool)
        for k, t in enumerate(ids):
            tx, ty = divmod(t, nty)
            blk = got[k].reshape(64, 64, 3)
            x1, y1 = min(W, tx * 64 + 64), min(H, ty * 64 + 64)
            assert np.array_equal(blk[:x1 - tx * 64, :y1 - ty * 64], frames[1][tx * 64:x1, ty * 64:y1, :3])
            culled[tx * 64:x1, ty * 64:y1] = False
        assert np.all(frames[1][culled][:, :3] == np.array(list(p.background), F)[:3])   # (the cull is valid)
        # a batch of three cameras equals three renders
        batch = r.render_batch(p, cams)
        for f in range(len(cams)):
            assert_bits(batch[f], frames[f], ("batch", f))
        # the headless saveImage of an SDVR frame
        png = tmp_path / "sdvr.png"
        assert vr.lib().vr_render_png(r._ctx, C.byref(p), C.byref(cams[1]), 2, str(png).encode()) == 0
        assert png.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    # a two-part group on one GPU farms the tiles and assembles the same frame
    with vr.VolumeRenderer(vol, cal, devices=[0, 0]) as g:
        for f, c in enumerate(cams):
            assert_bits(g.render(p, c), frames[f], ("group", f))


@pytest.mark.parametrize("frames_in_flight", [0, 3])
def test_first_call_is_a_batch(frames_in_flight):
    """The mode builds DVR's lazy state (ensure_dvr) with its first frame; a context whose first call is a
    batch gives the frames of single renders on another context, bit for bit."""
    vol, cal = sc.volume("avg152")
    cases = sc.paths_cases(*sc.FRAMES[0])
    p = cases[0].gpu_params(E)
    cams = [c.gpu_camera() for c in cases]
    for dvr_volume in (0, 1):
        with vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=dvr_volume)) as single:
            want = [single.render(p, c) for c in cams]
        for f, case in enumerate(cases):
            assert_bits(want[f], sc.reference(case)[0], ("single", f))
        opts = vr.default_options(dvr_volume=dvr_volume, frames_in_flight=frames_in_flight)
        with vr.VolumeRenderer(vol, cal, device=0, options=opts) as r:
            batch = r.render_batch(p, cams)   # the context's first call
            for f in range(len(cams)):
                assert_bits(batch[f], want[f], (dvr_volume, "first batch", f))


def test_state():
    """One context through DVR, SDVR, a TF change, SDVR, DVR, with new coefficients between frames and no
    other call: each frame is a fresh context's.  SDVR builds nothing of its own (device_bytes), in either
    order, and vr_set_isosurface changes no SDVR frame."""
    vol, cal = sc.volume("avg152")
    base = sc.paths_cases(*sc.FRAMES[0])[1]   # reset
    cam = base.gpu_camera()
    tf2 = "seeded17"
    c0, c1 = base.with_shade(pc.SH_N0), base.with_shade(pc.SH_KS0)
    c2 = sc.tf_cases(tf2)[1].with_shade(pc.SH_N0)
    assert c2.view == base.view

    def fresh(tf, params):
        with vr.VolumeRenderer(vol, cal, tf=sc.tf_of(tf), device=0) as f:
            return f.render(params, cam)

    with vr.VolumeRenderer(vol, cal, device=0) as r, vr.VolumeRenderer(vol, cal, device=0) as other:
        pd = base.gpu_params(E, mode=DVR)
        assert_bits(r.render(pd, cam), fresh("default", pd), "dvr first")
        dvr_bytes = r.info.device_bytes
        assert_bits(r.render(c0.gpu_params(0), cam), sc.reference(c0)[0], "sdvr after dvr")
        assert r.info.device_bytes == dvr_bytes                      # nothing of its own
        assert_bits(r.render(c1.gpu_params(E), cam), sc.reference(c1)[0], "new coefficients")
        r.set_isosurface(40.0, (0.2, 1.0, 0.5))
        assert_bits(r.render(c1.gpu_params(E), cam), sc.reference(c1)[0], "after set_isosurface")
        r.set_transfer_function(sc.tf_of(tf2))
        assert_bits(r.render(c2.gpu_params(0), cam), sc.reference(c2)[0], "after the TF change")
        assert_bits(r.render(c2.gpu_params(E), cam), sc.reference(c2)[0], "after the TF change, ess")
        assert_bits(r.render(pd, cam), fresh(tf2, pd), "dvr last")
        # the other way round: SDVR first, then DVR grows nothing
        assert_bits(other.render(c0.gpu_params(E), cam), sc.reference(c0)[0], "sdvr first")
        assert other.info.device_bytes == dvr_bytes
        assert_bits(other.render(pd, cam), fresh("default", pd), "dvr after sdvr")
        assert other.info.device_bytes == dvr_bytes


def test_refusals():
    vol, cal = sc.volume("avg152")
    W, H, S = 32, 24, 16
    cam = vr.default_camera(W, H)
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        for fl in (vr.VR_FLAG_SHADE, vr.VR_FLAG_CONIC):
            with pytest.raises(vr.VRError) as e:
                r.render(vr.default_params(W, H, S, mode=SDVR, flags=fl), cam)
            assert e.value.code == -1
        p = vr.default_params(W, H, S, mode=SDVR)
        for call in (r.count_samples, r.count_marched, r.count_work):
            with pytest.raises(vr.VRError) as e:
                call(p, cam)
            assert e.value.code == -1
        assert r.axis_columns_plan(p, cam)["columns"] is False
        assert r.render(p, cam).shape == (W, H, 4)   # (the context still renders)
    with vr.VolumeRenderer(vol, -1.0, device=0) as r:   # the mode needs a positive cal_max
        with pytest.raises(vr.VRError) as e:
            r.render(vr.default_params(W, H, S, mode=SDVR), cam)
        assert e.value.code == -1
