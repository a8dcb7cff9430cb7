"""VR_MODE_ISO on the GPU (iso_march_kernel): the shaded first-hit isosurface of the trilinear scalar
field, held bit for bit to the numpy restatement tests/iso_ref.py (itself held to the MIP restatement
and to a closed-form surface by tests/test_iso_ref.py).

Every frame is compared bitwise, in all four flag combinations (0, ESS, ERT, ESS | ERT): a skipped
sample is one below the isovalue, and everything after the hit is a function of (x, y, s_h) alone.  The
one tolerance in this file is test_gpu_shade.TOL_EXACT on the two coefficient sets whose specular term
goes through the hardware exp2 / log2 (SH_GEN, SH_SHARP).  Shapes are test_gpu_mip.py's.
"""
import ctypes as C

import numpy as np
import pytest

import iso_ref
import param_cases as pc
import volumerenderingproject_amd as vr
from test_dvr_ref import random_volume, seeded_tf
from test_gpu_dvr import assert_bits, camera_pair
from test_gpu_shade import TOL_EXACT

pytestmark = pytest.mark.gpu

E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
ISO, MIP, DVR = vr.VR_MODE_ISO, vr.VR_MODE_MIP, vr.VR_MODE_DVR
F = np.float32
RGB = (0.9, 0.8, 0.7)
_REFS = {}


def reference(O, key, vol, W, H, S, cam_name, iso, rgb=RGB, shade=pc.SH_KS0, xs=None):
    """The restatement's (frame, record), computed once per (volume, frame, view, surface, shade) and shared."""
    k = (key, W, H, S, cam_name, float(iso), tuple(rgb), tuple(shade), None if xs is None else tuple(xs))
    if k not in _REFS:
        _, ocam = camera_pair(O, cam_name, W, H)
        frame, rec = iso_ref.render(vol, O.params(W, H, S), ocam, iso, rgb, shade, xs=xs)
        frame.setflags(write=False)
        for a in rec.values():
            a.setflags(write=False)
        _REFS[k] = (frame, rec)
    return _REFS[k]


def params(W, H, S, flags=0, shade=pc.SH_KS0):
    p = vr.default_params(W, H, S, mode=ISO, flags=flags)
    p.shade_ambient, p.shade_diffuse, p.shade_specular, p.shade_shininess = shade
    return p


def check_all_flags(r, ref, W, H, S, cam, what, shade=pc.SH_KS0, make=params, tol=None):
    exact = r.render(make(W, H, S, 0, shade), cam)
    if tol is None:
        assert_bits(exact, ref, (what, "exact"))
    else:
        err = float(np.abs(exact - ref).max())
        print(what, "largest deviation", err)
        assert err <= tol, (what, err)
    for fl in (E, T, E | T):
        assert_bits(r.render(make(W, H, S, fl, shade), cam), exact, (what, fl))
    return exact


FRAMES = [(64, 48, 64), (37, 91, 50)]
VIEWS = ["default", "reset", "inside"]


@pytest.mark.parametrize("W,H,S", FRAMES)
def test_bitwise_byte_and_float_paths(avg152, oracle_mod, W, H, S):
    vol, cal = avg152
    with vr.VolumeRenderer(vol, cal, device=0) as a, \
            vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for r in (a, b):
            r.set_isosurface(100.0, RGB)
        for name in VIEWS:
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref, rec = reference(oracle_mod, "avg", vol, W, H, S, name, 100.0)
            hit = rec["hit"]
            if name == "inside":
                assert hit.any()
            else:   # the case is not vacuous (from the restatement's record)
                from mip_ref import sample_values
                _, inside = sample_values(vol, oracle_mod.params(W, H, S), camera_pair(oracle_mod, name, W, H)[1])
                assert hit.sum() >= 200 and rec["refinable"].sum() >= 200, name
                assert (inside.any(axis=2) & ~hit).sum() >= 40, name
                assert len(np.unique(ref[hit][:, 0])) > 150, name
                if name == "reset":
                    assert (hit & ~rec["refinable"]).sum() >= 10
                    assert (hit & (~rec["has_normal"] | (rec["d"] == 0))).sum() >= 5
            fa = check_all_flags(a, ref, W, H, S, cam, ("byte", name))
            fb = check_all_flags(b, ref, W, H, S, cam, ("float", name))
            assert_bits(fa, fb, name)
        assert a.info.device_bytes - b.info.device_bytes == vol.size + 64   # (the byte copy was taken)


@pytest.mark.parametrize("iso", [-1.0, 0.0, 40.0, 100.3, 127.5, 255.0, 256.0])
def test_isovalue_sweep(avg152, oracle_mod, iso):
    vol, cal = avg152
    W, H, S = 64, 48, 64
    ref, rec = reference(oracle_mod, "avg", vol, W, H, S, "reset", iso)
    bg = np.array(list(vr.default_params(W, H, S).background), F)[:3]
    if iso == -1.0:   # every first in-volume sample hits: on the faces, never refined
        from mip_ref import sample_values
        _, inside = sample_values(vol, oracle_mod.params(W, H, S), camera_pair(oracle_mod, "reset", W, H)[1])
        assert np.array_equal(rec["hit"], inside.any(axis=2)) and rec["hit"].sum() >= 200
        assert np.array_equal(rec["s_h"][rec["hit"]], inside.argmax(axis=2)[rec["hit"]])
        assert not rec["refinable"].any()
    if iso == 256.0:
        assert not rec["hit"].any() and np.all(ref[..., :3] == bg)
    with vr.VolumeRenderer(vol, cal, device=0) as a, \
            vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for r in (a, b):
            r.set_isosurface(iso, RGB)
            check_all_flags(r, ref, W, H, S, vr.reset_camera(), iso)


@pytest.mark.parametrize("W,H,S", FRAMES)
def test_fractional_volume_takes_float_path(avg152, oracle_mod, W, H, S):
    vol, cal = avg152
    frac = (vol + np.random.default_rng(3).random(vol.shape, dtype=F)).astype(F)
    with vr.VolumeRenderer(frac, cal, device=0) as a, \
            vr.VolumeRenderer(frac, cal, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for r in (a, b):
            r.set_isosurface(100.0, RGB)
        for name in VIEWS:
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref, rec = reference(oracle_mod, "frac", frac, W, H, S, name, 100.0)
            assert rec["hit"].any(), name
            fa = check_all_flags(a, ref, W, H, S, cam, ("auto", name))
            assert_bits(fa, b.render(params(W, H, S), cam), name)
        assert a.info.device_bytes == b.info.device_bytes   # no byte copy kept: both read the float volume


def test_edge_clamp_cube_filling_volume(oracle_mod):
    """The volume filled to every face: hits and gradient taps in the last voxel layer of every axis."""
    vol = random_volume()
    W, H, S = 90, 70, 160
    with vr.VolumeRenderer(vol, 255.0, device=0) as a, \
            vr.VolumeRenderer(vol, 255.0, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for r in (a, b):
            r.set_isosurface(128.0, RGB)
        for name in ("reset", "default", "x", "-y"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref, rec = reference(oracle_mod, "cube", vol, W, H, S, name, 128.0)
            assert rec["hit"].any(), name
            for r in (a, b):
                check_all_flags(r, ref, W, H, S, cam, name)


TINY_SHAPES = [(1, 1, 1), (1, 9, 4), (7, 1, 2), (3, 3, 1), (9, 8, 7), (65, 3, 2)]


@pytest.mark.parametrize("shape", TINY_SHAPES)
def test_tiny_volumes(shape):
    """d_a = 1 (the gradient's span is 0 on that axis) and cells larger than the volume."""
    vol = pc.tiny_volume(shape)
    iso = float(np.median(vol))
    W, H, S = 24, 16, 12
    hits = 0
    with vr.VolumeRenderer(vol, 255.0, device=0) as r:
        r.set_isosurface(iso, RGB)
        for view in ("z", "x", "obl"):
            case = pc.Case(view, ISO, rsw=pc.TINY[shape], frame=(W, H, S))
            ref, rec = iso_ref.render(vol, case.oracle_params(), case.oracle_camera(), iso, RGB, pc.SH_KS0)
            hits += int(rec["hit"].sum())

            def make(W_, H_, S_, fl, shade, case=case):
                p = case.gpu_params(flags=fl)
                p.shade_ambient, p.shade_diffuse, p.shade_specular, p.shade_shininess = shade
                return p
            check_all_flags(r, ref, W, H, S, case.gpu_camera(), (shape, view), make=make)
    assert hits > 0, shape


@pytest.mark.parametrize("S", [4088, 4089, 9000])
def test_long_rays(avg152, oracle_mod, S):
    """S = 4088 is the last frame with the B table in LDS, 4089 the first without it, 9000 TEST's long-ray
    size; the refinement's fractional positions are computed beside both."""
    vol, cal = avg152
    W, H = 20, 14
    with vr.VolumeRenderer(vol, cal, device=0) as a, \
            vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for r in (a, b):
            r.set_isosurface(100.0, RGB)
        for name in ("reset", "default"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref, rec = reference(oracle_mod, "avg", vol, W, H, S, name, 100.0)
            assert rec["refinable"].sum() >= 40, name
            check_all_flags(a, ref, W, H, S, cam, ("byte", S, name))
            check_all_flags(b, ref, W, H, S, cam, ("float", S, name))


@pytest.mark.parametrize("kind", ["negative", "nonfinite"])
def test_negative_and_non_finite_voxels(oracle_mod, kind):
    rng = np.random.default_rng(9)
    vol = rng.random((24, 24, 24), dtype=F) * F(7.0)
    if kind == "negative":
        vol = -(vol + F(0.25))
    else:
        bad = rng.random(vol.shape) < 0.15
        vol[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(bad.sum()))
    W, H, S = 32, 24, 16
    iso = -3.0 if kind == "negative" else 3.0
    with vr.VolumeRenderer(vol, 5.0, device=0) as r:
        r.set_isosurface(iso, RGB)
        for name in ("default", "reset"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref, rec = reference(oracle_mod, kind, vol, W, H, S, name, iso)
            assert rec["hit"].any() and np.all(np.isfinite(ref)), name
            check_all_flags(r, ref, W, H, S, cam, (kind, name))


@pytest.mark.parametrize("W,H,S", [(1, 1, 1), (1, 130, 2), (257, 3, 1)])
def test_degenerate_frames(avg152, oracle_mod, W, H, S):
    """S = 1 has no light direction: d = 1 on every hit."""
    vol, cal = avg152
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        r.set_isosurface(0.0, RGB)
        for name in ("default", "reset"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref, rec = reference(oracle_mod, "avg", vol, W, H, S, name, 0.0)
            if S == 1:
                assert np.all(rec["d"] == 1.0)
            check_all_flags(r, ref, W, H, S, cam, name)


def test_margin_case(oracle_mod):
    """MIP's block of float32(0.1) with iso one ulp above it: an unfused lerp of equal corners can land
    there, and a cell bound without its margin (max = 0.1 < iso) would skip those cells."""
    vol = np.zeros((24, 24, 24), F)
    vol[4:20, 4:20, 4:20] = F(0.1)
    W, H, S = 32, 32, 64
    iso = float(np.nextafter(F(0.1), F(np.inf)))
    ref, rec = reference(oracle_mod, "margin", vol, W, H, S, "reset", iso)
    assert int(rec["hit"].sum()) >= 100   # the case bites
    with vr.VolumeRenderer(vol, 1.0, device=0) as r:
        r.set_isosurface(iso, RGB)
        assert r.isosurface[0] == F(iso)
        check_all_flags(r, ref, W, H, S, vr.reset_camera(), "margin")


@pytest.mark.parametrize("name", list(pc.SHADE_SETS))
def test_shading_coefficients(avg152, oracle_mod, name):
    vol, cal = avg152
    W, H, S = 64, 48, 64
    shade = pc.SHADE_SETS[name]
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        r.set_isosurface(100.0, RGB)
        for view in ("default", "reset"):
            cam, _ = camera_pair(oracle_mod, view, W, H)
            ref, rec = reference(oracle_mod, "avg", vol, W, H, S, view, 100.0, shade=shade)
            tol = None if name in pc.SHADE_BITWISE else TOL_EXACT
            got = check_all_flags(r, ref, W, H, S, cam, (name, view), shade=shade, tol=tol)
            if name == "id":
                assert np.all(got[rec["hit"]][:, :3] == np.array(RGB, F))


def test_live_state(avg152, oracle_mod):
    import torch
    vol, cal = avg152
    W, H, S = 64, 48, 64
    cam = vr.reset_camera()
    surf = [(100.0, RGB), (40.0, (0.2, 1.0, 0.5))]
    refs = [reference(oracle_mod, "avg", vol, W, H, S, "reset", i, rgb=c)[0] for i, c in surf]
    p, pm = params(W, H, S, E | T), vr.default_params(W, H, S, mode=MIP, flags=E)
    with vr.VolumeRenderer(vol, cal, device=0) as r, vr.VolumeRenderer(vol, cal, device=0) as fresh_mip:
        iso0, rgb0 = r.isosurface
        assert iso0 == F(0.5 * cal) and rgb0 == (1.0, 1.0, 1.0)
        mip_fresh = fresh_mip.render(pm, cam)
        r.set_isosurface(*surf[0])
        assert r.isosurface == (F(surf[0][0]), tuple(float(F(c)) for c in surf[0][1]))
        assert_bits(r.render(p, cam), refs[0], "first")
        before = r.info.device_bytes
        r.set_isosurface(*surf[1])
        assert r.isosurface[0] == F(40.0)
        assert_bits(r.render(p, cam), refs[1], "second surface")
        assert r.info.device_bytes == before
        # MIP after ISO is MIP on a fresh context, and builds nothing more
        assert_bits(r.render(pm, cam), mip_fresh, "mip after iso")
        assert r.info.device_bytes == before
        # ISO after MIP equals ISO on a fresh context
        mip_bytes = fresh_mip.info.device_bytes
        fresh_mip.set_isosurface(*surf[1])
        assert_bits(fresh_mip.render(p, cam), refs[1], "iso after mip")
        assert fresh_mip.info.device_bytes == mip_bytes   # (the bounds were there already)
        # the TF plays no part, an opaque TF(0) included
        opaque0 = [(0.0, 1.0, (0.1, 0.2, 0.3, 0.05)), (0.3, 0.6, (0.9, 0.5, 0.1, 0.4))]
        for tf in (seeded_tf(17, 17), opaque0):
            r.set_transfer_function(tf)
            now = r.info.device_bytes
            assert_bits(r.render(p, cam), refs[1], "tf")
            assert_bits(r.render(params(W, H, S, 0), cam), refs[1], "tf exact")
            assert r.info.device_bytes == now
        # a DVR frame in between does not disturb ISO
        r.render(vr.default_params(W, H, S, mode=DVR, flags=E), cam)
        assert_bits(r.render(p, cam), refs[1], "after dvr")
        # two queued frames with a set_isosurface between them
        t = torch.empty((2, W, H, 4), dtype=torch.float32, device="cuda:0")
        r.set_isosurface(*surf[0])
        r.render_device(p, cam, t[0].data_ptr(), asynchronous=True)
        r.set_isosurface(*surf[1])
        r.render_device(p, cam, t[1].data_ptr(), asynchronous=True)
        r.synchronize()
        got = t.cpu().numpy()
        assert_bits(got[0], refs[0], "async 0")
        assert_bits(got[1], refs[1], "async 1")


def test_tiles_group_and_batch(avg152, oracle_mod, tmp_path):
    import torch
    vol, cal = avg152
    W, H, S = 200, 150, 70
    p = params(W, H, S, E | T)
    names = ("default", "reset", "inside")
    cams = [camera_pair(oracle_mod, n, W, H)[0] for n in names]
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        r.set_isosurface(100.0, RGB)
        frames = [r.render(p, c) for c in cams]
        for f, n in enumerate(names):
            assert_bits(frames[f], reference(oracle_mod, "avg", vol, W, H, S, n, 100.0)[0], n)
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
        # a tile list: the visible tiles of the view, each block equal to the frame
        ids = [int(t) for t in r.visible_tiles(p, cams[1], 64, 64)]
        assert 0 < len(ids) <= ((W + 63) // 64) * nty
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
        for f, c in enumerate(cams):
            assert_bits(batch[f], frames[f], ("batch", f))
        # the headless saveImage of an ISO frame
        png = tmp_path / "iso.png"
        assert vr.lib().vr_render_png(r._ctx, C.byref(p), C.byref(cams[1]), 2, str(png).encode()) == 0
        assert png.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    # a two-part group on one GPU farms the tiles and assembles the same frame: the setter reached both parts
    with vr.VolumeRenderer(vol, cal, devices=[0, 0]) as g:
        g.set_isosurface(100.0, RGB)
        for f, c in enumerate(cams):
            assert_bits(g.render(p, c), frames[f], ("group", f))


def test_refusals(avg152):
    vol, cal = avg152
    W, H, S = 32, 24, 16
    cam = vr.default_camera(W, H)
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        for fl in (vr.VR_FLAG_SHADE, vr.VR_FLAG_CONIC):
            with pytest.raises(vr.VRError) as e:
                r.render(params(W, H, S, fl), cam)
            assert e.value.code == -1
        p = params(W, H, S)
        for call in (r.count_samples, r.count_marched, r.count_work):
            with pytest.raises(vr.VRError) as e:
                call(p, cam)
            assert e.value.code == -1
        assert r.axis_columns_plan(p, cam)["columns"] is False
        for bad in (float("nan"), float("inf")):
            with pytest.raises(vr.VRError) as e:
                r.set_isosurface(bad)
            assert e.value.code == -1
        with pytest.raises(vr.VRError) as e:
            r.set_isosurface(1.0, (0.5, float("nan"), 0.5))
        assert e.value.code == -1
        assert vr.lib().vr_set_isosurface(r._ctx, 1.0, None) == -1   # a null colour
        assert r.isosurface == (F(0.5 * cal), (1.0, 1.0, 1.0))       # (a refused call changed nothing)
        assert r.render(p, cam).shape == (W, H, 4)                   # (the context still renders)
    with vr.VolumeRenderer(vol, -1.0, device=0) as r:   # the mode needs a positive cal_max
        with pytest.raises(vr.VRError) as e:
            r.render(params(W, H, S), cam)
        assert e.value.code == -1


def test_midsize_mni(mni_standin, oracle_mod):
    """MNI stand-in (182 x 218 x 182) at 480 x 270 x 500, on the device: the four flag combinations
    equal, alpha 1; five seeded columns bitwise against the restatement."""
    import torch
    vol, cal = mni_standin
    W, H, S = 480, 270, 500
    iso = float(F(0.5 * cal))
    xs = sorted(int(x) for x in np.random.default_rng(5).choice(W, 5, replace=False))
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        r.set_isosurface(iso, RGB)
        for name in ("default", "reset"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            out = {}
            for fl in (0, E, T, E | T):
                t = torch.empty((W, H, 4), dtype=torch.float32, device="cuda:0")
                r.render_device(params(W, H, S, fl), cam, t.data_ptr())
                out[fl] = t
            for fl in (E, T, E | T):
                assert torch.equal(out[fl], out[0]), (name, fl)
            assert torch.all(out[0][..., 3] == 1.0)
            ref, rec = reference(oracle_mod, "mni", vol, W, H, S, name, iso, xs=xs)
            assert rec["hit"].any(), name
            assert_bits(out[0][xs].cpu().numpy(), ref, name)
