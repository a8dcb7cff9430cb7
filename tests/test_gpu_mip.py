"""VR_MODE_MIP on the GPU (mip_march_kernel): the maximum of the trilinear scalar field over a ray's
in-volume samples, held bit for bit to the numpy restatement tests/mip_ref.py (itself pinned to the DVR
restatement by tests/test_mip_ref.py).

Every frame is compared bitwise, in all four flag combinations (0, ESS, ERT, ESS | ERT): the maximum
is order-free and a skipped sample is one that could not have replaced it, so there is no tolerance
anywhere in this file.  Shapes are test_gpu_dvr.py's: the smallest with W != H, S not a multiple of
the batch of 4 and volume dims that are unequal and no multiple of the 8-voxel cell.
"""
import numpy as np
import pytest

import mip_ref
import volumerenderingproject_amd as vr
from test_dvr_ref import random_volume, seeded_tf
from test_gpu_dvr import assert_bits, camera_pair

pytestmark = pytest.mark.gpu

E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
MIP = vr.VR_MODE_MIP
F = np.float32
_REFS = {}


def reference(O, key, vol, cal, W, H, S, cam_name, xs=None):
    """The restatement's (frame, m, any), computed once per (volume, frame, view) and shared."""
    k = (key, W, H, S, cam_name, None if xs is None else tuple(xs))
    if k not in _REFS:
        _, ocam = camera_pair(O, cam_name, W, H)
        _REFS[k] = mip_ref.render(vol, cal, O.params(W, H, S), ocam, xs=xs)
        for a in _REFS[k]:
            a.setflags(write=False)
    return _REFS[k]


def check_all_flags(r, ref, W, H, S, cam, what):
    exact = r.render(vr.default_params(W, H, S, mode=MIP), cam)
    assert_bits(exact, ref, (what, "exact"))
    for fl in (E, T, E | T):
        assert_bits(r.render(vr.default_params(W, H, S, mode=MIP, flags=fl), cam), exact, (what, fl))
    return exact


FRAMES = [(64, 48, 64), (37, 91, 50)]
VIEWS = ["default", "reset", "inside"]


@pytest.mark.parametrize("W,H,S", FRAMES)
def test_bitwise_byte_and_float_paths(avg152, oracle_mod, W, H, S):
    vol, cal = avg152
    with vr.VolumeRenderer(vol, cal, device=0) as a, \
            vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for name in VIEWS:
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref, m, hit = reference(oracle_mod, "avg", vol, cal, W, H, S, name)
            fa = check_all_flags(a, ref, W, H, S, cam, ("byte", name))
            fb = check_all_flags(b, ref, W, H, S, cam, ("float", name))
            assert_bits(fa, fb, name)
            assert not np.all(ref[..., :3] == ref[0, 0, :3]), name   # (the view draws something)
            assert hit.any() and len(np.unique(m[hit])) > 50, name   # (and many different maxima)
        # the automatic choice took the byte copy (avg152 holds integers 0..255): n + 64 bytes more
        assert a.info.device_bytes - b.info.device_bytes == vol.size + 64


@pytest.mark.parametrize("W,H,S", FRAMES)
def test_fractional_volume_takes_float_path(avg152, oracle_mod, W, H, S):
    vol, cal = avg152
    frac = (vol + np.random.default_rng(3).random(vol.shape, dtype=F)).astype(F)
    with vr.VolumeRenderer(frac, cal, device=0) as a, \
            vr.VolumeRenderer(frac, cal, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for name in VIEWS:
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref, _, _ = reference(oracle_mod, "frac", frac, cal, W, H, S, name)
            fa = check_all_flags(a, ref, W, H, S, cam, ("auto", name))
            assert_bits(fa, b.render(vr.default_params(W, H, S, mode=MIP), cam), name)
        assert a.info.device_bytes == b.info.device_bytes   # no byte copy kept: both read the float volume


def test_margin_case(oracle_mod):
    """A block of float32(0.1): an unfused lerp of equal corners can land one ulp above 0.1, and on many
    rays such a sample follows one equal to 0.1 -- a cell bound without its margin (max = 0.1 <= m) skips
    it and fails ESS == exact."""
    vol = np.zeros((24, 24, 24), F)
    vol[4:20, 4:20, 4:20] = F(0.1)
    W, H, S = 32, 32, 64
    ref, m, hit = reference(oracle_mod, "margin", vol, 1.0, W, H, S, "reset")
    assert int((m > F(0.1)).sum()) >= 100   # the case bites
    with vr.VolumeRenderer(vol, 1.0, device=0) as r:
        check_all_flags(r, ref, W, H, S, vr.reset_camera(), "margin")


def test_edge_clamp_cube_filling_volume(oracle_mod):
    """The volume filled to every face: samples in the last voxel layer of every axis read their
    clamped neighbour."""
    vol = random_volume()
    W, H, S = 90, 70, 160
    with vr.VolumeRenderer(vol, 255.0, device=0) as a, \
            vr.VolumeRenderer(vol, 255.0, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for name in ("reset", "default", "x", "-y"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref, _, hit = reference(oracle_mod, "cube", vol, 255.0, W, H, S, name)
            assert hit.any(), name
            for r in (a, b):
                check_all_flags(r, ref, W, H, S, cam, name)


@pytest.mark.parametrize("S", [4088, 4089, 9000])
def test_long_rays(avg152, oracle_mod, S):
    """The per-frame B table in LDS is kept while S + 8 <= kMaxTestTab = 4096: S = 4088 is the last frame
    with it, 4089 the first whose positions are all computed per sample (the same expressions), 9000
    TEST's long-ray size.  Adjacent samples are 0.02 voxel apart here, so a cell jump covers hundreds of
    them.  Bitwise in all four flag combinations, from the byte copy and from the float volume."""
    vol, cal = avg152
    W, H = 20, 14
    with vr.VolumeRenderer(vol, cal, device=0) as a, \
            vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for name in ("reset", "default"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref, m, hit = reference(oracle_mod, "avg", vol, cal, W, H, S, name)
            assert hit.sum() >= 80 and len(np.unique(m[hit])) > 50, name   # (135 / 87 and 90 / 64)
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
    with vr.VolumeRenderer(vol, 5.0, device=0) as r:
        for name in ("default", "reset"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref, m, hit = reference(oracle_mod, kind, vol, 5.0, W, H, S, name)
            assert hit.any(), name
            if kind == "negative":   # black where the ray met the volume, the background elsewhere
                assert np.all(m[hit] < 0) and np.all(ref[hit][:, :3] == 0.0)
            check_all_flags(r, ref, W, H, S, cam, (kind, name))


@pytest.mark.parametrize("W,H,S", [(1, 1, 1), (1, 130, 2), (257, 3, 1)])
def test_degenerate_frames(avg152, oracle_mod, W, H, S):
    vol, cal = avg152
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        for name in ("default", "reset"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref, _, _ = reference(oracle_mod, "avg", vol, cal, W, H, S, name)
            check_all_flags(r, ref, W, H, S, cam, name)


def test_transfer_function_plays_no_part(avg152, oracle_mod):
    """A TF set on a live context (17 intervals; an opaque TF(0), under which the other modes give up
    their culls and clip), a DVR frame in between, and contexts created with those TFs that never
    rendered DVR: the same MIP frames, bit for bit."""
    vol, cal = avg152
    W, H, S = 64, 48, 64
    opaque0 = [(0.0, 1.0, (0.1, 0.2, 0.3, 0.05)), (0.3, 0.6, (0.9, 0.5, 0.1, 0.4))]
    views = {n: camera_pair(oracle_mod, n, W, H)[0] for n in ("default", "reset")}
    refs = {n: reference(oracle_mod, "avg", vol, cal, W, H, S, n)[0] for n in views}

    def check(r, what):
        for n, cam in views.items():
            for fl in (0, E | T):
                assert_bits(r.render(vr.default_params(W, H, S, mode=MIP, flags=fl), cam), refs[n], (what, n, fl))

    with vr.VolumeRenderer(vol, cal, device=0) as live:
        check(live, "first")
        for key, tf in (("seeded17", seeded_tf(17, 17)), ("opaque0", opaque0)):
            live.set_transfer_function(tf)
            before = live.info.device_bytes
            check(live, key)
            assert live.info.device_bytes == before   # (a MIP frame builds nothing that follows the TF)
            with vr.VolumeRenderer(vol, cal, tf=tf, device=0) as fresh:
                check(fresh, ("fresh", key))
        dvr_p = vr.default_params(W, H, S, mode=vr.VR_MODE_DVR, flags=E)
        dvr = live.render(dvr_p, views["reset"])
        assert live.info.device_bytes > before    # (DVR's tables came on top)
        check(live, "after dvr")
        # and DVR after MIP (the shared byte copy and cells built by MIP) is DVR without it
        with vr.VolumeRenderer(vol, cal, tf=opaque0, device=0) as fresh:
            assert_bits(dvr, fresh.render(dvr_p, views["reset"]), "dvr after mip")


def test_tiles_group_and_batch(avg152, oracle_mod, tmp_path):
    import ctypes as C
    import torch
    vol, cal = avg152
    W, H, S = 200, 150, 70
    p = vr.default_params(W, H, S, mode=MIP, flags=E | T)
    names = ("default", "reset", "inside")
    cams = [camera_pair(oracle_mod, n, W, H)[0] for n in names]
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        frames = [r.render(p, c) for c in cams]
        for f, n in enumerate(names):
            assert_bits(frames[f], reference(oracle_mod, "avg", vol, cal, W, H, S, n)[0], n)
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
        # the headless saveImage of a MIP frame
        png = tmp_path / "mip.png"
        assert vr.lib().vr_render_png(r._ctx, C.byref(p), C.byref(cams[1]), 2, str(png).encode()) == 0
        assert png.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    # a two-part group on one GPU farms the tiles and assembles the same frame
    with vr.VolumeRenderer(vol, cal, devices=[0, 0]) as g:
        for f, c in enumerate(cams):
            assert_bits(g.render(p, c), frames[f], ("group", f))


def test_refusals(avg152):
    vol, cal = avg152
    W, H, S = 32, 24, 16
    cam = vr.default_camera(W, H)
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        for fl in (vr.VR_FLAG_SHADE, vr.VR_FLAG_CONIC):
            with pytest.raises(vr.VRError) as e:
                r.render(vr.default_params(W, H, S, mode=MIP, flags=fl), cam)
            assert e.value.code == -1
        p = vr.default_params(W, H, S, mode=MIP)
        for call in (r.count_samples, r.count_marched, r.count_work):
            with pytest.raises(vr.VRError) as e:
                call(p, cam)
            assert e.value.code == -1
        assert r.axis_columns_plan(p, cam)["columns"] is False
        assert r.render(p, cam).shape == (W, H, 4)   # (the context still renders)
    with vr.VolumeRenderer(vol, -1.0, device=0) as r:   # the mode needs a positive cal_max
        with pytest.raises(vr.VRError) as e:
            r.render(vr.default_params(W, H, S, mode=MIP), cam)
        assert e.value.code == -1


def test_midsize_mni(mni_standin, oracle_mod):
    """MNI stand-in (182 x 218 x 182) at 480 x 270 x 500, on the device: the four flag combinations
    equal, alpha 1; five seeded columns bitwise against the restatement."""
    import torch
    vol, cal = mni_standin
    W, H, S = 480, 270, 500
    xs = sorted(int(x) for x in np.random.default_rng(5).choice(W, 5, replace=False))
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        for name in ("default", "reset"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            out = {}
            for fl in (0, E, T, E | T):
                t = torch.empty((W, H, 4), dtype=torch.float32, device="cuda:0")
                r.render_device(vr.default_params(W, H, S, mode=MIP, flags=fl), cam, t.data_ptr())
                out[fl] = t
            for fl in (E, T, E | T):
                assert torch.equal(out[fl], out[0]), (name, fl)
            assert torch.all(out[0][..., 3] == 1.0)
            ref, _, hit = reference(oracle_mod, "mni", vol, cal, W, H, S, name, xs=xs)
            assert hit.any(), name
            assert_bits(out[0][xs].cpu().numpy(), ref, name)
