"""VR_MODE_DVR on the GPU (dvr_march_kernel): trilinear sample of the scalar field, then TF
classification, held bit for bit to the numpy restatement tests/dvr_ref.py (itself pinned to the
oracle by tests/test_dvr_ref.py).

Exact (back-to-front) frames are bitwise the restatement's -- from the byte copy of the volume and
from the float volume (vr_options.dvr_volume = 1) alike -- and unchanged by VR_FLAG_ESS; front to back
(VR_FLAG_ERT) is within the project's 1e-4.  Shapes are the smallest with W != H, S not a multiple of
the batch of 4 and volume dims that are unequal and no multiple of the 8-voxel cell.
"""
import numpy as np
import pytest

import dvr_ref
import volumerenderingproject_amd as vr
from test_dvr_ref import random_volume, seeded_tf

pytestmark = pytest.mark.gpu

E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
DVR = vr.VR_MODE_DVR
TOL = 1e-4
F = np.float32
_REFS = {}


def camera_pair(O, name, W, H):
    """(the library's camera, the oracle's) for one of the named views."""
    up = tuple(vr.default_camera(W, H).up)
    rsw, rsh = 2.0, 2.0 * H / W
    if name == "default":
        return vr.default_camera(W, H), O.camera_default(W, H)
    if name == "reset":
        return vr.reset_camera(), O.camera_oblique(W, H)
    pos, upv = {"inside": ((0.0, 0.0, 0.45), up), "x": ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
                "-y": ((0.0, -1.0, 0.0), (0.0, 0.0, 1.0))}[name]
    return vr.derive_camera(pos, upv, rsw, rsh), O.camera_derive(pos, upv, rsw, rsh)


def reference(O, key, vol, cal, tf, W, H, S, cam_name, xs=None):
    """The restatement's frame, computed once per (volume, TF, frame, view) and shared."""
    k = (key, W, H, S, cam_name, None if xs is None else tuple(xs))
    if k not in _REFS:
        _, ocam = camera_pair(O, cam_name, W, H)
        _REFS[k] = dvr_ref.render(vol, cal, tf, O.params(W, H, S), ocam, xs=xs)
        _REFS[k].setflags(write=False)
    return _REFS[k]


def assert_bits(got, ref, what=""):
    same = got.view(np.uint32) == ref.view(np.uint32)
    assert same.all(), (what, int((~same).sum()), float(np.abs(got - ref).max()))


def check_all_flags(r, ref, W, H, S, cam, what):
    exact = r.render(vr.default_params(W, H, S, mode=DVR), cam)
    assert_bits(exact, ref, (what, "exact"))
    assert_bits(r.render(vr.default_params(W, H, S, mode=DVR, flags=E), cam), exact, (what, "ess"))
    for fl in (T, E | T):
        fast = r.render(vr.default_params(W, H, S, mode=DVR, flags=fl), cam)
        assert np.abs(fast - exact).max() <= TOL, (what, fl)
        assert np.all(fast[..., 3] == 1.0)
    return exact


FRAMES = [(64, 48, 64), (37, 91, 50)]
VIEWS = ["default", "reset", "inside"]


@pytest.mark.parametrize("W,H,S", FRAMES)
def test_exact_bitwise_byte_and_float_paths(avg152, oracle_mod, W, H, S):
    vol, cal = avg152
    tf = vr.default_transfer_function()
    with vr.VolumeRenderer(vol, cal, device=0) as a, \
            vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for name in VIEWS:
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref = reference(oracle_mod, "avg", vol, cal, tf, W, H, S, name)
            fa = check_all_flags(a, ref, W, H, S, cam, ("byte", name))
            fb = check_all_flags(b, ref, W, H, S, cam, ("float", name))
            assert_bits(fa, fb, name)
            assert not np.all(ref[..., :3] == ref[0, 0, :3]), name   # (the view draws something)
        # the automatic choice took the byte copy (avg152 holds integers 0..255): n + 64 bytes more
        assert a.info.device_bytes - b.info.device_bytes == vol.size + 64


@pytest.mark.parametrize("W,H,S", FRAMES)
def test_fractional_volume_takes_float_path(avg152, oracle_mod, W, H, S):
    vol, cal = avg152
    frac = (vol + np.random.default_rng(3).random(vol.shape, dtype=F)).astype(F)
    tf = vr.default_transfer_function()
    with vr.VolumeRenderer(frac, cal, device=0) as a, \
            vr.VolumeRenderer(frac, cal, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for name in VIEWS:
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref = reference(oracle_mod, "frac", frac, cal, tf, W, H, S, name)
            fa = check_all_flags(a, ref, W, H, S, cam, ("auto", name))
            assert_bits(fa, b.render(vr.default_params(W, H, S, mode=DVR), cam), name)
        assert a.info.device_bytes == b.info.device_bytes   # no byte copy kept: both read the float volume


def test_margin_case(oracle_mod):
    """A block of float32(0.1) whose class boundary sits one ulp above 0.1: an unfused lerp of equal
    corners can land on that ulp, so the cell bits need their margin (a zero margin skips opaque
    samples here and fails ESS == exact)."""
    vol = np.zeros((24, 24, 24), F)
    vol[4:20, 4:20, 4:20] = F(0.1)
    tf = [(0.0, float(F(0.1)), (0.0, 0.0, 0.0, 0.0)),
          (float(np.nextafter(F(0.1), F(1.0))), 1.0, (1.0, 0.0, 0.0, 0.5))]
    W, H, S = 32, 32, 64
    ref = reference(oracle_mod, "margin", vol, 1.0, tf, W, H, S, "reset")
    bg = np.array([0.2, 0.2, 0.2], F)
    assert np.any(np.any(ref[..., :3] != bg, axis=-1))   # the case bites: opaque samples exist
    with vr.VolumeRenderer(vol, 1.0, tf=tf, device=0) as r:
        cam = vr.reset_camera()
        exact = r.render(vr.default_params(W, H, S, mode=DVR), cam)
        assert_bits(exact, ref, "exact")
        assert_bits(r.render(vr.default_params(W, H, S, mode=DVR, flags=E), cam), exact, "ess")


def test_edge_clamp_cube_filling_volume(oracle_mod):
    """Opaque faces: samples in the last voxel layer of every axis read their clamped neighbour."""
    vol = random_volume()
    tf = vr.default_transfer_function()
    W, H, S = 90, 70, 160
    with vr.VolumeRenderer(vol, 255.0, device=0) as a, \
            vr.VolumeRenderer(vol, 255.0, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for name in ("reset", "default", "x", "-y"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref = reference(oracle_mod, "cube", vol, 255.0, tf, W, H, S, name)
            for r in (a, b):
                assert_bits(r.render(vr.default_params(W, H, S, mode=DVR), cam), ref, name)
                fast = r.render(vr.default_params(W, H, S, mode=DVR, flags=T), cam)
                assert np.abs(fast - ref).max() <= TOL, name


def test_tf_paths(avg152, oracle_mod):
    """An opaque class of 0 (no clip, no skipping), 17 and 256 intervals (the LDS search), and a TF set
    on a live context against a fresh context."""
    vol, cal = avg152
    W, H, S = 64, 48, 64
    tfs = {"opaque0": [(0.0, 1.0, (0.1, 0.2, 0.3, 0.05)), (0.3, 0.6, (0.9, 0.5, 0.1, 0.4))],
           "seeded17": seeded_tf(17, 17), "seeded256": seeded_tf(256, 256)}
    with vr.VolumeRenderer(vol, cal, device=0) as live:
        for key, tf in tfs.items():
            live.set_transfer_function(tf)
            with vr.VolumeRenderer(vol, cal, tf=tf, device=0) as fresh:
                for name in ("default", "reset"):
                    cam, _ = camera_pair(oracle_mod, name, W, H)
                    ref = reference(oracle_mod, key, vol, cal, tf, W, H, S, name)
                    got = check_all_flags(fresh, ref, W, H, S, cam, (key, name))
                    assert_bits(live.render(vr.default_params(W, H, S, mode=DVR), cam), got, (key, name, "live"))
                    assert_bits(live.render(vr.default_params(W, H, S, mode=DVR, flags=E), cam), got, (key, name))


@pytest.mark.parametrize("W,H,S", [(1, 1, 1), (1, 130, 2), (257, 3, 1)])
def test_degenerate_frames(avg152, oracle_mod, W, H, S):
    vol, cal = avg152
    tf = vr.default_transfer_function()
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        for name in ("default", "reset"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            ref = reference(oracle_mod, "avg", vol, cal, tf, W, H, S, name)
            check_all_flags(r, ref, W, H, S, cam, name)


def test_tiles_group_and_batch(avg152, oracle_mod, tmp_path):
    import ctypes as C
    import torch
    vol, cal = avg152
    W, H, S = 200, 150, 70
    p = vr.default_params(W, H, S, mode=DVR, flags=E | T)
    cams = [camera_pair(oracle_mod, n, W, H)[0] for n in ("default", "reset", "inside")]
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        frames = [r.render(p, c) for c in cams]
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
        # a batch of three cameras equals three renders
        batch = r.render_batch(p, cams)
        for f, c in enumerate(cams):
            assert_bits(batch[f], frames[f], ("batch", f))
        # the headless saveImage of a DVR frame
        png = tmp_path / "dvr.png"
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
                r.render(vr.default_params(W, H, S, mode=DVR, flags=fl), cam)
            assert e.value.code == -1
        p = vr.default_params(W, H, S, mode=DVR)
        for call in (r.count_samples, r.count_marched, r.count_work):
            with pytest.raises(vr.VRError) as e:
                call(p, cam)
            assert e.value.code == -1
        assert r.axis_columns_plan(p, cam)["columns"] is False
        assert r.render(p, cam).shape == (W, H, 4)   # (the context still renders)
    with vr.VolumeRenderer(vol, -1.0, device=0) as r:   # the mode needs a positive cal_max
        with pytest.raises(vr.VRError) as e:
            r.render(vr.default_params(W, H, S, mode=DVR), cam)
        assert e.value.code == -1


def test_midsize_mni(mni_standin, oracle_mod):
    """MNI stand-in (182 x 218 x 182) at 480 x 270 x 500, on the device: ESS == exact, ESS + ERT within
    1e-4, alpha 1; five seeded columns bitwise against the restatement."""
    import torch
    vol, cal = mni_standin
    W, H, S = 480, 270, 500
    tf = vr.default_transfer_function()
    xs = sorted(int(x) for x in np.random.default_rng(5).choice(W, 5, replace=False))
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        for name in ("default", "reset"):
            cam, _ = camera_pair(oracle_mod, name, W, H)
            out = {}
            for key, fl in (("exact", 0), ("ess", E), ("fast", E | T)):
                t = torch.empty((W, H, 4), dtype=torch.float32, device="cuda:0")
                r.render_device(vr.default_params(W, H, S, mode=DVR, flags=fl), cam, t.data_ptr())
                out[key] = t
            assert torch.equal(out["ess"], out["exact"]), name
            assert (out["fast"] - out["exact"]).abs().max().item() <= TOL, name
            assert torch.all(out["exact"][..., 3] == 1.0)
            ref = reference(oracle_mod, "mni", vol, cal, tf, W, H, S, name, xs=xs)
            assert_bits(out["exact"][xs].cpu().numpy(), ref, name)
