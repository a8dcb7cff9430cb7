"""vr_set_crop_box on the GPU: the six field modes under a crop box, held to tests/crop_ref.py (the numpy
restatement built from the modes' own restatements; tests/test_crop_ref.py holds it to them).

Exact and ESS frames are bitwise the restatement's; ERT and ESS | ERT frames are within the bound the mode's
own GPU tests use (test_gpu_dvr.TOL = test_gpu_shade.TOL_ERT = 1e-4, and for the long rays
test_gpu_params.ert_bound with the operative sample count, as test_gpu_dvr.check_long); MIP and ISO are
bitwise in all four flag combinations.  Boxes, ingredients and the shared references are test_crop_ref's.
"""
import numpy as np
import pytest

import crop_ref
import param_cases as pc
import scdvr_cases as xc
import test_crop_ref as tc
import volumerenderingproject_amd as vr
from test_gpu_dvr import TOL, assert_bits, camera_pair
from test_gpu_shade import TOL_ERT

pytestmark = pytest.mark.gpu

E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
F = np.float32
MODE = {"dvr": vr.VR_MODE_DVR, "sdvr": vr.VR_MODE_SDVR, "cdvr": vr.VR_MODE_CDVR, "scdvr": vr.VR_MODE_SCDVR,
        "mip": vr.VR_MODE_MIP, "iso": vr.VR_MODE_ISO}
BITWISE_FLAGS = ("mip", "iso")
assert TOL == TOL_ERT


def setup(r, cal, variant="zt"):
    """Every mode's ingredients on a context (test_crop_ref's)."""
    if variant == "fog":
        r.set_transfer_function(tc.tf_of("fog"))
    r.set_colormap(tc.map_of(variant, cal))
    r.set_gradient_opacity(xc.gopa_of(tc.GOPA))
    r.set_isosurface(tc.ISO_VALUE, tc.ISO_RGB)


def params(mode, W, H, S, flags=0):
    p = vr.default_params(W, H, S, mode=MODE[mode], flags=flags)
    p.shade_ambient, p.shade_diffuse, p.shade_specular, p.shade_shininess = tc.ISO_SHADE if mode == "iso" else tc.SHADE
    return p


def set_box(r, box):
    if box is None:
        r.set_crop_box(None)
    else:
        r.set_crop_box(*box)
        assert r.crop_box == (tuple(float(F(c)) for c in box[0]), tuple(float(F(c)) for c in box[1]))


def check_all_flags(r, mode, ref, W, H, S, cam, what, tol=TOL, make=None, seen=None):
    """The rule of comparison.  make: flags -> the frame's parameters where they are not the default ones
    (tests/test_gpu_crop_params.py); tol: a number, or a bound per colour channel; seen: a list that takes the
    deviation of every ERT frame."""
    make = make or (lambda fl: params(mode, W, H, S, fl))
    exact = r.render(make(0), cam)
    assert_bits(exact, ref, (what, "exact"))
    assert_bits(r.render(make(E), cam), exact, (what, "ess"))
    for fl in (T, E | T):
        fast = r.render(make(fl), cam)
        if mode in BITWISE_FLAGS:
            assert_bits(fast, exact, (what, fl))
        else:
            err = float(np.abs(fast - exact).max())
            if seen is not None:
                seen.append(err)
            if np.ndim(tol):
                per = np.abs(fast[..., :3].astype(np.float64) - exact[..., :3]).max(axis=(0, 1))
                assert np.all(per <= tol), (what, fl, per, tol)
            else:
                assert err <= tol, (what, fl, err)
            assert np.all(fast[..., 3] == 1.0)
    return exact


def contexts(vol, cal):
    """The byte-copy context and the float-volume one."""
    return (vr.VolumeRenderer(vol, cal, device=0),
            vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1)))


def draws(frame, W, H, S):
    return bool(np.any(frame[..., :3] != tc.background(W, H, S)))


# ---- every mode x box, frames and views of the modes' own files, byte copy and float volume -----------

@pytest.mark.parametrize("view", tc.VIEWS)
@pytest.mark.parametrize("W,H,S", tc.FRAMES)
@pytest.mark.parametrize("mode", tc.MODES)
def test_modes_and_boxes(avg152, oracle_mod, mode, W, H, S, view):
    vol, cal = avg152
    cam, ocam = camera_pair(oracle_mod, view, W, H)
    a, b = contexts(vol, cal)
    with a, b:
        for r in (a, b):
            setup(r, cal)
        for name in tc.BOX_NAMES:
            box = tc.box_of(name, vol.shape, oracle_mod.params(W, H, S), ocam)
            ref, _ = tc.reference(mode, "avg", vol, cal, W, H, S, view, box)
            assert draws(ref, W, H, S) == (name not in tc.DRAWS_NOTHING), (mode, view, name)
            for r, path in ((a, "byte"), (b, "float")):
                set_box(r, box)
                check_all_flags(r, mode, ref, W, H, S, cam, (mode, view, name, path))


# ---- whole, off and the modes that ignore the box -----------------------------------------------------

def test_whole_and_off_are_the_frame_before(avg152, oracle_mod):
    vol, cal = avg152
    W, H, S = 64, 48, 64
    views = [camera_pair(oracle_mod, v, W, H)[0] for v in ("default", "reset")]
    other = [vr.default_params(W, H, S, mode=m, flags=fl) for m in (vr.VR_MODE_VRC, vr.VR_MODE_TEST) for fl in (0, E | T)]
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        setup(r, cal)
        assert r.crop_box is None
        before = {(m, fl, i): r.render(params(m, W, H, S, fl), cam)
                  for m in tc.MODES for fl in (0, E, T, E | T) for i, cam in enumerate(views)}
        before_other = [[r.render(p, cam) for cam in views] for p in other]
        for box in (tc.AVG_BOXES["whole"], ((0.0, 0.0, 0.0), tuple(float(d) for d in vol.shape)), None):
            set_box(r, box)
            for (m, fl, i), f in before.items():
                assert_bits(r.render(params(m, W, H, S, fl), views[i]), f, ("whole/off", box, m, fl, i))
        # VRC and TEST ignore the box
        set_box(r, tc.AVG_BOXES["roi"])
        for p, fs in zip(other, before_other):
            for cam, f in zip(views, fs):
                assert_bits(r.render(p, cam), f, ("ignored", p.mode, p.flags))
        # and the box did bite meanwhile
        assert not np.array_equal(r.render(params("mip", W, H, S), views[1]), before[("mip", 0, 1)])


# ---- not zero transparent: the samples outside the box are fog, the clip must not narrow the range -----

@pytest.mark.parametrize("mode", ["dvr", "sdvr", "cdvr", "scdvr"])
def test_fog_outside_the_box(avg152, oracle_mod, mode):
    vol, cal = avg152
    W, H, S = 64, 48, 64
    box = tc.AVG_BOXES["roi"]
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        setup(r, cal, "fog")
        set_box(r, box)
        for view in ("reset", "default"):
            cam, _ = camera_pair(oracle_mod, view, W, H)
            ref, _ = tc.reference(mode, "avg", vol, cal, W, H, S, view, box, "fog")
            off, _ = tc.reference(mode, "avg", vol, cal, W, H, S, view, None, "fog")
            assert not tc.bits_equal(ref, off)
            # every pixel is fogged: nothing is the background, so no tile may be culled
            assert np.all(np.any(ref[..., :3] != tc.background(W, H, S), axis=-1))
            check_all_flags(r, mode, ref, W, H, S, cam, (mode, view, "fog"))


# ---- long rays: the clip's margins at 0.02-voxel steps -------------------------------------------------

@pytest.mark.parametrize("view", ["reset", "default"])
@pytest.mark.parametrize("mode", ["dvr", "iso"])
def test_long_rays(avg152, oracle_mod, mode, view):
    """roi at 20 x 14 x 9000.  DVR's ERT frames: test_gpu_dvr.check_long's bound, ert_bound(tf, bg, 1e-5, S_op)
    per channel with S_op the largest number of samples with a non-zero alpha on a ray of the reference, and
    the flat TOL, as there."""
    from test_gpu_params import ert_bound
    import dvr_ref
    vol, cal = avg152
    W, H, S = 20, 14, 9000
    box = tc.AVG_BOXES["roi"]
    cam, ocam = camera_pair(oracle_mod, view, W, H)
    ref, _ = tc.reference(mode, "avg", vol, cal, W, H, S, view, box)
    assert draws(ref, W, H, S)
    a, b = contexts(vol, cal)
    with a, b:
        for r in (a, b):
            setup(r, cal)
            set_box(r, box)
            exact = check_all_flags(r, mode, ref, W, H, S, cam, (mode, view, "long"))
            if mode == "dvr":
                p = oracle_mod.params(W, H, S)
                col = dvr_ref.sample_colors(vol, cal, tc.tf_of("zt"), p, ocam)
                keep = crop_ref.in_box(vol.shape, p, ocam, box)
                s_op = int(((col[..., 3] != 0.0) & keep).sum(axis=2).max())
                assert 0 < s_op <= S
                bound = ert_bound(tc.tf_of("zt"), (0.2, 0.2, 0.2), 1e-5, s_op)
                for fl in (T, E | T):
                    fast = r.render(params(mode, W, H, S, fl), cam)
                    err = np.abs(fast[..., :3].astype(np.float64) - ref[..., :3]).max(axis=(0, 1))
                    assert np.all(err <= bound), (view, fl, s_op, err, bound)


# ---- tiny volumes --------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 1), (3, 2, 5)])
def test_tiny_volumes(oracle_mod, shape):
    """A box inside the volume (the middle half of every axis), and one that cuts it at a voxel centre."""
    vol = pc.tiny_volume(shape)
    cal = 255.0
    W, H, S = pc.TW, pc.TH, pc.TS
    boxes = [(tuple(0.25 * d for d in shape), tuple(0.75 * d for d in shape)),
             ((0.0, 0.0, 0.0), tuple(d - 0.5 for d in shape))]
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        setup(r, cal)
        for view in ("reset", "default"):
            cam, _ = camera_pair(oracle_mod, view, W, H)
            for i, box in enumerate(boxes):
                set_box(r, box)
                for mode in tc.MODES:
                    ref, _ = tc.reference(mode, ("tiny", shape), vol, cal, W, H, S, view, box)
                    check_all_flags(r, mode, ref, W, H, S, cam, (shape, mode, view, i))
            assert draws(tc.reference("mip", ("tiny", shape), vol, cal, W, H, S, view, boxes[0])[0], W, H, S)


# ---- state: a sequence of boxes, a batch, queued frames -------------------------------------------------

def test_state_sequence_batch_and_queued_frames(avg152, oracle_mod):
    import torch
    vol, cal = avg152
    W, H, S = 64, 48, 64
    names = ("default", "reset", "inside")
    cams = [camera_pair(oracle_mod, v, W, H)[0] for v in names]
    seq = [tc.AVG_BOXES["cut"], tc.AVG_BOXES["roi"], None]
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        setup(r, cal)
        for box in seq:   # set cut -> render -> set roi -> render -> off -> render
            set_box(r, box)
            assert (r.crop_box is None) == (box is None)
            for mode in tc.MODES:
                for fl in (0, E):
                    ref, _ = tc.reference(mode, "avg", vol, cal, W, H, S, "reset", box)
                    assert_bits(r.render(params(mode, W, H, S, fl), cams[1]), ref, ("sequence", box, mode, fl))
        # vr_render_batch with a box set
        set_box(r, tc.AVG_BOXES["roi"])
        for mode in tc.MODES:
            batch = r.render_batch(params(mode, W, H, S, E), cams)
            for i, v in enumerate(names):
                ref, _ = tc.reference(mode, "avg", vol, cal, W, H, S, v, tc.AVG_BOXES["roi"])
                assert_bits(batch[i], ref, ("batch", mode, v))
        # three queued frames, the box changed between them: each shows the box it was enqueued under
        for mode in tc.MODES:
            out = torch.zeros((3, W, H, 4), dtype=torch.float32, device="cuda:0")
            p = params(mode, W, H, S, E)
            for i, box in enumerate(seq):
                set_box(r, box)
                r.render_device(p, cams[1], out[i].data_ptr(), asynchronous=True)
            r.set_crop_box(None)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            for i, box in enumerate(seq):
                ref, _ = tc.reference(mode, "avg", vol, cal, W, H, S, "reset", box)
                assert_bits(got[i], ref, ("queued", mode, i))


def test_arguments(avg152):
    vol, cal = avg152
    nan, inf = float("nan"), float("inf")
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        assert r.crop_box is None
        for lo, hi in (((0, 0, 0), (1, nan, 1)), ((0, -inf, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, inf)),
                       ((0, 2, 0), (1, 1, 1))):
            with pytest.raises(vr.VRError) as e:
                r.set_crop_box(lo, hi)
            assert e.value.code == -1
        import ctypes as C
        three = (C.c_float * 3)(0, 0, 0)
        assert vr.lib().vr_set_crop_box(r._ctx, three, None) == -1
        assert vr.lib().vr_set_crop_box(r._ctx, None, three) == -1
        assert r.crop_box is None
        r.set_crop_box((1, 2, 3), (1, 2.5, 300))    # lo == hi is allowed, and the box may pass the volume
        assert r.crop_box == ((1.0, 2.0, 3.0), (1.0, 2.5, 300.0))
        r.set_crop_box(None)
        assert r.crop_box is None


# ---- tiles ---------------------------------------------------------------------------------------------

def test_tiles_under_a_box(avg152, oracle_mod):
    import torch
    from volumerenderingproject_amd.renderer import tiles_per_rank
    vol, cal = avg152
    # 160 x 96: ten by six 16 x 16 tiles, the volume over most of them (test_gpu_cmap's cull frame)
    W, H, S = 160, 96, 64
    tw = th = 16
    ntx, nty = (W + tw - 1) // tw, (H + th - 1) // th
    box = tc.AVG_BOXES["roi"]
    bg = tc.background(W, H, S)
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        setup(r, cal)
        for view in ("reset", "default"):
            cam, _ = camera_pair(oracle_mod, view, W, H)
            for mode in ("dvr", "mip", "iso", "scdvr"):
                p = params(mode, W, H, S, E)
                r.set_crop_box(None)
                vis_off = set(int(t) for t in r.visible_tiles(p, cam, tw, th))
                set_box(r, box)
                ref, _ = tc.reference(mode, "avg", vol, cal, W, H, S, view, box)
                off, _ = tc.reference(mode, "avg", vol, cal, W, H, S, view, None)
                whole = r.render(p, cam)
                assert_bits(whole, ref, ("whole", mode, view))
                # vr_render_tiles + vr_assemble_tiles equal the whole frame
                world = 3
                mt = max(tiles_per_rank(W, H, 32, 32, k, world) for k in range(world))
                tiles = torch.zeros((world, mt, 32 * 32, 4), dtype=torch.float32, device="cuda:0")
                for rank in range(world):
                    assert r.render_tiles(p, cam, 32, 32, rank, world, tiles[rank].data_ptr()) == \
                        tiles_per_rank(W, H, 32, 32, rank, world)
                frame = torch.zeros((W, H, 4), dtype=torch.float32, device="cuda:0")
                r.assemble_tiles(W, H, 32, 32, world, mt, tiles.data_ptr(), frame.data_ptr())
                assert_bits(frame.cpu().numpy(), ref, ("tiles", mode, view))
                # vr_visible_tiles: a subset of the box-off list, every omitted tile background in the restatement
                vis = set(int(t) for t in r.visible_tiles(p, cam, tw, th))
                assert vis <= vis_off

                def tile_draws(f, t):
                    tx, ty = divmod(t, nty)
                    return not np.all(f[tx * tw:(tx + 1) * tw, ty * th:(ty + 1) * th, :3] == bg)
                for t in range(ntx * nty):
                    if t not in vis:
                        assert not tile_draws(ref, t), (mode, view, t)
                # the restatement itself shows fewer non-background tiles under the box: the list is shorter
                n_ref = sum(tile_draws(ref, t) for t in range(ntx * nty))
                n_off = sum(tile_draws(off, t) for t in range(ntx * nty))
                assert n_ref < n_off, (mode, view, n_ref, n_off)
                assert len(vis) < len(vis_off), (mode, view, len(vis), len(vis_off))
        # an empty box culls every tile
        set_box(r, tc.AVG_BOXES["empty"])
        cam, _ = camera_pair(oracle_mod, "reset", W, H)
        for mode in ("dvr", "mip", "iso"):
            assert len(r.visible_tiles(params(mode, W, H, S, E), cam, tw, th)) == 0


def test_peer_copy_group_under_a_box(avg152, oracle_mod):
    vol, cal = avg152
    W, H, S = 200, 150, 70
    box = tc.AVG_BOXES["roi"]
    cams = [camera_pair(oracle_mod, v, W, H)[0] for v in ("default", "reset")]
    with vr.VolumeRenderer(vol, cal, device=0) as r, vr.VolumeRenderer(vol, cal, devices=[0, 0]) as g:
        for c in (r, g):
            setup(c, cal)
            set_box(c, box)
        assert g.crop_box == r.crop_box
        for mode in tc.MODES:
            p = params(mode, W, H, S, E | T)
            for i, cam in enumerate(cams):
                one = r.render(p, cam)
                assert_bits(g.render(p, cam), one, ("group", mode, i))
                assert draws(one, W, H, S)
        g.set_crop_box(None)
        r.set_crop_box(None)
        p = params("mip", W, H, S, E)
        assert_bits(g.render(p, cams[1]), r.render(p, cams[1]), "group off")
