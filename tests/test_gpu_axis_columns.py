"""The column path of axis-aligned VRC views (vr_options.axis_columns) on the GPU.

Along a volume axis every ray stays in one leaf column and its march is a function of that column
and the frame-wide sample table alone, so the column path marches each leaf column of the visible
rectangle once and copies the result to every pixel over it.  Nothing is reassociated: its frames
must equal the per-pixel march's (axis_columns = 0) bit for bit in every mode, ERT included.  Every
comparison first asserts through vr_axis_columns_plan that the forced context took the column
path -- an equality test that compared the per-pixel march with itself would prove nothing.
"""
import numpy as np
import pytest

import volumerenderingproject_amd as vr
from test_gpu_parity import TOL, _tf_n, assert_bitwise

pytestmark = pytest.mark.gpu

E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
SIZES = [(320, 240), (203, 157), (96, 80)]   # several pixels per column; ragged tiles; fewer pixels than columns


def views(W, H):
    """name -> (camera, real screen width): along +-x, +-y, +-z (test_gpu_test_mode.py's recipes), a
    90-degree roll, the volume overflowing the screen and a far view with background all round."""
    up = tuple(vr.default_camera(W, H).up)
    rsw = 2.0

    def cam(pos, u, w=rsw):
        return vr.derive_camera(pos, u, w, w * H / W), w

    return {
        "z": (vr.default_camera(W, H), rsw),
        "z_back": cam((0.0, 0.0, -1.0), up),
        "x": cam((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
        "x_back": cam((-1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
        "y": cam((0.0, 1.0, 0.0), (0.0, 0.0, 1.0)),
        "y_back": cam((0.0, -1.0, 0.0), (0.0, 0.0, 1.0)),
        "rolled": cam((0.0, 0.0, 1.0), (1.0, 0.0, 0.0)),
        "zoomed": cam((0.0, 0.0, 1.0), up, 0.55),
        "far": cam((0.0, 0.0, 1.0), up, 6.0),
    }


def params(W, H, S, rsw, flags=0, mode=vr.VR_MODE_VRC):
    p = vr.default_params(W, H, S, mode=mode, flags=flags)
    p.real_screen_width, p.real_screen_height = rsw, rsw * H / W
    return p


@pytest.fixture(scope="module")
def pair(avg152):
    """(forced, off): one context with the column path forced, one with it off (default TF)."""
    vol, cal = avg152
    a = vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=2))
    b = vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=0))
    yield a, b
    a.close()
    b.close()


@pytest.mark.parametrize("n_tf", [4, 10, 20])   # 2-, 4- and 8-bit classes
def test_columns_bitwise_on_off(avg152, n_tf):
    vol, cal = avg152
    tf = _tf_n(n_tf)
    a = vr.VolumeRenderer(vol, cal, tf=tf, device=0, options=vr.default_options(axis_columns=2))
    b = vr.VolumeRenderer(vol, cal, tf=tf, device=0, options=vr.default_options(axis_columns=0))
    S = 96
    for W, H in SIZES:
        for name, (cam, rsw) in views(W, H).items():
            for flags in (0, E, T, E | T):
                p = params(W, H, S, rsw, flags)
                plan = a.axis_columns_plan(p, cam)
                assert plan["columns"], (name, W, H, flags, plan)
                assert not b.axis_columns_plan(p, cam)["columns"]
                fa, fb = a.render(p, cam), b.render(p, cam)
                assert np.array_equal(fa, fb), (name, W, H, flags, float(np.abs(fa - fb).max()),
                                                int((fa != fb).any(axis=-1).sum()))
    a.close()
    b.close()


def test_columns_match_oracle(pair, avg152, avg152_octree, oracle_mod):
    """Columns forced: exact frames equal the oracle's bitwise, ESS | ERT frames within the ERT tolerance."""
    a, _ = pair
    vol, cal = avg152
    O = oracle_mod
    W, H, S = 120, 90, 100
    up = tuple(vr.default_camera(W, H).up)
    rsh = 2.0 * H / W
    cases = {
        "z": (vr.default_camera(W, H), O.camera_default(W, H)),
        "z_back": (vr.derive_camera((0.0, 0.0, -1.0), up, 2.0, rsh), O.camera_derive((0.0, 0.0, -1.0), up, 2.0, rsh)),
        "x": (vr.derive_camera((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 2.0, rsh),
              O.camera_derive((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 2.0, rsh)),
    }
    for name, (cam, ocam) in cases.items():
        ref = avg152_octree.render_vrc(cal, O.default_tf(), O.params(W, H, S), ocam)
        p = vr.default_params(W, H, S)
        assert a.axis_columns_plan(p, cam)["columns"], name
        assert_bitwise(a.render(p, cam), ref)
        p = vr.default_params(W, H, S, flags=E | T)
        assert a.axis_columns_plan(p, cam)["columns"], name
        assert np.abs(a.render(p, cam) - ref).max() <= TOL, name


@pytest.mark.parametrize("in_flight", [1, 0])
def test_columns_frames_in_flight(avg152, in_flight):
    """A batch of 7 distinct dolly views along z, one column buffer per stream: a stale or overwritten
    buffer would show as another camera's frame."""
    import torch
    vol, cal = avg152
    W, H, S = 203, 157, 96
    up = tuple(vr.default_camera(W, H).up)
    zcams = [vr.derive_camera((0.0, 0.0, z), up, 2.0, 2.0 * H / W) for z in (0.15, 0.3, 0.45, 0.6, 0.8, 1.0, 1.3)]
    # the same with views along x in between: a batch marches the columns of the frames that share
    # its first frame's kernel variant in one launch; the others march on their own in-flight streams
    xcams = [vr.derive_camera((x, 0.0, 0.0), (0.0, 1.0, 0.0), 2.0, 2.0 * H / W) for x in (0.2, 0.5, 0.9, 1.2)]
    mixed = [c for pair_ in zip(zcams, xcams) for c in pair_] + zcams[4:]
    a = vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=2, frames_in_flight=in_flight))
    b = vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=0))
    for flags, cams in ((0, zcams), (E | T, zcams), (E | T, mixed)):
        p = vr.default_params(W, H, S, flags=flags)
        for cam in cams:
            assert a.axis_columns_plan(p, cam)["columns"]
        out = torch.zeros((len(cams), W, H, 4), dtype=torch.float32, device="cuda:0")
        for _ in range(2):   # (the second batch reuses the streams' buffers)
            a.render_batch_device(p, cams, out.data_ptr())
        got = out.cpu().numpy()
        refs = [b.render(p, cam) for cam in cams]
        for i in range(len(cams)):
            assert np.array_equal(got[i], refs[i]), (flags, i, float(np.abs(got[i] - refs[i]).max()))
        assert all(not np.array_equal(refs[i], refs[i + 1]) for i in range(len(cams) - 1))   # distinct views
    a.close()
    b.close()


def test_columns_gate(avg152):
    vol, cal = avg152
    S = 96
    auto = vr.VolumeRenderer(vol, cal, device=0)
    assert vr.default_options().axis_columns == 1
    big, small = vr.default_params(640, 480, S, flags=E | T), vr.default_params(96, 80, S, flags=E | T)
    plan = auto.axis_columns_plan(big, vr.default_camera(640, 480))
    assert plan["columns"] and plan["pixels"] >= 2 * plan["n0"] * plan["n1"]
    plan = auto.axis_columns_plan(small, vr.default_camera(96, 80))
    assert not plan["columns"] and plan["pixels"] < 2 * plan["n0"] * plan["n1"]
    # out of scope, whatever the ratio (auto and forced): oblique, conic, TEST, opaque TF(0), 64-bit offsets
    forced = vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=2))
    cam = vr.default_camera(640, 480)
    for r in (auto, forced):
        assert not r.axis_columns_plan(big, vr.reset_camera())["columns"]
        assert not r.axis_columns_plan(vr.default_params(640, 480, S, flags=vr.VR_FLAG_CONIC), cam)["columns"]
        assert not r.axis_columns_plan(vr.default_params(640, 480, S, mode=vr.VR_MODE_TEST), cam)["columns"]
    opaque0 = [(0.0, 0.3, (0.1, 0.2, 0.3, 0.4)), (0.3, 1.0, (0.9, 0.5, 0.1, 0.6))]
    for ac in (1, 2):
        with vr.VolumeRenderer(vol, cal, tf=opaque0, device=0, options=vr.default_options(axis_columns=ac)) as r:
            assert not r.axis_columns_plan(big, cam)["columns"]
        with vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=ac, force_idx64=1)) as r:
            assert not r.axis_columns_plan(big, cam)["columns"]
    # the counting pass counts the per-ray march either way
    off = vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=0))
    p = vr.default_params(160, 120, S, flags=E | T)
    c = vr.default_camera(160, 120)
    assert forced.axis_columns_plan(p, c)["columns"]
    assert forced.count_marched(p, c) == off.count_marched(p, c)
    assert forced.count_work(p, c) == off.count_work(p, c)
    # and an auto frame over the threshold is the per-pixel frame
    assert np.array_equal(auto.render(big, cam), off.render(big, cam))
    for r in (auto, forced, off):
        r.close()


def test_columns_rectangle_bounds_every_pixel(pair, avg152):
    """The host's leaf rectangle and gate against a numpy restatement over every pixel of a 203 x 157
    frame: the rectangle spans the leaf columns of every pixel that can see the dataset (those pixels
    all lie in the visible rectangle), is at most one leaf wider each way than the span of the whole
    frame's pixels, and the auto gate is pixels >= 2 columns."""
    a, _ = pair
    vol, cal = avg152
    W, H, S = 203, 157, 96
    from volumerenderingproject_amd.renderer import octree_leaf_maps
    maps, depth = octree_leaf_maps(*vol.shape)
    nleaf = 1 << depth
    f32 = np.float32
    auto = vr.VolumeRenderer(vol, cal, device=0)
    for name, (cam, rsw) in views(W, H).items():
        p = params(W, H, S, rsw, E | T)
        front = np.array(cam.front, f32)
        ma = int(np.flatnonzero(front)[0])
        a0, a1 = (1 if ma == 0 else 0), (1 if ma == 2 else 2)
        x = np.arange(W, dtype=f32)[:, None]
        y = np.arange(H, dtype=f32)[None, :]
        A = x * f32(p.real_screen_width) / f32(W)
        B = y * f32(p.real_screen_height) / f32(H)
        span, span_all = [], []
        sees = np.ones((W, H), bool)
        idx = []
        for ax in (a0, a1):
            P0 = (f32(cam.top_left[ax]) + A * f32(cam.right[ax])) + B * (-f32(cam.up[ax]))
            q = P0 + f32(0.5)
            v = q * f32(nleaf)
            i = np.clip(np.nan_to_num(v), 0, nleaf - 1).astype(np.int64)
            sees &= (q >= 0) & (q < 1) & (maps[ax][i] >= 0)
            idx.append(i)
            span_all.append(int(i.max() - i.min() + 1))
        plan = a.axis_columns_plan(p, cam)
        assert plan["columns"], name
        for k, n in enumerate((plan["n0"], plan["n1"])):
            if sees.any():
                assert n >= int(idx[k][sees].max() - idx[k][sees].min() + 1), (name, k, plan)
            assert 1 <= n <= span_all[k] + 2, (name, k, plan)
        assert int(sees.sum()) <= plan["pixels"] <= W * H, (name, plan)
        pa = auto.axis_columns_plan(p, cam)
        assert (pa["n0"], pa["n1"], pa["pixels"]) == (plan["n0"], plan["n1"], plan["pixels"])
        assert pa["columns"] == (pa["pixels"] >= 2 * pa["n0"] * pa["n1"]), (name, pa)
    auto.close()
