"""The fused column march (vr_options.column_fused) on the GPU: one kernel marches the leaf columns under a
tile of pixels and stores the tile.

Nothing is reassociated and every pixel's column comes from the expand pass's own per-pixel code, so a
fused frame must equal the two-kernel column path's (column_fused = 0) and the per-pixel march's
(axis_columns = 0) bit for bit, whatever the flags.  Whether a frame is fused, and in which tile shape,
depends on how many leaf columns lie under a tile: the library reports it (vr_column_fused_plan) and the
tests restate the rule (`expected_shape`) and assert both, so that no comparison here passes by comparing
the two-kernel path with itself unnoticed.

The views are test_gpu_axis_columns.views' by name.  With their own screen widths a small frame has many
leaf columns per pixel and no tile shape fits (such frames take the two-kernel path: test_issue_sizes keeps
them, as cases of that rule); the other tests keep each view's position and roll and choose the real screen
width from the wanted pixels per leaf column, which is what selects the tile shape.
"""
import numpy as np
import pytest

import volumerenderingproject_amd as vr
from fused_cases import LADDER, shape_rule
from test_gpu_axis_columns import params, views

pytestmark = pytest.mark.gpu

E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
FLAGS = (0, E, T, E | T)   # every flag set the column path admits; T marches front to back, 0 and E back to front
S = 96
assert LADDER == [(64, 48), (48, 48), (48, 32), (32, 32), (32, 16), (16, 16)]
TILE = 16
VIEW_NAMES = ("zoomed", "far", "rolled", "x", "y", "z_back")   # z_back: the -z view
# 16 x 16 ... 203 x 157: frames smaller than a tile, tiles clipped by the frame's edge; then one row of 1 to 17 tiles
ISSUE_SIZES = [(16, 16), (48, 48), (49, 47), (17, 33), (203, 157)] + [(TILE * k, TILE) for k in range(1, 18)]
# (position, up or None = the default camera's) of the views above
POSES = {
    "zoomed": ((0.0, 0.0, 1.0), None), "far": ((0.0, 0.0, 1.0), None), "rolled": ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0)),
    "x": ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)), "y": ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), "z_back": ((0.0, 0.0, -1.0), None),
}


def expected_shape(p, cam, nleaf):
    """The documented rule (fused_cases.shape_rule, where fused_cases.expected_shape applies it to a case) of
    the library's own parameters and camera."""
    return shape_rule(p.width, p.height, p.real_screen_width, p.real_screen_height, cam.right, cam.up, cam.front, nleaf)


def pose_camera(W, H, name, rsw, dist=1.0):
    pos, up = POSES[name]
    up = tuple(vr.default_camera(W, H).up) if up is None else up
    return vr.derive_camera(tuple(dist * c for c in pos), up, rsw, rsw * H / W)


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def nleaf(avg152):
    from volumerenderingproject_amd.renderer import octree_leaf_maps
    return 1 << octree_leaf_maps(*avg152[0].shape)[1]


@pytest.fixture(scope="module")
def trio(avg152):
    """(fused, two, off): the column path forced with column_fused 1 and 0, and the per-pixel march."""
    vol, cal = avg152
    ctx = [vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(**o))
           for o in (dict(axis_columns=2, column_fused=1), dict(axis_columns=2, column_fused=0), dict(axis_columns=0))]
    yield ctx
    for r in ctx:
        r.close()


def check_frame(trio, p, cam, nleaf, what):
    """One frame through the three contexts; returns the tile shape the fused context used (None: two kernels)."""
    fused, two, off = trio
    assert fused.axis_columns_plan(p, cam)["columns"] and two.axis_columns_plan(p, cam)["columns"], what
    assert not off.axis_columns_plan(p, cam)["columns"], what
    shape = fused.column_fused_plan(p, cam)
    assert shape == expected_shape(p, cam, nleaf), (what, shape)
    assert two.column_fused_plan(p, cam) is None and off.column_fused_plan(p, cam) is None, what
    ref = off.render(p, cam)
    got = fused.render(p, cam)
    assert same(got, ref), ("fused against the per-pixel march", what, shape, int((got != ref).any(axis=-1).sum()))
    assert same(two.render(p, cam), ref), ("two kernels against the per-pixel march", what)
    return shape


def test_defaults():
    assert vr.default_options().column_fused in (0, 1)
    with pytest.raises(Exception):
        vr.VolumeRenderer(np.zeros((4, 4, 4), np.float32), 255.0, device=0, options=vr.default_options(column_fused=2))


@pytest.mark.parametrize("name", VIEW_NAMES)
def test_issue_sizes(trio, nleaf, name):
    """The views with their own screen widths at every size: whatever path the rule selects, bitwise."""
    used = set()
    for W, H in ISSUE_SIZES:
        cam, rsw = views(W, H)[name]
        for flags in FLAGS:
            used.add(check_frame(trio, params(W, H, S, rsw, flags), cam, nleaf, (name, W, H, flags)))
    print(name, "tile shapes in use:", used)


# pixels per leaf column -> the tile shape it selects for a view whose right and up lie along one fixed axis each
PPC_SHAPES = [(4.0, (64, 48)), (3.3, (48, 48)), (2.8, (48, 32)), (2.3, (32, 32)), (1.6, (32, 16)), (1.1, (16, 16)),
              (0.9, None)]


@pytest.mark.parametrize("name", VIEW_NAMES)
def test_fused_sizes(trio, nleaf, name):
    """Every size with the screen width that gives 4 and 1.1 pixels per leaf column -- the largest tile, so
    that most of these frames are smaller than one tile or have tiles clipped by the frame's edge, and the
    smallest, one row of 1 to 17 tiles of it -- fused every time."""
    for W, H in ISSUE_SIZES:
        for ppc, want in (PPC_SHAPES[0], PPC_SHAPES[5]):
            rsw = W / (ppc * nleaf)
            cam = pose_camera(W, H, name, rsw)
            for flags in FLAGS:
                assert check_frame(trio, params(W, H, S, rsw, flags), cam, nleaf, (name, W, H, ppc, flags)) == want


@pytest.mark.parametrize("name", VIEW_NAMES)
def test_ladder(trio, nleaf, name):
    """Screen widths that put each tile shape in use on frames with background round the dataset (the
    visible rectangle's edge inside a tile, background-only tiles on every side of it, tiles clipped by the
    frame's edge), and one that no shape fits, which must take the two-kernel path."""
    cases = [(640, 520, 4.0), (600, 440, 3.3), (520, 390, 2.8), (420, 300, 2.3), (300, 220, 1.6), (203, 157, 1.1),
             (203, 157, 0.9)]
    for (W, H, ppc), (ppc_, want) in zip(cases, PPC_SHAPES):
        assert ppc == ppc_
        rsw = W / (ppc * nleaf)
        assert min(rsw, rsw * H / W) > 1.0   # the dataset's projection is at most 0.86 wide: background all round
        cam = pose_camera(W, H, name, rsw)
        for flags in (0, E | T):
            p = params(W, H, S, rsw, flags)
            plan = trio[0].axis_columns_plan(p, cam)
            assert plan["pixels"] < W * H, (name, W, H, plan)   # a visible rectangle smaller than the frame
            assert check_frame(trio, p, cam, nleaf, (name, W, H, ppc, flags)) == want, (name, W, H, ppc)


@pytest.mark.parametrize("n_tf", [10, 20])   # 4- and 8-bit classes (the default TF's are 2-bit)
def test_fused_class_widths(avg152, nleaf, n_tf):
    from test_gpu_parity import _tf_n
    vol, cal = avg152
    tf = _tf_n(n_tf)
    ctx = [vr.VolumeRenderer(vol, cal, tf=tf, device=0, options=vr.default_options(**o))
           for o in (dict(axis_columns=2, column_fused=1), dict(axis_columns=2, column_fused=0), dict(axis_columns=0))]
    W, H = 203, 157
    for name in ("rolled", "x", "z_back"):
        for ppc, want in (PPC_SHAPES[3], PPC_SHAPES[5]):
            rsw = W / (ppc * nleaf)
            cam = pose_camera(W, H, name, rsw)
            for flags in FLAGS:
                assert check_frame(ctx, params(W, H, S, rsw, flags), cam, nleaf, (n_tf, name, ppc, flags)) == want
    for r in ctx:
        r.close()




def batch_cameras(n, W, H, rsw):
    """n cameras: views along z at distinct distances and screen positions, every fifth along x, and an oblique one (out of the
    column path's scope) at frames 2, 3 and 6 -- either side of the seam between a call's first launch
    (three frames) and the next, and where a call of seven ends."""
    cams = []
    for i in range(n):
        d = 0.15 + 0.02 * i   # (two and a half leaves further along the view axis each, the dataset in reach of all)
        if i in (2, 3, 6):
            cams.append(vr.reset_camera())
            continue
        cam = pose_camera(W, H, "x" if i % 5 == 4 else "zoomed", rsw, d)
        for a in range(3):   # and a window of its own: a leaf further along the screen's x each
            cam.top_left[a] += i / 128.0 * cam.right[a]
        cams.append(cam)
    return cams


@pytest.fixture(scope="module")
def batch_refs(avg152, nleaf):
    """The 33 cameras and their per-frame vr_render frames from the per-pixel march, shared by the batch tests."""
    vol, cal = avg152
    W, H = 96, 64
    rsw = W / (2.3 * nleaf)
    p = params(W, H, S, rsw, E | T)
    cams = batch_cameras(33, W, H, rsw)
    with vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=0)) as off:
        refs = [off.render(p, c) for c in cams]
    # distinct frames but for the three oblique ones: a frame stored in another's place would show
    assert len({r.tobytes() for r in refs}) == 31
    return p, cams, refs


@pytest.mark.parametrize("timing", [False, True])
@pytest.mark.parametrize("in_flight", [0, 1])
def test_fused_batch(avg152, batch_refs, in_flight, timing):
    """vr_render_batch calls of 1, 6, 7 and 33 frames against per-frame vr_render: one launch with kernel
    arguments, a first launch and one from device memory, out-of-scope frames at the seams and views of
    another axis in between; with per-launch timing on, the two-kernel path and today's order."""
    import torch
    vol, cal = avg152
    p, cams, refs = batch_refs
    W, H = p.width, p.height
    with vr.VolumeRenderer(vol, cal, device=0,
                           options=vr.default_options(axis_columns=2, column_fused=1, frames_in_flight=in_flight)) as a:
        a.timing_enable(timing)
        for c in cams:
            fused = a.column_fused_plan(p, c)
            scope = a.axis_columns_plan(p, c)["columns"]
            assert fused == ((32, 32) if scope and not timing else None), (fused, scope, timing)
        assert sum(a.axis_columns_plan(p, c)["columns"] for c in cams[:7]) == 4
        for n in (1, 6, 7, 33):
            out = torch.zeros((n, W, H, 4), dtype=torch.float32, device="cuda:0")
            for _ in range(2):   # (the second call reuses the frame array and its staging ring)
                a.render_batch_device(p, cams[:n], out.data_ptr())
            got = out.cpu().numpy()
            for i in range(n):
                assert same(got[i], refs[i]), (n, i, in_flight, timing, int((got[i] != refs[i]).any(axis=-1).sum()))
