"""The expand pass of the column path (axis_expand_kernel) over grouped work tiles, on the GPU.

A workgroup of the expand takes several consecutive work tiles of the visible rectangle, and a
background-only workgroup several culled ones; neither group size is visible outside the library, so
the frame sizes here make the number of 16 x 16 tiles of the visible rectangle take every value from
1 to 17: whatever the group sizes (up to 8 and 16), some case has fewer tiles than one group, some a
tail group and some exactly whole groups.  Every frame is compared bit for bit with the per-pixel
march's (axis_columns = 0), after asserting through vr_axis_columns_plan that the forced context
took the column path, and every case asserts, from the plan's numbers, the tile count it stands for.
"""
import numpy as np
import pytest

import volumerenderingproject_amd as vr
from test_gpu_axis_columns import params, views

pytestmark = pytest.mark.gpu

S = 96
FLAGS = vr.VR_FLAG_ESS | vr.VR_FLAG_ERT
TILE = 16
# one row of k tiles, k = 1 .. 17, then ragged frames (2 x 3 and 13 x 10 tiles)
SIZES = [(TILE * k, TILE) for k in range(1, 18)] + [(17, 33), (203, 157)]
# test_gpu_axis_columns.views by name -> (unit position, up or None for the default camera's, real screen width):
# `zoomed` has no background tile at all, `far` has background all round, `x` and `y` march the other axes
VIEWS = {
    "zoomed": ((0.0, 0.0, 1.0), None, 0.55),
    "far": ((0.0, 0.0, 1.0), None, 6.0),
    "rolled": ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), 2.0),
    "x": ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 2.0),
    "y": ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0), 2.0),
}
DOLLY = (0.15, 0.3, 0.45, 0.6, 0.8, 1.0, 1.3)   # 7 distinct distances along the view axis
WORK_ORDERS = (0, 2)                            # the list dealt on the device, and a host-built one


def camera(W, H, name, dist=1.0):
    pos, up, rsw = VIEWS[name]
    up = tuple(vr.default_camera(W, H).up) if up is None else up
    return vr.derive_camera(tuple(dist * c for c in pos), up, rsw, rsw * H / W), rsw


def frame_tiles(W, H):
    return -(-W // TILE) * -(-H // TILE)


def rect_tiles(W, H, plan):
    """Tiles of the visible rectangle from the plan's pixel count; None where that does not determine
    them (a ragged frame whose rectangle is not the whole frame)."""
    if plan["pixels"] == W * H:
        return frame_tiles(W, H)
    if H == TILE and plan["pixels"] % (TILE * TILE) == 0:   # one tile row: the rectangle is whole tiles of it
        return plan["pixels"] // (TILE * TILE)
    return None


@pytest.fixture(scope="module")
def contexts(avg152):
    """{(work_order, frames_in_flight): forced context}, and the per-pixel context."""
    vol, cal = avg152
    forced = {(wo, fif): vr.VolumeRenderer(vol, cal, device=0,
                                           options=vr.default_options(axis_columns=2, work_order=wo,
                                                                      frames_in_flight=fif))
              for wo in WORK_ORDERS for fif in (0, 1)}
    off = vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=0))
    yield forced, off
    for r in forced.values():
        r.close()
    off.close()


def test_views_are_the_axis_column_tests():
    """The cameras built here at distance 1 are test_gpu_axis_columns.views' own."""
    W, H = 203, 157
    theirs = views(W, H)
    for name in VIEWS:
        cam, rsw = camera(W, H, name)
        ref, ref_rsw = theirs[name]
        assert rsw == ref_rsw
        for field in ("top_left", "right", "up", "front"):
            assert tuple(getattr(cam, field)) == tuple(getattr(ref, field)), (name, field)


def test_sizes_cover_every_tile_count():
    assert sorted({frame_tiles(W, H) for W, H in SIZES} & set(range(1, 18))) == list(range(1, 18))


def test_expand_ungrouped_fallback(avg152):
    """A persistent-grid context's expand takes one work entry per workgroup, culled ones among them."""
    vol, cal = avg152
    a = vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=2, persist_wgs=2))
    off = vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=0))
    for W, H in ((TILE * 5, TILE), (TILE * 17, TILE), (17, 33), (203, 157)):
        for name in ("zoomed", "far", "x"):
            cam, rsw = camera(W, H, name)
            p = params(W, H, S, rsw, FLAGS)
            assert a.axis_columns_plan(p, cam)["columns"], (name, W, H)
            got, ref = a.render(p, cam), off.render(p, cam)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, W, H)
    a.close()
    off.close()


@pytest.mark.parametrize("name", list(VIEWS))
@pytest.mark.parametrize("W,H", SIZES)
def test_expand_groups_bitwise(contexts, W, H, name):
    import torch
    forced, off = contexts
    cam, rsw = camera(W, H, name)
    cams = [camera(W, H, name, d)[0] for d in DOLLY]
    p = params(W, H, S, rsw, FLAGS)

    # the tile count this case stands for, from the plan's numbers
    plan = forced[(0, 0)].axis_columns_plan(p, cam)
    n_rect, n_frame = rect_tiles(W, H, plan), frame_tiles(W, H)
    print(f"{name} {W}x{H}: plan {plan}, rectangle tiles {n_rect} of {n_frame}")
    if name == "zoomed":   # the volume overflows the screen: every tile is the rectangle's, none is background
        assert plan["pixels"] == W * H and n_rect == n_frame, (name, W, H, plan)
    else:
        assert 0 < plan["pixels"] <= W * H, (name, W, H, plan)
        if H == TILE:
            assert n_rect is not None and 1 <= n_rect <= n_frame, (name, W, H, plan)
        if name == "far" and H == TILE and W >= 8 * TILE:   # W / 6 + margin + tile rounding < W: background tiles
            assert n_rect < n_frame, (name, W, H, plan)

    ref = off.render(p, cam)
    refs = [off.render(p, c) for c in cams]
    for (wo, fif), a in forced.items():
        for c in [cam] + cams:
            assert a.axis_columns_plan(p, c)["columns"], (name, W, H, wo, fif)
            assert not off.axis_columns_plan(p, c)["columns"]
        if fif == 0:
            got = a.render(p, cam)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (
                "vr_render", name, W, H, wo, int((got != ref).any(axis=-1).sum()))
        out = torch.zeros((len(cams), W, H, 4), dtype=torch.float32, device="cuda:0")
        a.render_batch_device(p, cams, out.data_ptr())
        got = out.cpu().numpy()
        for i in range(len(cams)):
            assert np.array_equal(got[i].view(np.uint32), refs[i].view(np.uint32)), (
                "vr_render_batch", name, W, H, wo, fif, i, int((got[i] != refs[i]).any(axis=-1).sum()))
