"""VR_MODE_MIP on the CPU: the numpy restatement (tests/mip_ref.py) pinned to the DVR restatement
(tests/dvr_ref.py, itself pinned to the oracle) bit for bit, through a step transfer function (no GPU).

With cal_max = 1 and tf = [(0, 1, transparent), (t, 2, opaque red)], t > 0, on a volume of values in
[0, 1], an exact dvr_ref.render pixel is (1, 0, 0) iff one of its in-volume samples has v >= t, that
is iff the ray's maximum m >= t: an opaque sample replaces whatever lies behind it (f * 0 + c * 1),
a transparent one leaves it (f * 1 + c * 0).  So t = m gives red and t = nextafter(m, +inf) does not,
which holds m to the very float.
"""
import numpy as np
import pytest

import dvr_ref
import mip_ref
import volumerenderingproject_amd as vr
from test_dvr_ref import random_volume

F = np.float32
RED = np.array([1.0, 0.0, 0.0], F)


def test_mode_id():
    assert vr.VR_MODE_MIP == 7
    assert vr.VR_MODE_DVR == 6


def step_tf(t):
    return [(0.0, 1.0, (0.0, 0.0, 0.0, 0.0)), (float(t), 2.0, (1.0, 0.0, 0.0, 1.0))]


@pytest.mark.parametrize("case", ["random_oblique", "avg_default"])
def test_maximum_equals_dvr_step_threshold(avg152, oracle_mod, case):
    O = oracle_mod
    if case == "random_oblique":
        vol, (W, H, S), cam = (random_volume() / F(255.0)).astype(F), (30, 22, 50), O.camera_oblique(30, 22)
    else:
        vol, (W, H, S) = (avg152[0] / F(avg152[1])).astype(F), (33, 21, 40)
        cam = O.camera_default(W, H)
    assert vol.min() >= 0.0 and vol.max() <= 1.0
    p = O.params(W, H, S)
    frame, m, hit = mip_ref.render(vol, 1.0, p, cam)
    bg = np.array(list(p.background), F)[:3]
    # a pixel without an in-volume sample is exactly the background; every alpha is 1
    assert (~hit).any() and hit.any()
    assert np.array_equal(frame[~hit][:, :3], np.broadcast_to(bg, ((~hit).sum(), 3)))
    assert np.all(frame[..., 3] == 1.0)
    # cal_max = 1, values in [0, 1] (an ulp above at most): the grey is the maximum, clamped
    assert np.array_equal(frame[hit][:, 0], np.minimum(m[hit], F(1.0)))
    cand = np.argwhere(hit & (m > 0))
    assert len(cand) >= 16
    pick = cand[np.random.default_rng(11).choice(len(cand), 16, replace=False)]
    for x, y in pick:
        t = m[x, y]
        at = dvr_ref.render(vol, 1.0, step_tf(t), p, cam, xs=[x])[0, y, :3]
        above = dvr_ref.render(vol, 1.0, step_tf(np.nextafter(t, F(np.inf))), p, cam, xs=[x])[0, y, :3]
        assert np.array_equal(at, RED), (x, y, t, at)
        assert not np.array_equal(above, RED), (x, y, t, above)
    # the column subset is the frame's columns
    xs = [1, W // 2, W - 1]
    sub = mip_ref.render(vol, 1.0, p, cam, xs=xs)
    assert np.array_equal(sub[0].view(np.uint32), frame[xs].view(np.uint32))
    assert np.array_equal(sub[1].view(np.uint32), m[xs].view(np.uint32)) and np.array_equal(sub[2], hit[xs])


def test_negative_volume_is_black_not_background(oracle_mod):
    O = oracle_mod
    W, H, S = 20, 16, 24
    vol = -(np.random.default_rng(2).random((12, 10, 14), dtype=F) + F(0.5))
    p = O.params(W, H, S)
    frame, m, hit = mip_ref.render(vol, 3.0, p, O.camera_oblique(W, H))
    assert hit.any() and np.all(m[hit] < 0)
    assert np.all(frame[hit][:, :3] == 0.0) and not np.any(np.signbit(frame[hit][:, :3]))
    assert np.all(np.array(list(p.background), F)[:3] != 0.0)   # (so black is not the background)
    assert np.all(np.isneginf(m[~hit]))


def test_non_finite_voxels_read_as_zero(oracle_mod):
    O = oracle_mod
    W, H, S = 20, 16, 24
    rng = np.random.default_rng(4)
    vol = rng.random((12, 10, 14), dtype=F)
    bad = rng.random(vol.shape) < 0.2
    dirty = vol.copy()
    dirty[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(bad.sum()))
    clean = np.where(bad, F(0.0), vol)
    p, cam = O.params(W, H, S), O.camera_oblique(W, H)
    a, b = mip_ref.render(dirty, 1.0, p, cam), mip_ref.render(clean, 1.0, p, cam)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.all(np.isfinite(a[1][a[2]]))
    # a ray through NaN voxels only: every sample reads 0, the pixel is black, not the background
    f, m, hit = mip_ref.render(np.full((12, 10, 14), np.nan, F), 1.0, p, cam)
    assert hit.any() and np.all(m[hit] == 0.0) and np.all(f[hit][:, :3] == 0.0)
