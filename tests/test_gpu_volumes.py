"""Volumes off the beaten path on the GPU: dimensions smaller than a brick, a macro cell or a leaf-column
mask, a needle 1500 voxels long, voxels that are NaN, infinite, negative, fractional, subnormal or above
cal_max, and the gate that keeps VR_MODE_DVR's byte copy.  References and cases: tests/param_cases.py;
rules: tests/test_gpu_params.py (VR_MODE_MIP and VR_MODE_ISO: check_flags_bitwise, bitwise in every flag
combination; ISO's isovalues: param_cases.ISO_*).

VRC on a volume with non-finite voxels is held to the closed-form octree (x > 0 ? x : 0 per leaf): the
literal tree's search does not terminate on a NaN leaf.
"""
import numpy as np
import pytest

import param_cases as pc
import volumerenderingproject_amd as vr
from param_cases import DVR, ISO, MIP, TEST, VRC, Case
from test_gpu_params import assert_same, check_flags, check_flags_mip, check_mode

pytestmark = pytest.mark.gpu

F = np.float32

TINY_CONTEXTS = [(VRC, {"axis_columns": 0}), (VRC, {"axis_columns": 2}), (TEST, {"test_corners": 0}),
                 (TEST, {"test_corners": 2}), (DVR, {"dvr_volume": 0}), (DVR, {"dvr_volume": 1}),
                 (MIP, {"dvr_volume": 0}), (MIP, {"dvr_volume": 1}),
                 (ISO, {"dvr_volume": 0}), (ISO, {"dvr_volume": 1})]


@pytest.mark.parametrize("shape", list(pc.TINY), ids=lambda s: "x".join(map(str, s)))
def test_tiny_volumes(shape):
    """(ISO at the volume's median: d_a = 1 has no gradient on that axis, (1, 1, 1) none at all)"""
    ref = pc.Reference(pc.tiny_volume(shape), 255.0)
    frame = (pc.TW, pc.TH, pc.TS)
    iso = float(np.median(ref.vol))
    for mode, opts in TINY_CONTEXTS:
        with vr.VolumeRenderer(ref.vol, ref.cal, device=0, options=vr.default_options(**opts)) as r:
            info = r.info
            assert tuple(info.dim) == shape
            assert info.octree_depth == ref.octree.depth, (shape, opts)
            assert info.longest_dimension == ref.octree.longest_dimension, (shape, opts)
            for view in ("z", "x", "y_back", "obl"):
                case = Case(view, mode, rsw=pc.TINY[shape], frame=frame, iso=iso)
                check_mode(r, ref.frame(case), case, (shape, mode, opts, view))


@pytest.mark.parametrize("name", ["special", "special200", "special_tf0"])
def test_special_voxels(name):
    """special_tf0: under the default TF a NaN leaf classified as NaN and one classified as the 0 it
    reads as both land in class 0; with the class of 0 visible they differ."""
    import torch
    ref = pc.shared_reference(name)
    assert not ref.literal
    with vr.VolumeRenderer(ref.vol, ref.cal, tf=ref.tf, device=0) as r, \
            vr.VolumeRenderer(ref.vol, ref.cal, tf=ref.tf, device=0, options=vr.default_options(dvr_volume=1)) as rf:
        for view in pc.VIEWS:
            for mode in (VRC, TEST, DVR):
                case = Case(view, mode)
                exact = check_flags(r, ref.frame(case), case, (name, mode, view))
                if mode == DVR:
                    assert_same(check_flags(rf, ref.frame(case), case, (name, "float", view)), exact, (name, view))
            # MIP: a pixel carries a voxel's value itself (1e30 and 3.4e38 clamp to 1, 1e-40 is a subnormal
            # maximum's contribution, -1e30 a cell minimum whose magnitude sets the bound's margin)
            case = Case(view, MIP)
            exact = check_flags_mip(r, ref.frame(case), case, (name, "mip", view))
            assert_same(check_flags_mip(rf, ref.frame(case), case, (name, "mip float", view)), exact, (name, view))
            # ISO: the threshold of the cell bounds anywhere from below every voxel to 1e30, where the
            # gradient's len2 overflows (tests/test_param_cases.py)
            # (the mode reads neither cal_max nor the TF: one reference serves the three names)
            for iso in pc.ISO_SPECIAL:
                case = Case(view, ISO, iso=iso)
                want = pc.shared_reference("special").frame(case)
                exact = check_mode(r, want, case, (name, "iso", iso, view))
                assert_same(check_mode(rf, want, case, (name, "iso float", iso, view)), exact, (name, iso, view))
        out = torch.empty((ref.vol.size, 7), dtype=torch.float32, device="cuda:0")
        r.point_cloud_device(out.data_ptr())
        want = pc.oracle.point_cloud(ref.vol, ref.cal, ref.otf)
        assert_same(out.cpu().numpy()[:, 3:], want[:, 3:], (name, "point cloud colours"))
    # a volume with fractional or out-of-range voxels keeps no byte copy (built with the first DVR
    # frame): two contexts that rendered the same DVR frame hold the same device memory
    case = Case("obl", DVR)
    with vr.VolumeRenderer(ref.vol, ref.cal, tf=ref.tf, device=0) as a, \
            vr.VolumeRenderer(ref.vol, ref.cal, tf=ref.tf, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for r in (a, b):
            assert_same(r.render(case.gpu_params(0), case.gpu_camera()), ref.frame(case), (name, "fresh"))
        assert a.info.device_bytes == b.info.device_bytes


@pytest.mark.parametrize("name", list(pc.DEEP))
def test_deep_shapes_dvr_mip(name):
    """A needle 1500 voxels long: 188 cells along one axis and one across, so every ray that meets it
    crosses a cell in a sample or two -- and the oblique rays of the 1.2 screen step over it (a frame
    of background through the march, not through the cull)."""
    ref = pc.shared_reference(name)
    for dvr_volume in (0, 1):
        with vr.VolumeRenderer(ref.vol, ref.cal, device=0, options=vr.default_options(dvr_volume=dvr_volume)) as r:
            assert tuple(r.info.dim) == pc.DEEP[name]
            for mode in (DVR, MIP):
                for case in pc.deep_volume_cases(mode):
                    check_mode(r, ref.frame(case), case, (name, dvr_volume, mode, case.view, case.rsw))


@pytest.mark.parametrize("name", list(pc.DEEP))
def test_deep_shapes_iso(name):
    """The needles at their median: a surface met by one to 17 rays of the tiny frame, cells crossed in
    a sample or two from the ray's first sample on (the threshold is fixed), and the frame of
    background along obl."""
    ref = pc.shared_reference(name)
    for dvr_volume in (0, 1):
        with vr.VolumeRenderer(ref.vol, ref.cal, device=0, options=vr.default_options(dvr_volume=dvr_volume)) as r:
            for case in pc.deep_volume_cases(ISO, iso=pc.ISO_DEEP):
                check_mode(r, ref.frame(case), case, (name, dvr_volume, "iso", case.view, case.rsw))


def test_subnormal_voxels():
    """Every voxel a subnormal (k * 2^-140): vr_api.h's "every operation rounded on its own" holds down
    there too -- a march that flushed subnormals on a load, in a lerp or in a compare would render the
    all-zero volume's frame (tests/test_param_cases.py: a different one).  The cells' relative margin
    rounds to 0 at these magnitudes; ESS == exact in both modes says no lerp passed its cell's maximum."""
    ref = pc.shared_reference("subnormal")
    for dvr_volume in (0, 1):
        with vr.VolumeRenderer(ref.vol, pc.SUBNORMAL_CAL, device=0,
                               options=vr.default_options(dvr_volume=dvr_volume)) as r:
            for view in ("z", "x", "obl"):
                case = Case(view, DVR)
                check_flags(r, ref.frame(case), case, ("subnormal", dvr_volume, "dvr", view))
                case = Case(view, MIP)
                got = check_flags_mip(r, ref.frame(case), case, ("subnormal", dvr_volume, "mip", view))
                assert pc.non_background(got) >= 40
                # ISO at 128 * 2^-140: the blob's surface, and a gradient whose squares underflow: no
                # normal on any hit (tests/test_param_cases.py)
                case = Case(view, ISO, iso=pc.ISO_SUBNORMAL)
                got = check_mode(r, ref.frame(case), case, ("subnormal", dvr_volume, "iso", view))
                assert pc.non_background(got) >= 40


def test_small_voxels_iso():
    """Every voxel k * 2^-72, a normal float32, and len2 a non-zero subnormal on every hit: the normal
    is -g / sqrt(len2) with the correctly rounded square root of a subnormal and an IEEE division, and
    differs from the unscaled blob's on most rays (tests/test_param_cases.py) -- a device that flushed
    len2 or took the root as of a normal input renders another frame.  No voxel but 0 is an integer, so
    neither context keeps a byte copy."""
    ref = pc.shared_reference("small")
    bytes_ = []
    for dvr_volume in (0, 1):
        with vr.VolumeRenderer(ref.vol, pc.SMALL_CAL, device=0,
                               options=vr.default_options(dvr_volume=dvr_volume)) as r:
            for view in ("z", "x", "obl"):
                case = Case(view, ISO, iso=pc.ISO_SMALL)
                got = check_mode(r, ref.frame(case), case, ("small", dvr_volume, view))
                assert pc.non_background(got) >= 40
            bytes_.append(r.info.device_bytes)
    assert bytes_[0] == bytes_[1]


GATE = [(255.0, True), (255.5, False), (256.0, False), (-1.0, False), (-0.0, True), (np.nan, False)]


@pytest.mark.parametrize("value,kept", GATE, ids=[repr(v) for v, _ in GATE])
def test_dvr_byte_copy_gate(value, kept):
    """One voxel decides: the byte copy is lossless only for integers 0..255 (-0.0 is 0)."""
    vol = pc.blob()
    vol[10, 12, 9] = F(value)
    ref = pc.Reference(vol, 255.0, literal=False)
    with vr.VolumeRenderer(vol, 255.0, device=0) as a, \
            vr.VolumeRenderer(vol, 255.0, device=0, options=vr.default_options(dvr_volume=1)) as b:
        for view in ("z", "obl"):
            case = Case(view, DVR)
            want = ref.frame(case)
            for r in (a, b):
                assert_same(r.render(case.gpu_params(0), case.gpu_camera()), want, (value, view))
        # (the copy is built with the first DVR frame) kept: n + 64 bytes more than the float-only context
        assert a.info.device_bytes - b.info.device_bytes == (vol.size + 64 if kept else 0)
