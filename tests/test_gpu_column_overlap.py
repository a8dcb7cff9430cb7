"""vr_options.column_overlap on the GPU: a vr_render_batch call's column marches pipelined under its
expand passes.

Only the order of the launches changes, so every frame must equal, bit for bit, the per-frame render
of a context with the column path off (axis_columns = 0).  Every frame of a call has its own camera,
pairwise distinct over the whole pool, so an expand that ran ahead of its march, or read another
frame's slice of the column buffer, shows up as a wrong (another camera's, or a stale) frame.  Every
comparison first asserts through vr_axis_columns_plan that the forced context takes the column path.
"""
import ctypes

import numpy as np
import pytest

import volumerenderingproject_amd as vr
from test_gpu_parity import _tf_n

pytestmark = pytest.mark.gpu

E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
W, H, S = 203, 157, 96
OVERLAPS = [0, 1]   # every vr_options.column_overlap value


def _p():
    return vr.default_params(W, H, S, flags=E | T)


def _pool():
    """40 views along z: ten dollies, from the front and from behind, upright and rolled by 90 degrees
    (pairwise distinct frames in the CPU oracle too; dollies a multiple of the sample step apart are not)."""
    up = tuple(vr.default_camera(W, H).up)
    cams = []
    for z in np.linspace(0.12, 0.95, 10):
        for sign in (1.0, -1.0):
            for u in (up, (1.0, 0.0, 0.0)):
                cams.append(vr.derive_camera((0.0, 0.0, sign * float(z)), u, 2.0, 2.0 * H / W))
    return cams


def _xcams():
    """10 views along x, pairwise distinct and distinct from the pool's (checked with the CPU oracle)."""
    return [vr.derive_camera((x, 0.0, 0.0), u, 2.0, 2.0 * H / W)
            for u in ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0)) for x in (0.2, 0.5, 0.9, 1.2, -0.6)]


def _distinct(frames):
    return len({f.tobytes() for f in frames}) == len(frames)


@pytest.fixture(scope="module")
def ref(avg152):
    """(cameras, frames): the pool and its per-frame renders with the column path off (default TF)."""
    vol, cal = avg152
    cams = _pool()
    with vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=0)) as b:
        frames = [b.render(_p(), cam) for cam in cams]
    for f in frames:
        f.setflags(write=False)
    assert _distinct(frames)
    return cams, frames


def _ctx(avg152, fif=1, ov=1, tf=None):
    vol, cal = avg152
    return vr.VolumeRenderer(vol, cal, tf=tf, device=0,
                             options=vr.default_options(axis_columns=2, frames_in_flight=fif, column_overlap=ov))


def _call(a, cams, fill=0.0, asynchronous=False):
    import torch
    for cam in cams:
        assert a.axis_columns_plan(_p(), cam)["columns"]
    out = torch.full((len(cams), W, H, 4), fill, dtype=torch.float32, device="cuda:0")
    # the fill runs on torch's stream, the call on the context's own non-blocking one: wait for the fill
    # alone -- torch's stream, not the device, so the context's queued calls stay in flight
    torch.cuda.current_stream().synchronize()
    a.render_batch_device(_p(), cams, out.data_ptr(), asynchronous=asynchronous)
    return out


def _same(out, want, what=""):
    got = out.cpu().numpy()
    for i in range(len(want)):
        assert np.array_equal(got[i], want[i]), (what, i, float(np.abs(got[i] - want[i]).max()))


def test_default_is_pipelined():
    assert vr.default_options().column_overlap == 1


@pytest.mark.parametrize("ov", OVERLAPS)
@pytest.mark.parametrize("fif", [0, 1, 3])
def test_chunk_counts(avg152, ref, fif, ov):
    """Calls of 2, 7, 13 and 20 frames: the first chunk alone, a first chunk and one more (full, and
    with a frame over), and four chunks with an uneven tail."""
    cams, frames = ref
    with _ctx(avg152, fif, ov) as a:
        for n, first in ((20, 0), (2, 20), (7, 22), (13, 27), (20, 20)):
            _same(_call(a, cams[first:first + n]), frames[first:first + n], (fif, ov, n))


@pytest.mark.parametrize("ov", OVERLAPS)
def test_back_to_back_asynchronous_calls(avg152, ref, ov):
    """Three asynchronous calls, no synchronisation between them: the column buffer is reused from call
    to call, and no call's marches may overwrite what an earlier call's expands still read."""
    cams, frames = ref
    with _ctx(avg152, 1, ov) as a:
        cuts = ((0, 13), (13, 27), (27, 40))
        outs = [_call(a, cams[lo:hi], asynchronous=True) for lo, hi in cuts]
        a.synchronize()
        for (lo, hi), out in zip(cuts, outs):
            _same(out, frames[lo:hi], (ov, lo))


@pytest.mark.parametrize("ov", OVERLAPS)
def test_tf_change_between_calls(avg152, ref, ov):
    """A 4-interval TF, then the default again, between asynchronous calls: no march runs ahead of the
    classification it has to read."""
    vol, cal = avg152
    cams, frames = ref
    tf4 = _tf_n(4)
    with vr.VolumeRenderer(vol, cal, tf=tf4, device=0, options=vr.default_options(axis_columns=0)) as fresh:
        want4 = [fresh.render(_p(), cam) for cam in cams[:20]]
    assert _distinct(want4 + list(frames[:20]))
    with _ctx(avg152, 1, ov) as a:
        o1 = _call(a, cams[:20], asynchronous=True)
        a.set_transfer_function(tf4)
        o2 = _call(a, cams[:20], asynchronous=True)
        a.set_transfer_function(vr.default_transfer_function())
        o3 = _call(a, cams[:20], asynchronous=True)
        a.synchronize()
        _same(o1, frames[:20], "default")
        _same(o2, want4, "tf4")
        _same(o3, frames[:20], "default again")


def test_options_change_between_calls(avg152, ref):
    """vr_set_options between asynchronous calls: the march's batch (16 samples a batch is not bitwise
    8's under ERT, so that call has its own reference), and column_overlap itself."""
    vol, cal = avg152
    cams, frames = ref
    with vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=0, batch=16)) as b:
        want16 = [b.render(_p(), cam) for cam in cams[1:21]]
    steps = (({"batch": 8}, frames[0:20]), ({"batch": 16}, want16), ({"batch": 8, "column_overlap": 0}, frames[2:22]),
             ({"column_overlap": 1}, frames[3:23]))
    with _ctx(avg152, 1, 1) as a:
        outs = []
        for i, (kw, _) in enumerate(steps):
            o = a.options
            for k, v in kw.items():
                setattr(o, k, v)
            a.set_options(o)
            outs.append(_call(a, cams[i:i + 20], asynchronous=True))
        a.synchronize()
        for i, (out, (_, want)) in enumerate(zip(outs, steps)):
            _same(out, want, i)


@pytest.mark.parametrize("ov", OVERLAPS)
@pytest.mark.parametrize("fif", [1, 3])
def test_caller_stream_ordering(avg152, ref, fif, ov):
    """The caller fills the frames with NaN on its stream, calls asynchronously and reads the frames on
    that stream, with no device-wide synchronise: the call starts after the fill and is complete, on
    the caller's stream, when it returns."""
    import torch
    cams, frames = ref
    st = torch.cuda.Stream(device=0)
    with _ctx(avg152, fif, ov) as a:
        a.set_stream(st.cuda_stream)
        for cam in cams[:20]:
            assert a.axis_columns_plan(_p(), cam)["columns"]
        out = torch.zeros((20, W, H, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            out.fill_(float("nan"))
        a.render_batch_device(_p(), cams[:20], out.data_ptr(), asynchronous=True)
        with torch.cuda.stream(st):
            snap = out.clone()
        st.synchronize()
        assert not bool(torch.isnan(snap).any())
        _same(snap, frames[:20], (fif, ov))
        a.set_stream(0)


@pytest.mark.parametrize("ov", OVERLAPS)
def test_stream_change_between_calls(avg152, ref, ov):
    """vr_set_stream to a new caller stream between two asynchronous calls, the old stream destroyed
    afterwards: the second call's marches and expands follow the first call's on the device."""
    import torch  # noqa: F401  (loads the HIP runtime libvr shares)
    hip = ctypes.CDLL("libamdhip64.so.7")
    cams, frames = ref
    with _ctx(avg152, 1, ov) as a:
        s1, s2 = ctypes.c_void_p(), ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(s1)) == 0
        assert hip.hipStreamCreate(ctypes.byref(s2)) == 0
        a.set_stream(s1.value)
        o1 = _call(a, cams[:20], asynchronous=True)
        a.set_stream(s2.value)
        o2 = _call(a, cams[20:40], asynchronous=True)
        assert hip.hipStreamDestroy(s1) == 0
        o3 = _call(a, cams[10:30], asynchronous=True)
        a.synchronize()
        _same(o1, frames[:20], "first stream")
        _same(o2, frames[20:40], "second stream")
        _same(o3, frames[10:30], "second stream, old one destroyed")
        a.set_stream(0)
        assert hip.hipStreamDestroy(s2) == 0
        _same(_call(a, cams[5:25]), frames[5:25], "own stream")


@pytest.mark.parametrize("ov", OVERLAPS)
def test_mixed_batch(avg152, ref, ov):
    """Views along z and along x alternate: the x frames march on their own in-flight streams between
    the chunks' expands, and the 10 z frames of the 20 make a short chunk, a full one and a tail."""
    vol, cal = avg152
    cams, frames = ref
    xc = _xcams()
    with vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(axis_columns=0)) as b:
        xf = [b.render(_p(), cam) for cam in xc]
    mixed = [c for pair in zip(cams[:10], xc) for c in pair]
    want = [f for pair in zip(frames[:10], xf) for f in pair]
    assert _distinct(want)
    with _ctx(avg152, 1, ov) as a:
        for _ in range(2):
            _same(_call(a, mixed), want, ov)


def test_overlap_off_equals_on(avg152, ref):
    cams, _ = ref
    with _ctx(avg152, 1, 0) as a0, _ctx(avg152, 1, 1) as a1:
        g0, g1 = _call(a0, cams[:20]).cpu().numpy(), _call(a1, cams[:20]).cpu().numpy()
    assert g0.tobytes() == g1.tobytes()
