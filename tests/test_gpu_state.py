"""One long-lived context held to the references through state changes, on the GPU.

tests/state_cases.py's chain: eight transfer functions in turn on ONE context per kind, and under each
the five modes in a seeded order with set_isosurface, set_options (one render field at a time) and
set_stream between them, every frame delivered one of four ways (tests/test_state_cases.py keeps the
script from being vacuous).  A table that survives a change it should not -- class volumes and their
layouts, the corner volume and plane table, the DVR segments, view / axis / frame-list tables per
stream, the visible-tile cache, the column path's gate -- gives a plausible frame of an earlier state;
here it fails the frame's comparison with the reference of the CURRENT state.

Per frame, the project's rules with nothing loosened: VRC, TEST and DVR exact (flags 0) and ESS frames
equal the reference's values (np.array_equal); ERT and ESS | ERT are within ert_bound per channel in
VRC and TEST and within TOL = 1e-4 in DVR; MIP and ISO (SH_KS0: the specular term is exact) equal the
reference under all four flag combinations; alpha is 1.  And every frame, ERT ones too, equals bit for
bit the frame a FRESH one-GPU context -- created with the epoch's TF, given the same options and
isosurface, closed at the epoch's end -- renders with a plain vr_render: a kernel variant is a
function of TF, options and params alone, not of the context's history, its stream or the delivery.
(No option pair is exempt: the fresh context has the long-lived one's options, batch included.)
"""
import time

import numpy as np
import pytest

import param_cases as pc
import state_cases as sc
import volumerenderingproject_amd as vr
from test_gpu_params import TOL, assert_same, ert_bound

pytestmark = pytest.mark.gpu

E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
F = np.float32
TILE = 16

# kind -> (layout options, devices).  group2 is the peer-copy rehearsal on one GPU; its farm tile is 16
# so that both parts render tiles of these small frames (the default 64 would give part 1 none)
KINDS = {
    "defaults": ({}, None),
    "corners3": ({"test_corners": 3}, None),
    "corners1": ({"test_corners": 1}, None),
    "idx64": ({"force_idx64": 1}, None),
    "float_field": ({"dvr_volume": 1}, None),
    "cell_columns": ({"leaf_columns": 0}, None),
    "group2": ({"farm_tile": 16}, [0, 0]),
}


def check_frame(got, want, fresh, step, tf, what):
    """One frame against the reference's exact frame `want` and the fresh context's frame.  `what` is a
    string (pytest prints a string message whole): epoch, TF, mode, view, flags, frame, delivery, stream
    and the last mutation."""
    assert got.shape == want.shape, what
    assert np.all(got[..., 3] == 1.0), f"{what}: alpha is not 1"
    if step.mode in ("mip", "iso") or not (step.flags & T):
        assert_same(got, want, f"{what}: against the reference")
    else:
        err = np.abs(got[..., :3].astype(np.float64) - want[..., :3]).max(axis=(0, 1))
        bound = TOL if step.mode == "dvr" else ert_bound(tf, pc.DEFAULT_BG, 1e-5, step.frame[2])
        assert np.all(err <= bound), f"{what}: ERT frame off the reference by {err}, bound {bound}"
    assert_same(got, fresh, f"{what}: against the fresh context")


class Driver:
    """The long-lived context of one kind, its model, and the device buffers the deliveries write."""

    def __init__(self, kind):
        import torch
        self.torch = torch
        self.kind = kind
        self.layout, self.devices = KINDS[kind]
        self.group = self.devices is not None
        self.model = sc.Model()
        ref = sc.reference("default")
        self.vol, self.cal = ref.vol, ref.cal
        kw = {"devices": self.devices} if self.group else {"device": 0}
        self.r = vr.VolumeRenderer(self.vol, self.cal, options=self.options(), **kw)
        self.fresh = None
        self.streams = {"own": None, "caller1": torch.cuda.Stream(device=0), "caller2": torch.cuda.Stream(device=0)}
        self.on = "own"
        self.bufs = {}
        self.pending = None    # the open async pair's frames: (step, device frame, want, fresh, what, tf)
        self.frames = 0

    def options(self):
        return vr.default_options(**self.layout, **self.model.options)

    def close(self):
        if self.fresh is not None:
            self.fresh.close()
        self.r.set_stream(0)
        self.r.close()

    def buf(self, name, shape):
        key = (name,) + tuple(shape)
        if key not in self.bufs:
            self.bufs[key] = self.torch.empty(shape, dtype=self.torch.float32, device="cuda:0")
            self.torch.cuda.current_stream().synchronize()
        return self.bufs[key]

    def use_stream(self, name):
        if name != self.on:
            st = self.streams[name]
            self.r.set_stream(st.cuda_stream if st is not None else 0)
            self.on = name

    # ---- state changes: the long-lived context, the epoch's fresh one and the model alike ----

    def begin_epoch(self, epoch):
        m = self.model
        m.set_epoch(epoch)
        if epoch:
            self.r.set_transfer_function(m.tf)
        info = self.r.info
        assert info.n_tf == m.n_tf, (self.kind, epoch, m.tf_name)
        assert info.zero_transparent == int(m.zero_transparent), (self.kind, epoch, m.tf_name)
        # the visible tiles follow the TF (the same three queries every epoch: a cached answer of an
        # earlier TF would be returned here): none under all_clear, and never a tile short
        W, H, _ = sc.FRAME_A
        nty = -(-H // TILE)
        for view in sc.VIEW_NAMES:
            case = pc.Case(view, pc.VRC, frame=sc.FRAME_A)
            ids = set(self.r.visible_tiles(case.gpu_params(0), case.gpu_camera(), TILE, TILE).tolist())
            what = f"{self.kind}: epoch {epoch} tf {m.tf_name} visible_tiles of VRC {view}: {sorted(ids)}"
            assert (len(ids) == 0) == (m.tf_name == "all_clear"), what
            want = sc.reference(m.tf_name).frame(case)
            for t in set(range(-(-W // TILE) * nty)) - ids:
                tx, ty = divmod(t, nty)
                blk = want[tx * TILE:(tx + 1) * TILE, ty * TILE:(ty + 1) * TILE]
                assert np.all(blk[..., :3] == np.array(pc.DEFAULT_BG[:3], F)), f"{what}: tile {t} is drawn"
        if self.fresh is not None:
            self.fresh.close()
        self.fresh = vr.VolumeRenderer(self.vol, self.cal, tf=m.tf, device=0, options=self.options())
        self.fresh.set_isosurface(*m.iso)

    def mutate(self, op):
        self.model.apply(op)
        if op[0] == "iso":
            self.r.set_isosurface(*op[1])
            self.fresh.set_isosurface(*op[1])
            got = self.r.isosurface
            assert got[0] == F(op[1][0]) and got[1] == tuple(F(c) for c in op[1][1]), (self.kind, op, got)
        else:
            o = self.options()
            self.r.set_options(o)
            self.fresh.set_options(o)
            assert getattr(self.r.options, op[1][0]) == op[1][1], (self.kind, op)

    # ---- one step ----

    def step(self, st):
        m, r = self.model, self.r
        self.use_stream(st.stream)   # (a pair's second frame carries the first one's stream)
        W, H, _ = st.frame
        views = st.views()
        cases = [m.case(st, v) for v in views]
        whats = [f"{self.kind}: {m.what(st, v)}" for v in views]
        wants = [m.expected(st, v) for v in views]
        params = cases[0].gpu_params(st.flags)
        cams = [c.gpu_camera() for c in cases]
        fresh = [self.fresh.render(params, cam) for cam in cams]
        # the column path's gate follows the TF and the options (asked of the context's own plan)
        for v, cam, what in zip(views, cams, whats):
            plan = r.axis_columns_plan(params, cam)["columns"]
            gate = m.columns(st, v, one_gpu_32bit=not self.group and self.kind != "idx64")
            if gate is not None:
                assert plan == gate, f"{what}: column plan {plan}, the gate says {gate}"
        if st.delivery == "host":
            got = [r.render(params, cams[0])]
        elif st.delivery == "batch":
            out = self.buf("batch", (len(cams), W, H, 4))
            r.render_batch_device(params, cams, out.data_ptr(), asynchronous=True)
            r.synchronize()
            got = list(out.cpu().numpy())
        elif st.delivery == "tiles":
            ids = r.visible_tiles(params, cams[0], TILE, TILE)
            if m.tf_name == "all_clear" and st.mode == "vrc":
                assert len(ids) == 0, f"{whats[0]}: visible tiles {ids}"
            tiles = self.buf("tiles", (max(1, (-(-W // TILE)) * (-(-H // TILE))), TILE * TILE, 3))
            frame = self.buf("frame", (W, H, 4))
            frame.fill_(-7.0)
            self.torch.cuda.current_stream().synchronize()   # (the fill runs on torch's stream, not the context's)
            assert r.render_tile_list(params, cams[0], TILE, TILE, ids, 0, 1, tiles.data_ptr(), rgb=True) == len(ids)
            r.assemble_tile_list(W, H, TILE, TILE, ids, 1, max(1, len(ids)), tiles.data_ptr(), list(pc.DEFAULT_BG),
                                 frame.data_ptr(), rgb=True)
            r.synchronize()
            got = [frame.cpu().numpy()]
        else:   # async_pair: this frame and the next one queued into two device frames, one synchronize
            out = self.buf("pair1" if st.second else "pair0", (W, H, 4))
            r.render_device(params, cams[0], out.data_ptr(), asynchronous=True)
            if not st.second:
                self.pending = [(st, out, wants[0], fresh[0], whats[0], m.tf)]
                return
            self.pending.append((st, out, wants[0], fresh[0], whats[0], m.tf))
            r.synchronize()
            for pst, pout, pwant, pfresh, pwhat, ptf in self.pending:   # each under the state it was queued in
                check_frame(pout.cpu().numpy(), pwant, pfresh, pst, ptf, pwhat)
                self.frames += 1
            self.pending = None
            return
        for g, want, fr, what in zip(got, wants, fresh, whats):
            check_frame(g, want, fr, st, m.tf, what)
            self.frames += 1

    def run(self, epochs):
        for epoch in epochs:
            self.begin_epoch(epoch)
            for op in sc.round(epoch, sc.SEED, sc.GROUP_DELIVERIES if self.group else sc.DELIVERIES):
                if op[0] == "step":
                    self.step(op[1])
                else:
                    self.mutate(op)
            assert self.pending is None, (self.kind, epoch)


@pytest.mark.parametrize("kind", list(KINDS))
def test_one_context_through_the_chain(kind):
    """The whole chain on one context of the kind (see the module's docstring for the rules).

    The two frames of an async pair are compared under the state each was queued in: a set_isosurface
    or set_options between them must not reach the first."""
    t0 = time.perf_counter()
    d = Driver(kind)
    try:
        d.run(range(len(sc.CHAIN)))
    finally:
        d.close()
    print(f"state chain {kind}: {d.frames} frames, {time.perf_counter() - t0:.2f} s")
    assert d.frames >= 8 * 64


def test_test_corners_agree_past_the_plane_table_cutoff():
    """Fresh contexts with test_corners 0, 1, 2 and 3 on blob() under the default TF at frame B (1100
    samples: past the plane table's cutoff, state_cases.FRAME_B): the four exact frames equal each other
    and the oracle, and the four ESS | ERT frames equal each other -- no plane table, all four read the TF."""
    ref = sc.reference("default")
    case = pc.Case("obl", pc.TEST, frame=sc.FRAME_B)
    cam = case.gpu_camera()
    want = ref.frame(case)
    assert pc.non_background(want) >= 40
    exact, fast = {}, {}
    for mode in (0, 1, 2, 3):
        with vr.VolumeRenderer(ref.vol, ref.cal, device=0, options=vr.default_options(test_corners=mode)) as r:
            exact[mode] = r.render(case.gpu_params(0), cam)
            fast[mode] = r.render(case.gpu_params(E | T), cam)
    for mode in (0, 1, 2, 3):
        assert_same(exact[mode], want, ("test_corners", mode, "exact"))
        assert_same(fast[mode], fast[0], ("test_corners", mode, "ess | ert against test_corners 0"))
        assert np.all(fast[mode][..., 3] == 1.0)
    err = np.abs(fast[0][..., :3].astype(np.float64) - want[..., :3]).max(axis=(0, 1))
    assert np.all(err <= ert_bound(ref.tf, case.bg, 1e-5, sc.FRAME_B[2])), err
