"""The fused column march's cases (tests/fused_cases.py) on the CPU, the oracle alone: what
tests/test_gpu_fused_params.py claims of a case -- its tile shape, where its drawn rectangle sits, a tile
with all 256 columns in use, a rolled footprint that leaves lanes unused -- holds for the reference, so no
GPU comparison there passes on a frame that does not exercise what it is named for.
"""
import numpy as np

import fused_cases as fc
import param_cases as pc

F = np.float32
SIDES = ("left", "right", "top", "bottom")
MARGIN = 4


def drawn(e):
    """The reference frame's mask [W, H] of pixels off the case's background."""
    f = fc.reference(e.volume).frame(e.case)
    assert np.all(np.isfinite(f)) and np.all(f[..., 3] == 1.0), e.id
    return np.any(f[..., :3] != np.array(e.case.bg[:3], F), axis=-1)


def all_entries():
    return fc.ENTRIES + fc.batch_entries(33) + fc.living_entries()


def test_leaf_counts_are_the_oracles_and_cover_the_list():
    """nleaf_of is 2^depth of the oracle's octree, and the fused cases render 1, 2, 4, 8, 16, 32, 64, 128 and
    2048 leaves a side; the needles hold an 8 KB leaf map; box16 lies strictly inside its volume; the
    2^k + 1 shapes (leaf maps with an empty half) and a volume that fills the cube are among them."""
    counts = set()
    for name in sorted({e.volume for e in all_entries()}):
        ref = fc.reference(name)
        assert fc.nleaf_of(name) == 1 << ref.octree.depth, name
        if any(e.fused for e in all_entries() if e.volume == name):
            counts.add(fc.nleaf_of(name))
    assert counts >= {1, 2, 4, 8, 16, 32, 64, 128, 2048}, counts
    v = fc.box16()
    assert v.shape == fc.BOX16_SHAPE and fc.nleaf_of("box16") == 16
    assert not (v[0].any() or v[-1].any() or v[:, 0].any() or v[:, -1].any() or v[..., 0].any() or v[..., -1].any())
    assert v.max() <= 255 and v.min() == 0 and np.array_equal(v, np.floor(v)) and len(np.unique(v)) > 100
    shapes = {fc.reference(e.volume).vol.shape for e in fc.ENTRIES if e.fused}
    assert (17, 5, 33) in shapes and (65, 3, 2) in shapes     # 2^k + 1: half of the leaf map is empty
    assert (32, 17, 32) in shapes and (1, 1, 1) in shapes     # x and z fill the cube; a single voxel
    assert int((~np.isfinite(fc.reference("special").vol)).sum()) >= 100


def test_claimed_shapes_and_gates():
    """Every case claimed fused has a shape under the rule, within which the restated pixel formula puts
    no tile over the rule's bound nor the bound over 256; every gate case has no shape or names its reason."""
    for e in all_entries():
        n = fc.nleaf_of(e.volume)
        if e.fused:
            shape = fc.expected_shape(e.case, n)
            assert shape is not None and e.gate is None, e.id
            bound = fc.shape_bound(e.case, n, *shape)
            tc = fc.tile_columns(e.case, n, *shape)
            assert int((tc.n0 * tc.n1).max()) <= bound <= fc.FUSE_COLS, (e.id, shape, bound)
        else:
            assert e.gate, e.id
            if e.gate == "no tile shape fits":
                assert fc.expected_shape(e.case, n) is None, e.id
    reasons = {e.gate for e in all_entries() if not e.fused}
    assert reasons == {"a zero step has no column path", "no tile shape fits", "nothing visible",
                       "TF(0) is visible: no column path", "an oblique view has no column path"}, reasons


def test_every_shape_is_selected():
    """Each of the six shapes by at least three fused cases; the largest and the smallest by every SD_FC
    row (sd_zero's by the rule alone: its frames are cases of the gate)."""
    by_shape = {s: [] for s in fc.LADDER}
    for e in fc.ENTRIES:
        if e.fused:
            by_shape[fc.claimed_shape(e)].append(e.id)
    for s, ids in by_shape.items():
        assert len(ids) >= 3, (s, ids)
    for name in pc.SD_FC:
        got = {fc.expected_shape(e.case, 64) for e in fc.group("march-" + name)}
        assert got == {fc.LADDER[0], fc.LADDER[-1]}, (name, got)
        assert len(fc.group("march-" + name)) == 2 * len(pc.AXIS_VIEWS)
    # the shapes the batch and the living context mix
    assert {fc.claimed_shape(e) for e in fc.batch_entries(33)} == {(16, 16)}
    assert {fc.claimed_shape(e) for e in fc.living_entries()} == {(32, 32), (32, 16), None}


def test_frames_draw_and_march_rows_differ():
    """Every drawn frame has at least 40 non-background pixels (the frames of fewer than 40 pixels: all of
    them; the window that misses the dataset: none; the tiny volumes and the needles 40 like the rest:
    tiny_65x3x2 and the needles seen along their length draw exactly 40), and every non-default SD_FC frame
    differs from the default row's of its view."""
    for e in all_entries():
        n = int(drawn(e).sum())
        assert n >= e.min_drawn, (e.id, n)
        if e.gate == "nothing visible":
            assert n == 0 and e.min_drawn == 0, e.id
        else:   # no floor under 40 but a frame's own pixel count
            assert e.min_drawn == min(40, e.case.W * e.case.H), (e.id, e.min_drawn)
    for scr in fc.MARCH_SCREENS:
        for view in pc.AXIS_VIEWS:
            ref = fc.reference("blob")
            base = ref.frame(fc.march_case("default", scr, view))
            for name in pc.SD_FC:
                if name != "default":
                    f = ref.frame(fc.march_case(name, scr, view))
                    assert int(np.any(f != base, axis=-1).sum()) >= 40, (name, scr, view)
    # the samples-per-ray frames are not each other's either
    frames = [fc.reference("blob").frame(e.case) for e in fc.group("samples") if e.case.view == "z"]
    assert len({f.tobytes() for f in frames}) == len(fc.SAMPLES)


def test_rectangle_positions():
    """A rectangle case has drawn pixels in the first tile column / row (of its claimed shape, and of the
    16 x 16 work tiles) on every side it names and at least one whole tile column / row of background, and
    MARGIN more pixels of it (the cull widens the dataset's projection by 2 pixels), on every other side; the
    nine positions and the single tile are all there."""
    for e in all_entries():
        if e.touch is None:
            continue
        d = drawn(e)
        W, H = d.shape
        P, Q = fc.claimed_shape(e)
        cols, rows = d.any(axis=1), d.any(axis=0)
        first = {"left": cols[:16].any(), "right": cols[(W - 1) // 16 * 16:].any(),
                 "top": rows[:16].any(), "bottom": rows[(H - 1) // 16 * 16:].any()}
        margin = {"left": cols[:min(W, P + MARGIN)].any(), "right": cols[max(0, (W - 1) // P * P - MARGIN):].any(),
                  "top": rows[:min(H, Q + MARGIN)].any(), "bottom": rows[max(0, (H - 1) // Q * Q - MARGIN):].any()}
        for side in SIDES:
            if side in e.touch:
                assert first[side], (e.id, side)
            else:
                assert not margin[side], (e.id, side)
    for fname, _, _, shape in fc.RECT_FRAMES:
        g = fc.group("rect-" + fname)
        assert {fc.claimed_shape(e) for e in g if e.touch is not None and len(e.touch) < 4} == {shape}
        assert len({e.touch for e in g if e.touch is not None}) == 10   # nine positions and the single tile
        assert sum(e.gate == "nothing visible" for e in g) == 1
    assert len({e.touch for e in fc.batch_entries(9)}) == 9
    # the batch's frames are 33 different frames: one stored in another's place would show
    batch = fc.batch_entries(33)
    assert len({fc.reference("cube").frame(e.case).tobytes() for e in batch}) == 33
    assert len({(e.case.W, e.case.H, e.case.S, e.case.rsw, e.case.rsh, e.case.sd, e.case.fc, e.case.bg) for e in batch}) == 1


def test_background_cases_have_culled_tiles():
    for e in fc.group("background"):
        d = drawn(e)
        W, H = d.shape
        clear = [not d[x:x + 16, y:y + 16].any() for x in range(0, W, 16) for y in range(0, H, 16)]
        assert sum(clear) >= 4 and not all(clear), e.id
    assert [tuple(b) for b in fc.BACKGROUNDS] == [e.case.bg for e in fc.group("background")][::2]


def test_full_tile_and_rolled_footprints():
    """The full-tile cases have a tile whose column rectangle is exactly 16 x 16 -- lane 255 marches a
    column -- under a rule's bound of exactly 256.  Every rolled case has a tile whose rectangle has more
    cells than the tile's pixels have distinct columns (lanes that march a column no pixel reads), and its
    right and up have non-zero components of both signs on the fixed axes."""
    for e in fc.group("full"):
        assert fc.claimed_shape(e) == (16, 16) and fc.shape_bound(e.case, 64, 16, 16) == 256, e.id
        tc = fc.tile_columns(e.case, 64, 16, 16)
        assert bool(((tc.n0 == 16) & (tc.n1 == 16)).any()), (e.id, tc.n0.max(), tc.n1.max())
        assert bool(((tc.n0 == 16) & (tc.n1 == 16) & (tc.distinct == 256)).any()), e.id
    rolled = [e for e in all_entries() if e.case.view.startswith("roll")]
    assert len(rolled) >= 18 + 2 + 2
    signs = set()
    for e in rolled:
        cam = e.case.oracle_camera()
        ma = int(np.flatnonzero(np.array(cam.front, F))[0])
        assert np.count_nonzero(np.array(cam.front, F)) == 1 and cam.right[ma] == 0.0 and cam.up[ma] == 0.0, e.id
        comps = [v[a] for v in (cam.right, cam.up) for a in range(3) if a != ma]
        assert all(c != 0.0 for c in comps) and min(comps) < 0.0 < max(comps), (e.id, comps)
        signs.add(tuple(c > 0 for c in comps))
        shape = fc.expected_shape(e.case, 64)
        for P, Q in ([shape] if shape else [(16, 16)]):
            tc = fc.tile_columns(e.case, 64, P, Q)
            assert bool((tc.n0 * tc.n1 > tc.distinct).any()), (e.id, P, Q)
    assert len(signs) >= 2   # both roll signs


def test_shift_moves_the_window_alike():
    """An FCase's shift is top_left += sx right + sy up on the oracle's camera, nothing else; its key
    tells two shifts and two rolls apart (Reference.frame caches by key)."""
    a = fc.FCase("z", frame=fc.FRAME, rsw=1.2)
    b = fc.FCase("z", frame=fc.FRAME, rsw=1.2, shift=(0.25, -0.125))
    ca, cb = a.oracle_camera(), b.oracle_camera()
    for k in ("pos", "front", "right", "up"):
        assert list(getattr(ca, k)) == list(getattr(cb, k))
    for i in range(3):
        assert cb.top_left[i] == F(ca.top_left[i] + 0.25 * ca.right[i] - 0.125 * ca.up[i])
    assert a.key() != b.key()
    rolls = [fc.FCase("r", *fc.roll(axis, deg), frame=fc.FRAME, rsw=0.6) for axis in "zxy" for deg in fc.ROLLS]
    assert len({c.key() for c in rolls}) == 6


def test_avg152_cases():
    assert fc.nleaf_of("avg152") == 128
    assert [fc.claimed_shape(e) for e in fc.group("avg152")] == [(16, 16), (32, 32)]
