"""The table of tests/crop_cases.py on the CPU (the numpy restatements only, no GPU): the rows, boxes and
ingredients tests/test_gpu_crop_params.py and test_gpu_random.py hold vr_set_crop_box to are not vacuous.

Conditions on tests/crop_ref.py's frames and on the samples in the volume and in the box, against the numbers
crop_cases.CAUGHT records as literals (measured from the restatement; floors are half of what it gives)."""
import numpy as np
import pytest

import crop_cases as cx
import crop_ref
import field_param_cases as fp
import param_cases as pc
import test_crop_ref as tc

F = np.float32
VPD18 = [(vpd, scale, v) for vpd, scale in pc.VPD for v in cx.CUBE_VPD_VIEWS]
GROUPS = {"blob vpd": cx.vpd_rows, "blob screens": lambda: [r for r in cx.view_rows() if r.label[1] != "vpd"],
          "faces": lambda: cx.blob_face_rows() + cx.cube_rows(),
          "awkward": lambda: [r for n in cx.AWKWARD for r in cx.awkward_rows(n)],
          "deep": lambda: [r for n in pc.DEEP for r in cx.deep_rows(n)]}


def test_the_table_has_the_rows_and_they_are_param_cases_rows():
    """The rows are field_param_cases' (every VPD and SCREENS row in every view, the S = 1 rows, the deep rows,
    the cal_max rows), vpd = 0 is 0 and not quietly 0.1, the S = 1 rows have S == 1, the needles' cells are the
    8-voxel ones, and the table lists every row with every box it is paired with."""
    rows = cx.all_rows()
    labels = [r.label for r in rows]
    assert len(labels) == len(set(labels)) == len(cx.CAUGHT) == 112 and set(labels) == set(cx.CAUGHT)
    assert len(cx.view_rows()) == (len(pc.VPD) + len(pc.SCREENS)) * len(pc.VIEWS) + 4
    assert [r.label[1:] for r in cx.view_rows()] == [l for l, _ in fp.view_rows()]
    zero = [r for r in cx.view_rows() + cx.cube_rows() if r.label[1] == "vpd" and r.label[2:4] == fp.NO_LIGHT_VPD]
    assert len(zero) == len(pc.VIEWS) + 3 and all(r.view.vpd == 0.0 and r.view.oracle_params().viewplane_distance == 0.0
                                                  for r in zero)
    neg = [r for r in cx.vpd_rows() if r.label[2] < 0]
    assert len(neg) == len(pc.VIEWS) and all(r.view.vpd == -0.5 and r.view.scale == -0.2 for r in neg)
    s1 = [r for r in rows if r.label[1] == "s1"]
    assert len(s1) == 4 and all(r.view.S == 1 and r.frame == fp.S1_FRAME for r in s1)
    assert [(r.label[2], r.label[3], r.label[4]) for r in cx.cube_rows()[:18]] == VPD18
    for r in rows:
        assert len(cx.CAUGHT[r.label]) == 1 + len(r.boxes), r.label
        assert r.view.mode == pc.DVR and r.view.shade is None and r.view.bg == pc.DEFAULT_BG
        assert r.frame == (fp.DEEP_FRAME if r.vol in pc.DEEP else r.frame) and r.view.S <= 64
    for name, shape in pc.DEEP.items():
        assert cx.cell_edge(shape) == 8 and cx.cell_edge((4096, 4096, 64)) == 16
        for b in ("deep_cells", "deep_off"):
            lo, hi = cx.deep_box(b, shape)
            a = int(np.argmax(shape))
            assert ((lo[a] % 8 == 0 and hi[a] % 8 == 0) == (b == "deep_cells")) and 0 < lo[a] < hi[a] < shape[a]
    assert cx.AWKWARD_ISOS["special"] == pc.ISO_SPECIAL and len(cx.awkward_rows("special")[0].isos) == 7
    # the ingredient sets: zero transparent the first, the value 0 visible under the second
    assert crop_ref.tf_outside(255.0, cx.tf_of("sdvr", 0))[3] == 0 and crop_ref.tf_outside(255.0, cx.tf_of("sdvr", 1))[3] != 0
    for vol in ("blob", "small", "subnormal"):
        assert crop_ref.cmap_outside(cx.map_of(vol, 0))[3] == 0
    assert crop_ref.cmap_outside(cx.map_of("blob", 1))[3] != 0


def test_fixed_boxes_are_what_the_table_says():
    for shape in (cx.BLOB_SHAPE, cx.CUBE_SHAPE):
        lo, hi = cx.fixed_box("cells", shape)
        assert all(c % 8 == 0 for c in lo + hi) and all(0 < a < b < d for a, b, d in zip(lo, hi, shape))
        lo, hi = cx.fixed_box("roi", shape)
        assert all(c % 8 != 0 for c in lo + hi)
        assert cx.fixed_box("last_z", shape) == ((0.0, 0.0, shape[2] - 1.0), tuple(float(d) for d in shape))
        assert cx.fixed_box("last_x", shape) == ((shape[0] - 1.0, 0.0, 0.0), tuple(float(d) for d in shape))
        lo, hi = cx.fixed_box("thin", shape)
        assert (lo[2], hi[2]) == (13.25, 13.5) and int(lo[2]) == int(hi[2]) and lo[0] < 0 and hi[0] > shape[0]
        lo, hi = cx.fixed_box("poke", shape)
        assert lo[0] < 0 and np.signbit(lo[1]) and lo[1] == 0 and hi[1] > shape[1] and 0 < lo[2] < hi[2] < shape[2]
    assert cx.fixed_box("cells", cx.BLOB_SHAPE) == ((8.0, 8.0, 8.0), (24.0, 32.0, 24.0))
    assert cx.fixed_box("cells", cx.CUBE_SHAPE) == ((8.0, 8.0, 8.0), (24.0, 16.0, 24.0))
    assert cx.fixed_box("roi", cx.BLOB_SHAPE) == ((6.25, 9.5, 4.75), (20.5, 30.25, 19.0))


@pytest.mark.parametrize("group", list(GROUPS))
def test_boxes_catch_what_the_table_records_and_the_derived_ones_bite(group):
    """Per row: the in-volume and in-box sample counts against the table (a fixed box's 0 exactly: a
    draws-nothing pair, whose frame is all background in every mode; otherwise at least half the recorded
    count).  Each derived box changes the frame of every mode that draws with the box off, and still draws --
    but for crop_cases.ISO_MISSES (ISO alone draws nothing) and DEEP_WHOLE (the box holds every sample)."""
    for row in GROUPS[group]():
        s = cx.samples(row)
        assert int(s.inside.sum()) == cx.CAUGHT[row.label][0], row.label
        off = {m: cx.reference(m, 0, row, None)[0] for m in cx.MODES}
        for name in row.boxes:
            bx = cx.box(name, row)
            n, want = int(s.caught(bx).sum()), cx.caught(row, name)
            assert (n == 0) == (want == 0) and n >= want // 2, (row.label, name, n, want)
            if want == 0:
                for m in cx.MODES:
                    f = cx.reference(m, 0, row, bx)[0]
                    assert not cx.draws(f, row) and np.all(f[..., 3] == 1.0), (row.label, name, m)
            if name not in cx.DERIVED:
                continue
            lo, hi = crop_ref.box_arrays(bx)
            assert np.all(lo < hi), (row.label, name, bx)
            for m in cx.MODES:
                if not cx.draws(off[m], row):
                    continue
                f = cx.reference(m, 0, row, bx)[0]
                if row.label in cx.DEEP_WHOLE:
                    assert n == int(s.inside.sum()) and tc.bits_equal(f, off[m]), (row.label, name, m)
                    continue
                assert not tc.bits_equal(f, off[m]), (row.label, name, m)
                assert cx.draws(f, row) == (m != "iso" or (row.label, name) not in cx.ISO_MISSES), (row.label, name, m)
        if row.vol in pc.DEEP and row.label[2:] == ("obl", 1.2):
            assert cx.CAUGHT[row.label] == (0, 0, 0, 0) and not any(cx.draws(f, row) for f in off.values())
        elif row.vol not in ("subnormal", "small"):
            assert all(cx.draws(f, row) for f in off.values()), row.label
        else:   # (EDGES gives the gradients of the two scaled volumes, 2^-72 and less, the weight 0)
            assert [m for m, f in off.items() if not cx.draws(f, row)] == ["scdvr"], row.label


def test_shared_samples_give_crop_refs_frames():
    """The frames built from one evaluation of a row's samples are crop_ref's own, bit for bit, in every mode
    and under both ingredient sets (one row with a light, the one without, a single-sample one)."""
    rows = {r.label: r for r in cx.view_rows()}
    for label in (("blob", "vpd", -0.5, -0.2, "obl"), ("blob", "vpd", 0.0, 0.2, "z"), ("blob", "s1", 0.6, 0.2, "obl")):
        row = rows[label]
        s = cx.samples(row)
        vol, cal, p, cam = s.vol, s.cal, s.p, s.cam
        for bx in (cx.box("roi", row), cx.box("faces", row), None):
            for k in (0, 1):
                own = {"sdvr": crop_ref.sdvr(vol, cal, cx.tf_of("sdvr", k), p, cam, cx.shade_of("sdvr", k), bx)[0],
                       "cdvr": crop_ref.cdvr(vol, cx.map_of("blob", k), p, cam, bx)}
                if k == 0:
                    own["dvr"] = crop_ref.dvr(vol, cal, cx.tf_of("dvr", 0), p, cam, bx)
                    own["scdvr"] = crop_ref.scdvr(vol, cx.map_of("blob", 0), cx.xc.gopa_of(cx.GOPA), p, cam,
                                                  cx.shade_of("scdvr", 0), bx)[0]
                    own["mip"] = crop_ref.mip(vol, cal, p, cam, bx)[0]
                    own["iso"] = crop_ref.iso(vol, p, cam, row.isos[0], cx.ISO_RGB, cx.ISO_SHADE, bx)[0]
                for m, f in own.items():
                    assert tc.bits_equal(cx.reference(m, k, row, bx)[0], f), (label, m, k, bx)


def test_every_fixed_box_catches_in_a_third_of_its_rows():
    """From the table: each fixed box has samples in at least a third of the rows it is paired with; on the 18
    rows VPD x (z, obl, x_back) of the blob cells has them in 16, roi in 15, last_z in 9 and thin in 8, and on
    the same rows of the cube last_z or last_x in 10."""
    rows = cx.all_rows()
    for name in cx.FIXED + ("deep_cells", "deep_off"):
        with_box = [r for r in rows if name in r.boxes]
        n = sum(cx.caught(r, name) > 0 for r in with_box)
        assert len(with_box) >= 10 and 3 * n >= len(with_box), (name, n, len(with_box))
    blob18 = [r for r in cx.vpd_rows() if r.label[4] in cx.CUBE_VPD_VIEWS]
    got = {name: sum(cx.caught(r, name) > 0 for r in blob18) for name in ("cells", "roi", "last_z", "thin")}
    assert len(blob18) == 18 and got == {"cells": 16, "roi": 15, "last_z": 9, "thin": 8}
    cube18 = cx.cube_rows()[:18]
    assert sum(cx.caught(r, "last_z") > 0 or cx.caught(r, "last_x") > 0 for r in cube18) == 10


def test_last_layer_boxes_reach_the_clamp():
    """last_z and last_x on the cube: every caught sample has (int)p + 1 == d on the cut axis, so its upper
    corner is the clamped one; 3714 and 4276 of them over the cube's rows, in 8 rows each, and the frames
    draw in every mode (no face of the cube is empty)."""
    for name, axis, floor, nrows in (("last_z", 2, 1850, 8), ("last_x", 0, 2100, 8)):
        total = rows = 0
        for row in cx.cube_rows():
            if cx.caught(row, name) == 0:
                continue
            s = cx.samples(row)
            c = s.caught(cx.box(name, row))
            i1 = s.P[axis][c].astype(np.int32) + 1
            assert c.any() and np.all(i1 == row.shape[axis]), (row.label, name)
            total += int(c.sum())
            rows += 1
            for m in cx.MODES:
                assert cx.draws(cx.reference(m, 0, row, cx.box(name, row))[0], row), (row.label, name, m)
        print(name, "clamped samples", total, "rows", rows)
        assert total >= floor and rows == nrows, (name, total, rows)


def test_cells_has_samples_exactly_on_its_faces():
    """The axis views put samples exactly on faces of `cells` (a multiple of 8 in float32): kept on lo, dropped
    on hi, as test_crop_ref.test_faces_keep_lo_and_drop_hi; and the box moved by one ulp on either kind of face
    differs in its sample set."""
    on_lo_total = on_hi_total = 0
    for row in cx.blob_face_rows() + cx.cube_rows()[:3]:
        s = cx.samples(row)
        bx = cx.box("cells", row)
        lo, hi = crop_ref.box_arrays(bx)
        keep = crop_ref.points_in_box(s.P, bx)
        on_lo, on_hi = np.zeros(keep.shape, bool), np.zeros(keep.shape, bool)
        for a in range(3):
            others = np.ones(keep.shape, bool)
            for b in range(3):
                if b != a:
                    others &= (s.P[b] >= lo[b]) & (s.P[b] < hi[b])
            on_lo |= (s.P[a] == lo[a]) & others
            on_hi |= (s.P[a] == hi[a]) & others
        assert keep[on_lo & ~on_hi].all() and not keep[on_hi].any(), row.label
        n_lo, n_hi = int((on_lo & ~on_hi & s.inside).sum()), int((on_hi & s.inside).sum())
        if n_lo and n_hi:
            grown = (tuple(np.nextafter(lo, F(-np.inf))), tuple(np.nextafter(hi, F(np.inf))))
            assert crop_ref.points_in_box(s.P, grown).sum() >= keep.sum() + on_hi.sum(), row.label
            shrunk = (tuple(np.nextafter(lo, F(np.inf))), bx[1])
            assert crop_ref.points_in_box(s.P, shrunk).sum() <= keep.sum() - (on_lo & ~on_hi).sum(), row.label
        on_lo_total += n_lo
        on_hi_total += n_hi
    print("cells: samples on lo faces", on_lo_total, "on hi faces", on_hi_total)
    assert on_lo_total >= ON_FACES[0] // 2 and on_hi_total >= ON_FACES[1] // 2


ON_FACES = (324, 471)   # measured: samples of the eight rows above exactly on a lo face (kept) and on a hi face


def test_opaque_zero_sets_leave_no_background():
    """SDVR under zero_visible and CDVR under OPAQUE0 on the vpd rows: the samples outside the box are fog, so
    every pixel whose ray has a sample outside the box or the volume is off the background -- no tile may be
    culled and the clip must not narrow the range; that is every pixel of the frame under the boxes that catch
    nothing, and at least nine in ten under the others -- and the box still changes the frame where it catches
    samples."""
    for row in cx.vpd_rows()[::5]:
        s = cx.samples(row)
        for mode in ("sdvr", "cdvr"):
            off = cx.reference(mode, 1, row, None)[0]
            for name in ("roi", "thin", "slab"):
                f = cx.reference(mode, 1, row, cx.box(name, row))[0]
                fog = ~s.caught(cx.box(name, row)).all(axis=2)
                drawn = fp.drawn(f, row.view.bg)
                assert np.all(drawn[fog]) and 10 * int(fog.sum()) >= 9 * fog.size, (row.label, mode, name)
                if cx.caught(row, name):
                    assert not tc.bits_equal(f, off), (row.label, mode, name)


@pytest.mark.parametrize("seed", fp.RANDOM_SEEDS)
def test_random_boxes(seed):
    """The boxes of test_gpu_random.test_random_views_crop: lo < hi by at least 3 voxels on every cut axis,
    within [-2, d + 2]; a quarter of the axes whole; and at least half of the views of each seed draw under their
    box (the count, and the samples caught over the seed's views, are printed)."""
    from volumerenderingproject_amd import volumes
    vol = volumes.avg152()[0]
    boxes = cx.random_boxes(seed, vol.shape)
    views = fp.random_view_cases(seed)
    assert len(boxes) == len(views) == fp.RANDOM_VIEWS
    whole = 0
    for lo, hi in boxes:
        for a in range(3):
            if (lo[a], hi[a]) == (-5.0, vol.shape[a] + 5.0):
                whole += 1
            else:
                assert -2.0 <= lo[a] and hi[a] <= vol.shape[a] + 2.0 and hi[a] - lo[a] >= 3.0 - 1e-4
    assert 4 <= whole <= 22, whole   # (48 axes at 1/4)
    assert cx.random_boxes(seed, vol.shape) == boxes and cx.random_boxes(seed + 1, vol.shape) != boxes
    drawing = caught = 0
    for view, bx in zip(views, boxes):
        s = cx.Samples(cx.Row(("random",), "avg152", view, (tc.ISO_VALUE,)))
        n = int(s.caught(bx).sum())
        caught += n
        f = s.frame("dvr", 0, bx)[0]
        drawing += bool(fp.drawn(f, view.bg).any())
        assert (n > 0) or not fp.drawn(f, view.bg).any()
    print("seed", seed, "views drawing under their box", drawing, "samples caught", caught)
    assert 2 * drawing >= len(views), (seed, drawing)
    assert caught >= RANDOM_CAUGHT[seed] // 2, (seed, caught)


RANDOM_CAUGHT = {1: 133880, 2: 91726, 3: 177447}   # measured samples in the volume and in the box over the 16 views of a seed
