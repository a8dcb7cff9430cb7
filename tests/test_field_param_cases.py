"""The cases of tests/field_param_cases.py on the CPU (the numpy restatements only, no GPU): the rows that
tests/test_gpu_field_params.py and test_gpu_random.py hold VR_MODE_SDVR, CDVR and SCDVR to are not vacuous.

Conditions on the restatements' records (sdvr_ref: shaded, has_normal, ndl; scdvr_ref: lit, ndl, g).  The
floors are about half of what the restatements give on the row they stand beside (the measured extremes
over the views are in the tables' comments), not one global constant."""
import numpy as np
import pytest

import cmap_cases as cc
import field_param_cases as fp
import param_cases as pc
import scdvr_cases as xc
import sdvr_cases as sc

F = np.float32
BACKGROUNDS = [(0.7, -0.25, 1.5, 0.3), (0.0, 0.0, 0.0, 0.0), (1e6, 1e-30, 0.5, 9.0)]   # test_gpu_params.BACKGROUNDS

# rows with a light direction: (kind, a, b) -> floors (SDVR shaded samples, ndl < 0, ndl > 0, pixels where the
# SDVR frame differs from DVR's, SCDVR lit samples, non-background CDVR pixels), each over the seven views.
# Measured minimum over the views:
#   vpd 2.0 / 1.0       1787  840  839  209   4023  209
#   vpd 0.9 / 1.0        611  168  443  156   1281  158    (obl)
#   vpd 3.5 / 1.0        965  426  484  207   2249  207
#   vpd 0.6 / 0.3       5615 2686 2725  209  12503  209    (the camera inside the box)
#   vpd -0.5 / -0.2      879  739  140  203   1697  203
#   screen 2.0 x 0.7    3891 1829 1830  433   8746  433
#   screen 0.8 x 2.6    2828 1356 1356  304   6199  304
#   screen 3.1 x 2.325   696  330  330   88   1579   88
LIGHT_FLOORS = {
    ("vpd", 2.0, 1.0): (890, 420, 420, 100, 2000, 100),
    ("vpd", 0.9, 1.0): (300, 80, 220, 75, 640, 75),
    ("vpd", 3.5, 1.0): (480, 210, 240, 100, 1100, 100),
    ("vpd", 0.6, 0.3): (2800, 1300, 1350, 100, 6200, 100),
    ("vpd", -0.5, -0.2): (440, 370, 70, 100, 850, 100),
    ("screen", 2.0, 0.7): (1900, 900, 900, 215, 4300, 215),
    ("screen", 0.8, 2.6): (1400, 680, 680, 150, 3100, 150),
    ("screen", 3.1, 3.1 * pc.H / pc.W): (350, 165, 165, 44, 790, 44),
}
# vpd = 0, scale 0.2 (SDVR shaded 3392 (obl) to 6784 (x_back), differing pixels 53 to 106; SCDVR lit 7488 to
# 14528, non-background CDVR pixels 117 to 227)
NO_LIGHT_FLOORS = (1700, 26, 3700, 58)
# S = 1: view -> (SDVR shaded samples, SCDVR lit samples); 92 / 225 along z, 53 / 117 along obl, at both distances
S1_FLOORS = {"z": (46, 112), "obl": (26, 58)}
# the random views, seed -> (SDVR shaded samples, SCDVR lit samples) over the 16 views; measured 251721 / 554145,
# 178942 / 386054, 228722 / 494535
RANDOM_FLOORS = {1: (125000, 275000), 2: (89000, 190000), 3: (114000, 245000)}


def records(view):
    """Of a view under the first ingredient sets: SDVR (frame, record), the DVR frame, SCDVR (frame, record) and
    the CDVR frame under the same colour map."""
    s = fp.sdvr_case(view, 0)
    x = fp.scdvr_case(view, 0)
    return sc.reference(s), sc.dvr_reference(s), xc.reference(x), cc.reference(x.base, fp.SCDVR_SETS[0][0])


def differing(a, b):
    return np.any(a != b, axis=-1)


def test_rows_are_param_cases_rows():
    """The rows are param_cases' (every VPD and SCREENS row in every view) and the row without a light is one
    of them; the S = 1 rows have one sample; every ingredient set's coefficients are a bitwise set."""
    labels = [label for label, _ in fp.view_rows()]
    assert len(labels) == len(set(labels)) == (len(pc.VPD) + len(pc.SCREENS)) * len(pc.VIEWS) + 4
    assert fp.NO_LIGHT_VPD in pc.VPD
    assert set(l[:3] for l in labels if fp.has_light(l)) == set(LIGHT_FLOORS)
    assert sum(not fp.has_light(l) for l in labels) == len(pc.VIEWS) + 4
    for label, view in fp.s1_rows():
        assert view.S == 1 and (view.W, view.H) == (pc.W, pc.H)
    for label, view in fp.vpd_rows() + fp.screen_rows():
        assert (view.W, view.H, view.S) == fp.FRAME and view.mode == pc.DVR and view.shade is None


@pytest.mark.parametrize("row", list(LIGHT_FLOORS), ids=lambda r: "%s_%g_%.3g" % r)
def test_rows_with_a_light(row):
    """In every view SDVR shades, essentially every shaded sample has a normal, the two-sided flip is taken
    (ndl < 0) and not taken (ndl > 0), the lit frames differ from the unlit ones: SDVR's from DVR's on every
    pixel with a shaded sample, SCDVR's from CDVR's on every non-background pixel of the latter."""
    n_sh, n_neg, n_pos, n_diff, n_lit, n_drawn = LIGHT_FLOORS[row]
    rows = [(l, v) for l, v in fp.view_rows() if l[:3] == row]
    assert len(rows) == len(pc.VIEWS)
    for label, view in rows:
        (fs, rec), fd, (fx, xrec), fc = records(view)
        sh = rec["shaded"]
        n = int(sh.sum())
        assert n >= n_sh, (label, n)
        assert int(rec["has_normal"][sh].sum()) >= 0.99 * n, label
        ndl = rec["ndl"][sh]
        assert int((ndl < 0).sum()) >= n_neg and int((ndl > 0).sum()) >= n_pos, (label, int((ndl < 0).sum()), int((ndl > 0).sum()))
        diff = differing(fs, fd)
        assert int(diff.sum()) >= n_diff, (label, int(diff.sum()))
        assert np.array_equal(diff, sh.any(axis=2)), label          # (wherever something was shaded, and only there)
        lit = xrec["lit"]
        assert int(lit.sum()) >= n_lit, (label, int(lit.sum()))
        xndl = xrec["ndl"][lit]
        assert (xndl < 0).any() and (xndl > 0).any(), label
        drawn = fp.drawn(fc, view.bg)
        assert int(drawn.sum()) >= n_drawn, (label, int(drawn.sum()))
        assert np.all(differing(fx, fc)[drawn]), label
        assert fs.shape[0] * fs.shape[1] - int(drawn.sum()) >= 40, label   # (and background is left)


def test_row_without_a_light():
    """vpd = 0: every sample lies in the camera plane, e = p(S - 1) - p(0) = 0.  Thousands of shaded samples,
    all with a normal and none with a light (ndl = 0, d = 1); the frames still differ from the unlit ones,
    because SH_N0 has ka + kd = 0.7."""
    n_sh, n_diff, n_lit, n_drawn = NO_LIGHT_FLOORS
    rows = [(l, v) for l, v in fp.vpd_rows() if (l[1], l[2]) == fp.NO_LIGHT_VPD]
    assert len(rows) == len(pc.VIEWS)
    for label, view in rows:
        assert view.vpd == 0.0
        (fs, rec), fd, (fx, xrec), fc = records(view)
        sh, lit = rec["shaded"], xrec["lit"]
        assert int(sh.sum()) >= n_sh and int(lit.sum()) >= n_lit, (label, int(sh.sum()), int(lit.sum()))
        assert np.all(rec["has_normal"][sh]) and np.all(xrec["has_normal"][lit]), label
        assert np.all(rec["ndl"][sh] == 0) and np.all(rec["d"][sh] == 1), label
        assert np.all(xrec["ndl"][lit] == 0) and np.all(xrec["d"][lit] == 1), label
        assert int(differing(fs, fd).sum()) >= n_diff, (label, int(differing(fs, fd).sum()))
        drawn = fp.drawn(fc, view.bg)
        assert int(drawn.sum()) >= n_drawn and np.all(differing(fx, fc)[drawn]), (label, int(drawn.sum()))


def test_single_sample_rows():
    """S = 1: p(S - 1) is p(0).  The one sample of a ray is shaded on 92 (z) and 53 (obl) rays in SDVR, lit on
    225 and 117 in SCDVR; none has a light, and every such pixel differs from its DVR / CDVR pixel."""
    rows = fp.s1_rows()
    assert len(rows) == 4
    for label, view in rows:
        (fs, rec), fd, (fx, xrec), fc = records(view)
        sh, lit = rec["shaded"][..., 0], xrec["lit"][..., 0]
        assert rec["shaded"].shape[2] == 1
        n_sh, n_lit = S1_FLOORS[view.view]
        assert int(sh.sum()) >= n_sh and int(lit.sum()) >= n_lit, (label, int(sh.sum()), int(lit.sum()))
        assert np.all(rec["ndl"][..., 0][sh] == 0) and np.all(rec["d"][..., 0][sh] == 1), label
        assert np.all(xrec["ndl"][..., 0][lit] == 0) and np.all(xrec["d"][..., 0][lit] == 1), label
        assert rec["has_normal"][..., 0][sh].any() and xrec["has_normal"][..., 0][lit].any(), label
        assert np.array_equal(differing(fs, fd), sh), label
        assert np.all(differing(fx, fc)[lit]), label


def test_negative_viewplane_distance_turns_the_light():
    """(-0.5, -0.2): the march axis runs the other way and so does L.  ndl < 0 dominates (982 of 1398 along z;
    at least 60 % in every view), where the camera inside the box at (0.6, 0.3) has the two signs in balance
    (between 46 % and 53 %): a march that ignored the flipped axis in L cannot reproduce the distribution."""
    for view in pc.VIEWS:
        share = {}
        for vpd, scale in ((-0.5, -0.2), (0.6, 0.3)):
            rec = sc.reference(fp.sdvr_case(pc.Case(view, pc.DVR, vpd=vpd, scale=scale), 0))[1]
            ndl = rec["ndl"][rec["shaded"]]
            share[vpd] = float((ndl < 0).sum()) / ndl.size
        assert share[-0.5] >= 0.6 and 0.4 <= share[0.6] <= 0.6, (view, share)
    rec = sc.reference(fp.sdvr_case(pc.Case("z", pc.DVR, vpd=-0.5, scale=-0.2), 0))[1]
    ndl = rec["ndl"][rec["shaded"]]
    assert int((ndl < 0).sum()) >= 900 and ndl.size <= 1500


@pytest.mark.parametrize("bg", BACKGROUNDS, ids=["mixed", "zero", "huge"])
def test_backgrounds(bg):
    """In every mode and under both ingredient sets the reference's undrawn region -- the pixels that are
    background under the default background -- equals the given background, and its drawn pixels do not.
    The first sets leave background (a transparent zero: 240 to 360 drawn pixels on the default screen, 100
    to 156 on the far one), the second ones draw every pixel (TF(0) / C(0) visible: 1728)."""
    import test_gpu_params
    assert BACKGROUNDS == test_gpu_params.BACKGROUNDS
    want = np.array(bg[:3], F)
    rows = fp.background_rows(bg)
    assert [l[1] for l, _ in rows] == list(fp.BG_VIEWS) * 2
    for label, view in rows:
        view_name = label
        plain = pc.Case(view.view, pc.DVR, rsw=view.rsw, rsh=view.rsh)
        assert view.bg == tuple(float(b) for b in bg) and plain.bg == pc.DEFAULT_BG
        for k in range(fp.N_SETS):
            pairs = [(sc.reference(fp.sdvr_case(view, k))[0], sc.reference(fp.sdvr_case(plain, k))[0]),
                     (cc.reference(fp.cdvr_case(view), fp.CDVR_SETS[k]), cc.reference(fp.cdvr_case(plain), fp.CDVR_SETS[k])),
                     (xc.reference(fp.scdvr_case(view, k))[0], xc.reference(fp.scdvr_case(plain, k))[0])]
            for mode, (f, f0) in zip(fp.MODES, pairs):
                assert np.all(np.isfinite(f)) and np.all(f[..., 3] == 1.0), (mode, k, view_name)
                drawn = fp.drawn(f0, pc.DEFAULT_BG)
                n = int(drawn.sum())
                assert (n >= 50 and drawn.size - n >= 1000) if k == 0 else n == drawn.size, (mode, k, view_name, n)
                assert np.all(f[~drawn][:, :3] == want), (mode, k, view_name)
                assert np.all(np.any(f[drawn][:, :3] != want, axis=-1)), (mode, k, view_name)


@pytest.mark.parametrize("vol", list(sc.BLOB_CALS))
def test_fractional_cal_max_changes_the_frames(vol):
    """SDVR classifies v / cal_max: its frame at 200.7 and at 1000.25 differs from the one at 255 on every
    drawn pixel along z (240) and on 344 to 357 along obl.  CDVR reads cal_max through a context's first map
    alone, the grey ramp to float32(cal_max): that frame changes on every drawn pixel (240 and 391), a set
    map's does not."""
    assert sc.volume(vol)[1] == sc.BLOB_CALS[vol] and np.array_equal(sc.volume(vol)[0], sc.volume("blob")[0])
    assert cc.map_of("grey", sc.volume(vol)[1])[1][0] == float(F(sc.BLOB_CALS[vol]))
    for (label, view), floor in zip(fp.cal_rows(), (120, 170)):
        a, b = (sc.reference(fp.sdvr_case(view, 0, v))[0] for v in (vol, "blob"))
        assert int(differing(a, b).sum()) >= floor, (label, int(differing(a, b).sum()))
        assert fp.drawn(a, view.bg).sum() >= 100, label
        ga, gb = (cc.reference(fp.cdvr_case(view, v), "grey") for v in (vol, "blob"))
        assert int(differing(ga, gb).sum()) >= floor, (label, int(differing(ga, gb).sum()))
        sa, sb = (cc.reference(fp.cdvr_case(view, v), "smooth5") for v in (vol, "blob"))
        assert np.array_equal(sa, sb), label
        xa = xc.reference(fp.scdvr_case(view, 0, vol))
        assert int(xa[1]["lit"].sum()) >= 2000, label


@pytest.mark.parametrize("name", list(pc.DEEP))
def test_deep_shapes(name):
    """The needles through param_cases.deep_volume_cases: every mode draws along z, x and y_back at the 1.2
    screen and along obl at the 0.02 screen (1 to 31 non-background pixels, 7 to 18 shaded samples in SDVR, 12
    to 31 lit in SCDVR of which 4 to 12 have G < 1 under EDGES); the obl frame at 1.2 is pure background."""
    assert sc.volume(name)[0].shape == pc.DEEP[name]
    assert np.array_equal(sc.volume(name)[0], pc.shared_reference(name).vol)
    rows = fp.deep_rows()
    assert len(rows) == 5
    for label, view in rows:
        assert (view.W, view.H, view.S) == fp.DEEP_FRAME
        fs, rec = sc.reference(fp.sdvr_case(view, 0, name))
        fc = cc.reference(fp.cdvr_case(view, name), fp.CDVR_SETS[0])
        fx, xrec = xc.reference(fp.scdvr_case(view, 0, name))
        drawn = [int(fp.drawn(f, view.bg).sum()) for f in (fs, fc, fx)]
        lit = xrec["lit"]
        if view.view == "obl" and view.rsw == 1.2:
            assert drawn == [0, 0, 0] and not rec["shaded"].any() and not lit.any(), (name, label, drawn)
            continue
        assert min(drawn) >= 1, (name, label, drawn)
        assert int(rec["shaded"].sum()) >= 4 and int(lit.sum()) >= 6, (name, label)
        assert int((xrec["g"][lit] < 1).sum()) >= 2, (name, label)
        assert not np.array_equal(fx, fc), (name, label)


@pytest.mark.parametrize("seed", fp.RANDOM_SEEDS)
def test_random_views(seed):
    """test_gpu_random's 16 views per seed on avg152: the restatements shade 178,942 to 251,721 samples in
    SDVR and light 386,054 to 554,145 in SCDVR, and every mode's frames draw."""
    import test_gpu_random
    views = fp.random_view_cases(seed)
    assert len(views) == fp.RANDOM_VIEWS
    for v, (W, H, S, pos, up) in zip(views, test_gpu_random.random_views(fp.RANDOM_VIEWS, seed)):
        assert (v.W, v.H, v.S) == (W, H, S) and v.pos_up() == (tuple(pos), tuple(up)) and v.rsw == 2.0
    assert max(v.S for v in views) > 250   # (where the derived ERT bound passes 1e-4)
    shaded = lit = 0
    for v in views:
        frames, ns, nl = fp.random_references(v)
        shaded += ns
        lit += nl
        for mode, f in frames.items():
            assert np.all(np.isfinite(f)) and fp.drawn(f, v.bg).sum() >= 40, (seed, mode, v.key())
    print("seed", seed, "shaded", shaded, "lit", lit)
    assert shaded >= RANDOM_FLOORS[seed][0] and lit >= RANDOM_FLOORS[seed][1], (seed, shaded, lit)
    assert fp.random_ert_bound(64) == 1e-4 < fp.random_ert_bound(319) < 1.4e-4
