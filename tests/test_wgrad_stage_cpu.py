"""CPU tests of the weight-gradient oracle (oracle/wgrad_stage.py): the plan mirror, the branch coverage of its cases, the float64
reference, and the bound -- loose enough for a float32 implementation of each algorithm, tight enough for every planted fault.
No GPU and no library call: tests/test_gpu_wgrad_stage.py asserts the mirror against ``adyolo_wgrad_plan``."""
import numpy as np
import pytest

from oracle import wgrad_stage as ws


def _p(form, *shape):
    p = ws.plan(form, *shape)
    return (p["nsplit"], p["nitems"], p["nseg"], p["seg"], p["last_seg"], p["items_per_split_max"], p["items_per_split_min"])


def test_cases_cover_every_named_branch_of_every_form():
    table = ws.coverage()
    assert set(table) == set(ws.FORMS)
    for form, want in (("wino4", ("several_items_nb1", "several_items_nb2", "several_items_short_last_segment")),
                       ("wino2", ("several_items_nt1", "several_items_nt2", "several_items_ragged", "several_items_affine")),
                       ("direct", ("several_items_ragged",)), ("stem", ("nblk_capped", "chunk_spans_two_samples"))):
        for b in want:
            assert table[form][b], (form, b)
    names = [c["name"] for c in ws.cases()]
    assert len(names) == len(set(names))


def test_older_geometries_stay_in_the_list():
    have = {(c["form"], c["n"], c["h"], c["w"], c["cin"], c["cout"], c["affine"]) for c in ws.cases()}
    for s in ((2, 8, 16, 32, 64, False), (4, 300, 32, 64, 64, True), (6, 132, 16, 256, 256, False), (9, 16, 4, 32, 32, True)):
        assert ("wino4",) + s in have
    for f in ("direct", "wino2"):
        assert (f, 6, 132, 16, 256, 256, False) in have and (f, 2, 21, 19, 96, 32, False) in have
        assert (f, 2, 37, 16, 128, 64, True) in have
    for s in ((2, 20, 64), (3, 11, 37), (1, 5, 64), (5, 3, 6)):
        assert ("stem",) + s + (8, 32, False) in have


def test_plan_pinned_against_hand_checked_values():
    # (nsplit, nitems, nseg, seg, last_seg, items per split max, min), worked out by hand from the three geometry functions
    # F(4x4): runs of 16 columns in pairs, 256 / channel blocks splits
    assert _p("wino4", 18, 16, 16, 256, 256) == (8, 9, 1, 4, 4, 2, 1)          # 18 runs = 9 pairs; 4 x 8 blocks -> 8 splits
    assert _p("wino4", 6, 64, 16, 512, 512) == (2, 6, 2, 8, 8, 3, 3)           # 3 pairs; 16 steps: 2 x (8 + 2) beats 2 x (16 + 2)
    assert _p("wino4", 40, 16, 4, 512, 512) == (2, 5, 1, 4, 4, 3, 2)           # runs of four samples: 10 runs = 5 pairs
    assert _p("wino4", 9, 32, 16, 256, 512) == (4, 5, 1, 8, 8, 2, 1)           # 9 runs = 5 pairs, the last half empty
    assert _p("wino4", 4, 300, 32, 64, 64) == (36, 36, 9, 9, 3, 1, 1)          # the older test's "several items": one each
    assert _p("wino4", 6, 132, 16, 256, 256) == (6, 6, 2, 17, 16, 1, 1)        # likewise
    assert _p("wino4", 5, 68, 16, 512, 512) == (2, 6, 2, 9, 8, 3, 3)           # 17 steps = 9 + 8: 3 x 11 beats 2 x 19
    assert _p("wino4", 12, 16, 16, 256, 480) == (2, 6, 1, 4, 4, 3, 3)          # NB = 1: 15 x 8 = 120 blocks -> 2 splits
    assert _p("wino4", 2, 292, 16, 32, 32) == (9, 9, 9, 9, 1, 1, 1)            # 73 steps: 9 segments (9 + 2 beats 10 + 2), the last of one
    # F(2x2): strips of 16 columns, segments of at least 8 tile rows, 512 / block pairs splits
    assert _p("wino2", 6, 132, 16, 256, 256) == (16, 30, 5, 14, 10, 2, 1)      # 30 items on 16 slabs (not 18)
    assert _p("wino2", 1, 18, 16, 64, 128) == (2, 2, 2, 8, 1, 1, 1)            # 9 tile rows = 8 + 1
    assert _p("wino2", 40, 16, 16, 256, 96) == (21, 40, 1, 8, 8, 2, 1)         # NT = 1: 3 x 8 pairs -> 21 splits
    assert _p("wino2", 1, 6, 5, 32, 32) == (1, 1, 1, 8, 3, 1, 1)               # three tile rows in a segment of eight
    # direct: tiles of 256 pixels, 1024 / channel blocks splits
    assert _p("direct", 6, 132, 16, 256, 256) == (16, 54, 1, 16, 16, 4, 3)     # 6 x 9 tiles on 16 splits
    assert _p("direct", 32, 16, 16, 256, 256) == (16, 32, 1, 16, 16, 2, 2)
    assert _p("direct", 2, 16, 64, 32, 32) == (8, 8, 1, 8, 8, 1, 1)            # TW = 32: tiles of 8 x 32
    # stem: rows of the batch in contiguous runs over min(tiles, 512) workgroups
    p = ws.plan("stem", 4, 1043, 32, 8, 32)
    assert (p["nsplit"], p["nblk"], p["rows"], p["per"], p["used"], p["last_seg"]) == (524, 512, 4172, 9, 464, 5)
    p = ws.plan("stem", 5, 3, 6, 8, 32)
    assert (p["nsplit"], p["nblk"], p["per"], p["used"]) == (5, 5, 3, 5)
    assert ws.plan_out8(ws.plan("stem", 4, 1043, 32, 8, 32)) == [524, 4172, 1, 9, 1, 64, 512, 1]
    assert ws.plan_out8(ws.plan("wino4", 18, 16, 16, 256, 256)) == [8, 9, 1, 4, 2, 16, 0, 1]


def test_plan_refusals():
    for shape in ((2, 10, 16, 32, 32), (2, 4, 16, 32, 32), (2, 16, 24, 32, 32), (2, 16, 12, 32, 32), (2, 16, 16, 48, 32)):
        assert not ws.plan("wino4", *shape)["supported"], shape
    assert not ws.plan("wino4", 64, 512, 64, 256, 256)["supported"]            # 2 GiB: nothing is launched at that size
    assert ws.plan("wino4", 63, 512, 64, 256, 256)["supported"]
    assert not ws.plan("wino2", 2, 16, 16, 48, 32)["supported"] and not ws.plan("stem", 2, 16, 16, 8, 64)["supported"]
    assert ws.plan_out8(ws.plan("wino4", 2, 10, 16, 32, 32)) == [0] * 8


def _naive(case, inp):
    """dw[co][ci][ky][kx] = sum dy[n][y][x][co] * x'[n][y + ky - 1][x + kx - 1][ci], x' = 0 outside the image: plain loops."""
    n, h, w, cin, cout = (case[k] for k in ("n", "h", "w", "cin", "cout"))
    x = inp["x"].astype(np.float64)
    if case["affine"]:
        x = x * inp["scale"].astype(np.float64) + inp["shift"].astype(np.float64)
    dy = inp["dy"].astype(np.float64)
    dw = np.zeros((cout, case["cin_real"], 3, 3))
    for s in range(n):
        for y in range(h):
            for xx in range(w):
                for ky in range(3):
                    for kx in range(3):
                        yy, xc = y + ky - 1, xx + kx - 1
                        if 0 <= yy < h and 0 <= xc < w:
                            dw[:, :, ky, kx] += np.outer(dy[s, y, xx], x[s, yy, xc, :case["cin_real"]])
    return dw


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 6, 32, 32, 32), (1, 3, 4, 8, 32, 7)])
def test_reference_pads_after_the_affine(shape, affine):
    case = ws.make_case("direct", *shape[:5], affine=affine, cin_real=shape[5])
    inp = ws.build(case)
    ref, naive = ws.reference(case, inp), _naive(case, inp)
    assert ref.shape == naive.shape
    assert np.abs(ref - naive).max() <= 1e-12 * np.abs(naive).max()
    if affine:                                  # the other order is a different number: the shift would reach the border taps
        assert np.abs(ws.reference(case, inp, pad_value_shift=True) - naive).max() > 1e-3 * np.abs(naive).max()


def test_winograd_matrices_give_the_convolution():
    """The documented algorithm with the module's matrices, in float64, is the weight gradient: S is built from the right ones."""
    case = ws.make_case("wino4", 2, 12, 16, 32, 32, affine=True)
    inp = ws.build(case)
    ref = ws.reference(case, inp)
    for form in ("wino2", "wino4"):
        m, bt, am, g = ws.WINO[form]
        got = ws.winograd_wgrad(ws._affine64(case, inp), ws._dy64(inp), m, bt, am, g).numpy()
        assert np.abs(got - ref).max() <= 1e-11 * np.abs(ref).max(), form


EMULATED = [("direct", ws.make_case("direct", 3, 19, 21, 32, 32, affine=True)),
            ("direct", ws.make_case("stem", 3, 11, 37, 8, 32, cin_real=7)),
            ("wino2", ws.make_case("wino2", 3, 19, 21, 32, 64, affine=True)),
            ("wino2", ws.make_case("wino2", 2, 40, 16, 32, 32)),
            ("wino4", ws.make_case("wino4", 3, 24, 16, 32, 64, affine=True)),
            ("wino4", ws.make_case("wino4", 5, 16, 4, 32, 32, cin_real=10))]


@pytest.mark.parametrize("algorithm,case", EMULATED, ids=[c["name"] for _, c in EMULATED])
def test_bound_holds_for_a_float32_implementation(algorithm, case):
    inp = ws.build(case)
    ref, bnd = ws.reference(case, inp), ws.bound(case, inp)
    ratio = ws.check(case, ref, bnd, ws.emulate(case, inp, algorithm))
    print("%s by %s: err / bound %.3f" % (case["name"], algorithm, ratio))
    assert ratio < 1.0


def test_check_wants_every_element_written_and_the_guards_kept():
    case, inp, ref, bnd = ws.prepared("wino2_1x6x5_c32_32")
    good = ws.new_dw_buffer(case)
    good[ws.GUARD:-ws.GUARD] = ref.astype(np.float32).reshape(-1)
    assert ws.check(case, ref, bnd, good) < 1.0
    for where in (ws.GUARD - 1, good.size - ws.GUARD):
        bad = good.copy()
        bad[where] = 0.0
        with pytest.raises(AssertionError, match="guard"):
            ws.check(case, ref, bnd, bad)
    bad = good.copy()
    bad[ws.GUARD + 5] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        ws.check(case, ref, bnd, bad)


@pytest.mark.parametrize("form", ws.FORMS)
def test_every_mutation_exceeds_the_bound(form):
    """Every case is caught by the three row mutations; the affine and the padded-channel mutation on every case they apply to."""
    applied = {m: 0 for m in ws.MUTATIONS}
    for cs in ws.cases(form):
        case, inp, ref, bnd = ws.prepared(cs["name"])
        for what in ws.MUTATIONS:
            buf = ws.mutate(case, inp, ref, what)
            if buf is None:
                assert what in ("shift_on_padding", "write_padded_channels")
                continue
            applied[what] += 1
            with pytest.raises(AssertionError):
                ws.check(case, ref, bnd, buf)
                pytest.fail("%s: %s stays inside the bound" % (case["name"], what))
    assert all(applied[m] == len(ws.cases(form)) for m in ws.MUTATIONS[:3])
    assert applied["write_padded_channels"] >= 1 and (form == "stem" or applied["shift_on_padding"] >= 1)


def test_roundings_follow_the_plan():
    c = {cs["name"]: ws.roundings(cs) for cs in ws.cases()}
    assert c["direct_6x132x16_c256_256"] == 4 * 64 + 5
    assert c["stem_4x1043x32_c8_32_real7"] == 3 * 32 + 5
    assert c["wino2_6x132x16_c256_256"] == 2 * 14 * 8 + 10
    assert c["wino4_6x64x16_c512_512_aff"] == 3 * 8 * 8 + 13 + 2
    assert max(c.values()) < 1024
