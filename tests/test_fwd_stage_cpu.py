"""CPU tests of the forward / data-gradient oracle (oracle/fwd_stage.py): the plan mirror and the walks of the persistent kernel,
the branch coverage of its cases, the float64 reference, and the bound -- loose enough for a float32 implementation of each
algorithm on every case, tight enough for every planted fault.  No GPU and no library call: tests/test_gpu_fwd_stage.py asserts the
mirror against ``adyolo_conv_fwd_plan``.

Figures of this module (float32 emulation of the case's own algorithm, worst err / bound over the cases of a form): direct 0.147,
stem 0.143, F(2x2) 0.070, F(4x4) 0.069; every planted fault exceeds the bound on every case it applies to."""
import numpy as np
import pytest
import torch

from oracle import fwd_stage as fs


def _p(form, *a, **kw):
    p = fs.plan(form, *a, **kw)
    return tuple(p[k] for k in ("kernel", "ph", "pw", "nsp", "nb", "ncb", "xcd_div", "grid_x", "slots"))


def test_cases_cover_every_named_branch_of_every_form():
    table = fs.coverage()
    assert set(table) == set(fs.FORMS)
    # every persistent body has a walk of at least three patches (k >= 2), and every operand set a multi-patch walk
    for body in fs.PERSISTENT_BODIES:
        assert table["wino4"]["%s:walk3plus" % body], body
    for s in fs.PERSISTENT_SETS:
        assert table["wino4"]["multi_patch_set%d" % s], s
    names = [c["name"] for c in fs.CASES]
    assert len(names) == len(set(names))


def test_coverage_fails_by_name_when_a_branch_is_lost(monkeypatch):
    kept = tuple(c for c in fs.CASES if c["name"] != "wino4_33x2x17_c512_512_e0_dgrad")
    monkeypatch.setattr(fs, "CASES", kept)
    with pytest.raises(AssertionError, match="ring2:cin512"):
        fs.coverage()


def test_older_geometries_stay_in_the_list():
    have = {(c["form"], c["n"], c["h"], c["w"], c["cin"], c["cout"]) for c in fs.cases()}
    for s in ((2, 13, 16, 32, 32), (1, 5, 5, 32, 64), (2, 37, 40, 64, 64), (2, 9, 64, 32, 128), (1, 33, 16, 64, 256), (2, 70, 48, 32, 32)):
        for f in ("direct", "wino2", "wino4"):
            assert (f,) + s in have, (f, s)
    assert ("direct", 3, 20, 32, 64, 96) in have and ("wino2", 3, 20, 32, 64, 96) in have       # three channel blocks: no F(4x4) set 27
    for s in ((2, 70, 4, 64, 64), (3, 133, 8, 64, 128), (2, 260, 3, 64, 64)):
        assert ("wino4",) + s in have
    for s in ((2, 20, 64), (3, 11, 37), (1, 5, 64)):
        assert ("stem",) + s + (8, 32) in have


def test_plan_pinned_against_hand_checked_values():
    # (kernel, patch rows, patch columns, nsp, nb, ncb, xcd_div, grid, slots), worked out by hand from the launchers
    # persistent F(4x4): 16 x 32 patches for W >= 32, 32 x 16 below, one workgroup per CU: 32 slots on each of 8 XCDs
    assert _p("wino4", 29, 33, 65, 64, 64, 1, 0, True) == (5, 16, 32, 261, 2, 1, 8, 256, 32)        # 3 x 3 patches per sample
    assert _p("wino4", 65, 33, 17, 32, 64) == (5, 32, 16, 260, 2, 1, 8, 256, 32)
    assert _p("wino4", 9, 37, 24, 32, 512, 9) == (5, 32, 16, 36, 2, 8, 1, 256, 32)                  # 8 channel blocks: one per XCD
    assert _p("wino4", 129, 129, 3, 64, 64) == (5, 128, 4, 258, 2, 1, 8, 256, 32)                   # narrow: 128 x 4
    assert _p("wino4", 3, 133, 8, 64, 128) == (5, 64, 8, 9, 2, 2, 4, 24, 3)                         # narrow: 64 x 8; 9 patches on 3 slots
    assert _p("wino4", 2, 2400, 64, 32, 32, 31, 3) == (5, 16, 32, 600, 1, 1, 8, 256, 32)
    assert _p("wino4", 1, 5, 5, 32, 64, 9) == (5, 32, 16, 1, 2, 1, 8, 8, 1)                         # seven of eight workgroups return
    # one-patch F(4x4): a bias, float masks, an operand set that is not built, three channel blocks
    assert _p("wino4", 2, 21, 40, 64, 64, 33) == (4, 16, 32, 8, 2, 1, 8, 8, 0)
    assert _p("wino4", 1, 20, 16, 64, 192) == (4, 32, 16, 1, 2, 3, 0, 3, 0)
    assert _p("wino4", 2, 13, 16, 32, 32, 33)[0] == 0 and _p("wino4", 2, 13, 16, 32, 32, 27)[0] == 0  # 32-channel block: bias, float masks
    # F(2x2): 8 x 16 patches
    assert _p("wino2", 1, 20, 40, 32, 256) == (3, 8, 16, 9, 2, 4, 2, 40, 0)                         # 9 patches dealt in twos: 5 x 8
    assert _p("wino2", 3, 9, 17, 32, 192) == (3, 8, 16, 12, 2, 3, 0, 36, 0)
    # direct: 256-pixel tiles; the stem kernel 8 x 32
    assert _p("direct", 2, 19, 45, 64, 96, 27) == (1, 8, 32, 12, 1, 3, 0, 12, 0)
    assert _p("direct", 2, 12, 20, 8, 32, 1, 0, True) == (1, 16, 16, 4, 1, 1, 0, 4, 0)
    assert _p("stem", 3, 5, 70, 8, 32, 33) == (2, 8, 32, 9, 1, 1, 0, 9, 0)
    assert _p("stem", 2, 12, 20, 8, 32)[0] == 0 and _p("direct", 2, 20, 64, 8, 32, 1)[0] == 0       # the entry point takes the other kernel
    # the variants
    v = lambda *a, **k: tuple(fs.plan("wino4", *a, **k)[x] for x in ("tc", "aff", "nb", "bres", "full", "mkm", "narrow"))  # noqa: E731
    assert v(2, 64, 64, 32, 32, 1, 0, True) == (8, 1, 1, 1, 0, 0, 0)
    assert v(2, 64, 64, 32, 32, 31, 3) == (8, 0, 1, 0, 1, 1, 0)
    assert v(2, 64, 66, 32, 32, 31, 3) == (8, 0, 1, 0, 1, 0, 0)
    assert v(2, 64, 64, 32, 32, 15, 1, True) == (8, 1, 1, 0, 0, 0, 0)         # an affine with set 15: the B ring
    assert v(2, 64, 64, 32, 64, 27, 3) == (8, 0, 2, 0, 0, 2, 0)
    assert v(2, 64, 64, 32, 128, 27, 3) == (8, 0, 2, 0, 0, 0, 0)
    assert v(2, 64, 4, 64, 64) == (1, 0, 2, 0, 0, 0, 1) and v(2, 64, 4, 64, 64, 1) == (4, 0, 2, 0, 0, 0, 0)


def test_refusals_of_the_mirror():
    assert fs.plan("wino4", 2, 16, 16, 48, 32)["kernel"] == 0 and fs.plan("wino4", 2, 16, 16, 32, 48)["kernel"] == 0
    assert fs.plan("wino2", 2, 16, 16, 544, 32)["kernel"] == 0 and fs.plan("wino4", 2, 16, 16, 544, 64)["kernel"] == 0
    assert fs.plan("wino4", 2, 13, 17, 32, 64, 31, 3)["kernel"] == 0                  # mask bits: H W Cout / 4 % 64
    assert fs.plan("direct", 2, 16, 16, 32, 32, 1 | 4, 0)["kernel"] == 0              # addend_mask without addend
    assert fs.plan("wino2", 2, 16, 16, 32, 32, 8, 0)["kernel"] == 0                   # stat_aux without statistics
    assert fs.plan_out24(fs.plan("wino4", 2, 16, 16, 48, 32)) == [0] * 24


def test_walks_follow_the_kernels_formula():
    p = fs.plan("wino4", 29, 33, 65, 64, 64, 1, 0, True)
    w = fs.walks(p)
    assert len(w) == 256 and w[0] == [0, 256] and w[4] == [4, 260] and w[5] == [5] and w[8] == [8] and w[255] == [255]
    assert sorted(sp for wk in w for sp in wk) == list(range(261))
    p = fs.plan("wino4", 9, 37, 24, 32, 512, 9)                      # ncb = 8: every XCD walks all patches for its channel block
    w = fs.walks(p)
    assert w[0] == [0, 32] and w[7] == [0, 32] and w[8 * 3 + 5] == [3, 35] and w[8 * 4] == [4]
    p = fs.plan("wino4", 1, 5, 5, 32, 64, 9)
    assert [len(x) for x in fs.walks(p)] == [1, 0, 0, 0, 0, 0, 0, 0]
    assert fs.patch_box(fs.plan("wino4", 29, 33, 65, 64, 64, 1, 0, True), 33, 65, 260) == (28, 32, 64, 1, 1, True)
    # fewer CUs: the walks get longer
    assert fs.plan("wino4", 29, 33, 65, 64, 64, 1, 0, True, ncus=64)["slots"] == 8


def _naive(case, inp):
    """y[n][r][c][o] = sum x'[n][r + ky - 1][c + kx - 1][i] g[o][i][ky][kx], x' = 0 outside the image: plain loops over the taps."""
    x = inp["x"].astype(np.float64)
    if case["affine"]:
        x = x * inp["scale"].astype(np.float64) + inp["shift"].astype(np.float64)
    g = fs.equivalent_filter(case, inp).numpy()
    n, h, w = case["n"], case["h"], case["w"]
    y = np.zeros((n, h, w, case["cout"]))
    xp = np.zeros((n, h + 2, w + 2, case["cin"]))
    xp[:, 1:-1, 1:-1] = x
    for ky in range(3):
        for kx in range(3):
            y += xp[:, ky:ky + h, kx:kx + w] @ g[:, :, ky, kx].T
    return y


@pytest.mark.parametrize("dgrad", [False, True])
@pytest.mark.parametrize("affine", [False, True])
def test_reference_pads_after_the_affine_and_transposes_for_a_data_gradient(affine, dgrad):
    case = fs.make_case("direct", 2, 5, 6, 32, 64, affine=affine, dgrad=dgrad)
    inp = fs.build(case)
    ref, naive = fs.conv64(case, inp).numpy(), _naive(case, inp)
    assert np.abs(ref - naive).max() <= 1e-12 * np.abs(naive).max()
    if dgrad:                                    # the autograd gradient of the layer the filter belongs to
        xin = torch.zeros(2, 64, 5, 6, dtype=torch.float64, requires_grad=True)
        wl = torch.from_numpy(inp["wt"]).double()
        torch.nn.functional.conv2d(xin, wl, None, padding=1).backward(fs.input_nchw(case, inp).contiguous())
        assert np.abs(xin.grad.permute(0, 2, 3, 1).numpy() - naive).max() <= 1e-12 * np.abs(naive).max()


def test_winograd_matrices_give_the_convolution():
    case = fs.make_case("wino4", 2, 13, 18, 32, 32, affine=True)
    inp = fs.build(case)
    ref = fs.conv64(case, inp)
    for form in ("wino2", "wino4"):
        m, bt, at, gm = fs.WINO[form]
        got = fs.winograd_conv(fs.input_nchw(case, inp).contiguous(), fs.equivalent_filter(case, inp), m, bt, at, gm)
        assert float((got - ref).abs().max()) <= 1e-11 * float(ref.abs().max()), form


def test_roundings_follow_the_code():
    c = {cs["name"]: fs.roundings(cs) for cs in fs.cases()}
    assert c["direct_2x19x45_c64_96_e27_float_relu"] == 9 * 64 + 1 + 1
    assert c["stem_3x5x70_c8_32_e1_bias_relu"] == 72 + 1 + 1
    assert c["wino2_3x9x20_c64_128_e1_aff"] == 64 + 11 + 2
    assert c["wino4_29x33x65_c64_64_e1_aff"] == 64 + 12 + 2
    assert c["wino4_33x2x17_c512_512_e0_dgrad"] == 512 + 12
    assert c["wino4_2x21x40_c64_64_e1_bias_relu"] == 64 + 12 + 1


def test_check_wants_every_element_written_and_the_guards_kept():
    case, inp, ref, bnd = fs.prepared("wino4_1x5x5_c32_64_e9")
    ybuf, sbuf = fs.emulated_outputs(case, inp, fs.emulate_conv(case, inp))
    assert fs.check(case, inp, ref, bnd, ybuf, sbuf) < 1.0
    for buf, what in ((ybuf, "y"), (sbuf, "stats")):
        for where in (fs.GUARD - 1, buf.size - fs.GUARD):
            bad = buf.copy()
            bad[where] = 0.0
            with pytest.raises(AssertionError, match="guard words beside %s" % what):
                fs.check(case, inp, ref, bnd, *((bad, sbuf) if what == "y" else (ybuf, bad)))
        bad = buf.copy()
        bad[fs.GUARD + 5] = np.nan
        with pytest.raises(AssertionError, match="not finite"):
            fs.check(case, inp, ref, bnd, *((bad, sbuf) if what == "y" else (ybuf, bad)))
    with pytest.raises(AssertionError, match="no statistics buffer"):
        fs.check(case, inp, ref, bnd, ybuf, None)


@pytest.mark.parametrize("form", fs.FORMS)
def test_emulation_stays_inside_and_every_fault_exceeds_the_bound(form):
    """On every case: the float32 emulation of the case's algorithm passes ``check``; each fault of MUTATIONS planted into it
    fails, wherever it applies."""
    worst = (0.0, None)
    applied = {m: 0 for m in fs.MUTATIONS}
    some = fs.cases(form)
    for cs in some:
        case, inp, ref, bnd = fs.prepared(cs["name"])
        conv32 = fs.emulate_conv(case, inp)
        ratio = fs.check(case, inp, ref, bnd, *fs.emulated_outputs(case, inp, conv32))
        worst = max(worst, (ratio, case["name"]))
        for what in fs.MUTATIONS:
            bufs = fs.mutate(case, inp, conv32, what)
            if bufs is None:
                continue
            applied[what] += 1
            with pytest.raises(AssertionError):
                fs.check(case, inp, ref, bnd, *bufs)
                pytest.fail("%s: %s stays inside the bound" % (case["name"], what))
    print("%s: %d cases, float32 emulation worst err / bound %.3f at %s; faults applied %s" % (form, len(some), worst[0], worst[1], applied))
    assert worst[0] < 1.0
    assert applied["halo_row_from_neighbouring_sample"] == len(some)
    assert applied["halo_column_wrapped_to_neighbouring_row"] == sum(1 for c in some if c["h"] > 1)
    assert applied["halo_row_dropped_at_patch_boundary"] >= 1 and (form == "stem" or applied["shift_on_padding"] >= 1)
    if form != "stem":
        assert applied["addend_mask_shifted"] >= 1
    if form == "wino4":
        assert min(applied["pair0_from_previous_patch"], applied["b_fragments_of_last_group_after_patch_change"]) >= 25
        assert applied["stats_of_second_patch_in_first_slot"] >= 10


@pytest.mark.parametrize("algorithm", ["direct", "wino2", "wino4"])
def test_each_algorithm_stays_inside_the_bound_of_its_form(algorithm):
    """The three float32 emulations on one shape each, through the bound of the form that runs the algorithm."""
    form = algorithm
    case = fs.make_case(form, 3, 19, 37, 64, 64, epi=3, affine=True, relu=True)
    inp = fs.build(case)
    ref, bnd = fs.reference(case, inp), fs.roundings(case) * fs.U * fs.magnitude(case, inp)
    ratio = fs.check(case, inp, ref, bnd, *fs.emulated_outputs(case, inp, fs.emulate_conv(case, inp, algorithm)))
    print("%s: err / bound %.3f" % (algorithm, ratio))
    assert ratio < 1.0


def test_a_fault_no_value_check_can_see():
    """Input rows two or more below the image (row H + 1 onwards of a ragged patch) taken from the next sample instead of zeros: in
    the direct algorithm no stored output depends on them -- bit-identical y.  (The Winograd forms transform all six rows of a tile
    into every output row of it, so there the same fault does reach y, by rounding if the rows are finite and as NaN if they are
    not: which is why the GPU module puts NaN rows behind every sample.)  Only the reads themselves could show it."""
    case = fs.make_case("direct", 3, 13, 20, 32, 32)
    inp = fs.build(case)
    x = torch.from_numpy(inp["x"]).permute(0, 3, 1, 2)
    g = fs.equivalent_filter(case, inp, dtype=torch.float32)
    # the tile is 16 rows: rows 13 (the padding) .. 16; rows 14, 15, 16 hold zeros, or the next sample's first rows
    tall = torch.zeros(3, 32, 13 + 1 + 3, 20)
    tall[:, :, :13] = x
    good = torch.nn.functional.conv2d(tall, g, None, padding=1)[:, :, :13]
    tall[:-1, :, 14:] = x[1:, :, :3]
    faulty = torch.nn.functional.conv2d(tall, g, None, padding=1)[:, :, :13]
    assert torch.equal(good, faulty) and float(tall[:-1, :, 14:].abs().max()) > 100
    m, bt, at, gm = fs.WINO["wino4"]
    w_good = fs.winograd_conv(tall[:, :, :16] * (torch.arange(16) < 13)[None, None, :, None], g, m, bt, at, gm, dtype=torch.float32)[:, :13]
    w_faulty = fs.winograd_conv(tall[:, :, :16], g, m, bt, at, gm, dtype=torch.float32)[:, :13]
    assert not torch.equal(w_good, w_faulty)
