"""CPU: the cases, references, checker and emulation of the implicit-GEMM convolution's tests (oracle/conv_gemm_stage.py;
tests/test_gpu_conv_gemm_stage.py runs ``adyolo_conv_gemm`` against them on the GPU).  The case list holds every form of every
mode and the edges listed below; the float64 tap-loop references equal torch's float64 convolution and its two gradients; the
float32 emulation of the staging passes ``check`` on every run, and with one planted fault it does not."""
import functools

import numpy as np
import pytest
import torch

from oracle import conv_gemm_stage as cs

# the forms the shapes of the list were classified into by hand (mode 0 / 1 / 2): the mirror must say the same
CLASSIFIED = {
    (2, 9, 4, 32, 64, 3, 3, 1, 1, 1, 1): ("GA", "GA", "fastp"),
    (3, 7, 5, 64, 68, 3, 3, 1, 1, 1, 1): ("GA", "div+general", "div"),
    (2, 37, 1, 32, 32, 3, 1, 1, 1, 1, 0): ("GA", "GA", "fastp"),
    (1, 1, 40, 32, 4, 1, 3, 1, 1, 0, 1): ("GA", "div+general", "div"),
    (2, 10, 6, 32, 64, 3, 3, 2, 2, 1, 1): ("GA", "carry", "div"),
    (2, 9, 8, 64, 32, 3, 3, 1, 2, 1, 1): ("GA", "carry", "fastp"),
    (2, 11, 7, 32, 32, 1, 1, 2, 2, 0, 0): ("GA", "carry", "div"),
    (2, 12, 9, 32, 64, 3, 3, 3, 2, 0, 1): ("GA", "carry", "div"),
    (2, 6, 6, 16, 16, 2, 2, 1, 1, 1, 1): ("div+descriptor", "div+descriptor", "div"),
    (2, 6, 6, 16, 48, 2, 2, 2, 2, 0, 0): ("div+descriptor", "div+descriptor", "div"),
    (1, 20, 16, 8, 64, 7, 7, 1, 2, 3, 3): ("div+general", "carry", "fastp"),
    (2, 8, 4, 48, 40, 3, 3, 1, 1, 1, 1): ("div+general", "div+general", "fastp"),
    (2, 9, 5, 12, 20, 3, 3, 2, 1, 1, 1): ("div+general", "div+general", "div"),
    (3, 13, 3, 4, 4, 1, 1, 1, 1, 0, 0): ("div+general", "div+general", "div"),
    (1, 16, 8, 32, 132, 3, 3, 1, 1, 1, 1): ("GA", "div+general", "fastp"),
    (2, 5, 5, 32, 32, 3, 3, 1, 1, 2, 2): ("GA", "GA", "div"),
    (5, 5, 5, 32, 32, 3, 3, 1, 1, 1, 1): ("GA", "GA", "div"),
    (2, 33, 2, 32, 32, 3, 3, 1, 2, 1, 1): ("GA", "carry", "fastp"),
    (2, 3, 64, 32, 32, 1, 3, 1, 1, 0, 1): ("GA", "GA", "div"),
    (2, 2, 16, 32, 32, 3, 3, 1, 1, 1, 1): ("GA", "GA", "fastp"),
}


def _label(case, mode):
    pixel, filt = cs.form_of(case, mode)
    return pixel if mode == 2 or pixel in ("GA", "carry") else pixel + "+" + filt


def test_plan_hand_worked_values():
    c = (2, 9, 4, 32, 64, 3, 3, 1, 1, 1, 1)                       # Ho x Wo = 9 x 4: 72 output pixels
    assert cs.plan_row(c, 0) == [72, 64, 288, 288, 1, 6, 1, 0]
    assert cs.plan_row(c, 1) == [72, 32, 576, 576, 1, 6, 1, 0]
    assert cs.plan_row(c, 2, 1) == [64, 288, 72, 96, 1, 0, 0, 1]   # 72 pixels are no whole number of K tiles: no bit 0
    p = cs.plan(c, 2, 2)
    assert (p["klen"], p["splits"], p["last"]) == (64, 2, 8)
    for s in (3, 7, 64):
        p = cs.plan(c, 2, s)
        assert (p["klen"], p["splits"], p["last"]) == (32, 3, 8)
    assert cs.plan(c, 0, 7)["splits"] == 1 and cs.plan(c, 2, 0)["splits"] == 1        # splits only count in mode 2, and < 1 is 1
    c = (2, 3, 64, 32, 32, 1, 3, 1, 1, 0, 1)                      # 384 pixels: whole K tiles, dy may take bit 0 (the kernel does not)
    assert cs.plan_row(c, 2, 3) == [32, 96, 384, 128, 3, 1, 0, 0]
    c = (2, 10, 6, 32, 64, 3, 3, 2, 2, 1, 1)                      # strided data gradient: carried triple, no descriptor gather
    assert cs.plan_row(c, 1) == [120, 32, 576, 576, 1, 2, 1, 0]
    # the 2^29 switch of the descriptor gather: source floats + (KH Ws + KW) Cs must stay below 2^29.  Samples of 2^17 floats:
    # 4095 of them are the last GA batch; at 4096 a forward launch takes the carried triple, which no small shape reaches
    for mode, (cin, cout) in ((0, (128, 4)), (1, (4, 128))):
        p = cs.plan((4095, 16, 64, cin, cout, 3, 3, 1, 1, 1, 1), mode)
        assert (p["fastg"], p["pixel"], p["filter"]) == (6, "GA", "descriptor")
        p = cs.plan((4096, 16, 64, cin, cout, 3, 3, 1, 1, 1, 1), mode)
        assert (p["fastg"], p["pixel"], p["filter"]) == (2, "carry", "descriptor")
    c = (2, 1, 16, 8, 12, 1, 3, 1, 1, 0, 1)                       # Wo = 16 divides 32, but Ho = 1 < 2
    assert cs.plan(c, 2)["fastp"] == 0 and cs.plan((2, 2, 16, 32, 32, 3, 3, 1, 1, 1, 1), 2)["fastp"] == 1


def test_forms_are_the_classified_ones_and_every_feasible_form_occurs():
    for case, want in CLASSIFIED.items():
        assert case in cs.CASES
        assert tuple(_label(case, m) for m in cs.MODES) == want, case
    for mode in cs.MODES:
        have = {cs.form_of(c, mode) for c in cs.CASES}
        assert have == set(cs.FEASIBLE[mode]), (mode, have ^ set(cs.FEASIBLE[mode]))


def test_case_list_covers_the_edges():
    geo = {c: (cs.out_hw(c), cs.plan(c, 2)["fastp"]) for c in cs.CASES}
    fastp_wo = {wo for (ho, wo), fp in geo.values() if fp}
    assert fastp_wo == {1, 2, 4, 8, 16, 32}
    exact = {wo for (ho, wo), fp in geo.values() if fp and ho == 32 // wo}
    assert exact == {1, 2, 4, 8, 16, 32}, "Ho == 32 / Wo exactly, at every width that has the carried form"
    assert any((ho, wo) == (1, 16) and not fp for (ho, wo), fp in geo.values())
    assert {3, 5, 7, 40, 64} <= {wo for (ho, wo), fp in geo.values() if not fp}
    assert any((ho * wo) % 32 for (ho, wo), _ in geo.values() for _ in (0,))
    assert any((c[1] * c[2]) % 32 and c[0] > 1 for c in cs.CASES)                           # mode 1: pixels of dx per sample
    for mode in (0, 1):                                                                      # the gathered M
        ms = {cs.plan(c, mode)["M"] for c in cs.CASES}
        assert any(m < 128 for m in ms) and any(m > 128 and m % 128 for m in ms), mode
    assert 128 in {cs.plan(c, 0)["M"] for c in cs.CASES}
    assert {4, 64, 68, 132} <= {c[4] for c in cs.CASES}
    assert 108 in {cs.plan(c, 2)["Nn"] for c in cs.CASES}
    assert any(cs.plan(c, 2)["Nn"] > 64 and (cs.plan(c, 2)["Nn"] % 64) % c[3] for c in cs.CASES), "a tap straddles a 64-column tile"
    assert {4, 8, 16} <= {cs.plan(c, m)["K"] % 32 for c in cs.CASES for m in (0, 1)}
    assert any(cs.plan(c, 2)["K"] % 32 for c in cs.CASES)
    assert {(1, 1), (3, 1), (1, 3), (3, 3), (5, 3), (7, 7), (2, 2)} <= {(c[5], c[6]) for c in cs.CASES}
    assert {(1, 1), (1, 2), (2, 1), (2, 2), (3, 2)} <= {(c[7], c[8]) for c in cs.CASES}
    assert any(c[7] > c[5] and c[8] > c[6] for c in cs.CASES)
    pads = {(k, p) for c in cs.CASES for k, p in ((c[5], c[9]), (c[6], c[10]))}
    assert any(p == 0 and k > 1 for k, p in pads) and any(p == k // 2 and k > 1 for k, p in pads)
    assert any(p == k - 1 and k > 2 for k, p in pads)
    assert any((c[1] + 2 * c[9] - c[5]) % c[7] for c in cs.CASES)
    assert any(c[1] == 1 for c in cs.CASES) and any(c[2] == 1 for c in cs.CASES)
    assert {1, 2, 3, 5} <= {c[0] for c in cs.CASES}
    # split-K: empty trailing slices (fewer effective splits than asked for) and a K tail in the last slice
    assert any(cs.plan(c, 2, s)["splits"] < s for c in cs.CASES for s in cs.SPLITS)
    assert any(cs.plan(c, 2, s)["splits"] > 1 and cs.plan(c, 2, s)["last"] % 32 and cs.plan(c, 2, s)["fastp"]
               for c in cs.CASES for s in cs.SPLITS)
    # elements without a term exist in both gradients
    assert any((cs.reference(c)[1][2] == 0).any() for c in cs.CASES) and any((cs.reference(c)[2][2] == 0).any() for c in cs.CASES)
    assert len(cs.CASES) <= 30


def test_front_guard_holds_the_tap_bias():
    for case in cs.CASES:
        for mode in (0, 1):
            inp = cs.build(case, mode)
            assert inp["src0"] % 4 == 0 and inp["src0"] >= cs.tap_bias(case, mode) + 64
            assert np.isnan(inp["srcbuf"][:inp["src0"]]).all() and np.isnan(inp["srcbuf"][-cs.POST:]).all()


@pytest.mark.parametrize("case", cs.CASES, ids=cs.name)
def test_references_equal_torch_float64(case):
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw = case
    x, wt, dy = (torch.from_numpy(np.array(t, dtype=np.float64)) for t in cs.tensors(case))
    for absolute in (False, True):
        xa, wa, dya = (t.abs() if absolute else t for t in (x, wt, dy))
        xa = xa.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        wa = wa.clone().requires_grad_(True)
        y = torch.nn.functional.conv2d(xa, wa, stride=(sh, sw), padding=(ph, pw))
        y.backward(dya.permute(0, 3, 1, 2).contiguous())
        want = {0: y.detach().permute(0, 2, 3, 1).reshape(-1, cout).numpy(),
                1: xa.grad.permute(0, 2, 3, 1).reshape(-1, cin).numpy(),
                2: cs.pack_wk(wa.grad.numpy())}
        for mode in cs.MODES:
            got = cs.reference(case)[mode][1 if absolute else 0]
            scale = np.abs(cs.reference(case)[mode][1]).max()
            assert got.shape == want[mode].shape
            assert np.abs(got - want[mode]).max() <= 1e-12 * scale, (mode, absolute)
    # elements without a term are exact zeros of the reference
    for mode in cs.MODES:
        ref, mag, terms = cs.reference(case)[mode]
        assert (ref[terms == 0] == 0.0).all() and (mag[terms == 0] == 0.0).all() and (mag[terms > 0] > 0.0).all()


def test_pack_round_trip():
    w = np.arange(8 * 12 * 3 * 2, dtype=np.float32).reshape(8, 12, 3, 2)
    wk = cs.pack_wk(w)
    assert wk.shape == (8, 72) and wk[5, (2 * 2 + 1) * 12 + 7] == w[5, 7, 2, 1]
    assert np.array_equal(cs.unpack_wk(wk, 8, 12, 3, 2), w)


@functools.lru_cache(maxsize=None)
def honest(case, mode, splits):
    """The inputs of a run and its honest emulation, computed once for the tests below (and left unchanged by them)."""
    inp = cs.build(case, mode, splits)
    out = cs.emulate(case, mode, splits, inp=inp)
    out.setflags(write=False)
    return inp, out


def test_check_passes_the_honest_emulation_everywhere():
    worst = {}
    for case, mode, splits in cs.runs():
        inp, out = honest(case, mode, splits)
        ratio = cs.check(case, mode, inp, out)
        key = (mode, inp["plan"]["pixel"])
        worst[key] = max(worst.get(key, 0.0), ratio)
    print({k: round(v, 3) for k, v in sorted(worst.items())})
    assert set(worst) == {(m, f[0]) for m in cs.MODES for f in cs.FEASIBLE[m]}


def test_check_refuses_a_touched_guard_and_a_kept_sentinel():
    case = cs.CASES[0]
    inp = cs.build(case, 0)
    good = cs.emulate(case, 0, inp=inp)
    assert cs.check(case, 0, inp, good) < 1.0
    for where in (inp["out0"] - 1, inp["out0"] + inp["ref"].size):
        bad = good.copy()
        bad[where] = 0.0
        with pytest.raises(AssertionError, match="outside the output window"):
            cs.check(case, 0, inp, bad)
    bad = good.copy()
    bad[inp["out0"] + 5] = cs.SENT
    with pytest.raises(AssertionError, match="sentinel"):
        cs.check(case, 0, inp, bad)
    case = (2, 11, 7, 32, 32, 1, 1, 2, 2, 0, 0)                     # an element without a term must be exactly zero
    inp = cs.build(case, 1)
    bad = cs.emulate(case, 1, inp=inp)
    row = int(np.argmax((inp["terms"] == 0).all(axis=1)))
    bad[inp["out0"] + row * inp["ref"].shape[1]] = 1e-30
    with pytest.raises(AssertionError, match="exactly 0"):
        cs.check(case, 1, inp, bad)


# the forms (mode, pixel form) in which a fault has something to change: ``check`` must refuse it in each of them
FAULT_FORMS = {
    "no_row_mask": {(0, "GA"), (0, "div"), (1, "GA"), (1, "carry"), (1, "div"), (2, "fastp"), (2, "div")},
    "no_col_mask": {(0, "GA"), (0, "div"), (1, "GA"), (1, "carry"), (1, "div"), (2, "fastp"), (2, "div")},
    "no_divisibility_test": {(1, "carry"), (1, "div")},
    "no_tap_flip": {(1, "GA"), (1, "carry"), (1, "div")},
    "no_kw_carry": {(0, "GA"), (1, "GA"), (1, "carry")},
    "no_sample_carry": {(2, "fastp")},
    "fastp_from_zero": {(2, "fastp")},
    "no_ktail_zero_fill": {(0, "div"), (1, "div"), (2, "fastp"), (2, "div")},
    "drop_last_split": {(2, "fastp"), (2, "div")},
    "bias_off_by_one_pixel": {(0, "GA"), (1, "GA")},
}


@pytest.mark.parametrize("fault", cs.FAULTS)
def test_check_catches_every_planted_fault(fault):
    """Per fault: the runs whose emulation with the fault differs from the honest one at all, and of those the ones ``check``
    refuses.  ``check`` refuses every run the fault changes -- none hides inside the bound -- and that in every form the fault
    can touch, and the fault changes no run of another form."""
    assert set(FAULT_FORMS) == set(cs.FAULTS)
    changed, caught, forms = [], [], set()
    for case, mode, splits in cs.runs():
        inp, good = honest(case, mode, splits)
        bad = cs.emulate(case, mode, splits, fault=fault, inp=inp)
        if np.array_equal(good.view(np.int32), bad.view(np.int32)):
            continue
        changed.append((cs.name(case), mode, splits))
        try:
            cs.check(case, mode, inp, bad)
        except AssertionError:
            caught.append(changed[-1])
            forms.add((mode, inp["plan"]["pixel"]))
    print("%s: changes %d runs, %d refused" % (fault, len(changed), len(caught)))
    assert caught, "%s: no run refused (%d changed)" % (fault, len(changed))
    assert caught == changed, "%s: hides inside the bound at %s" % (fault, [c for c in changed if c not in caught][:4])
    assert forms == FAULT_FORMS[fault], (fault, forms ^ FAULT_FORMS[fault])
