"""CPU: the cases, references and the checker of the GEMM-family tests (oracle/gemm_stage.py; tests/test_gpu_gemm_stage.py runs
csrc/gemm.hip against them on the GPU).  ``plan`` against hand-worked values; the case list holds every form the kernel can
take and every pair of the edge values; a float32 NumPy emulation of the tiled kernel passes ``check`` on every case, and the
same emulation with one planted fault does not."""
import itertools

import numpy as np
import pytest

from oracle import gemm_stage as gs


def test_plan_hand_worked_values():
    p = gs.plan(8, 8, 100, 100, 100, False, False, 3)
    assert (p["klen"], p["splits"], p["last"]) == (64, 2, 36) and p["fastg"] == 0             # 100 is no whole number of K tiles
    p = gs.plan(8, 8, 96, 96, 96, False, False, 64)
    assert (p["klen"], p["splits"], p["last"], p["fastg"]) == (32, 3, 32, 3)
    p = gs.plan(8, 8, 32, 32, 32, False, False, 4)
    assert (p["klen"], p["splits"], p["last"], p["epilogue"]) == (32, 1, 32, "vector")
    p = gs.plan(8, 8, 36, 36, 36, False, False, 2)
    assert (p["klen"], p["splits"], p["last"], p["epilogue"]) == (32, 2, 4, "slabs")
    assert gs.plan(8, 8, 64, 64, 64, False, False, 0)["splits"] == 1                            # splits < 1 counts as 1


def test_plan_fetch_and_epilogue_rules():
    # descriptors: K and every split whole tiles, the extent below 2^29 - 64 floats, and only for a k-major operand
    assert gs.plan(8, 8, 64, 64, 64, False, False)["fetch_a"] == "descriptor"
    p = gs.plan(8, 8, 64, 8, 64, True, False)
    assert (p["fastg"], p["fetch_a"], p["fetch_b"]) == (3, "general", "descriptor")
    p = gs.plan(8, 8, 64, 64, 8, False, True)
    assert (p["fetch_a"], p["fetch_b"]) == ("descriptor", "general")
    assert gs.plan(8, 8, 36, 36, 36, False, False)["fastg"] == 0
    # the 2^29 switch, M = 3, K = 64: extent 2 lda + 64.  lda = 2^28 - 68 is the last descriptor-eligible leading dimension;
    # 2^28 - 64 gives an extent of exactly 2^29 - 64, which is not below the limit
    assert gs.plan(3, 4, 64, 2 ** 28 - 68, 64, False, False)["fetch_a"] == "descriptor"
    assert gs.plan(3, 4, 64, 2 ** 28 - 64, 64, False, False)["fastg"] == 0
    assert gs.plan(3, 4, 64, 2 ** 28, 64, False, False)["fastg"] == 0
    assert gs.plan(3, 4, 64, 64, 178956924, False, False)["fetch_b"] == "descriptor"       # N = 4: extent 3 ldb + 64
    assert gs.plan(3, 4, 64, 64, 178956928, False, False)["fastg"] == 0
    # epilogue: vector needs !TA, N % 4, ldc % 4, C and the bias 16-byte aligned
    assert gs.plan(8, 8, 64, 64, 64, False, False, 1, 12, 0, 0)["epilogue"] == "vector"
    assert gs.plan(8, 8, 64, 64, 64, False, False, 1, 9, 0, 0)["epilogue"] == "scalar"
    assert gs.plan(8, 8, 64, 64, 64, False, False, 1, 8, 8, None)["epilogue"] == "scalar"
    assert gs.plan(8, 8, 64, 64, 64, False, False, 1, 8, 0, 4)["epilogue"] == "scalar"
    assert gs.plan(8, 8, 64, 64, 64, False, False, 1, 8, 0, None)["epilogue"] == "vector"
    assert gs.plan(8, 6, 64, 64, 64, False, False, 1, 8, 0, None)["epilogue"] == "scalar"
    assert gs.plan(8, 8, 64, 8, 64, True, False, 1, 8, 0, None)["epilogue"] == "scalar"


def test_case_list_holds_every_form():
    """Every combination of (TA, TB), fetch form per operand, epilogue form, accumulate and bias that the kernel can take
    (``feasible_forms`` says which it cannot, and why)."""
    cases = [c for c in gs.all_cases() if c["kind"] == "plain"]
    have = set(gs.form_of(c) for c in cases)
    want = set(gs.feasible_forms())
    assert len(want) == 72 and not (want - have), sorted(want - have)
    assert not (have - want), "a case claims a form the kernel cannot take: %s" % sorted(have - want)
    # and the forms of the pairwise list alone reach each epilogue and each fetch
    pw = set(gs.form_of(c)[2:5] for c in gs.pairwise_cases())
    assert {f[2] for f in pw} == {"vector", "scalar", "slabs"} and {f[0] for f in pw} == {"descriptor", "general"}


def test_pairwise_list_covers_every_pair():
    rows = gs.pairwise_rows()
    assert len(rows) * 4 == len(gs.pairwise_cases()) and len(rows) <= 80, len(rows)
    factors = gs._FACTORS
    for i, j in itertools.combinations(range(len(factors)), 2):
        for vi, vj in itertools.product(factors[i], factors[j]):
            if i == 0 and ((j == 1 and vi[0] and vj % 4) or (j == 2 and vi[1] and vj % 4)):
                continue                                     # a transposed operand's contiguous axis is a multiple of 4
            assert any(r[i] == vi and r[j] == vj for r in rows), (i, vi, j, vj)
    for cs in gs.pairwise_cases():
        assert cs["lda"] % 4 == 0 and cs["ldb"] % 4 == 0
        assert (cs["m"] if cs["ta"] else cs["k"]) % 4 == 0 and (cs["n"] if cs["tb"] else cs["k"]) % 4 == 0


def test_alignment_and_batched_lists():
    bases = gs.alignment_bases()
    assert len(bases) == 8
    for b in bases:
        p = gs.case_plan(b)
        assert p["fastg"] == (3 if b["k"] == 64 else 0) and p["epilogue"] == ("scalar" if b["ta"] else "vector")
    assert len(gs.ALIGN_OFFSETS) == 16 and all(len(o) == 4 for o in gs.ALIGN_OFFSETS)
    singles = [o for o in gs.ALIGN_OFFSETS if sum(1 for x in o if x) == 1]
    assert sorted(singles) == sorted(tuple(v if i == j else 0 for j in range(4)) for i in range(4) for v in (1, 2, 3))
    # an offset C or bias turns the vector epilogue into the scalar one
    assert gs.case_plan(gs.variant(bases[0], offs=(0, 0, 0, 1)))["epilogue"] == "scalar"
    assert gs.case_plan(gs.variant(bases[0], offs=(0, 0, 2, 0)))["epilogue"] == "scalar"
    assert gs.case_plan(gs.variant(bases[0], offs=(3, 3, 0, 0)))["epilogue"] == "vector"
    names = [c["name"] for c in gs.batched_cases()]
    assert names[:4] == ["wino1d_conv_FF", "wino1d_wgrad_TT_rows5", "wino1d_wgrad_TT_rows20", "wino1d_wgrad_TT_rows33"]
    g = gs.batched_cases()[4]
    oa, ia, ob, ib, oc, ic = g["strides"]
    assert (g["outer"], g["inner"], ia, g["alpha"], g["acc"]) == (3, 2, 0, 0.125, True) and ic > g["m"] * g["ldc"] and oc > 2 * ic
    assert all(s % 4 == 0 for s in (oa, ia, ob, ib))


def test_build_surrounds_operands_with_nan_and_output_with_sentinel():
    cs = gs.variant(gs.form_base(False, False, "general", "general", "vector"), gap_a=4, gap_b=4, acc=True, bias=True,
                    offs=(1, 2, 3, 0))
    inp = gs.build(cs)
    (a0, b0, c0), = inp["probs"]
    assert (a0, b0, c0, inp["bias0"]) == (gs.PRE + 1, gs.PRE + 2, gs.PRE, gs.PRE + 3)
    a = inp["A"][a0]
    assert a.shape == (36, 36) and int(np.isfinite(inp["abuf"]).sum()) == a.size
    assert np.isnan(inp["abuf"][:a0]).all() and np.isnan(inp["abuf"][a0 + 36:a0 + 40]).all()
    assert np.isnan(inp["abuf"][a0 + 35 * 40 + 36:]).all()
    assert int(np.isfinite(inp["bbuf"]).sum()) == 68 * 36 and int(np.isfinite(inp["biasbuf"]).sum()) == 68
    assert int((inp["cbuf"] != gs.SENT).sum()) == 36 * 68 and (inp["cbuf"][:c0] == gs.SENT).all()
    bias = inp["biasbuf"][inp["bias0"]:inp["bias0"] + 68].astype(np.float64)
    ref = a.astype(np.float64) @ inp["B"][b0].astype(np.float64).T + bias + inp["C0"][0]
    assert np.allclose(ref, inp["ref"][0], rtol=0, atol=1e-13)             # (float64; the terms added in another order)
    assert float(inp["bound"][0].min()) > 0 and inp["bound"][0].shape == (36, 68)


@pytest.fixture(scope="module")
def cases():
    return gs.all_cases()


def test_emulation_passes_on_every_case(cases):
    worst = {}
    for cs in cases:
        inp = gs.build(cs)
        stats = {}
        r = gs.check(cs, inp, gs.emulate(cs, inp, stats=stats))
        assert stats["outside_reads"] == 0, cs["name"]
        group = cs["name"].split("_")[0][:2]
        worst[group] = max(worst.get(group, 0.0), r)
    print("worst err / bound of the float32 emulation per group:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) < 1.0


@pytest.mark.parametrize("fault", [f for f in gs.FAULTS if f != "no_row_zero_fill"])
def test_planted_fault_fails_check(cases, fault):
    caught = 0
    for cs in cases:
        inp = gs.build(cs)
        try:
            gs.check(cs, inp, gs.emulate(cs, inp, fault))
        except AssertionError:
            caught += 1
    print("%s: caught on %d of %d cases" % (fault, caught, len(cases)))
    assert caught >= 1


def test_skipped_row_zero_fill_cannot_change_the_output(cases):
    """The planted fault "zero-fill of rows past M skipped" cannot fail ``check``, and no checker of C could see it: a row of
    A (a column of B) past M (N) feeds only accumulator rows (columns) past M (N), which are never stored.  What is wrong with
    it is the read itself; the NaN rows show that a row past M never lands in a STORED row.  So: the output keeps its bits on
    every case, and the emulation's own record of its fetches does see the reads outside the operand."""
    seen = 0
    for cs in cases[::7]:
        inp = gs.build(cs)
        stats = {}
        out = gs.emulate(cs, inp, "no_row_zero_fill", stats)
        assert np.array_equal(out.view(np.int32), gs.emulate(cs, inp).view(np.int32)), cs["name"]
        seen += stats["outside_reads"] > 0
    assert seen > 0


def test_check_itself():
    cs = gs.form_base(False, False, "descriptor", "descriptor", "vector")
    inp = gs.build(cs)
    good = gs.emulate(cs, inp)
    assert gs.check(cs, inp, good) < 1.0
    (_, _, c0), = inp["probs"]
    bad = good.copy()
    bad[c0 + cs["ldc"] + 3] += np.float32(4.0 * inp["bound"][0][1, 3])         # one element four bounds off
    with pytest.raises(AssertionError, match="over the bound"):
        gs.check(cs, inp, bad)
    bad = good.copy()
    bad[c0 + cs["n"]] = np.float32(0.0)                                         # the first gap float after row 0
    with pytest.raises(AssertionError, match="outside the output window"):
        gs.check(cs, inp, bad)
    bad = good.copy()
    bad[-1] = -gs.SENT
    with pytest.raises(AssertionError, match="outside the output window"):
        gs.check(cs, inp, bad)
    bad = good.copy()
    bad[c0] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        gs.check(cs, inp, bad)


def test_colsum_and_linear_references():
    assert gs.colsum_rows_per_block(64) == 64 and gs.colsum_rows_per_block(65) == 33 and gs.colsum_rows_per_block(129) == 43
    assert gs.colsum_rows_per_block(65601) == 65 and gs.colsum_rows_per_block(65536) == 64     # 1024 workgroups at the most
    buf, first, ld, a, old = gs.colsum_inputs(5, 3)
    assert ld == 6 and int(np.isfinite(buf).sum()) == 15 and np.array_equal(buf[first + ld:first + ld + 3], a[1])
    assert np.allclose(gs.colsum_bound(a), 7 * gs.U * np.abs(a.astype(np.float64)).sum(axis=0), rtol=0, atol=0)
    li = gs.linear_inputs(70, 64, 13)
    ref = gs.linear_reference(li)
    assert ref["y"][0].shape == (70, 13) and ref["dx"][0].shape == (70, 64)
    assert ref["dw"][0].shape == (13, 64) and ref["db"][0].shape == (13,)
    assert len(gs.colsum_cases()) == 54 and len(gs.LINEAR_RK) == 4 and len(gs.LINEAR_N) == 4          # the full products
    x = li["x"].astype(np.float64)
    assert np.array_equal(ref["dw"][0], li["dy"].astype(np.float64).T @ x)
    ady, aw = np.abs(li["dy"].astype(np.float64)), np.abs(li["w"].astype(np.float64))
    assert np.array_equal(ref["dx"][1], (13 + 5) * gs.U * (ady @ aw))                # n = 13 terms, not the padded 16
