"""GPU tests of the GEMM family (run with ``-m gpu`` on an MI355X): ``gemm_kernel<TA,TB>`` behind ``adyolo_gemm`` and
``adyolo_gemm_batched``, ``gemm_slab_reduce_kernel``, ``colsum``, ``add`` / ``mul`` / ``scale_dev`` (K7, csrc/gemm.hip) and
``ops.linear`` / ``ops.linear_bwd`` / ``functional.LinearFn`` on top of them, against float64.  Cases, inputs, references and the
checker: oracle/gemm_stage.py, pinned on the CPU by tests/test_gemm_stage_cpu.py.

Every operand is a view into a NaN-filled buffer, every output a view into a sentinel-filled one: a read outside the logical
operand that reaches the matrix core, or a store outside the M x N window, fails the case.  The bar is derived, not measured:

    |got - ref| <= (K + S + 4) * 2^-24 * ( |alpha| (|A| |B|)[m,n] + |bias[n]| + |C0[m,n]| )

and runs that differ only in how the operands are fetched (compact / NaN-gapped, aligned / offset pointer, descriptor / general
fetch at the 2^29 switch), and a second identical call, must agree bit for bit.

16-byte loads at 4-byte-aligned addresses (the pointers ``dist.FlatParameters`` hands out).  The general fetch loads through a
float4 type declared ``aligned(4)`` (``load4_a4`` in gemm.hip), the descriptor fetch through a builtin that promises no
alignment; they compile to ``global_load_dwordx4`` and ``buffer_load_dwordx4`` (no flat or scratch access).  The vector
epilogue's ``global_store_dwordx4`` is taken only when C and the bias are 16-byte aligned.  The HSA ABI runs compute queues
with SH_MEM_CONFIG.ALIGNMENT_MODE = UNALIGNED (LLVM's AMDGPU backend turns ``unaligned-access-mode`` on for every amdhsa target
for that reason), in which global and buffer accesses of any width need no more than byte alignment.  So every form is legal
in the source and on the chip, nothing is refused, and the offset cases below are value and bit checks.

Worst err / bound on an MI355X (28 tests, 3.0 s): pairwise list 0.323, forms 0.093, offset pointers 0.101, batched 0.262, colsum
0.306, linear 0.188; the comment at each test has its own figures, DESIGN.md (K7) the table.  No case missed its bound."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gemm_stage as gs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    return t


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def window(cs, inp, out, prob=0):
    return gs._window(out, inp["probs"][prob][2], cs["m"], cs["n"], cs["ldc"]).copy()


def run_plain(ops, cs, inp):
    """One ``ops.gemm`` call on device copies of the case's buffers -> the whole output buffer."""
    (a0, b0, c0), = inp["probs"]
    a, b, c = dev(inp["abuf"]), dev(inp["bbuf"]), dev(inp["cbuf"])
    bias = dev(inp["biasbuf"])[inp["bias0"]:] if cs["bias"] else None
    ops.gemm(a[a0:], b[b0:], cs["m"], cs["n"], cs["k"], cs["lda"], cs["ldb"], trans_a=cs["ta"], trans_b=cs["tb"], bias=bias,
             out=c[c0:], ldc=cs["ldc"], accumulate=cs["acc"], splits=cs["splits"])
    torch.cuda.synchronize()
    return c.cpu().numpy()


def run_and_check(ops, cs, repeat=True):
    inp = gs.build(cs)
    out = run_plain(ops, cs, inp)
    ratio = gs.check(cs, inp, out)
    if repeat:                                   # split-K sums its slabs in a fixed order: the same bits again
        assert np.array_equal(bits(run_plain(ops, cs, inp)), bits(out)), "%s: a second identical call differs" % cs["name"]
    return inp, out, ratio


def lib_plan(m, n, k, lda, ldb, ta, tb, splits):
    from adyolo_amd import _lib
    klen, eff, fastg = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.call("adyolo_gemm_plan", m, n, k, lda, ldb, int(ta), int(tb), splits, ctypes.byref(klen), ctypes.byref(eff),
              ctypes.byref(fastg))
    return klen.value, eff.value, fastg.value


# ================================================================================================================ the plan
SWITCH_LDA = (2 ** 28 - 68, 2 ** 28 - 64, 2 ** 28)                      # M = 3: extent 2 lda + 64 against 2^29 - 64
SWITCH_LDB = (178956924, 178956928, 2 ** 28 - 64, 2 ** 28)              # N = 4: extent 3 ldb + 64


def test_plan_mirror_agrees_with_the_library(ops):
    args = set()
    for cs in gs.all_cases(gpu_only=True):
        if cs["kind"] == "plain":
            args.add((cs["m"], cs["n"], cs["k"], cs["lda"], cs["ldb"], cs["ta"], cs["tb"], cs["splits"]))
    args |= {(3, 4, 64, lda, 64, False, False, 1) for lda in SWITCH_LDA}
    args |= {(3, 4, 64, 64, ldb, False, False, 1) for ldb in SWITCH_LDB}
    args |= {(3, 4, 64, 2 ** 28, 4, True, True, 1), (8, 8, 100, 100, 100, False, False, 3), (8, 8, 96, 96, 96, False, False, 64),
             (8, 8, 32, 32, 32, False, False, 4), (8, 8, 36, 36, 36, False, False, 2), (8, 8, 64, 64, 64, False, False, 0),
             (8, 8, 64, 64, 64, False, False, -3)}
    for a in sorted(args):
        p = gs.plan(*a)
        assert lib_plan(*a) == (p["klen"], p["splits"], p["fastg"]), a
    print("%d distinct argument sets" % len(args))


# ======================================================================================================= 1. plain adyolo_gemm
@pytest.mark.parametrize("ta,tb", gs.TRANS, ids=["FF", "FT", "TF", "TT"])
def test_gemm_pairwise_edges(ops, ta, tb):
    # MI355X, worst err / bound: FF 0.323 (84 runs), FT 0.253 (76), TF 0.285 (56), TT 0.307 (36); every second call bit-equal
    cases = [c for c in gs.pairwise_cases() if (c["ta"], c["tb"]) == (ta, tb)]
    assert len(cases) >= 32                      # (TA, TB) meets each of the eight K values in a row of its own
    worst, failed = 0.0, []
    for cs in cases:
        try:
            worst = max(worst, run_and_check(ops, cs)[2])
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])
    print("%d cases, worst err / bound %.3f" % (len(cases), worst))
    assert not failed, "%d of %d: %s" % (len(failed), len(cases), "; ".join(failed[:8]))


def test_gemm_every_form_and_compact_equals_gapped(ops):
    """Every (TA, TB, fetch, fetch, epilogue, accumulate, bias) the kernel can take: by value, and bit-equal between the compact
    operands and the same numbers in views with four NaN columns after every row."""
    # MI355X, worst err / bound: 0.093 over the 72 forms; compact and gapped bit-equal in all
    worst, failed = 0.0, []
    cases = gs.form_cases()
    for cs in cases:
        try:
            inp, out, ratio = run_and_check(ops, cs)
            worst = max(worst, ratio)
            gapped = gs.variant(cs, gap_a=4, gap_b=4)
            assert gs.form_of(gapped) == gs.form_of(cs)
            inp_g, out_g, _ = run_and_check(ops, gapped, repeat=False)
            same = np.array_equal(bits(window(cs, inp, out)), bits(window(gapped, inp_g, out_g)))
            assert same, "%s: compact and gapped runs differ" % cs["name"]
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])
    print("%d forms, worst err / bound %.3f" % (len(cases), worst))
    assert not failed, "%d of %d: %s" % (len(failed), len(cases), "; ".join(failed[:8]))


# ========================================================================================================= 2. pointer alignment
@pytest.mark.parametrize("base", gs.alignment_bases(), ids=lambda b: b["name"])
def test_gemm_pointers_at_4_and_8_byte_alignment(ops, base):
    """A, B, bias and C each 1, 2 and 3 floats into their allocation, one at a time and all together: correct, and the bits of
    the aligned run wherever the epilogue form is the same (an offset C or bias turns the vector epilogue into the scalar one,
    which rounds alike: v = acc * alpha + bias is one multiplication and one addition in both)."""
    # MI355X, worst err / bound: FF 0.052 / 0.073 (K 64 / 36), FT 0.071 / 0.086, TF 0.047 / 0.101, TT 0.043 / 0.095; offset runs
    # with the aligned run's epilogue (6 of 16 under the vector epilogue, all 16 under the scalar one) bit-equal to it
    inp0, out0, worst = run_and_check(ops, base)
    ref_bits = bits(window(base, inp0, out0))
    epi0 = gs.case_plan(base)["epilogue"]
    same = 0
    for offs in gs.ALIGN_OFFSETS:
        cs = gs.variant(base, offs=offs)
        inp, out, ratio = run_and_check(ops, cs, repeat=False)
        worst = max(worst, ratio)
        if gs.case_plan(cs)["epilogue"] == epi0:
            same += 1
            assert np.array_equal(bits(window(cs, inp, out)), ref_bits), "%s: differs from the aligned run" % cs["name"]
    print("%s: worst err / bound %.3f, %d of %d offset runs keep the epilogue form %s" % (
        base["name"], worst, same, len(gs.ALIGN_OFFSETS), epi0))
    assert same == (16 if base["ta"] else 6)          # offsets of A and B alone keep the vector epilogue


# ============================================================================================================ 3. the 2^29 switch
def test_gemm_fetch_switch_at_2_pow_29_floats(ops):
    """M = 3, N = 4, K = 64 with one operand's rows 2^28 floats apart, more or less: the descriptor fetch with byte offsets just
    below 2^31, the general fetch with 64-bit addresses, bit-equal to the compact run.  (The extent of lda = 2^28 - 64 is exactly
    2^29 - 64, which is the first the host sends to the general fetch; 2^28 - 68 is the last descriptor-eligible one.)"""
    rng = np.random.default_rng(77)
    a, b = rng.standard_normal((3, 64)).astype(np.float32), rng.standard_normal((4, 64)).astype(np.float32)
    ad, bd = dev(a), dev(b)
    want = ops.gemm(ad, bd, 3, 4, 64, 64, 64).cpu()
    ref = a.astype(np.float64) @ b.astype(np.float64).T
    assert (np.abs(want.numpy() - ref) <= 69 * gs.U * (np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64)).T)).all()
    big = torch.empty(3 * 2 ** 28 + 64 + 1024, dtype=torch.float32, device="cuda:0")
    try:
        forms = []
        for lda in SWITCH_LDA:
            for r in range(3):
                big[r * lda:r * lda + 64] = ad[r]
            p = gs.plan(3, 4, 64, lda, 64, False, False)
            assert lib_plan(3, 4, 64, lda, 64, False, False, 1) == (p["klen"], p["splits"], p["fastg"])
            forms.append(p["fetch_a"])
            got = ops.gemm(big, bd, 3, 4, 64, lda, 64).cpu()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "lda %d (%s fetch)" % (lda, p["fetch_a"])
        assert forms == ["descriptor", "general", "general"]
        forms = []
        for ldb in SWITCH_LDB:
            for r in range(4):
                big[r * ldb:r * ldb + 64] = bd[r]
            p = gs.plan(3, 4, 64, 64, ldb, False, False)
            assert lib_plan(3, 4, 64, 64, ldb, False, False, 1) == (p["klen"], p["splits"], p["fastg"])
            forms.append(p["fetch_b"])
            got = ops.gemm(ad, big, 3, 4, 64, 64, ldb).cpu()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "ldb %d (%s fetch)" % (ldb, p["fetch_b"])
        assert forms == ["descriptor", "general", "general", "general"]
    finally:
        del big
        torch.cuda.empty_cache()


# ========================================================================================================= 4. adyolo_gemm_batched
@pytest.mark.parametrize("cs", [c for c in gs.batched_cases() if c["gpu"]], ids=lambda c: c["name"])
def test_gemm_batched(ops, cs):
    # MI355X, worst err / bound: wino1d_conv_FF 0.055, wino1d_wgrad_TT rows 5 / 20 / 33 0.262 / 0.120 / 0.086, general_o3_i2 0.076
    inp = gs.build(cs)
    a0, b0, c0 = inp["probs"][0]

    def run():
        a, b, c = dev(inp["abuf"]), dev(inp["bbuf"]), dev(inp["cbuf"])
        ops.gemm_batched(a[a0:], b[b0:], c[c0:], cs["m"], cs["n"], cs["k"], cs["lda"], cs["ldb"], cs["ldc"], cs["ta"], cs["tb"],
                         cs["outer"], cs["inner"], *cs["strides"], alpha=cs["alpha"], accumulate=cs["acc"])
        torch.cuda.synchronize()
        return c.cpu().numpy()
    out = run()
    ratio = gs.check(cs, inp, out)
    print("%s: %d problems, worst err / bound %.3f" % (cs["name"], len(inp["probs"]), ratio))
    assert np.array_equal(bits(run()), bits(out))


# ================================================================================================================== 5. refusals
def test_refusals_come_before_any_launch(ops):
    from adyolo_amd import _lib
    from adyolo_amd.ops import NULL, _p, _stream
    a = dev(np.ones(4096, dtype=np.float32))
    b = dev(np.ones(4096, dtype=np.float32))
    c = dev(np.full(4096, gs.SENT, dtype=np.float32))
    slabs = dev(np.full(4096, gs.SENT, dtype=np.float32))

    def gemm(m, n, k, lda, ldb, ta, tb, splits=1, sl=None):
        _lib.call("adyolo_gemm", _p(a), _p(b), NULL, _p(c), _p(sl), m, n, k, lda, ldb, n, int(ta), int(tb), splits, 0, _stream())

    def batched(outer, inner, strides):
        _lib.call("adyolo_gemm_batched", _p(a), _p(b), _p(c), 8, 8, 8, 8, 8, 8, 0, 0, outer, inner, *strides, 1.0, 0, _stream())
    refused = {
        "lda % 4": lambda: gemm(8, 8, 8, 10, 8, False, False),
        "ldb % 4": lambda: gemm(8, 8, 8, 8, 10, False, False),
        "K % 4 with k-major operands": lambda: gemm(8, 8, 6, 8, 8, False, False),
        "M % 4 with a transposed A": lambda: gemm(6, 8, 8, 8, 8, True, False),
        "N % 4 with a transposed B": lambda: gemm(8, 6, 8, 8, 8, False, True),
        "K % 4 with a k-major B beside a transposed A": lambda: gemm(8, 8, 6, 8, 8, True, False),
        "splits > 1 without slabs": lambda: gemm(8, 8, 64, 64, 64, False, False, splits=2),
        "batch stride oA % 4": lambda: batched(2, 1, (66, 0, 64, 0, 64, 0)),
        "batch stride iB % 4": lambda: batched(1, 2, (0, 64, 0, 62, 0, 64)),
        "65536 problems": lambda: batched(256, 256, (0, 0, 0, 0, 0, 0)),
        "add with n % 4": lambda: _lib.call("adyolo_add", _p(a), _p(b), _p(c), 6, _stream()),
        "mul with n % 4": lambda: _lib.call("adyolo_mul", _p(a), _p(b), _p(c), 6, _stream()),
    }
    for what, call in refused.items():
        with pytest.raises(_lib.AdyoloHipError):
            call()
            pytest.fail("%s was not refused" % what)
        torch.cuda.synchronize()
        untouched = bool((c == float(gs.SENT)).all()) and bool((slabs == float(gs.SENT)).all())
        assert untouched, "%s: refused, yet the output changed" % what
    gemm(8, 8, 64, 64, 64, False, False, splits=2, sl=slabs)              # the same call with slabs goes through
    torch.cuda.synchronize()
    assert bool((c[:64] == 64.0).all()) and bool((c[64:] == float(gs.SENT)).all())


# ==================================================================================================================== 6. colsum
def test_colsum(ops):
    # MI355X, worst err / bound: 0.306 (4 x 64) over the 54 cases
    worst, failed = (0.0, None), []
    for r, c in gs.colsum_cases():
        buf, first, ld, a, old = gs.colsum_inputs(r, c)
        view = torch.as_strided(dev(buf), (r, c), (ld, 1), first)
        got = ops.colsum(view)
        guard = dev(np.full(c + 8, gs.SENT, dtype=np.float32))
        guard[3:3 + c] = dev(old)
        ops.colsum(view, out=guard[3:3 + c], accumulate=True)
        torch.cuda.synchronize()
        got, guard = got.cpu().numpy(), guard.cpu().numpy()
        err = np.abs(got.astype(np.float64) - a.astype(np.float64).sum(axis=0))
        bound = gs.colsum_bound(a)
        ratio = float((err / bound).max())
        if ratio > worst[0]:
            worst = (ratio, (r, c))
        if not (np.isfinite(got).all() and (err <= bound).all()):
            failed.append("%d x %d: err / bound %.3f" % (r, c, ratio))
        if not np.array_equal(bits(guard[3:3 + c]), bits(old + got)):
            failed.append("%d x %d: accumulate is not out + colsum" % (r, c))
        if not ((guard[:3] == gs.SENT).all() and (guard[3 + c:] == gs.SENT).all()):
            failed.append("%d x %d: floats beside out changed" % (r, c))
    print("%d cases, worst err / bound %.3f at %s" % (len(gs.colsum_cases()), worst[0], worst[1]))
    assert not failed, "; ".join(failed[:8])


# =============================================================================================================== 7. elementwise
def test_elementwise_second_trip_of_the_grid_stride_loop(ops):
    """n4 = 4096 * 256 + 300 float4: 300 lanes go round the loop a second time; ``scale_dev`` with three more floats as well.
    One float32 operation per element: the bits of the same operation on the CPU."""
    n = 4 * (4096 * 256 + 300)
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(n + 3, generator=g), torch.randn(n + 3, generator=g)
    s = torch.tensor([0.3], dtype=torch.float32)
    ad, bd, sd = a.to("cuda:0"), b.to("cuda:0"), s.to("cuda:0")
    got = {"add": ops.add(ad[:n], bd[:n]), "mul": ops.mul(ad[:n], bd[:n]), "scale": ops.scale_dev(ad[:n], sd),
           "scale+3": ops.scale_dev(ad, sd)}
    torch.cuda.synchronize()
    want = {"add": a[:n] + b[:n], "mul": a[:n] * b[:n], "scale": a[:n] * s[0], "scale+3": a * s[0]}
    for key in want:
        assert torch.equal(got[key].cpu().view(torch.int32), want[key].view(torch.int32)), key


# ==================================================================================================================== 8. linear
def _within(what, got, ref_bound, failed):
    ref, bound = ref_bound
    got = got.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
    err = np.abs(got - ref)
    ratio = float((err / bound).max())
    if not (np.isfinite(got).all() and (err <= bound).all()):
        failed.append("%s: err / bound %.3f" % (what, ratio))
    return ratio


@pytest.mark.parametrize("n", gs.LINEAR_N)
def test_linear_forward_backward_any_width(ops, n):
    """n = 13, 39, 117: the class-wise heads at 13 classes (``linear_bwd`` pads dy and w to a multiple of 4 with zeros); 40: the
    unpadded path.  Plain returns, ``out_dw`` / ``out_db`` as slices at odd float offsets of a sentinel-filled flat buffer (the
    ``GradSink`` case), and ``functional.LinearFn`` under autograd."""
    # MI355X, worst err / bound: y, dx, dw, db over the three ways and the four (R, K): n 13 0.188, 39 0.085, 117 0.060, 40 0.087
    from adyolo_amd import functional as Fn
    worst, failed = 0.0, []
    for r, k in gs.LINEAR_RK:
        li = gs.linear_inputs(r, k, n)
        n4 = gs.cdiv(n, 4) * 4
        ref = gs.linear_reference(li, gs.plan(n4, k, r, n4, k, True, True, ops.wgrad_splits(n4, k, r))["splits"])
        x, w, b, dy = (dev(li[key]) for key in ("x", "w", "b", "dy"))
        tag = "n %d, R %d, K %d" % (n, r, k)
        y = ops.linear(x, w, b)
        dx, dw, db = ops.linear_bwd(x, w, dy)
        assert tuple(dw.shape) == (n, k) and tuple(dx.shape) == (r, k) and tuple(db.shape) == (n,)
        flat = dev(np.full(n * k + n + 64, gs.SENT, dtype=np.float32))
        o_w, o_b = 3, 3 + n * k + 6 + (n * k) % 2                              # both odd
        assert o_w % 2 == 1 and o_b % 2 == 1
        dx2, dw2, db2 = ops.linear_bwd(x, w, dy, out_dw=flat[o_w:o_w + n * k].view(n, k), out_db=flat[o_b:o_b + n])
        xg, wg, bg = (t.clone().requires_grad_(True) for t in (x, w, b))
        y3 = Fn.LinearFn.apply(xg.view(1, r, k), wg, bg)
        (y3 * dy.view(1, r, n)).sum().backward()
        torch.cuda.synchronize()
        for what, t, key in (("y", y, "y"), ("dx", dx, "dx"), ("dw", dw, "dw"), ("db", db, "db"), ("dx (sink)", dx2, "dx"),
                             ("dw (sink)", flat[o_w:o_w + n * k], "dw"), ("db (sink)", flat[o_b:o_b + n], "db"),
                             ("LinearFn y", y3, "y"),
                             ("LinearFn dx", xg.grad, "dx"), ("LinearFn dw", wg.grad, "dw"), ("LinearFn db", bg.grad, "db")):
            worst = max(worst, _within("%s: %s" % (tag, what), t, ref[key], failed))
        f = flat.cpu().numpy()
        keep = np.ones(f.size, dtype=bool)
        keep[o_w:o_w + n * k] = False
        keep[o_b:o_b + n] = False
        if not (f[keep] == gs.SENT).all():
            failed.append("%s: %d neighbours of out_dw / out_db changed" % (tag, int((f[keep] != gs.SENT).sum())))
        if dw2.data_ptr() != flat.data_ptr() + 4 * o_w:
            failed.append("%s: linear_bwd did not return out_dw" % tag)
    print("n %d: worst err / bound %.3f" % (n, worst))
    assert not failed, "; ".join(failed)


def test_linear_bwd_launches_are_unchanged_for_multiples_of_4(ops, monkeypatch):
    """n % 4 == 0: exactly the two GEMMs and the column sum of before, on the caller's tensors (no copy, no padding)."""
    li = gs.linear_inputs(70, 64, 40)
    x, w, dy = (dev(li[key]) for key in ("x", "w", "dy"))
    sink_w, sink_b = dev(np.zeros((40, 64), dtype=np.float32)), dev(np.zeros(40, dtype=np.float32))
    calls = []
    real_gemm, real_colsum = ops.gemm, ops.colsum

    def gemm(a, b, *args, **kw):
        calls.append(("gemm", a.data_ptr(), b.data_ptr(), args,
                      {k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in kw.items()}))
        return real_gemm(a, b, *args, **kw)

    def colsum(a, **kw):
        calls.append(("colsum", a.data_ptr(), {k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in kw.items()}))
        return real_colsum(a, **kw)
    monkeypatch.setattr(ops, "gemm", gemm)
    monkeypatch.setattr(ops, "colsum", colsum)
    ops.linear_bwd(x, w, dy, out_dw=sink_w, out_db=sink_b)
    torch.cuda.synchronize()
    assert calls == [("gemm", dy.data_ptr(), w.data_ptr(), (70, 64, 40, 40, 64), {"trans_b": True}),
                     ("gemm", dy.data_ptr(), x.data_ptr(), (40, 64, 70, 40, 64),
                      {"trans_a": True, "trans_b": True, "splits": ops.wgrad_splits(40, 64, 70), "out": sink_w.data_ptr()}),
                     ("colsum", dy.data_ptr(), {"out": sink_b.data_ptr()})]
    del calls[:]
    ops.linear_bwd(x[:, :64], dev(li["w"][:39]), dev(np.ascontiguousarray(li["dy"][:, :39])))
    assert [c[0] for c in calls] == ["gemm", "gemm", "colsum"]
    assert calls[0][3][:4] == (70, 64, 40, 40) and calls[1][3][:4] == (40, 64, 70, 40)
