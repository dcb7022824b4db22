"""GPU tests of the implicit-GEMM convolution (run with ``-m gpu`` on an MI355X): ``gemm_kernel<false,false,1>`` (forward, data
gradient) and ``gemm_kernel<true,true,2>`` (weight gradient, with ``gemm_slab_reduce_kernel`` under split-K) behind
``adyolo_conv_gemm`` (K7, csrc/gemm.hip), ``pack_wk`` / ``unpack_wk``, and ``ops.conv_gemm`` / ``functional.ConvFn`` on top of
them, against float64.  Cases, inputs, references, the checker and the form names: oracle/conv_gemm_stage.py, pinned on the CPU
by tests/test_conv_gemm_stage_cpu.py.

The gathered operand lies in NaN (in front of it at least the tap bias + 64 floats: where the descriptor of the "GA" form points),
the filter / dy and the slab workspace in NaN, the output in a sentinel.  The bar is derived, not measured:

    |got - ref| <= (K + S + 4) * 2^-24 * (|A| |B|)            K: contraction length of the mode, S: effective splits

per element; an element whose sum has no term (dx rows no output touches, taps that only meet padding) must be exactly 0; no
float outside the output window may change.  Three invariants need no tolerance: a sample of a batched call has the bits of the
N = 1 call on it (modes 0 / 1); padding has the bits of explicit zero rows and columns with padding 0 (modes 0 / 2); two
``splits`` with the same effective count and klen have the same bits (mode 2).  ``adyolo_conv_gemm_plan`` must report what
``oracle.conv_gemm_stage.plan`` says on every run, so the forms a test logs as taken are the kernel's.

Worst err / bound on an MI355X (20 tests, 3.9 s for the module alone with its imports; measured, like every figure here, in
the run of this module at the commit that added it): forward GA 0.069, div + descriptor filter 0.047, div + general filter
0.227; data gradient GA 0.041, carry 0.085, div + descriptor 0.053, div + general 0.223; weight gradient fastp 0.141 (one
split) / 0.094 (2 to 5 effective splits), div 0.201 / 0.070 (2 to 12); at the 2^29 switch 0.002 / 0.003.  182 runs, every one
bit-equal on a second call and on a side stream; 98 single-sample calls, 132 padded / explicit pairs and every pair of
``splits`` with the same effective count bit-equal.  No case missed its bound.  The float32 NumPy emulation of the CPU module
reads 0.081 / 0.204 (forward GA / div), 0.018 / 0.085 / 0.187 (data gradient GA / carry / div) and 0.141 / 0.164 (weight
gradient fastp / div) on the same runs; those are CPU figures.  DESIGN.md (K7) has the table."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import conv_gemm_stage as cs

pytestmark = pytest.mark.gpu

BIG = (2, 16, 32, 8, 8, 3, 3, 1, 1, 1, 1)                # 1024 output pixels: ops.wgrad_splits gives 2
OPS_SHAPES = (cs.CASES[0], cs.CASES[4], cs.CASES[10], BIG)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def dev(a):
    t = torch.from_numpy(np.array(a, dtype=np.float32, order="C")).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    return t


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off) if t is not None else ctypes.c_void_p(0)


def lib_plan(case, mode, splits):
    from adyolo_amd import _lib
    out = (ctypes.c_int * 8)(*([-1] * 8))
    _lib.call("adyolo_conv_gemm_plan", mode, *case, splits, out)
    return list(out)


def conv_gemm(src, other, out, slabs, mode, case, splits, stream=None):
    """``adyolo_conv_gemm`` on pointers the test owns; src / other / out / slabs: (tensor, float offset)."""
    from adyolo_amd import _lib
    st = torch.cuda.current_stream() if stream is None else stream
    _lib.call("adyolo_conv_gemm", ptr(*src), ptr(*other), ptr(*out), ptr(*slabs) if slabs else ctypes.c_void_p(0), mode, *case,
              splits, ctypes.c_void_p(st.cuda_stream))


class Run:
    """The device copies of one (case, mode): operands uploaded once, a fresh output and slab buffer per call."""

    def __init__(self, case, mode):
        self.case, self.mode = case, mode
        self.inp = cs.build(case, mode)
        self.src, self.oth = dev(self.inp["srcbuf"]), dev(self.inp["othbuf"])

    def call(self, splits=1, stream=None):
        inp = cs.build(self.case, self.mode, splits) if self.mode == 2 else self.inp
        out = dev(inp["outbuf"])
        slabs = dev(inp["slabbuf"]) if self.mode == 2 else None
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        conv_gemm((self.src, inp["src0"]), (self.oth, inp["oth0"]), (out, inp["out0"]),
                  (slabs, inp["slab0"]) if slabs is not None else None, self.mode, self.case, splits, stream)
        (stream or torch.cuda.current_stream()).synchronize()
        return inp, out.cpu().numpy()


# ============================================================================================== 1. every case, mode and splits
@pytest.mark.parametrize("mode", cs.MODES, ids=["forward", "dgrad", "wgrad"])
def test_conv_gemm_against_float64(ops, mode):
    """Per run: the plan mirror against the library, ``check``, a second identical call and a call on a side stream with the
    same bits; in mode 2 equal bits between the ``splits`` that come to the same effective count and klen."""
    side = torch.cuda.Stream()
    worst, taken, failed, nruns = {}, {}, [], 0
    for case in cs.CASES:
        run = Run(case, mode)
        same_eff = {}
        for splits in (cs.SPLITS if mode == 2 else (1,)):
            tag = "%s mode %d splits %d" % (cs.name(case), mode, splits)
            try:
                assert lib_plan(case, mode, splits) == cs.plan_row(case, mode, splits), "%s: plan mirror" % tag
                inp, out = run.call(splits)
                p = inp["plan"]
                ratio = cs.check(case, mode, inp, out)
                key = (p["pixel"], p["filter"]) if mode != 2 else (p["pixel"], "S>1" if p["splits"] > 1 else "S=1")
                worst[key] = max(worst.get(key, 0.0), ratio)
                taken[key] = taken.get(key, 0) + 1
                nruns += 1
                assert np.array_equal(bits(run.call(splits)[1]), bits(out)), "%s: a second identical call differs" % tag
                assert np.array_equal(bits(run.call(splits, stream=side)[1]), bits(out)), "%s: the side-stream call differs" % tag
                first = same_eff.setdefault((p["splits"], p["klen"]), (splits, out))
                assert np.array_equal(bits(first[1]), bits(out)), "%s: differs from splits %d with the same effective %d x %d" % (
                    tag, first[0], p["splits"], p["klen"])
            except AssertionError as e:
                failed.append(str(e).splitlines()[0])
    for key in sorted(worst, key=str):
        print("mode %d form %-22s taken by %3d runs, worst err / bound %.3f" % (mode, "%s / %s" % key, taken[key], worst[key]))
    assert not failed, "%d failures in %d runs: %s" % (len(failed), nruns, "; ".join(failed[:8]))
    want = set(cs.FEASIBLE[mode]) if mode != 2 else {(f, s) for f, _ in cs.FEASIBLE[2] for s in ("S=1", "S>1")}
    assert set(taken) == want, "forms not taken: %s" % sorted(want - set(taken), key=str)


# ================================================================================================= 2. bitwise invariants
@pytest.mark.parametrize("mode", (0, 1), ids=["forward", "dgrad"])
def test_a_sample_of_a_batch_has_the_bits_of_its_own_call(ops, mode):
    """Every output element sums the same products in the same order whatever the batch around it."""
    failed, n_checked = [], 0
    for case in cs.CASES:
        if case[0] == 1:
            continue
        run = Run(case, mode)
        inp, out = run.call()
        m, nn = inp["ref"].shape
        per = m // case[0]
        one = (1,) + case[1:]
        assert cs.form_of(one, mode) == cs.form_of(case, mode)
        g = cs.geometry(case, mode)
        for b in range(case[0]):
            o1 = dev(np.full(cs.PRE + per * nn + cs.POST, cs.SENT, dtype=np.float32))
            conv_gemm((run.src, inp["src0"] + b * g["Hs"] * g["Ws"] * g["Cs"]), (run.oth, inp["oth0"]), (o1, cs.PRE), None, mode,
                      one, 1)
            torch.cuda.synchronize()
            got = o1.cpu().numpy()
            want = out[inp["out0"] + b * per * nn:inp["out0"] + (b + 1) * per * nn]
            n_checked += 1
            if not np.array_equal(bits(got[cs.PRE:cs.PRE + per * nn]), bits(want)):
                failed.append("%s mode %d sample %d" % (cs.name(case), mode, b))
            if not ((got[:cs.PRE] == cs.SENT).all() and (got[cs.PRE + per * nn:] == cs.SENT).all()):
                failed.append("%s mode %d sample %d: floats beside the output changed" % (cs.name(case), mode, b))
    print("%d single-sample calls" % n_checked)
    assert not failed, "; ".join(failed[:8])


@pytest.mark.parametrize("mode", (0, 2), ids=["forward", "wgrad"])
def test_padding_has_the_bits_of_explicit_zeros(ops, mode):
    """x with padding (PH, PW) against x with zero rows and columns written out and padding 0: the same GEMM shape, K order,
    form and splits; a masked tap and a tap that reads a zero add the same +0 product."""
    failed, n_checked = [], 0
    for case in cs.CASES:
        n, h, w, cin, cout, kh, kw, sh, sw, ph, pw = case
        if ph == 0 and pw == 0:
            continue
        x, wt, dy = cs.tensors(case)
        xp = np.zeros((n, h + 2 * ph, w + 2 * pw, cin), dtype=np.float32)
        xp[:, ph:ph + h, pw:pw + w] = x
        padded = (n, h + 2 * ph, w + 2 * pw, cin, cout, kh, kw, sh, sw, 0, 0)
        assert cs.out_hw(padded) == cs.out_hw(case)
        run = Run(case, mode)
        xpd = dev(xp.reshape(-1))
        for splits in (cs.SPLITS if mode == 2 else (1,)):
            inp, out = run.call(splits)
            p, pp = inp["plan"], cs.plan(padded, mode, splits)
            assert (pp["pixel"], pp["klen"], pp["splits"], pp["M"], pp["Nn"], pp["K"]) == (
                p["pixel"], p["klen"], p["splits"], p["M"], p["Nn"], p["K"])
            size = p["M"] * p["Nn"]
            o1 = dev(np.full(size, cs.SENT, dtype=np.float32))
            slabs = dev(np.full(p["splits"] * size, np.nan, dtype=np.float32)) if mode == 2 else None
            conv_gemm((xpd, 0), (run.oth, inp["oth0"]), (o1, 0), (slabs, 0) if slabs is not None else None, mode, padded, splits)
            torch.cuda.synchronize()
            n_checked += 1
            if not np.array_equal(bits(o1.cpu().numpy()), bits(out[inp["out0"]:inp["out0"] + size])):
                failed.append("%s mode %d splits %d" % (cs.name(case), mode, splits))
    print("%d padded / explicit pairs" % n_checked)
    assert not failed, "; ".join(failed[:8])


# =================================================================================================== 2b. the 2^29 switch
@pytest.mark.parametrize("mode", (0, 1), ids=["forward", "dgrad"])
def test_gather_at_the_2_pow_29_switch(ops, mode):
    """The one size in the module that is not small, because the fault it looks for exists only there: 16 x 64 x 128-channel
    samples of 2^17 floats.  4095 of them are the last batch the host gives the descriptor gather (byte offsets up to
    2^31 - 2^19, plus the tap in the scalar offset); with 4096 the source is 2^29 floats and the same launch takes the carried
    triple with 64-bit addresses -- in mode 0 the only way to that form.  The first, the middle and the last sample hold the
    oracle's data for N = 1: they must pass ``check`` against float64 and have the bits of the small N = 1 call, in both forms;
    the samples between are random."""
    h, w = 16, 64
    cin, cout = (128, 4) if mode == 0 else (4, 128)
    one = (1, h, w, cin, cout, 3, 3, 1, 1, 1, 1)
    small = Run(one, mode)
    inp1, out1 = small.call()
    assert inp1["plan"]["pixel"] == "GA"
    ratio = cs.check(one, mode, inp1, out1)
    per_src, per_out, front, o0 = h * w * 128, h * w * 4, inp1["src0"], inp1["out0"]
    want = out1[o0:o0 + per_out]
    buf = torch.full((front + 4096 * per_src + cs.POST,), float("nan"), dtype=torch.float32, device="cuda:0")
    try:
        buf[front:front + 4096 * per_src].normal_()
        sample = small.src[front:front + per_src]
        for b in (0, 2047, 2048, 4094, 4095):
            buf[front + b * per_src:front + (b + 1) * per_src] = sample
        for n, form in ((4095, "GA"), (4096, "carry")):
            big = (n,) + one[1:]
            assert lib_plan(big, mode, 1) == cs.plan_row(big, mode, 1)
            assert cs.plan(big, mode)["pixel"] == form
            out = torch.full((cs.PRE + n * per_out + cs.POST,), float(cs.SENT), dtype=torch.float32, device="cuda:0")
            conv_gemm((buf, front), (small.oth, inp1["oth0"]), (out, cs.PRE), None, mode, big, 1)
            torch.cuda.synchronize()
            for b in (0, n // 2, n - 1):
                got = out[cs.PRE + b * per_out:cs.PRE + (b + 1) * per_out].cpu().numpy()
                whole = inp1["outbuf"].copy()
                whole[o0:o0 + per_out] = got
                ratio = max(ratio, cs.check(one, mode, inp1, whole))
                assert np.array_equal(bits(got), bits(want)), "N %d (%s), sample %d: not the bits of the N = 1 call" % (n, form, b)
            assert bool((out[:cs.PRE] == float(cs.SENT)).all()) and bool((out[cs.PRE + n * per_out:] == float(cs.SENT)).all())
            assert bool(torch.isfinite(out).all())
            del out
        print("mode %d: worst err / bound %.3f" % (mode, ratio))
    finally:
        del buf
        torch.cuda.empty_cache()


# ================================================================================================== 3. ops.conv_gemm, ConvFn
@pytest.mark.parametrize("case", OPS_SHAPES, ids=cs.name)
def test_ops_and_convfn_return_the_bits_of_the_direct_calls(ops, case):
    from adyolo_amd import functional as Fn
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw = case
    ho, wo = cs.out_hw(case)
    x, wt, dy = (dev(t) for t in cs.tensors(case))
    kp = cs.geometry(case, 0)["K"]
    splits = ops.wgrad_splits(cout, kp, n * ho * wo)
    assert splits == (2 if case == BIG else 1)
    direct = {}
    for mode in cs.MODES:
        run = Run(case, mode)
        inp, out = run.call(splits if mode == 2 else 1)
        ratio = cs.check(case, mode, inp, out)
        print("%s mode %d: err / bound %.3f (%s)" % (cs.name(case), mode, ratio, inp["plan"]["pixel"]))
        direct[mode] = out[inp["out0"]:inp["out0"] + inp["ref"].size].reshape(inp["ref"].shape)
    wk, wkt = ops.pack_wk(wt), ops.pack_wk(wt.transpose(0, 1).contiguous())
    y = ops.conv_gemm(0, x, wk, *case)
    dx = ops.conv_gemm(1, dy, wkt, *case)
    dwk = ops.conv_gemm(2, x, dy, *case)
    assert tuple(y.shape) == (n, ho, wo, cout) and tuple(dx.shape) == (n, h, w, cin) and tuple(dwk.shape) == (cout, kp)
    for what, t, mode in (("y", y, 0), ("dx", dx, 1), ("dwk", dwk, 2)):
        assert np.array_equal(bits(t.cpu().numpy().reshape(direct[mode].shape)), bits(direct[mode])), "ops.conv_gemm %s" % what
    xg, wg = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y2 = Fn.ConvFn.apply(xg, wg, (sh, sw), (ph, pw))
    y2.backward(dy)
    torch.cuda.synchronize()
    assert np.array_equal(bits(y2.detach().cpu().numpy().reshape(direct[0].shape)), bits(direct[0])), "ConvFn y"
    assert np.array_equal(bits(xg.grad.cpu().numpy().reshape(direct[1].shape)), bits(direct[1])), "ConvFn dx"
    assert np.array_equal(bits(wg.grad.cpu().numpy()), bits(cs.unpack_wk(direct[2], cout, cin, kh, kw))), "ConvFn dw"


# ==================================================================================================== 4. pack_wk / unpack_wk
@pytest.mark.parametrize("shape", [(64, 32, 3, 3), (20, 12, 3, 3), (8, 8, 5, 3), (64, 8, 7, 7), (8, 3, 7, 7), (4, 4, 1, 1)],
                         ids=lambda s: "x".join(map(str, s)))
def test_pack_wk_is_the_permutation(ops, shape):
    """Plain and transposed (the data gradient's filter), against the NumPy permutation bit for bit, and back.  Cin = 3: the
    row is padded to a multiple of 4 with a zero."""
    rng = np.random.default_rng(sum(shape))
    w = rng.standard_normal(shape).astype(np.float32)
    for src in (w, np.ascontiguousarray(w.transpose(1, 0, 2, 3))):
        cout, cin, kh, kw = src.shape
        wk = ops.pack_wk(dev(src))
        assert tuple(wk.shape) == (cout, cs.cdiv(kh * kw * cin, 4) * 4)
        assert np.array_equal(bits(wk.cpu().numpy()), bits(cs.pack_wk(src)))
        guard = dev(np.full(src.size + 32, cs.SENT, dtype=np.float32))
        back = ops.unpack_wk(wk, cout, cin, kh, kw, out=guard[16:16 + src.size].view(cout, cin, kh, kw))
        torch.cuda.synchronize()
        assert np.array_equal(bits(back.cpu().numpy()), bits(src))
        gh = guard.cpu().numpy()
        assert (gh[:16] == cs.SENT).all() and (gh[16 + src.size:] == cs.SENT).all()


# =============================================================================================================== 5. refusals
def test_refusals_come_before_any_launch(ops):
    from adyolo_amd import _lib
    a = dev(np.ones(8192, dtype=np.float32))
    b = dev(np.ones(8192, dtype=np.float32))
    c = dev(np.full(8192, cs.SENT, dtype=np.float32))
    slabs = dev(np.full(8192, cs.SENT, dtype=np.float32))
    ok = (1, 4, 4, 8, 8, 3, 3, 1, 1, 1, 1)
    refused = {
        "Cin % 4": (0, (1, 4, 4, 6, 8, 3, 3, 1, 1, 1, 1), 1, -2),
        "Cout % 4": (0, (1, 4, 4, 8, 6, 3, 3, 1, 1, 1, 1), 1, -2),
        "empty output": (0, (1, 1, 4, 8, 8, 3, 3, 1, 1, 0, 1), 1, -1),
        "empty output, kernel one row taller than the map under stride 2": (0, (1, 2, 4, 8, 8, 3, 3, 2, 1, 0, 1), 1, -1),
        "mode 3": (3, ok, 1, -1),
        "splits > 1 without slabs": (2, ok, 2, -1),
    }
    for what, (mode, case, splits, code) in refused.items():
        with pytest.raises(_lib.AdyoloHipError, match=r"rc=%d\b" % code):
            conv_gemm((a, 0), (b, 0), (c, 0), None, mode, case, splits)
            pytest.fail("%s was not refused" % what)
        if what != "splits > 1 without slabs":                       # the plan entry takes no pointers: it refuses the rest alike
            with pytest.raises(_lib.AdyoloHipError, match=r"rc=%d\b" % code):
                lib_plan(case, mode, splits)
        torch.cuda.synchronize()
        untouched = bool((c == float(cs.SENT)).all()) and bool((slabs == float(cs.SENT)).all())
        assert untouched, "%s: refused, yet the output changed" % what
    with pytest.raises(_lib.AdyoloHipError, match=r"rc=-2\b"):             # a tensor of 2^31 elements (host arithmetic only)
        lib_plan((16384, 16, 64, 128, 4, 3, 3, 1, 1, 1, 1), 0, 1)
    assert lib_plan((16383, 16, 64, 128, 4, 3, 3, 1, 1, 1, 1), 0, 1) == cs.plan_row((16383, 16, 64, 128, 4, 3, 3, 1, 1, 1, 1), 0)
    conv_gemm((a, 0), (b, 0), (c, 0), (slabs, 0), 2, ok, 2)                # the same call with slabs goes through
    torch.cuda.synchronize()
    assert bool((c[:8 * 72] != float(cs.SENT)).all()) and bool((c[8 * 72:] == float(cs.SENT)).all())
