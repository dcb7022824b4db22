"""GPU tests of the 3x3 forward / data-gradient convolution (run with ``-m gpu`` on an MI355X): ``conv3x3_fwd_kernel<KC,BN,TW>`` and
``stem_fwd_kernel`` (csrc/conv.hip), ``wino_fwd_kernel<NT,ONE>`` (csrc/wino.hip), ``wino4_fwd_kernel<TC,AFF>`` (csrc/wino4.hip) and
the persistent ``wino4p_fwd_kernel<TC,AFF,EPI,NB,BRES,FULL,MKM>`` (csrc/wino4p.hpp), called through the three C entry points with
buffers the test owns, against float64.  Cases, inputs, references, bound and checker: oracle/fwd_stage.py, pinned on the CPU by
tests/test_fwd_stage_cpu.py.

Every case: x, addend and aux are 16-byte-aligned views into NaN-filled buffers with eight image rows of NaN either side; scale,
shift, bias, mean, invstd and masks given as floats are views into NaN-filled buffers; masks given as bits sit between words of
all ones; y and stats are pre-filled with NaN between sentinel guard words.  A read outside an operand that reaches a result, an
element of y or stats nobody wrote, or a store outside them fails the case.  The bar is derived, not measured (the module docstring
of the oracle has the derivation):

    |got - ref| <= c * 2^-24 * S        S: the algorithm evaluated on absolute values, c: the roundings on a term's way

the per-patch sums are compared patch by patch with the float64 sums of the y the launch wrote, and a second identical call and the
same call on a side stream must give the same bits.  Before it runs, every case asserts the oracle's mirror of the host decisions
against ``adyolo_conv_fwd_plan`` with the device's CU count: the persistent kernel's walks are what the mirror says.

Worst err / bound of y on an MI355X (13 tests over 116 cases, each run three times; 9 s): direct 0.124, stem 0.167, F(2x2) 0.088,
F(4x4) 0.059 (one-patch and persistent, walks of up to three patches in each of the eight bodies); per-patch sums 0.023, 0.017,
0.054, 0.016.  No kernel missed its bound, left an element of y or stats unwritten or NaN, touched a guard word, put a patch's sums
into another slot or differed between calls or streams; DESIGN.md (K2-fwd) has the table."""
import ctypes
import time

import numpy as np
import pytest
import torch

from oracle import fwd_stage as fs
from oracle import seresnet as onet

pytestmark = pytest.mark.gpu

ROWS_OF_NAN = 8                               # image rows of NaN in front of and behind x, addend and aux
ENTRY = {"direct": "adyolo_conv3x3_fwd", "stem": "adyolo_conv3x3_fwd", "wino2": "adyolo_wino_fwd", "wino4": "adyolo_wino4_fwd"}
# what ops.conv3x3 logs: it names a launch by its entry point and does not tell the stem kernel from conv3x3_fwd_kernel
OPS_NAME = {1: "conv3x3_fwd_kernel", 2: "conv3x3_fwd_kernel", 3: "wino_fwd_kernel", 4: "wino4_fwd_kernel", 5: "wino4p_fwd_kernel"}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def ncus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    return t


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def embed(a, guard):
    """a (float32 array) as a view into a NaN-filled device buffer with ``guard`` floats (a multiple of 4) either side."""
    assert guard % 4 == 0
    buf = torch.full((a.size + 2 * guard,), float("nan"), dtype=torch.float32, device="cuda:0")
    view = buf[guard:guard + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.data_ptr() % 16 == 0
    return buf, view


def embed_bits(mask):
    """A bool mask as the int64 words the kernels read, between 64 words of all ones either side."""
    words = onet.pack_relu_bits(mask)
    buf = torch.full((words.size + 128,), -1, dtype=torch.int64, device="cuda:0")
    view = buf[64:64 + words.size]
    view.copy_(torch.from_numpy(words))
    return buf, view


def lib_plan(form, n, h, w, cin, cout, operands, mask_bits, affine):
    from adyolo_amd import _lib
    out = (ctypes.c_int * 24)(*([-1] * 24))
    _lib.call("adyolo_conv_fwd_plan", fs.FORM_ID[form], n, h, w, cin, cout, operands, mask_bits, int(affine), out)
    return list(out)


def pack(case, inp):
    """The filter pack the launch reads, made by the pack entry point of the form (forward or data-gradient direction)."""
    from adyolo_amd import _lib
    from adyolo_amd.ops import _p, _stream
    w = dev(inp["wt"])
    lout, lin = w.shape[0], w.shape[1]                   # the layer's channel counts
    lin_pad = case["cout"] if case["dgrad"] else case["cin"]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda:0")      # noqa: E731
    if case["form"] in ("direct", "stem"):
        wf, wd = nan(lout, 9, lin_pad), nan(lin_pad, 9, lout)
        _lib.call("adyolo_pack_w3x3", _p(w), _p(wf), _p(wd), lout, lin, lin_pad, _stream())
    else:
        points = 16 if case["form"] == "wino2" else 36
        wf, wd = nan(points, lout // 32, lin_pad // 8, 256), nan(points, lin_pad // 32, lout // 8, 256)
        _lib.call("adyolo_wino_pack_w" if points == 16 else "adyolo_wino4_pack_w", _p(w), _p(wf), _p(wd), lout, lin, lin_pad, _stream())
    got = wd if case["dgrad"] else wf
    assert not torch.isnan(got).any()
    return got


class Operands:
    """The device operands of a case, uploaded once; ``run`` makes one call into fresh NaN-filled outputs."""

    def __init__(self, case, inp):
        self.case, self.plan = case, fs.case_plan(case, ncus())
        w, cin, cout, epi = case["w"], case["cin"], case["cout"], case["epi"]
        self.keep = []

        def up(a, guard):
            self.keep.append(embed(a, guard))
            return self.keep[-1][1]

        def mask(name):
            if case["maskform"] == "bits":
                self.keep.append(embed_bits(inp[name]))
                return self.keep[-1][1]
            return up(fs.float_mask(inp[name], case["seed"] + len(name)), ROWS_OF_NAN * w * cout)
        self.x = up(inp["x"], ROWS_OF_NAN * w * cin)
        self.wpk = pack(case, inp)
        self.bias = up(inp["bias"], 64) if case["bias"] else None
        self.sc, self.sh = (up(inp["scale"], 64), up(inp["shift"], 64)) if case["affine"] else (None, None)
        self.addend = up(inp["addend"], ROWS_OF_NAN * w * cout) if epi & fs.ADDEND else None
        self.amask = mask("amask") if epi & fs.ADDEND_MASK else None
        self.aux, self.mean, self.invstd = (up(inp["aux"], ROWS_OF_NAN * w * cout), up(inp["mean"], 64), up(inp["invstd"], 64)) \
            if epi & fs.STAT_AUX else (None, None, None)
        self.smask = mask("smask") if epi & fs.STAT_MASK else None

    def call(self, y, stats, over=None):
        """One call of the case's entry point; ``over``: arguments replaced (the refusal tests)."""
        from adyolo_amd import _lib
        from adyolo_amd.ops import _p, _stream
        cs = self.case
        a = {"x": self.x, "wpk": self.wpk, "bias": self.bias, "addend": self.addend, "amask": self.amask, "sc": self.sc, "sh": self.sh,
             "y": y, "stats": stats, "aux": self.aux, "mean": self.mean, "invstd": self.invstd, "smask": self.smask, "n": cs["n"],
             "h": cs["h"], "w": cs["w"], "cin": cs["cin"], "cout": cs["cout"], "relu": int(cs["relu"]), "mask_bits": fs.case_mask_bits(cs)}
        a.update(over or {})
        _lib.call(ENTRY[cs["form"]], _p(a["x"]), _p(a["wpk"]), _p(a["bias"]), _p(a["addend"]), _p(a["amask"]), _p(a["sc"]), _p(a["sh"]),
                  _p(a["y"]), _p(a["stats"]), _p(a["aux"]), _p(a["mean"]), _p(a["invstd"]), _p(a["smask"]), a["n"], a["h"], a["w"],
                  a["cin"], a["cout"], a["relu"], a["mask_bits"], _stream())

    def outputs(self):
        ybuf = dev(fs.new_buffer(fs.y_floats(self.case)))
        nst = fs.stats_floats(self.case, self.plan)
        sbuf = dev(fs.new_buffer(nst)) if nst else None
        return ybuf, sbuf

    def run(self):
        """-> (the whole y buffer, the whole stats buffer or None) after one call on the current stream."""
        ybuf, sbuf = self.outputs()
        self.call(ybuf[fs.GUARD:], sbuf[fs.GUARD:] if sbuf is not None else None)
        return ybuf, sbuf


FAULTED = []              # a HIP error (not a failed assertion) in a call: nothing more is launched by this module


def run_case(cs):
    """Mirror == library (a HIP error ends the module's launches: ``guarded_case``); three calls (twice on the current stream, once on a side stream) checked by value and bit for bit.
    -> worst err / bound of y"""
    from adyolo_amd import _lib
    case, inp, ref, bnd = fs.prepared(cs["name"])
    p = fs.case_plan(case, ncus())
    got = lib_plan(case["form"], case["n"], case["h"], case["w"], case["cin"], case["cout"], fs.case_operands(case), fs.case_mask_bits(case),
                   case["affine"])
    assert got == fs.plan_out24(p), "%s: the library plans %s, the mirror %s" % (case["name"], got, fs.plan_out24(p))
    assert p["kernel"], "%s is refused" % case["name"]
    op = Operands(case, inp)
    ybuf, sbuf = op.run()
    torch.cuda.synchronize()
    if case["form"] == "wino4":
        assert _lib.load().adyolo_wino4_last_form() == p["kernel"] - 3, "%s: the other F(4x4) kernel ran" % case["name"]
    ratio = fs.check(case, inp, ref, bnd, ybuf.cpu().numpy(), sbuf.cpu().numpy() if sbuf is not None else None)
    run_case.sums = fs.LAST.get("stats_ratio", 0.0)
    again = op.run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = op.run()
    side.synchronize()
    torch.cuda.synchronize()
    for what, (y2, s2) in (("a second identical call", again), ("the same call on a side stream", other)):
        assert torch.equal(bits(y2), bits(ybuf)), "%s: %s differs in y" % (case["name"], what)
        assert sbuf is None or torch.equal(bits(s2), bits(sbuf)), "%s: %s differs in stats" % (case["name"], what)
    return ratio


def guarded_case(cs):
    assert not FAULTED, "not run: %s raised %s before" % tuple(FAULTED[:2])
    try:
        return run_case(cs)
    except AssertionError:
        raise
    except Exception as e:
        FAULTED.extend([cs["name"], repr(e)[:200]])
        raise


# ================================================================================================================ the plan
def test_coverage_holds_with_this_devices_cu_count(ops):
    n = ncus()
    table = fs.coverage(n)                                    # a lost branch fails by name
    for body in fs.PERSISTENT_BODIES:
        assert table["wino4"]["%s:walk3plus" % body], body
    print("%d CUs: %d cases, every branch reached" % (n, len(fs.cases())))


def test_plan_mirror_agrees_with_the_library_beyond_the_cases(ops):
    n = ncus()
    shapes = set()
    for form in fs.FORMS:
        for s in ((2, 16, 16, 48, 32), (2, 16, 16, 32, 48), (2, 16, 16, 544, 64), (2, 13, 17, 32, 64), (2, 16, 16, 8, 32), (2, 16, 40, 8, 32),
                  (2, 16, 40, 8, 64), (1, 2048, 2048, 64, 64), (1, 4096, 2048, 64, 64), (3, 64, 64, 32, 32), (3, 64, 8, 64, 128),
                  (3, 64, 3, 128, 256), (300, 16, 32, 64, 384), (5, 200, 72, 32, 32), (5, 200, 72, 32, 64), (5, 200, 72, 64, 128)):
            for operands, mbits in ((0, 0), (1, 0), (2, 0), (9, 0), (15, 1), (15, 0), (27, 3), (27, 1), (31, 3), (31, 0), (33, 0), (3, 0),
                                    (5, 1), (8, 0), (17, 2)):
                for affine in (0, 1):
                    shapes.add((form,) + s + (operands, mbits, affine))
    for s in sorted(shapes):
        assert lib_plan(*s) == fs.plan_out24(fs.plan(*s, ncus=n)), s
    print("%d launches planned" % len(shapes))


def test_refusals_come_before_anything_is_written(ops):
    from adyolo_amd import _lib
    seen = []
    for form, epi, mf in (("direct", 31, "float"), ("wino2", 31, "float"), ("wino4", 31, "float"), ("wino4", 31, "bits")):
        cout = 32 if mf == "bits" else 64
        case = fs.make_case(form, 2, 16, 16, 32, cout, epi=epi, maskform=mf)
        inp = fs.build(case)
        op = Operands(case, inp)
        ybuf, sbuf = op.outputs()
        y, st = ybuf[fs.GUARD:], sbuf[fs.GUARD:]
        refused = {"Cin = 48": {"cin": 48}, "Cout = 48": {"cout": 48}, "mask bits with H W Cout / 4 % 64 != 0": {"h": 13, "w": 17, "mask_bits": 3},
                   "addend_mask without addend": {"addend": None}, "stat_aux without statistics": {"stats": None},
                   "stat_mask without statistics": {"stats": None, "aux": None, "mean": None, "invstd": None},
                   "scale without shift": {"sc": op.x[0, 0, 0]}}
        if form != "direct":
            refused["Cin = 544"] = {"cin": 544}
        if form == "wino4" and mf == "bits":                  # a 32-channel block: the persistent kernel or none
            refused["32 channels with a bias"] = {"bias": op.x[0, 0, 0]}
            refused["32 channels with float masks"] = {"mask_bits": 0}
            refused["32 channels with an operand set that is not built"] = {"amask": None, "smask": None, "mask_bits": 0, "aux": None,
                                                                            "mean": None, "invstd": None}
        for what, over in refused.items():
            with pytest.raises(_lib.AdyoloHipError):
                op.call(y, st, over)
                pytest.fail("%s %s was not refused" % (form, what))
            seen.append((form, what))
        torch.cuda.synchronize()
        assert np.array_equal(ybuf.cpu().numpy().view(np.int32), fs.new_buffer(fs.y_floats(case)).view(np.int32)), form
        assert np.array_equal(sbuf.cpu().numpy().view(np.int32), fs.new_buffer(fs.stats_floats(case)).view(np.int32)), form
        op.call(y, st)                                        # the call as the case states it goes through
        torch.cuda.synchronize()
        fs.check(case, inp, fs.reference(case, inp), fs.roundings(case) * fs.U * fs.magnitude(case, inp), ybuf.cpu().numpy(),
                 sbuf.cpu().numpy())
    # the refused case of the list: 32 -> 32 with float masks has no F(4x4) kernel
    cs = next(c for c in fs.CASES if c["name"] == fs.REFUSED_CASES[0])
    assert lib_plan("wino4", cs["n"], cs["h"], cs["w"], cs["cin"], cs["cout"], cs["epi"], 0, 1) == [0] * 24
    print("%d refusals" % len(seen))


# ================================================================================================================== values
@pytest.mark.parametrize("form", fs.FORMS)
def test_every_case_against_float64(ops, form):
    worst, failed, worst_sums = (0.0, None), [], 0.0
    cases = fs.cases(form)
    t0 = time.time()
    for cs in cases:
        try:
            ratio = guarded_case(cs)
            worst_sums = max(worst_sums, run_case.sums)
            print("%-58s err / bound %.3f  (c = %d)" % (cs["name"], ratio, fs.roundings(cs)))
            if ratio > worst[0]:
                worst = (ratio, cs["name"])
        except AssertionError as e:
            print("%-58s FAILED" % cs["name"])
            failed.append(str(e).splitlines()[0])
    cvals = [fs.roundings(c) for c in cases]
    print("%s: %d cases, c %d .. %d, worst err / bound %.3f at %s, per-patch sums %.3f, %.1f s" % (
        form, len(cases), min(cvals), max(cvals), worst[0], worst[1], worst_sums, time.time() - t0))
    assert not failed, "%d of %d: %s" % (len(failed), len(cases), "; ".join(failed[:8]))


# ============================================================================================================== through ops
OPS_CASES = (("direct_2x19x45_c64_96_e27_float_relu", "direct"), ("stem_3x5x70_c8_32_e1_bias_relu", "direct"),
             ("wino2_3x9x20_c64_128_e1_aff", "winograd"), ("wino4_2x21x40_c64_64_e1_bias_relu", "winograd4"),
             ("wino4_65x33x17_c32_64_e0", "winograd4"), ("wino4_29x33x65_c32_32_e1_aff", "winograd4"))


@pytest.mark.parametrize("name,algo", OPS_CASES, ids=[c[0] for c in OPS_CASES])
def test_ops_conv3x3_logs_the_kernel_the_mirror_predicts(ops, monkeypatch, name, algo):
    """``ops.conv3x3`` with a pack made by ``ops.pack_w3x3``: ``ops.DISPATCH_LOG`` names the kernel of the mirror's plan, and y
    passes the case's check."""
    monkeypatch.setenv("ADYOLO_W4_MIN_K", "32")
    monkeypatch.setenv("ADYOLO_W4_MIN_K_32", "32")
    case, inp, ref, bnd = fs.prepared(name)
    assert not case["dgrad"]
    p = fs.case_plan(case, ncus())
    op = Operands(case, inp)
    wpk, _ = ops.pack_w3x3(dev(inp["wt"]), case["cin"], want_dgrad=False, algo=algo, allow32=True)
    log = {}
    monkeypatch.setattr(ops, "DISPATCH_LOG", log)
    kw = {"want_stats": bool(case["epi"] & fs.STATS), "relu": case["relu"], "bias": op.bias, "addend": op.addend, "addend_mask": op.amask,
          "in_affine": (op.sc, op.sh) if case["affine"] else None, "stat_mask": op.smask,
          "stat_bn": (op.aux, op.mean, op.invstd) if case["epi"] & fs.STAT_AUX else None}
    out = ops.conv3x3(op.x, wpk, case["cout"], **kw)
    torch.cuda.synchronize()
    y, st = out if kw["want_stats"] else (out, None)
    assert list(log) == [(OPS_NAME[p["kernel"]], case["cin"], case["cout"], case["epi"])] and list(log.values()) == [1], log
    ybuf = fs.new_buffer(fs.y_floats(case))
    ybuf[fs.GUARD:-fs.GUARD] = y.cpu().numpy().reshape(-1)
    sbuf = None
    if st is not None:
        assert tuple(st.shape) == (2, p["nsp"], case["cout"])
        sbuf = fs.new_buffer(fs.stats_floats(case, p))
        sbuf[fs.GUARD:-fs.GUARD] = st.cpu().numpy().reshape(-1)
    fs.check(case, inp, ref, bnd, ybuf, sbuf)
