"""GPU tests of the 3x3 weight gradient (run with ``-m gpu`` on an MI355X): ``conv3x3_wgrad_kernel<TW>`` and ``stem_wgrad_kernel``
(csrc/conv.hip), ``wino_wgrad_kernel<NT,RAGGED>`` (csrc/wino.hip), ``wino4_wgrad_kernel<AFF,NB>`` (csrc/wino4w.hip) with their
slab-reduce and finish kernels, called through the C entry points with buffers the test owns, against float64; and the filter
packing launches every forward pass starts with.  Cases, inputs, references, bound and checker: oracle/wgrad_stage.py, pinned on
the CPU by tests/test_wgrad_stage_cpu.py.

Every case: x, dy, scale and shift are 16-byte-aligned views into NaN-filled buffers (eight image rows of NaN either side of x and
dy), slabs, du and dw are pre-filled with NaN, dw sits between sentinel guard words.  A read outside an operand that reaches an
accumulator, a slab / du / dw element the reduce and finish kernels read but nobody wrote, or a store outside dw fails the case.
The bar is derived, not measured (the module docstring of the oracle has the derivation):

    |got - ref| <= c(form) * 2^-24 * S        S: the algorithm evaluated on absolute values, c: the roundings on a term's way

and a second identical call and the same call on a side stream must give the same bits.

Worst err / bound on an MI355X (19 tests over 77 cases, each run three times; 6.8 s): direct 0.204, stem 0.301, F(2x2) 0.093,
F(4x4) 0.062; packs 0.551 (one rounding of the F(4x4) form against its c = 2).  No kernel missed its bound, left a NaN in a slab, in
du or in dw, touched a guard word or differed between calls or streams; DESIGN.md (K2-wgrad) has the table.  One read outside an
operand that no value check can see is described there too (the F(4x4) kernel's prologue, last segment of a single step)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import wgrad_stage as ws

pytestmark = pytest.mark.gpu

ROWS_OF_NAN = 8                               # image rows of NaN in front of and behind x and dy


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


def lib_plan(form, n, h, w, cin, cout):
    from adyolo_amd import _lib
    out = (ctypes.c_int * 8)(*([-1] * 8))
    _lib.call("adyolo_wgrad_plan", ws.FORM_ID[form], n, h, w, cin, cout, out)
    return list(out)


def lib_slabs(form, n, h, w, cin, cout):
    from adyolo_amd import _lib
    fn = {"direct": "adyolo_conv3x3_wgrad_slabs", "stem": "adyolo_conv3x3_wgrad_slabs", "wino2": "adyolo_wino_wgrad_slabs",
          "wino4": "adyolo_wino4_wgrad_slabs"}[form]
    return getattr(_lib.load(), fn)(n, h, w, cin, cout)


class Operands:
    """The device operands of a case, uploaded once; ``run`` makes one call into fresh NaN-filled workspaces."""

    def __init__(self, case, inp):
        self.case = case
        n, h, w, cin, cout = (case[k] for k in ("n", "h", "w", "cin", "cout"))
        self.keep = [embed(inp["x"], ROWS_OF_NAN * w * cin), embed(inp["dy"], ROWS_OF_NAN * w * cout)]
        self.x, self.dy = self.keep[0][1], self.keep[1][1]
        self.sc = self.sh = None
        if case["affine"]:
            self.keep += [embed(inp["scale"], 64), embed(inp["shift"], 64)]
            self.sc, self.sh = self.keep[2][1], self.keep[3][1]
        p = ws.case_plan(case)
        self.points = {"wino2": 16, "wino4": 36}.get(case["form"])
        if self.points:
            self.slab_floats = p["nsplit"] * self.points * cin * cout
        elif case["form"] == "stem":
            self.slab_floats = p["nblk"] * 32 * 72
        else:
            self.slab_floats = p["nsplit"] * cout * 9 * ws.cdiv(cin, 32) * 32

    def run(self):
        """-> (the whole dw buffer, slabs, du) after one call on the current stream."""
        from adyolo_amd import _lib
        from adyolo_amd.ops import _p, _stream
        cs = self.case
        n, h, w, cin, cout = (cs[k] for k in ("n", "h", "w", "cin", "cout"))
        slabs = torch.full((self.slab_floats + 64,), float("nan"), dtype=torch.float32, device="cuda:0")
        dwbuf = dev(ws.new_dw_buffer(cs))
        dw = dwbuf[ws.GUARD:]
        du = None
        if self.points:
            du = torch.full((self.points * cin * cout,), float("nan"), dtype=torch.float32, device="cuda:0")
            fn = "adyolo_wino_wgrad" if cs["form"] == "wino2" else "adyolo_wino4_wgrad"
            _lib.call(fn, _p(self.x), _p(self.dy), _p(self.sc), _p(self.sh), _p(slabs), _p(du), _p(dw), n, h, w, cin,
                      cs["cin_real"], cout, _stream())
        else:
            _lib.call("adyolo_conv3x3_wgrad", _p(self.x), _p(self.dy), _p(self.sc), _p(self.sh), _p(slabs), _p(dw), n, h, w, cin,
                      cs["cin_real"], cout, _stream())
        return dwbuf, slabs, du


def run_case(cs):
    """Three calls (twice on the current stream, once on a side stream) checked by value, for unwritten workspace and bit for
    bit.  -> worst err / bound"""
    case, inp, ref, bnd = ws.prepared(cs["name"])
    op = Operands(case, inp)
    dwbuf, slabs, du = op.run()
    torch.cuda.synchronize()
    assert torch.isnan(slabs[op.slab_floats:]).all(), "%s: floats behind the slabs were written" % case["name"]
    holes = int(torch.isnan(slabs[:op.slab_floats]).sum())
    assert holes == 0, "%s: %d of %d slab elements the reduce kernel reads were never written (or are NaN)" % (
        case["name"], holes, op.slab_floats)
    if du is not None:
        holes = int(torch.isnan(du).sum())
        assert holes == 0, "%s: %d du elements the finish kernel reads were never written" % (case["name"], holes)
    ratio = ws.check(case, ref, bnd, dwbuf.cpu().numpy())
    again = op.run()[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = op.run()[0]
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(bits(again), bits(dwbuf)), "%s: a second identical call differs" % case["name"]
    assert torch.equal(bits(other), bits(dwbuf)), "%s: the same call on a side stream differs" % case["name"]
    return ratio


# ================================================================================================================ the plan
def test_plan_mirror_agrees_with_the_library(ops):
    shapes = {(c["form"], c["n"], c["h"], c["w"], c["cin"], c["cout"]) for c in ws.cases()}
    # refusals and fall-backs of the F(4x4) kernel: H % 4, H < 8, W not in {4, 8} and not a multiple of 16, channels; 2 GiB
    shapes |= {("wino4",) + s for s in ((2, 10, 16, 32, 32), (2, 4, 16, 32, 32), (2, 16, 24, 32, 32), (2, 16, 12, 32, 32),
                                         (2, 16, 16, 48, 32), (64, 512, 64, 256, 256), (63, 512, 64, 256, 256))}
    shapes |= {("wino2", 2, 16, 16, 48, 32), ("stem", 2, 16, 16, 8, 64), ("stem", 2, 16, 16, 32, 32), ("direct", 2, 16, 16, 8, 32),
               ("direct", 2, 16, 16, 32, 48)}
    for s in sorted(shapes):
        p = ws.plan(*s)
        assert lib_plan(*s) == ws.plan_out8(p), s
        if s[0] != "stem" or p["supported"]:
            want = p["nsplit"] if p["supported"] else 0
            got = lib_slabs(*s)
            assert (got == want) if p["supported"] else (got <= 0), (s, got, want)
    print("%d shapes" % len(shapes))
    # at 2 GiB the F(4x4) kernel hands the launch to the F(2x2) one: host arithmetic only, nothing is launched at that size
    assert lib_slabs("wino4", 64, 512, 64, 256, 256) == 0
    assert ops.wgrad_form(256, 256, "winograd4", (64, 512, 64))[0] == "wino_wgrad_kernel"
    assert ops.wgrad_form(256, 256, "winograd4", (63, 512, 64))[0] == "wino4_wgrad_kernel"


def test_refusals_come_before_any_launch(ops):
    from adyolo_amd import _lib
    from adyolo_amd.ops import _p, _stream
    case = ws.make_case("wino4", 2, 16, 16, 32, 32, affine=True)
    inp = ws.build(case)
    op = Operands(case, inp)
    slabs = torch.full((op.slab_floats,), float("nan"), dtype=torch.float32, device="cuda:0")
    du = torch.full((36 * 32 * 32,), float("nan"), dtype=torch.float32, device="cuda:0")
    dwbuf = dev(ws.new_dw_buffer(case))
    scbuf, shbuf = op.keep[2][0], op.keep[3][0]

    def w4(x, dy, sc, sh, h=16, w=16):
        _lib.call("adyolo_wino4_wgrad", _p(x), _p(dy), _p(sc), _p(sh), _p(slabs), _p(du), _p(dwbuf[ws.GUARD:]), 2, h, w, 32, 32, 32,
                  _stream())
    refused = {
        "scale 4 bytes off": lambda: w4(op.x, op.dy, scbuf[65:], op.sh),
        "shift 8 bytes off": lambda: w4(op.x, op.dy, op.sc, shbuf[66:]),
        "x 4 bytes off": lambda: w4(op.keep[0][0][1:], op.dy, op.sc, op.sh),
        "dy 12 bytes off": lambda: w4(op.x, op.keep[1][0][3:], op.sc, op.sh),
        "scale without shift": lambda: w4(op.x, op.dy, op.sc, None),
        "H % 4": lambda: w4(op.x, op.dy, op.sc, op.sh, h=10),
        "H < 8": lambda: w4(op.x, op.dy, op.sc, op.sh, h=4),
        "W = 12": lambda: w4(op.x, op.dy, op.sc, op.sh, w=12),
    }
    for what, call in refused.items():
        with pytest.raises(_lib.AdyoloHipError):
            call()
            pytest.fail("%s was not refused" % what)
        torch.cuda.synchronize()
        assert torch.isnan(slabs).all() and torch.isnan(du).all(), "%s: refused, yet a workspace changed" % what
        assert np.array_equal(dwbuf.cpu().numpy().view(np.int32), ws.new_dw_buffer(case).view(np.int32)), what
    w4(op.x, op.dy, op.sc, op.sh)                               # the aligned call goes through
    torch.cuda.synchronize()
    ws.check(case, ws.reference(case, inp), ws.bound(case, inp), dwbuf.cpu().numpy())


# ================================================================================================================== values
@pytest.mark.parametrize("form", ws.FORMS)
def test_wgrad_every_case_against_float64(ops, form):
    # MI355X, worst err / bound: direct 0.204 (2 x 16 x 64, 32 -> 32; 18 cases), stem 0.301 (5 x 3 x 6; 7), wino2 0.093
    # (1 x 9 x 16, 256 -> 256; 21), wino4 0.062 (7 x 64 x 4, 128 -> 128; 31); every second call and side-stream call bit-equal
    worst, failed = (0.0, None), []
    cases = ws.cases(form)
    for cs in cases:
        try:
            ratio = run_case(cs)
            if ratio > worst[0]:
                worst = (ratio, cs["name"])
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])
    print("%s: %d cases, worst err / bound %.3f at %s" % (form, len(cases), worst[0], worst[1]))
    assert not failed, "%d of %d: %s" % (len(failed), len(cases), "; ".join(failed[:8]))


def test_padded_input_channels_do_not_leak(ops):
    """Cin_real < Cin (the MIC stem, 10 real channels of 32; the FOA stem, 7 of 8): the padded channels of x hold data (``build``
    fills all Cin), exactly Cout * Cin_real * 9 floats are written (NaN before, guard words behind), and filling the padded channels
    with other numbers changes no bit of dw."""
    some = [c for c in ws.cases() if c["cin_real"] < c["cin"]]
    assert {c["form"] for c in some} == set(ws.FORMS)
    assert {(c["cin_real"], c["cin"]) for c in some} == {(10, 32), (7, 8)}
    for cs in some:
        case, inp, ref, bnd = ws.prepared(cs["name"])
        assert np.abs(inp["x"][..., case["cin_real"]:]).min() > 0
        first = Operands(case, inp).run()[0]
        other = dict(inp)
        other["x"] = inp["x"].copy()
        other["x"][..., case["cin_real"]:] = 1e6
        second = Operands(case, other).run()[0]
        torch.cuda.synchronize()
        ws.check(case, ref, bnd, first.cpu().numpy())
        assert torch.equal(bits(first), bits(second)), "%s: the padded channels reach dw" % case["name"]


# ============================================================================================================== through ops
OPS_CASES = (("direct", "direct_2x21x19_c96_32", "direct"), ("stem", "stem_3x11x37_c8_32_real7", "direct"),
             ("wino2", "wino2_2x37x16_c128_64_aff", "winograd"), ("wino4", "wino4_18x16x16_c256_256", "winograd4"),
             ("wino4", "wino4_2x16x32_c32_32_real10", "winograd4"))


@pytest.mark.parametrize("form,name,algo", OPS_CASES, ids=[c[1] for c in OPS_CASES])
def test_ops_conv3x3_wgrad_into_a_slice(ops, monkeypatch, form, name, algo):
    """``ops.conv3x3_wgrad(..., out=slice of a flat buffer)``: the bits of the direct call, nothing outside the slice touched, and
    ``ops.DISPATCH_LOG`` names the kernel the mirror predicts."""
    monkeypatch.setenv("ADYOLO_W4W_MIN_WORK", "1")
    case, inp, ref, bnd = ws.prepared(name)
    assert case["form"] == form and ws.case_plan(case)["supported"]
    op = Operands(case, inp)
    direct = op.run()[0]
    log = {}
    monkeypatch.setattr(ops, "DISPATCH_LOG", log)
    nf = ws.dw_floats(case)
    flat = dev(np.full(nf + 2 * ws.GUARD + 3, ws.SENT, dtype=np.float32))
    out = flat[ws.GUARD:ws.GUARD + nf].view(case["cout"], case["cin_real"], 3, 3)
    got = ops.conv3x3_wgrad(op.x, op.dy, case["cin_real"], in_affine=(op.sc, op.sh) if case["affine"] else None, algo=algo, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert list(log) == [(ws.KERNEL[form], case["cin"], case["cout"], int(case["affine"]))] and list(log.values()) == [1]
    f = flat.cpu().numpy()
    assert (f[:ws.GUARD] == ws.SENT).all() and (f[ws.GUARD + nf:] == ws.SENT).all(), "floats beside the slice changed"
    assert np.array_equal(f[ws.GUARD:ws.GUARD + nf].view(np.int32), direct.cpu().numpy()[ws.GUARD:ws.GUARD + nf].view(np.int32))
    ws.check(case, ref, bnd, f[:nf + 2 * ws.GUARD])


# ================================================================================================================== packing
PACK_SHAPES = ((32, 32, 32), (64, 32, 32), (96, 64, 64), (128, 256, 256), (32, 10, 32), (64, 7, 32))      # cout, cin_real, cin_pad


def _filter(cout, cin_real, seed=0):
    g = torch.Generator().manual_seed(500 + cout + 3 * cin_real + seed)
    return torch.randn(cout, cin_real, 3, 3, generator=g) / float(np.sqrt(9 * cin_real))


def _pack_direct(w, cin_pad, points):
    """Both packs of one filter by the per-filter entry point of the form: u_fwd [P][Cout/32][cin_pad/8][256], u_dgrad
    [P][cin_pad/32][Cout/8][256], NaN-filled before the call."""
    from adyolo_amd import _lib
    from adyolo_amd.ops import _p, _stream
    cout, cin_real = w.shape[0], w.shape[1]
    uf = torch.full((points, cout // 32, cin_pad // 8, 256), float("nan"), dtype=torch.float32, device="cuda:0")
    ud = torch.full((points, cin_pad // 32, cout // 8, 256), float("nan"), dtype=torch.float32, device="cuda:0")
    _lib.call("adyolo_wino_pack_w" if points == 16 else "adyolo_wino4_pack_w", _p(w), _p(uf), _p(ud), cout, cin_real, cin_pad,
              _stream())
    return uf, ud


def _unpack(u):
    """[P][Nn/32][K/8][64 lanes][4] -> U[P][k][nn]: lane (n, h) element j = U_P[k = 8 g + 4 h + j][nn = 32 cb + n]."""
    p, nb, kg, _ = u.shape
    return u.view(p, nb, kg, 2, 32, 4).permute(0, 2, 3, 5, 1, 4).reshape(p, kg * 8, nb * 32)


def _positions(points):
    """position P -> (xi, nu): row-major for F(2x2); P = 9 w + s, accumulator s of wave w, for F(4x4) (csrc/wino4.hip)."""
    if points == 16:
        return [(p // 4, p % 4) for p in range(16)]
    out = []
    for wv in range(4):
        for s in range(9):
            nu = (0, 2, 3, 5)[wv] if s < 6 else (1 if wv < 2 else 4)
            xi = s if s < 6 else ((5, 3, 4)[s - 6] if wv & 1 else s - 6)
            out.append((xi, nu))
    assert sorted(out) == [(a, b) for a in range(6) for b in range(6)]
    return out


@pytest.mark.parametrize("cout,cin_real,cin_pad", PACK_SHAPES)
def test_pack_w_is_G_g_Gt_in_fragment_order(ops, cout, cin_real, cin_pad):
    """``adyolo_wino_pack_w`` / ``adyolo_wino4_pack_w``: un-packed by the documented fragment layout the packs are G g G^T of the
    float64 filter (forward) and of the flipped, transposed filter (data gradient) within
    c u (|G| |g| |G|^T) -- c = 4 for F(2x2) (float32: two additions per direction; the halvings are exact), c = 2 for F(4x4)
    (double arithmetic, one rounding to float32, one more u for the double roundings); padded channels pack to exact zeros and
    every element is written."""
    # MI355X, worst err / bound: 0.491, 0.498, 0.528, 0.551, 0.490, 0.492 in the order of PACK_SHAPES
    w = _filter(cout, cin_real)
    wd = w.to("cuda:0")
    g64 = torch.zeros(cout, cin_pad, 3, 3, dtype=torch.float64)
    g64[:, :cin_real] = w.double()
    worst = 0.0
    for points, gm, c in ((16, ws.G2, 4), (36, ws.G4, 2)):
        uf, ud = _pack_direct(wd, cin_pad, points)
        torch.cuda.synchronize()
        assert not torch.isnan(uf).any() and not torch.isnan(ud).any(), "elements of a pack were not written"
        gt = torch.from_numpy(gm)
        pos = _positions(points)
        for u, filt in ((uf, g64.permute(1, 0, 2, 3)), (ud, g64.flip(2, 3))):      # U[P][k][nn] of g[k][nn][3][3]
            full = torch.einsum("ai,knij,bj->abkn", gt, filt, gt)
            mag = torch.einsum("ai,knij,bj->abkn", gt.abs(), filt.abs(), gt.abs())
            ref = torch.stack([full[a, b] for a, b in pos])
            bnd = c * ws.U * torch.stack([mag[a, b] for a, b in pos])
            got = _unpack(u).double().cpu()
            err = (got - ref).abs()
            assert (err <= bnd).all(), "%d points: %d elements over the bound" % (points, int((err > bnd).sum()))
            worst = max(worst, float((err / bnd.clamp_min(1e-300)).max()))
        if cin_real < cin_pad:
            assert (_unpack(uf)[:, cin_real:, :] == 0).all() and (_unpack(ud)[:, :, cin_real:] == 0).all()
    print("(%d, %d, %d): worst err / bound %.3f" % (cout, cin_real, cin_pad, worst))


def test_pack_many_equals_per_filter_packs_and_follows_the_weights(ops, monkeypatch):
    """``WinoPackSet.refresh`` (both ``pack_many`` kernels, one launch each for all filters): bit-equal to the per-filter packs,
    forward and data gradient, F(2x2) and F(4x4) forms; a second ``refresh(frozen=True)`` launches nothing; after ``w.copy_()`` or
    ``ops.params_changed()`` it launches again and the packs follow."""
    monkeypatch.setenv("ADYOLO_CONV_ALGO", "winograd4")
    assert ops.conv_algo() == "winograd4"
    shapes = [s for s in PACK_SHAPES if s[1] == s[2]]
    assert len(shapes) == 4
    ws_ = [_filter(co, ci).to("cuda:0") for co, ci, _ in shapes]
    calls = []
    real = ops._c

    def counted(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(ops, "_c", counted)
    packs = ops.WinoPackSet().refresh(ws_)
    torch.cuda.synchronize()
    assert calls == ["adyolo_wino_pack_many", "adyolo_wino4_pack_many"]

    def compare(tag):
        n4 = 0
        for i, w in enumerate(ws_):
            cout, cin = w.shape[0], w.shape[1]
            for got, which in zip(packs.get(i), (0, 1)):
                f2 = got.f2 if isinstance(got, ops.DualPack) else got
                assert torch.equal(bits(f2), bits(_pack_direct(w, cin, 16)[which])), "%s: filter %d, F(2x2) pack %d" % (tag, i, which)
                if isinstance(got, ops.DualPack):
                    n4 += 1
                    assert torch.equal(bits(got.f4), bits(_pack_direct(w, cin, 36)[which])), "%s: filter %d, F(4x4) pack %d" % (
                        tag, i, which)
        return n4
    # F(4x4) forms: both directions of 32x32, 64x32 and 128x256; of 96x64 the data gradient only (three 32-channel output blocks)
    assert compare("first") == 7
    before = [bits(p.f2 if isinstance(p, ops.DualPack) else p).clone() for p in packs.get(3)]
    del calls[:]
    packs.refresh(ws_, frozen=True)
    assert calls == [], "a frozen refresh of unchanged filters launched %s" % calls
    ws_[3].copy_(_filter(128, 256, seed=1))
    packs.refresh(ws_, frozen=True)
    assert calls == ["adyolo_wino_pack_many", "adyolo_wino4_pack_many"]
    torch.cuda.synchronize()
    compare("after copy_")
    after = [bits(p.f2 if isinstance(p, ops.DualPack) else p) for p in packs.get(3)]
    assert not torch.equal(before[0], after[0]) and not torch.equal(before[1], after[1])
    del calls[:]
    packs.refresh(ws_, frozen=True)
    assert calls == []
    ops.params_changed()                                          # what the in-place optimizer kernels announce
    packs.refresh(ws_, frozen=True)
    assert calls == ["adyolo_wino_pack_many", "adyolo_wino4_pack_many"]
    torch.cuda.synchronize()
    compare("after params_changed")
