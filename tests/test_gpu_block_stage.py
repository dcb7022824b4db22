"""GPU tests of the SE-block stage (run with ``-m gpu`` on an MI355X): the statistics the convolution epilogues sum for
the BatchNorm / SE passes, the BatchNorm kernels at sizes where their loops loop, and the SE kernels -- each against plain
PyTorch in float64 on the CPU (oracle/seresnet.py: BatchNorm in training mode, squeeze - FC - ReLU - FC - sigmoid,
relu(bn2(c) s + r), AvgPool2d(2, 2); gradients by autograd).

Two kinds of bar, neither taken from what the kernels give:

* value: err = max |q - q64| / max |q64| must stay below max(4 err_ref, 16 * 2^-24), err_ref being the same error of a plain
  float32 PyTorch-CPU evaluation of the same formula on the same inputs (``value_check``);
* sums: |sum - sum64| <= T * 2^-24 * sum |terms| per entry, the a-priori bound of a float32 sum of at most T terms
  (``oracle.seresnet.fp32_sum_bound``), T = the pixels of a patch for the convolution epilogues, 512 for the reductions of
  norm.hip ("a thread sums <= a few hundred values"); the float64 stages behind them add nothing visible (``sum_check``).

Every check prints its figures; the measured ones of an MI355X run stand next to the asserts and in DESIGN.md (K3 / K4)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import seresnet as onet
from oracle.checks import d64, sum_check, value_check

pytestmark = pytest.mark.gpu

U = onet.U32
FLOOR = 16 * U
CHUNK = 512                       # terms a thread of norm.hip's reductions sums at most (its header: "a few hundred")
EPS = onet.BN_EPS


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def dev(t):
    return t.to("cuda:0").contiguous()


def invstd_bound(mean64, var64, b_sum, b_sq, count):
    """Bound on |invstd - invstd64| when the two sums behind it are off by at most b_sum / b_sq: var = q / R - m^2, so
    |d var| <= b_sq / R + 2 |m| b_sum / R (+ the square of the mean's own error, invisible), d invstd = -invstd^3 d var / 2;
    plus the float32 roundings of m and of invstd itself."""
    dvar = b_sq / count + 2 * mean64.abs() * (b_sum / count + U * mean64.abs())
    istd = 1.0 / torch.sqrt(var64 + EPS)
    return 0.5 * istd ** 3 * dvar + 2 * U * istd


# ============================================================================================ 1. convolution epilogues
FORMS = ("direct", "winograd", "winograd4-onepatch", "winograd4-persistent")
KERNEL = {"direct": "conv3x3_fwd_kernel", "winograd": "wino_fwd_kernel", "winograd4-onepatch": "wino4_fwd_kernel",
          "winograd4-persistent": "wino4p_fwd_kernel"}
SETS = (1, 9, 15, 27, 31)         # ADYOLO_W4_* bits: 1 statistics, 2 addend, 4 addend mask, 8 stat_bn, 16 stat mask
# (N, H, W, Cin, Cout): ragged patches in both directions, a map smaller than one patch, W in {16, 32, 64} and ragged widths,
# one / two / three channel blocks, 32-channel blocks (F(4x4): the persistent kernel only)
EPI_SMALL = [(2, 13, 16, 32, 32), (1, 5, 5, 32, 64), (2, 37, 40, 64, 64), (3, 20, 32, 64, 96), (2, 9, 64, 32, 128),
             (1, 33, 16, 64, 256), (2, 70, 48, 32, 32)]
# a few samples at each stage geometry of the benchmark (60 s clips: 2400 x 64 x 32 ... 600 x 16 x 256).  On 256 CUs only the first
# gives a workgroup of the persistent kernel a second patch (600 full patches on 256 workgroups, 32 -> 32 forms only); every other
# shape of this module deals one patch per workgroup (oracle/fwd_stage.py: ``walks``).  The hand-over between patches is
# tests/test_gpu_fwd_stage.py's.
EPI_BENCH = [(2, 2400, 64, 32, 32), (2, 1200, 32, 64, 64), (2, 600, 16, 128, 128), (2, 600, 16, 256, 256)]
EPI_LOG = {}                      # ops.DISPATCH_LOG of every epilogue launch of this module


def form_exists(form, cout, epi, maskform):
    """Mirror of adyolo_wino4_fwd_form / ops._w4_eligible (asserted against the library inside the test)."""
    if not form.startswith("winograd4"):
        return True
    if form == "winograd4-onepatch":
        return cout % 64 == 0
    nb = 2 if cout % 64 == 0 else 1
    return cout // (32 * nb) in (1, 2, 4, 8) and cout % (32 * nb) == 0 and maskform != "float"


def epi_cases():
    out = []
    for shape in EPI_SMALL + EPI_BENCH:
        n, h, w, cin, cout = shape
        bits_ok = (h * w * (cout // 4)) % 64 == 0
        for form in FORMS:
            for epi in SETS:
                maskforms = ("none",) if not epi & 20 else tuple(
                    m for m in ("float", "bits") if (m == "bits" and bits_ok) or (m == "float" and shape in EPI_SMALL))
                for mf in maskforms:
                    if form_exists(form, cout, epi, mf):
                        out.append(pytest.param(shape, form, epi, mf, id="%s-e%d-%s-%s" % (form, epi, mf, "x".join(map(str, shape)))))
    return out


def spike_positions(n, h, w):
    """(sample, row, column) of the large isolated values: the image corners, the last row and column, the corners where the
    patches of every form meet (8 x 16, 8 x 32, 16 x 16, 16 x 32, 32 x 16 pixels) and the edges of the ragged patches."""
    pos = {(0, 0, 0), (n - 1, h - 1, w - 1), (0, h - 1, 0), (n - 1, 0, w - 1), (0, h - 1, (w - 1) // 2), (n - 1, (h - 1) // 2, w - 1)}
    for ph, pw in ((8, 16), (8, 32), (16, 16), (16, 32), (32, 16)):
        for y, x in ((ph - 1, pw - 1), (ph, pw), (ph - 1, pw), (ph, pw - 1), (h - 1 - (h - 1) % ph, w - 1 - (w - 1) % pw)):
            if 0 <= y < h and 0 <= x < w:
                pos.add((n - 1, y, x))
    return sorted(pos)


@functools.lru_cache(maxsize=1)
def epi_inputs(shape):
    """float32 operands of one shape (CPU): every operand set takes its subset.  Large isolated values, about 1e3 x the
    tensor's rms, sit in x, addend and aux at ``spike_positions`` with the masks on at half of them: a dropped, doubled or
    mis-masked pixel moves a sum by orders of magnitude more than rounding can."""
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(h * 1000 + w * 10 + cout)
    t = {"x": torch.randn(n, h, w, cin, generator=g) * 0.5,
         "wt": torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin),
         "in_scale": torch.rand(cin, generator=g) + 0.5, "in_shift": torch.randn(cin, generator=g) * 0.3,
         "addend": torch.randn(n, h, w, cout, generator=g),
         "amask": torch.randn(n, h, w, cout, generator=g) > 0, "smask": torch.randn(n, h, w, cout, generator=g) > 0,
         "aux": (torch.randn(n, h, w, cout, generator=g) * 2 + 0.5).relu(),
         "gamma": torch.rand(cout, generator=g) + 0.5, "beta": torch.randn(cout, generator=g) * 0.2}
    _, mean, var, _ = onet.bn_train_nhwc(t["aux"].double())
    t["mean"], t["invstd"] = mean.float(), (1.0 / torch.sqrt(var + EPS)).float()
    for k, (s, y, x) in enumerate(spike_positions(n, h, w)):
        sign = 1.0 if k % 3 else -1.0
        ck = (7 * k + 3) % cout
        t["x"][s, y, x, ck % cin] = 500.0 * sign
        t["addend"][s, y, x, ck] = -1000.0 * sign
        t["amask"][s, y, x, ck] = k % 2 == 0
        t["smask"][s, y, x, ck] = k % 4 < 2
        t["aux"][s, y, x, (ck + 1) % cout] = 2000.0
        t["smask"][s, y, x, (ck + 1) % cout] = k % 2 == 1
    # float forms of the masks: > 0 where on; -1 or (half of them) exactly 0 where off
    z = torch.rand(n, h, w, cout, generator=g) < 0.5
    for m in ("amask", "smask"):
        f = torch.where(t[m], torch.ones(()), -torch.ones(()))
        f[(~t[m]) & z] = 0.0
        t[m + "_float"] = f
    return t


@functools.lru_cache(maxsize=2)
def epi_conv(shape, affine):
    """The bare convolution in float64 and in float32 (channels-last), x seen through the input affine when asked."""
    t = epi_inputs(shape)
    out = []
    for dt in (torch.float64, torch.float32):
        x = t["x"].to(dt)
        if affine:
            x = x * t["in_scale"].to(dt) + t["in_shift"].to(dt)          # (in-image pixels only: the zero padding stays zero)
        out.append(F.conv2d(x.permute(0, 3, 1, 2), t["wt"].to(dt), None, padding=1).permute(0, 2, 3, 1).contiguous())
    return tuple(out)


def patch_geometry(form, n, h, w):
    """(pixels per patch, patches): conv.hip / wino.hip / wino4.hip, their ``*_tiles`` entry points."""
    if form == "direct":
        tw = 32 if w >= 32 else 16
        th = 256 // tw
    elif form == "winograd":
        th, tw = 8, 16
    else:
        th, tw = (16, 32) if w >= 32 else (32, 16)
    return th * tw, n * (-(-h // th)) * (-(-w // tw))


def run_epilogue_case(ops, monkeypatch, shape, form, epi, maskform, log, value=True):
    n, h, w, cin, cout = shape
    algo = form.split("-")[0]
    monkeypatch.setenv("ADYOLO_W4_MIN_K", "32")
    monkeypatch.setenv("ADYOLO_W4_MIN_K_32", "32")
    monkeypatch.setenv("ADYOLO_W4_PERSIST", "0" if form == "winograd4-onepatch" else "1")
    monkeypatch.setattr(ops, "DISPATCH_LOG", log)
    lib = ops._lib.load()
    t = epi_inputs(shape)
    wpk, _ = ops.pack_w3x3(dev(t["wt"]), cin, want_dgrad=False, algo=algo, allow32=True)
    assert (wpk.dim() == 3) if form == "direct" else (wpk.shape[0] == (16 if form == "winograd" else 36)), "pack of %s" % form
    mbits = (1 if (epi & 4 and maskform == "bits") else 0) | (2 if (epi & 16 and maskform == "bits") else 0)
    if algo == "winograd4":
        want_form = 2 if form == "winograd4-persistent" else 1
        assert lib.adyolo_wino4_fwd_form(cout, epi, mbits) == want_form

    def mask_operand(name):
        if maskform == "bits":
            return dev(torch.from_numpy(onet.pack_relu_bits(t[name].numpy())))
        return dev(t[name + "_float"])
    kw = {"want_stats": True}
    if epi == 1:
        kw["in_affine"] = (dev(t["in_scale"]), dev(t["in_shift"]))          # conv2 of the block: BN1's affine on its input
    if epi & 2:
        kw["addend"] = dev(t["addend"])
    if epi & 4:
        kw["addend_mask"] = mask_operand("amask")
    if epi & 8:
        kw["stat_bn"] = (dev(t["aux"]), dev(t["mean"]), dev(t["invstd"]))
    if epi & 16:
        kw["stat_mask"] = mask_operand("smask")
    y, st = ops.conv3x3(dev(t["x"]), wpk, cout, **kw)
    torch.cuda.synchronize()
    if algo == "winograd4":
        assert lib.adyolo_wino4_last_form() == want_form, "the other F(4x4) kernel ran"
    pixels, tiles = patch_geometry(form, n, h, w)
    tiles_fn = {"direct": lib.adyolo_conv3x3_tiles, "winograd": lib.adyolo_wino_tiles}.get(form, lib.adyolo_wino4_tiles)
    assert tiles_fn(n, h, w) == tiles and tuple(st.shape) == (2, tiles, cout)
    tag = "%s e%d %s %s" % (form, epi, maskform, "x".join(map(str, shape)))

    # ---- structure: the sums against float64 sums of the tensor this launch wrote
    yd = d64(y)
    t0 = yd * t["smask"] if epi & 16 else yd
    if epi & 8:
        xh = onet.xhat_nhwc(t["aux"].double(), t["mean"].double(), t["invstd"].double())
        t1 = t0 * xh
    else:
        t1 = t0 * t0
    s0, a0 = t0.sum(dim=(1, 2)), t0.abs().sum(dim=(1, 2))                 # per sample [N][C]
    s1, a1 = t1.sum(dim=(1, 2)), t1.abs().sum(dim=(1, 2))
    b0, b1 = onet.fp32_sum_bound(a0, pixels), onet.fp32_sum_bound(a1, pixels)
    raw = d64(st).view(2, n, tiles // n, cout).sum(dim=2)                    # the patches of a sample are consecutive
    # measured (MI355X): worst err / bound over all cases 4.3e-2 (raw sums, F(2x2) set 15), 4.4e-2 (finished sums: dgamma, F(2x2) set 15), 2.9e-2 (invstd), 0.39 (running buffers, a bound of four roundings); y err_gpu <= 2.8e-6 (direct, set 9; err_ref 2.4e-6), dx <= 1.7e-6 (F(4x4); err_ref 7.1e-7)
    sum_check(tag + " raw per-sample sum 0", raw[0], s0, b0)
    sum_check(tag + " raw per-sample sum 1", raw[1], s1, b1)
    count = n * h * w
    if epi == 1:
        rm, rv = torch.randn(cout) * 0.1, torch.rand(cout) + 0.5
        rmg, rvg = dev(rm), dev(rv)
        ssum, mean, invstd, scale, shift = ops.bn_stats_tiles(st, n, h * w, rmg, rvg, onet.BN_MOM, EPS, dev(t["gamma"]), dev(t["beta"]))
        torch.cuda.synchronize()
        sum_check(tag + " bn_stats_tiles ssum", ssum, s0, b0)
        m64, q64 = s0.sum(0) / count, s1.sum(0) / count
        v64 = q64 - m64 * m64
        bm = b0.sum(0) / count + U * m64.abs()
        sum_check(tag + " bn_stats_tiles mean", mean, m64, bm)
        bi = invstd_bound(m64, v64, b0.sum(0), b1.sum(0), count)
        sum_check(tag + " bn_stats_tiles invstd", invstd, 1.0 / torch.sqrt(v64 + EPS), bi)
        # the affine and the running buffers are elementwise in the kernel's own mean / invstd
        md, isd = d64(mean), d64(invstd)
        sc64 = t["gamma"].double() * isd
        value_check(tag + " scale", scale, sc64, (t["gamma"] * invstd.cpu()))
        value_check(tag + " shift", shift, t["beta"].double() - md * sc64, t["beta"] - mean.cpu() * (t["gamma"] * invstd.cpu()))
        vard = 1.0 / isd ** 2 - EPS
        rm64, rv64 = onet.bn_running_update(rm.double(), rv.double(), md, vard, count)
        sum_check(tag + " running_mean", rmg, rm64, 4 * U * (rm.double().abs() + md.abs()))
        # (the kernel keeps var in double; 1 / invstd^2 - eps from the float32 invstd is off by 2 * 2^-24 (var + eps))
        sum_check(tag + " running_var", rvg, rv64, 4 * U * (rv.double().abs() + (vard + EPS).abs() * count / (count - 1.0)))
    elif epi in (9, 15):
        dx, dgamma, dbeta = ops.bn_bwd(y, dev(t["aux"]), dev(t["gamma"]), dev(t["mean"]), dev(t["invstd"]), relu_mask=True, tile_stats=st)
        torch.cuda.synchronize()
        sum_check(tag + " bn_bwd(tile_stats) dbeta", dbeta, s0.sum(0), b0.sum(0))
        sum_check(tag + " bn_bwd(tile_stats) dgamma", dgamma, s1.sum(0), b1.sum(0))
    else:
        sg, sgx = torch.empty(n, cout, device="cuda:0"), torch.empty(n, cout, device="cuda:0")
        ops._c("adyolo_se_tail_bwd_tiles", ops._p(st), ops._p(sg), ops._p(sgx), n, tiles // n, cout, ops._stream())
        torch.cuda.synchronize()
        sum_check(tag + " se_tail_bwd_tiles sg", sg, s0, b0)
        sum_check(tag + " se_tail_bwd_tiles sgx", sgx, s1, b1)
    if not value:
        return
    # ---- value: y and the gradient that comes out of the chain against the float64 reference
    c64, c32 = epi_conv(shape, epi == 1)
    y64, y32 = c64, c32
    if epi & 2:
        am = t["amask"] if epi & 4 else torch.ones((), dtype=torch.bool)
        y64, y32 = c64 + t["addend"].double() * am, c32 + t["addend"] * am
    value_check(tag + " y", y, y64, y32)
    if epi in (9, 15):
        r64 = onet.bn_bwd_nhwc(y64, t["aux"].double(), t["gamma"].double(), t["mean"].double(), t["invstd"].double(), relu_mask=True)
        r32 = onet.bn_bwd_nhwc(y32, t["aux"], t["gamma"], t["mean"], t["invstd"], relu_mask=True)
        value_check(tag + " bn_bwd(tile_stats) dx", dx, r64[0], r32[0])


@pytest.mark.parametrize("shape,form,epi,maskform", epi_cases())
def test_conv_epilogue_statistics(ops, monkeypatch, shape, form, epi, maskform):
    """Every operand set the SE-block step launches (functional.SEBlockFn: 1 forward, 9 conv2's data gradient, 15 / 27 / 31
    conv1's: first block, projection block, identity block above a linked one) on every convolution form that takes it."""
    run_epilogue_case(ops, monkeypatch, shape, form, epi, maskform, EPI_LOG)


def test_conv_epilogue_dispatch_covers_every_form_and_operand_set(ops, monkeypatch):
    """Which kernel ran, from ops.DISPATCH_LOG: direct / F(2x2) / one-patch F(4x4) / persistent F(4x4), each with the operand
    sets 1, 9, 15, 27 and 31 -- a silent fallback to another kernel would leave a hole here.  The launches are made here (64-
    and 32-channel output blocks; the one-patch F(4x4) kernel has no 32-channel form: adyolo_wino4_fwd_form says 0), so the
    test does not depend on which other tests of the module ran; what those logged must be kernels of the same table."""
    lib = ops._lib.load()
    log = {}
    for shape in ((2, 8, 16, 64, 64), (1, 8, 16, 32, 32)):
        cout = shape[4]
        for form in FORMS:
            for epi in SETS:
                mf = "bits" if epi & 20 else "none"
                if form_exists(form, cout, epi, mf):
                    run_epilogue_case(ops, monkeypatch, shape, form, epi, mf, log, value=False)
                elif form == "winograd4-onepatch":
                    monkeypatch.setenv("ADYOLO_W4_PERSIST", "0")
                    assert lib.adyolo_wino4_fwd_form(cout, epi, 3 if epi & 20 else 0) == 0
                    monkeypatch.setenv("ADYOLO_W4_PERSIST", "1")
    for cout in (64, 32):
        for form in FORMS:
            for epi in SETS:
                if form_exists(form, cout, epi, "bits" if epi & 20 else "none"):
                    assert log.get((KERNEL[form], cout, cout, epi), 0) == 1, "no %s launch with operand set %d at %d channels: %s" % (
                        KERNEL[form], epi, cout, sorted(log))
    assert len(log) == 5 * 4 + 5 * 3
    assert {k[0] for k in EPI_LOG} <= set(KERNEL.values()) and {k[3] for k in EPI_LOG} <= set(SETS)


# ============================================================================================ 2. BatchNorm kernels
def relu_like(g, *shape):
    """What the model feeds its BatchNorms: ReLU outputs, |mean| / std below 3."""
    return (torch.randn(*shape, generator=g) * 2 + 0.5).relu()


# (N, HW, C): C on the INV path of the streaming kernels (C / 4 divides 256) from 4 to 1024; N from 1 to 64; N HW = 1 (the
# unbiased-variance guard); rows such that pick_G gives G > 1 with a ragged last chunk (every case from HW = 130 on), float4
# counts that leave EW_U tails, and (8, 150001, 32): 9.6 M float4, the apply grid capped at 8192 workgroups;
# (64, 20001, 32): the batch of the benchmark, G = 16
BN_SHAPES = [(1, 1, 4), (1, 1, 32), (1, 7, 4), (3, 1000, 32), (2, 3001, 64), (5, 777, 128), (3, 515, 256), (2, 130, 1024),
             (64, 20001, 32), (8, 150001, 32)]


@pytest.mark.parametrize("n,hw,c", BN_SHAPES)
def test_bn_stats_scale_shift_affine_match_float64(ops, n, hw, c):
    g = torch.Generator().manual_seed(n * 7 + hw + c)
    x = relu_like(g, n, hw, c)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    rm, rv = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    xg, rmg, rvg = dev(x), dev(rm), dev(rv)
    ssum, mean, invstd = ops.bn_stats(xg, rmg, rvg, onet.BN_MOM, EPS)
    scale, shift = ops.bn_scale_shift(dev(gamma), dev(beta), mean, invstd)
    y = ops.affine(xg, scale, shift)
    torch.cuda.synchronize()
    tag = "bn (N=%d HW=%d C=%d)" % (n, hw, c)
    x64 = x.double()
    count = n * hw
    a0, a1 = x64.abs().sum(dim=1), (x64 * x64).sum(dim=1)
    b0, b1 = onet.fp32_sum_bound(a0, CHUNK), onet.fp32_sum_bound(a1, CHUNK)
    _, m64, v64, i64 = onet.bn_train_nhwc(x64)
    # measured (MI355X): worst err / bound 6.2e-3 (ssum), 5.6e-3 (mean), 0.46 (invstd, at N HW = 1), 0.27 / 0.22 (running buffers); err_gpu 5.7e-8 (scale), 4.3e-8 (shift), 5.1e-8 (affine; err_ref up to 2.3e-5 at N HW = 1: the kernel's fma)
    sum_check(tag + " ssum", ssum, x64.sum(dim=1), b0)
    sum_check(tag + " mean", mean, m64, b0.sum(0) / count + U * m64.abs())
    sum_check(tag + " invstd", invstd, i64, invstd_bound(m64, v64, b0.sum(0), b1.sum(0), count))
    rm64, rv64 = onet.bn_running_update(rm.double(), rv.double(), m64, v64, count)
    bvar = (b1.sum(0) / count + 2 * m64.abs() * b0.sum(0) / count) * (count / (count - 1.0) if count > 1 else 1.0)
    sum_check(tag + " running_mean", rmg, rm64, onet.BN_MOM * b0.sum(0) / count + 4 * U * (rm.double().abs() + m64.abs()))
    sum_check(tag + " running_var", rvg, rv64, onet.BN_MOM * bvar + 4 * U * (rv.double().abs() + 2 * v64.abs() + m64 * m64))
    md, isd = d64(mean), d64(invstd)
    value_check(tag + " scale", scale, gamma.double() * isd, gamma * invstd.cpu())
    value_check(tag + " shift", shift, beta.double() - md * d64(scale), beta - mean.cpu() * scale.cpu())
    value_check(tag + " affine", y, x64 * d64(scale) + d64(shift), x * scale.cpu() + shift.cpu())


@pytest.mark.parametrize("relu_mask", [False, True])
@pytest.mark.parametrize("n,hw,c", BN_SHAPES)
def test_bn_bwd_reduce_path_matches_float64(ops, n, hw, c, relu_mask):
    """bn_bwd with its own reduction: dgamma / dbeta against the a-priori bound of its chunked float32 sums, dx (with and without
    the folded ReLU mask) and the channel sums of dx (want_dx_colsum) against float64; out_dgamma / out_dbeta receive the sums."""
    g = torch.Generator().manual_seed(n * 11 + hw + c)
    x, dy = relu_like(g, n, hw, c), torch.randn(n, hw, c, generator=g)
    gamma = torch.rand(c, generator=g) + 0.5
    _, m64, v64, i64 = onet.bn_train_nhwc(x.double())
    mean, invstd = m64.float(), i64.float()
    out_dg, out_db = torch.full((c,), 7.0, device="cuda:0"), torch.full((c,), -7.0, device="cuda:0")
    dx, dgamma, dbeta, colsum = ops.bn_bwd(dev(dy), dev(x), dev(gamma), dev(mean), dev(invstd), relu_mask=relu_mask,
                                           out_dgamma=out_dg, out_dbeta=out_db, want_dx_colsum=True)
    torch.cuda.synchronize()
    assert dgamma.data_ptr() == out_dg.data_ptr() and dbeta.data_ptr() == out_db.data_ptr()
    tag = "bn_bwd reduce (N=%d HW=%d C=%d relu_mask=%d)" % (n, hw, c, relu_mask)
    dy64, x64 = dy.double(), x.double()
    xh = onet.xhat_nhwc(x64, mean.double(), invstd.double())
    # measured (MI355X): worst err / bound 1.5e-3 (dbeta), 1.6e-3 (dgamma), 7.7e-4 (colsum); dx err_gpu <= 1.6e-7 (err_ref 1.6e-7)
    sum_check(tag + " dbeta", dbeta, dy64.sum(dim=(0, 1)), onet.fp32_sum_bound(dy64.abs().sum(dim=(0, 1)), CHUNK))
    sum_check(tag + " dgamma", dgamma, (dy64 * xh).sum(dim=(0, 1)), onet.fp32_sum_bound((dy64 * xh).abs().sum(dim=(0, 1)), CHUNK))
    r64 = onet.bn_bwd_nhwc(dy64, x64, gamma.double(), mean.double(), invstd.double(), relu_mask)
    r32 = onet.bn_bwd_nhwc(dy, x, gamma, mean, invstd, relu_mask)
    value_check(tag + " dx", dx, r64[0], r32[0])
    dxd = d64(dx)
    sum_check(tag + " dx colsum", colsum, dxd.sum(dim=(0, 1)), onet.fp32_sum_bound(dxd.abs().sum(dim=(0, 1)), CHUNK))
    if not relu_mask:
        dx2, dg2, db2 = ops.bn_bwd(dev(dy), dev(x), dev(gamma), dev(mean), dev(invstd))
        torch.cuda.synchronize()
        assert torch.equal(dx2, dx) and torch.equal(dg2, dgamma) and torch.equal(db2, dbeta), "the optional outputs change the result"


def tile_tensor(dy64, term1_64, tiles):
    """[2][tiles][C] float32: the rows cut into ``tiles`` equal runs, each summed in float64 and rounded once."""
    c = dy64.shape[-1]
    a = dy64.reshape(tiles, -1, c).sum(dim=1)
    b = term1_64.reshape(tiles, -1, c).sum(dim=1)
    return torch.stack([a, b]).float()


# tiles: 1 and a prime above 256 (one stage), 256 k and a highly composite count (two stages: 256 / 240 groups); C = 96: C / 4
# does not divide 256, the apply kernel's other path (the reduce entry points refuse it, the tile path takes it)
@pytest.mark.parametrize("tiles,per,c,relu_mask", [(1, 40, 32, False), (257, 3, 64, True), (512, 5, 128, False), (720, 2, 96, True),
                                                   (5040, 1, 32, True), (263, 7, 96, False), (768, 3, 256, True), (2, 1, 1024, False)])
def test_bn_bwd_tile_path_matches_float64(ops, tiles, per, c, relu_mask):
    rows = tiles * per
    g = torch.Generator().manual_seed(tiles + c)
    x, dy = relu_like(g, 1, rows, c), torch.randn(1, rows, c, generator=g)
    gamma = torch.rand(c, generator=g) + 0.5
    _, m64, _, i64 = onet.bn_train_nhwc(x.double())
    mean, invstd = m64.float(), i64.float()
    dy64, x64 = dy.double(), x.double()
    xh = onet.xhat_nhwc(x64, mean.double(), invstd.double())
    st = tile_tensor(dy64[0], (dy64 * xh)[0], tiles)
    dx, dgamma, dbeta = ops.bn_bwd(dev(dy), dev(x), dev(gamma), dev(mean), dev(invstd), relu_mask=relu_mask, tile_stats=dev(st))
    torch.cuda.synchronize()
    tag = "bn_bwd tiles (tiles=%d rows=%d C=%d)" % (tiles, rows, c)
    # the kernels add the float32 tile sums in double and round once per stage (two stages at most): 2 * 2^-24 * sum |tile sums|
    std = st.double()
    # measured (MI355X): worst err / bound 0.50 (dbeta, dgamma: one or two roundings against a bound of two); dx err_gpu <= 1.2e-7
    sum_check(tag + " dbeta", dbeta, std[0].sum(0), 2 * U * std[0].abs().sum(0))
    sum_check(tag + " dgamma", dgamma, std[1].sum(0), 2 * U * std[1].abs().sum(0))
    r64 = onet.bn_bwd_nhwc(dy64, x64, gamma.double(), mean.double(), invstd.double(), relu_mask)
    r32 = onet.bn_bwd_nhwc(dy, x, gamma, mean, invstd, relu_mask)
    value_check(tag + " dx", dx, r64[0], r32[0])


def test_reduce_entry_points_refuse_channel_counts_they_cannot_take(ops):
    """C = 96 (C / 4 = 24 does not divide 256): bn_stats, bn_bwd's reduction and se_tail_bwd's reduction return an error; the
    apply and forward entry points take it (tested above and below)."""
    err = ops._lib.AdyoloHipError
    x = dev(torch.randn(2, 10, 96))
    mean, invstd, gamma = dev(torch.zeros(96)), dev(torch.ones(96)), dev(torch.ones(96))
    with pytest.raises(err, match="bn_stats"):
        ops.bn_stats(x)
    with pytest.raises(err, match="bn_bwd_reduce"):
        ops.bn_bwd(x, x, gamma, mean, invstd)
    cr = 12
    z = dev(torch.zeros(2, 96))
    with pytest.raises(err, match="se_tail_bwd_reduce"):
        ops.se_tail_bwd(x, x, x, gamma, mean, mean, invstd, z, z, dev(torch.zeros(2, cr)), z, dev(torch.zeros(cr, 96)),
                        dev(torch.zeros(96, cr)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,g_,c,hw", [(1, 1, 32, 1), (6, 5, 64, 400), (64, 19, 32, 4800), (4, 300, 256, 150000), (8, 37, 96, 9000)])
def test_bn_persample_finish_equal_bn_stats_tiles_bitwise_and_float64(ops, n, g_, c, hw):
    """The two halves of bn_stats_tiles as separate calls (exact data parallelism: the per-sample sums of all ranks are gathered
    between them): per-sample rows computed in two parts and concatenated give the statistics of the concatenated batch BIT FOR
    BIT, running buffers and scale / shift included -- and those meet the float64 sums of the tile tensor."""
    g = torch.Generator().manual_seed(n + g_ + c)
    per = hw / float(g_)
    s = torch.randn(n * g_, c, generator=g) * math.sqrt(per) + 0.7 * per
    q = (torch.rand(n * g_, c, generator=g) + 1.5) * per * 2.0
    st = dev(torch.stack([s, q]))
    gamma, beta = dev(torch.rand(c, generator=g) + 0.5), dev(torch.randn(c, generator=g))
    rm, rv = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    rm_a, rv_a, rm_b, rv_b = dev(rm), dev(rv), dev(rm), dev(rv)
    ssum, mean, invstd, scale, shift = ops.bn_stats_tiles(st, n, hw, rm_a, rv_a, onet.BN_MOM, EPS, gamma, beta)
    # two "ranks": the first n1 samples and the rest, each from its own tile tensor
    n1 = (n + 1) // 2
    ps0, ps1 = torch.empty(n, c, device="cuda:0"), torch.empty(n, c, device="cuda:0")
    for lo, hi in ((0, n1), (n1, n)):
        if hi > lo:
            part = st[:, lo * g_:hi * g_].contiguous()
            ops._c("adyolo_bn_persample", ops._p(part), ops._p(ps0[lo:hi]), ops._p(ps1[lo:hi]), hi - lo, g_, c, ops._stream())
    mean2, invstd2, scale2, shift2 = (torch.empty(c, device="cuda:0") for _ in range(4))
    ops._c("adyolo_bn_finish", ops._p(ps0), ops._p(ps1), ops._p(mean2), ops._p(invstd2), ops._p(rm_b), ops._p(rv_b), ops._p(gamma),
           ops._p(beta), ops._p(scale2), ops._p(shift2), n, hw, c, onet.BN_MOM, EPS, ops._stream())
    torch.cuda.synchronize()
    for a, b, what in ((ssum, ps0, "ssum"), (mean, mean2, "mean"), (invstd, invstd2, "invstd"), (rm_a, rm_b, "running_mean"),
                       (rv_a, rv_b, "running_var"), (scale, scale2, "scale"), (shift, shift2, "shift")):
        assert torch.equal(a, b), "bn_persample + bn_finish differ from bn_stats_tiles in %s" % what
    tag = "bn_stats_tiles (N=%d G=%d C=%d)" % (n, g_, c)
    # measured (MI355X): worst err / bound 1.00 (ssum: exactly one rounding of a sum of like-signed terms), 0.57 (mean), 0.43 (invstd)
    std = d64(st)
    count = n * hw
    # the float32 tile sums are added in double and rounded to float32 per sample: 2^-24 * sum |tile sums|
    b0, b1 = U * std[0].abs().view(n, g_, c).sum(1), U * std[1].abs().view(n, g_, c).sum(1)
    sum_check(tag + " ssum", ssum, std[0].view(n, g_, c).sum(1), b0)
    m64, q64 = std[0].sum(0) / count, std[1].sum(0) / count
    v64 = (q64 - m64 * m64).clamp_min(0)
    sum_check(tag + " mean", mean, m64, b0.sum(0) / count + U * m64.abs())
    sum_check(tag + " invstd", invstd, 1.0 / torch.sqrt(v64 + EPS), invstd_bound(m64, v64, b0.sum(0), b1.sum(0), count))
    rm64, rv64 = onet.bn_running_update(rm.double(), rv.double(), m64, v64, count)
    bvar = (b1.sum(0) / count + 2 * m64.abs() * b0.sum(0) / count) * (count / (count - 1.0) if count > 1 else 1.0)
    sum_check(tag + " running_mean", rm_a, rm64, onet.BN_MOM * b0.sum(0) / count + 4 * U * (rm.double().abs() + m64.abs()))
    sum_check(tag + " running_var", rv_a, rv64, onet.BN_MOM * bvar + 4 * U * (rv.double().abs() + 2 * v64.abs() + m64 * m64))
    value_check(tag + " scale", scale, d64(gamma) * d64(invstd), gamma.cpu() * invstd.cpu())
    value_check(tag + " shift", shift, d64(beta) - d64(mean) * d64(scale), beta.cpu() - mean.cpu() * scale.cpu())


@pytest.mark.parametrize("ratio,limit", [(1, None), (10, 2e-6), (100, 2e-4)])
def test_one_pass_variance_stays_within_its_documented_limit(ops, ratio, limit):
    """DESIGN.md ("Known limit"): the statistics are one-pass float32 sums, so invstd loses accuracy as |mean| / std grows:
    ~2e-6 at 10, ~2e-4 at 100 (a CPU emulation, oracle.seresnet.onepass_invstd_error: worst of four channels).  The kernel must
    not be worse than the limit it documents: its worst of four channels stays within a factor of two of those figures (the
    emulation's figure for numbers of the same distribution is printed beside it: the yardstick is not the kernel's own output).  At ratio 1,
    the regime of the model, the a-priori bound of the sums applies."""
    n, hw, c = 4, 19200, 4
    rng = np.random.default_rng(0)
    x = torch.from_numpy((ratio + rng.standard_normal((n, hw, c))).astype(np.float32))
    _, mean, invstd = ops.bn_stats(dev(x))
    torch.cuda.synchronize()
    x64 = x.double()
    _, m64, v64, i64 = onet.bn_train_nhwc(x64)
    err = float(((d64(invstd) - i64).abs() / i64).max())
    emu = onet.onepass_invstd_error(ratio, rows=n * hw, chunk=300, channels=4, seed=0)
    print("one-pass variance |mean|/std = %d: invstd rel err %.3e (emulation %.3e, documented limit %s)" % (ratio, err, emu, limit))
    if limit is None:
        b0, b1 = onet.fp32_sum_bound(x64.abs().sum(dim=(0, 1)), CHUNK), onet.fp32_sum_bound((x64 * x64).sum(dim=(0, 1)), CHUNK)
        sum_check("one-pass variance ratio 1 invstd", invstd, i64, invstd_bound(m64, v64, b0, b1, n * hw))
    else:
        # measured (MI355X): 2.2e-6 at 10 (emulation 1.7e-6), 9.2e-5 at 100 (emulation 1.8e-4); 8.7e-8 at 1
        assert err <= 2 * limit, "invstd off by %.3e at |mean|/std = %d: worse than the documented %.0e" % (err, ratio, limit)


# ============================================================================================ 3. SE kernels
def fc_params(g, c, cr):
    return (torch.randn(cr, c, generator=g) * (1.5 / math.sqrt(c)), torch.randn(cr, generator=g) * 0.2,
            torch.randn(c, cr, generator=g) * (1.5 / math.sqrt(cr)), torch.randn(c, generator=g) * 0.3)


def fc_edge_params(g, c, cr):
    """... with hidden units exactly at the ReLU boundary (a zero row and a zero bias: pre-activation 0 in any precision) and
    saturated sigmoids (|z| ~ 20 through the bias)."""
    w1, b1, w2, b2 = fc_params(g, c, cr)
    w1[0] = 0.0
    b1[0] = 0.0
    if cr > 4:
        w1[cr - 1] = 0.0
        b1[cr - 1] = 0.0
    b2[1] = 20.0
    b2[c - 2] = -20.0
    return w1, b1, w2, b2


SE_FC = [(c, cr, n) for (c, cr) in ((32, 4), (64, 8), (128, 16), (256, 32), (64, 4), (1024, 128), (96, 12)) for n in (1, 3, 64)]


@pytest.mark.parametrize("c,cr,n", SE_FC)
def test_se_fc_fwd_matches_float64(ops, c, cr, n):
    g = torch.Generator().manual_seed(c + cr + n)
    hw = 9600
    ssum = torch.randn(n, c, generator=g) * math.sqrt(hw) * 3 + 0.2 * hw
    scale, shift = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    w1, b1, w2, b2 = fc_edge_params(g, c, cr)
    pooled, hid, s = ops.se_fc_fwd(dev(ssum), dev(scale), dev(shift), dev(w1), dev(b1), dev(w2), dev(b2), hw)
    torch.cuda.synchronize()

    def ref(dt):
        p = scale.to(dt) * (ssum.to(dt) / hw) + shift.to(dt)
        h, sv = onet.se_gate(p, w1.to(dt), b1.to(dt), w2.to(dt), b2.to(dt))
        return p, h, sv
    r64, r32 = ref(torch.float64), ref(torch.float32)
    tag = "se_fc_fwd (C=%d Cr=%d N=%d)" % (c, cr, n)
    # measured (MI355X): err_gpu <= 5.1e-8 (pooled), 3.7e-7 (hid; err_ref 4.8e-7), 2.8e-7 (s; err_ref 4.3e-7)
    value_check(tag + " pooled", pooled, r64[0], r32[0])
    value_check(tag + " hid", hid, r64[1], r32[1])
    value_check(tag + " s", s, r64[2], r32[2])
    assert bool((hid[:, 0] == 0).all()), "a hidden unit at the ReLU boundary is not zero"
    assert float(s[:, 1].min()) > 1 - 1e-4 and float(s[:, c - 2].max()) < 1e-4, "the sigmoids meant to saturate do not"


def fc_bwd_reference(sg, sgx, ssum, gamma, beta, mean, invstd, w1, b1, w2, b2, hw, a_ds=None):
    """float64 (or any dtype): the six packed gradients [db2 | dw2 | db1 | dw1 | sdd | sddx] and dpool by autograd through
    J = sum_{n,c} ds[n][c] s[n][c], ds = sum_hw g d = gamma sgx + beta sg -- plus, when a_ds >= |ds| is given (the sum of
    |terms| behind ds), the same chain run on absolute values: what a relative perturbation of every elementary term can move."""
    scale = gamma * invstd
    shift = beta - mean * scale
    pooled = (scale * (ssum / hw) + shift).detach().requires_grad_(True)
    w1, b1, w2, b2 = (v.detach().clone().requires_grad_(True) for v in (w1, b1, w2, b2))
    hid, s = onet.se_gate(pooled, w1, b1, w2, b2)
    ds = gamma * sgx + beta * sg
    (ds * s).sum().backward()
    dpool = pooled.grad
    sxhat = (ssum - hw * mean) * invstd
    sd = s.detach()
    sdd = (sd * sg + dpool).sum(0)
    sddx = (sd * sgx + dpool / hw * sxhat).sum(0)
    packed = torch.cat([b2.grad, w2.grad.reshape(-1), b1.grad, w1.grad.reshape(-1), sdd, sddx])
    if a_ds is None:
        return packed, dpool
    hd = hid.detach()
    a_z2 = a_ds * sd * (1 - sd)
    a_z1 = (hd > 0) * (a_z2 @ w2.detach().abs())
    a_dp = a_z1 @ w1.detach().abs()
    a_packed = torch.cat([a_z2.sum(0), (a_z2.t() @ hd).reshape(-1), a_z1.sum(0), (a_z1.t() @ pooled.detach().abs()).reshape(-1),
                          (sd * sg.abs() + a_dp).sum(0), (sd * sgx.abs() + a_dp / hw * sxhat.abs()).sum(0)])
    return packed, dpool, a_packed, a_dp


@pytest.mark.parametrize("c,cr,n", SE_FC)
def test_se_fc_bwd_matches_float64(ops, c, cr, n):
    """All six packed gradients and dpool; ``packed`` is a slice of a larger buffer (the flat gradient buffer of the step) whose
    neighbours stay untouched.  Bar per entry: 512 * 2^-24 x the chain run on absolute values (every elementary product and
    sum term perturbed by 512 roundings: the a-priori bound of the reductions in front of and inside the kernel) + the floor of
    the value rule, 16 * 2^-24 of the tensor's absmax, for what the float32 sigmoid itself loses where it saturates."""
    g = torch.Generator().manual_seed(2 * c + cr + n)
    hw = 9600
    cc_rms = 1.3
    ssum = torch.randn(n, c, generator=g) * math.sqrt(hw) * cc_rms + 0.2 * hw
    mean = torch.full((c,), 0.2) + torch.randn(c, generator=g) * 0.01
    invstd = 1.0 / (cc_rms + torch.rand(c, generator=g) * 0.2)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.5
    sg, sgx = torch.randn(n, c, generator=g) * math.sqrt(hw), torch.randn(n, c, generator=g) * math.sqrt(hw)
    w1, b1, w2, b2 = fc_edge_params(g, c, cr)
    gm, gi, gg, gb = dev(mean), dev(invstd), dev(gamma), dev(beta)
    scale, shift = ops.bn_scale_shift(gg, gb, gm, gi)
    gs, gsg, gsgx, gw1, gb1, gw2, gb2 = (dev(v) for v in (ssum, sg, sgx, w1, b1, w2, b2))        # (kept alive across the raw calls)
    pooled, hid, s = ops.se_fc_fwd(gs, scale, shift, gw1, gb1, gw2, gb2, hw)
    pw = 2 * c * cr + cr + 3 * c
    assert ops._lib.load().adyolo_se_fc_bwd_words(c, cr) == pw
    big = torch.full((pw + 64,), 123.0, device="cuda:0")
    packed = big[32:32 + pw]
    part, cws, dpool = torch.empty(n, pw, device="cuda:0"), torch.empty(1024, pw, device="cuda:0"), torch.empty(n, c, device="cuda:0")
    ops._c("adyolo_se_fc_bwd", ops._p(gsg), ops._p(gsgx), ops._p(gs), ops._p(gg), ops._p(gb), ops._p(gm), ops._p(gi),
           ops._p(pooled), ops._p(hid), ops._p(s), ops._p(gw1), ops._p(gw2), ops._p(dpool), ops._p(part), ops._p(packed),
           ops._p(cws), n, hw, c, cr, ops._stream())
    torch.cuda.synchronize()
    assert bool((big[:32] == 123.0).all()) and bool((big[32 + pw:] == 123.0).all()), "se_fc_bwd wrote outside its packed slice"
    dd = [v.double() for v in (sg, sgx, ssum, gamma, beta, mean, invstd, w1, b1, w2, b2)]
    a_ds = dd[3].abs() * dd[1].abs() + dd[4].abs() * dd[0].abs()
    p64, dp64, a_p, a_dp = fc_bwd_reference(*dd, hw, a_ds=a_ds)
    tag = "se_fc_bwd (C=%d Cr=%d N=%d)" % (c, cr, n)
    o = 0
    # measured (MI355X): worst err / bound 3.1e-2 (db2), 4.9e-2 (dw2), 7.5e-4 (db1), 7.3e-3 (dw1), 2.2e-3 (sdd), 8.5e-3 (sddx), 2.8e-3 (dpool)
    for name, ln in (("db2", c), ("dw2", c * cr), ("db1", cr), ("dw1", cr * c), ("sdd (dbeta)", c), ("sddx (dgamma)", c)):
        ref = p64[o:o + ln]
        sum_check("%s %s" % (tag, name), packed[o:o + ln], ref, CHUNK * U * a_p[o:o + ln] + FLOOR * ref.abs().max())
        o += ln
    sum_check(tag + " dpool", dpool, dp64, CHUNK * U * a_dp + FLOOR * dp64.abs().max())


def tail_inputs(n, h, w, c, seed, r_affine):
    g = torch.Generator().manual_seed(seed)
    cr = max(c // 8, 4)
    t = {"cc": torch.randn(n, h, w, c, generator=g) * 1.3 + 0.2, "r": relu_like(g, n, h, w, c) * 0.5,
         "gamma": torch.rand(c, generator=g) + 0.5, "beta": torch.randn(c, generator=g) * 0.5,
         "de": torch.randn(n, h, w, c, generator=g), "cr": cr}
    t["w1"], t["b1"], t["w2"], t["b2"] = fc_params(g, c, cr)
    t["raff"] = (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3) if r_affine else None
    return t


def tail_margin(t, scale, shift, s, dt=torch.float64):
    """8 * 2^-24 * (sum of |terms| of the element's pre-activation c scale s + shift s + r [rs + rt])."""
    c = t["cc"].to(dt)
    sb = s.to(dt).view(s.shape[0], 1, 1, -1)
    r = t["r"].to(dt)
    ra = r.abs() if t["raff"] is None else (r * t["raff"][0].to(dt)).abs() + t["raff"][1].to(dt).abs()
    return 8 * U * ((c * scale.to(dt)).abs() * sb + shift.to(dt).abs() * sb + ra)


# (N, H, W, C, r_affine): INV path with EW_U tails, C = 96 (the other path; H W C / 4 a multiple of 64 for the bits), a slice
# at a stage geometry of the benchmark, a shape without mask bits
TAIL_FWD = [(2, 6, 32, 64, False), (3, 7, 16, 32, True), (2, 16, 8, 96, True), (1, 3, 5, 128, False), (4, 600, 16, 128, False),
            (2, 9, 8, 1024, True)]


@pytest.mark.parametrize("n,h,w,c,r_affine", TAIL_FWD)
def test_se_tail_fwd_and_its_mask_bits_match_float64(ops, n, h, w, c, r_affine):
    t = tail_inputs(n, h, w, c, 5 * c + h, r_affine)
    g = torch.Generator().manual_seed(c)
    scale, shift, s = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.5, torch.rand(n, c, generator=g)
    raff = tuple(dev(v) for v in t["raff"]) if r_affine else None
    e, bits = ops.se_tail_fwd(dev(t["cc"]), dev(t["r"]), dev(scale), dev(shift), dev(s), want_mask=True, r_affine=raff)
    e_nomask = ops.se_tail_fwd(dev(t["cc"]), dev(t["r"]), dev(scale), dev(shift), dev(s), r_affine=raff)
    torch.cuda.synchronize()
    assert torch.equal(e, e_nomask), "want_mask changes e"

    def ref(dt):
        rr = t["r"].to(dt)
        if r_affine:
            rr = rr * t["raff"][0].to(dt) + t["raff"][1].to(dt)
        return (t["cc"].to(dt) * scale.to(dt) + shift.to(dt)) * s.to(dt).view(n, 1, 1, c) + rr
    pre64, pre32 = ref(torch.float64), ref(torch.float32)
    tag = "se_tail_fwd (%dx%dx%dx%d r_affine=%d)" % (n, h, w, c, r_affine)
    # measured (MI355X): err_gpu <= 6.3e-8 (err_ref 1.1e-7); no element inside the sign margin
    value_check(tag + " e", e, pre64.relu(), pre32.relu())
    has_bits = (h * w * (c // 4)) % 64 == 0
    assert (bits is not None) == has_bits
    if has_bits:
        got = onet.unpack_relu_bits(bits.cpu().numpy(), (n, h, w, c))
        assert np.array_equal(got, (e > 0).cpu().numpy()), "the bits are not (e > 0) of the e this launch wrote"
        near = tail_margin(t, scale, shift, s) > pre64.abs()
        share = float(near.double().mean())
        print("%-58s %d of %d elements inside the sign margin" % (tag + " bits", int(near.sum()), near.numel()))
        assert share <= 1e-3
        assert np.array_equal(got[~near.numpy()], (pre64 > 0).numpy()[~near.numpy()]), "mask bits differ from float64 (e > 0)"


# every (H, W, C) family of the benchmark's stages for which se_tail_pool_ok is true (the tails in front of the two pooled
# stage boundaries: 2400 x 64 x 32 and 1200 x 32 x 64; 600 x 16 x 128 is followed by no pooling but is accepted) and the
# smallest accepted shapes (one row pair; C / 4 = 1 and 32)
TAIL_POOL = [(1, 2, 64, 4, False), (1, 2, 2, 128, True), (2, 2400, 64, 32, False), (2, 1200, 32, 64, True), (2, 600, 16, 128, False)]


@pytest.mark.parametrize("n,h,w,c,r_affine", TAIL_POOL)
def test_se_tail_fwd_pooled_matches_float64_avgpool(ops, n, h, w, c, r_affine):
    assert ops.se_tail_pool_ok(h, w, c)
    t = tail_inputs(n, h, w, c, 3 * c + h, r_affine)
    g = torch.Generator().manual_seed(c + 1)
    scale, shift, s = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.5, torch.rand(n, c, generator=g)
    raff = tuple(dev(v) for v in t["raff"]) if r_affine else None
    out, bits = ops.se_tail_fwd(dev(t["cc"]), dev(t["r"]), dev(scale), dev(shift), dev(s), want_mask=True, r_affine=raff, pool_hw=(h, w))
    torch.cuda.synchronize()

    def ref(dt):
        rr = t["r"].to(dt)
        if r_affine:
            rr = rr * t["raff"][0].to(dt) + t["raff"][1].to(dt)
        return (t["cc"].to(dt) * scale.to(dt) + shift.to(dt)) * s.to(dt).view(n, 1, 1, c) + rr
    pre64, pre32 = ref(torch.float64), ref(torch.float32)
    tag = "se_tail_fwd pooled (%dx%dx%dx%d r_affine=%d)" % (n, h, w, c, r_affine)
    ref64 = F.avg_pool2d(pre64.relu().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    ref32 = F.avg_pool2d(pre32.relu().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    # measured (MI355X): err_gpu <= 1.0e-7 (err_ref 1.1e-7)
    value_check(tag + " avgpool2(e)", out, ref64, ref32)
    got = onet.unpack_relu_bits(bits.cpu().numpy(), (n, h, w, c))
    near = (tail_margin(t, scale, shift, s) > pre64.abs()).numpy()
    assert near.mean() <= 1e-3
    assert np.array_equal(got[~near], (pre64 > 0).numpy()[~near]), "mask bits of the pooled tail differ from float64 (e > 0)"


def tail_reference(t, n, h, w, c, dt, pooled_out, de):
    """The whole tail from conv2's output on, with autograd: BatchNorm-2 in training mode, SE, shortcut, ReLU [, AvgPool2d]."""
    cc, r, gamma, beta, w1, b1, w2, b2 = (t[k].detach().to(dt, copy=True).requires_grad_(True)
                                          for k in ("cc", "r", "gamma", "beta", "w1", "b1", "w2", "b2"))
    _, mean, var, invstd = onet.bn_train_nhwc(cc)
    scale = gamma * invstd
    res = onet.se_tail_nhwc(cc, r, scale, beta - mean * scale, w1, b1, w2, b2, pool=pooled_out)
    out = res["out"] if pooled_out else res["e"]
    (out * de.to(dt)).sum().backward()
    grads = {"dc": cc.grad, "dr": r.grad, "dgamma": gamma.grad, "dbeta": beta.grad, "dw1": w1.grad, "db1": b1.grad, "dw2": w2.grad,
             "db2": b2.grad}
    return {k: v.detach() for k, v in res.items()}, grads, mean.detach(), invstd.detach()


TAIL_BWD = [(2, 6, 32, 64), (3, 8, 16, 32), (2, 16, 8, 96), (4, 600, 16, 128), (2, 64, 64, 32)]


@pytest.mark.parametrize("n,h,w,c", TAIL_BWD)
def test_se_tail_bwd_matches_float64_autograd(ops, n, h, w, c):
    """se_tail_bwd in every form the step uses -- its own reduction from e, the same from the mask bits, the reduction skipped
    (tile_stats built here: per-row-run float64 sums rounded to float32), want_dr on and off, the pooled-gradient form with
    de_out -- against autograd in float64 through BatchNorm-2 (training mode), the SE FCs, the shortcut add and the ReLU."""
    t = tail_inputs(n, h, w, c, 9 * c + h, False)
    cr, hw = t["cr"], h * w
    gcc, gr, gg, gb = dev(t["cc"]), dev(t["r"]), dev(t["gamma"]), dev(t["beta"])
    gw1, gb1, gw2, gb2 = (dev(t[k]) for k in ("w1", "b1", "w2", "b2"))
    inv_path = 256 % (c // 4) == 0
    if inv_path:
        ssum, mean, invstd = ops.bn_stats(gcc)
    else:                                     # C = 96: the statistics come from tiles in the step; here from float64
        _, m, v, i = onet.bn_train_nhwc(t["cc"].double())
        ssum, mean, invstd = dev(t["cc"].double().sum(dim=(1, 2)).float()), dev(m.float()), dev(i.float())
    scale, shift = ops.bn_scale_shift(gg, gb, mean, invstd)
    pooled, hid, s = ops.se_fc_fwd(ssum, scale, shift, gw1, gb1, gw2, gb2, hw)
    e, bits = ops.se_tail_fwd(gcc, gr, scale, shift, s, want_mask=True)
    torch.cuda.synchronize()
    assert bits is not None
    r64, g64, m64, i64 = tail_reference(t, n, h, w, c, torch.float64, False, t["de"])
    r32, g32, _, _ = tail_reference(t, n, h, w, c, torch.float32, False, t["de"])
    tag = "se_tail_bwd (%dx%dx%dx%d)" % (n, h, w, c)
    value_check(tag + " fwd e through the kernels' own statistics", e, r64["e"], r32["e"])
    # elements whose ReLU may legitimately fall the other way: |pre| < 8 * 2^-24 * sum |terms|
    sc64 = t["gamma"].double() * i64
    near = tail_margin(t, sc64, t["beta"].double() - m64 * sc64, r64["s"]) > r64["pre"].abs()
    share = float(near.double().mean())
    print("%-58s %d of %d elements inside the sign margin" % (tag, int(near.sum()), near.numel()))
    assert share <= 1e-3
    keep = ~near
    sb = r64["s"].view(n, 1, 1, c)
    gate = (r64["pre"] > 0)
    d64_ = t["cc"].double() * sc64 + (t["beta"].double() - m64 * sc64)
    xh = onet.xhat_nhwc(t["cc"].double(), m64, i64)
    o_sdd = 2 * c * cr + cr + c

    def abs_bounds(de64):
        """sums of |terms| behind the reduced gradients (float64) for the gradient de64 of e: the FC chain on absolute values
        (fc_bwd_reference) and, for sdd / sddx, the |terms| of the elementwise sums sum_hw |g s|, sum_hw |g s xhat| on top."""
        gq = de64 * gate
        a_ds = (gq * d64_).abs().sum(dim=(1, 2))
        dd = [gq.sum(dim=(1, 2)), (gq * xh).sum(dim=(1, 2)), t["cc"].double().sum(dim=(1, 2)), t["gamma"].double(), t["beta"].double(),
              m64, i64, t["w1"].double(), t["b1"].double(), t["w2"].double(), t["b2"].double()]
        _, _, a_p, a_dp = fc_bwd_reference(*dd, hw, a_ds=a_ds)
        a_p = a_p.clone()
        a_p[o_sdd:o_sdd + c] = ((gq * sb).abs().sum(dim=(1, 2)) + a_dp).sum(0)
        a_p[o_sdd + c:] = ((gq * sb * xh).abs().sum(dim=(1, 2)) + a_dp / hw * xh.abs().sum(dim=(1, 2))).sum(0)
        return a_p
    de64 = t["de"].double()
    a_p = abs_bounds(de64)
    offs = {"db2": (0, c), "dw2": (c, c * cr), "db1": (c + c * cr, cr), "dw1": (c + c * cr + cr, cr * c), "dbeta": (o_sdd, c),
            "dgamma": (o_sdd + c, c)}

    def check_all(form, res, want_dr):
        names = ("dc", "dr", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2")
        got = dict(zip(names, res))
        # measured (MI355X): dc err_gpu <= 1.7e-7 (2.0e-7 from the pooled gradient; err_ref 2.1e-7 / 2.4e-7), dr exact; reduced gradients worst err / bound 2.4e-2 (dw2, tile path); 2 of 4.9 M elements inside the sign margin at 4 x 600 x 16 x 128, none elsewhere
        value_check("%s %s dc" % (tag, form), got["dc"], g64["dc"], g32["dc"], keep=keep)
        if want_dr:
            value_check("%s %s dr" % (tag, form), got["dr"], g64["dr"], g32["dr"], keep=keep)
        else:
            assert got["dr"] is None
        for k, (o, ln) in offs.items():
            ref = g64[k].reshape(-1)
            sum_check("%s %s %s" % (tag, form, k), got[k].reshape(-1), ref, CHUNK * U * a_p[o:o + ln] + FLOOR * ref.abs().max())

    gde = dev(t["de"])
    args = (gcc, gg, gb, mean, invstd, ssum, pooled, hid, s, gw1, gw2)
    if inv_path:
        check_all("reduce from e", ops.se_tail_bwd(gde, e, *args, want_dr=True), True)
        check_all("reduce from bits", ops.se_tail_bwd(gde, None, *args, want_dr=False, mask=bits), False)
    # the reduction skipped: tiles of equal row runs per sample, summed in float64 from the kernel's own mask and statistics
    gk = de64 * d64(e > 0)
    xhk = onet.xhat_nhwc(t["cc"].double(), d64(mean), d64(invstd))
    for tiles_per in (1, 6):
        if hw % tiles_per:
            continue
        st = torch.stack([gk.reshape(n * tiles_per, -1, c).sum(1), (gk * xhk).reshape(n * tiles_per, -1, c).sum(1)]).float()
        pw = 2 * c * cr + cr + 3 * c
        big = torch.full((pw + 16,), 55.0, device="cuda:0")
        res = ops.se_tail_bwd(gde, e, *args, want_dr=True, tile_stats=dev(st), mask=bits, packed_out=big[8:8 + pw])
        torch.cuda.synchronize()
        assert bool((big[:8] == 55.0).all()) and bool((big[8 + pw:] == 55.0).all()), "packed_out: neighbours overwritten"
        assert res[7].data_ptr() == big[8:].data_ptr()
        check_all("tile_stats (%d per sample)" % tiles_per, res, True)
    if ops.se_tail_pool_ok(h, w, c):
        g = torch.Generator().manual_seed(h)
        dpo = torch.randn(n, h // 2, w // 2, c, generator=g)
        p64, gp64, _, _ = tail_reference(t, n, h, w, c, torch.float64, True, dpo)
        p32, gp32, _, _ = tail_reference(t, n, h, w, c, torch.float32, True, dpo)
        de_out = torch.empty_like(gcc)
        res = ops.se_tail_bwd(dev(dpo), None, *args, want_dr=True, mask=bits, pooled_hw=(h, w), de_out=de_out)
        torch.cuda.synchronize()
        spread = 0.25 * dpo.double().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        assert torch.equal(d64(de_out), spread), "de_out is not the pooled gradient spread over 2 x 2 (exact in float32)"
        got = dict(zip(("dc", "dr", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2"), res))
        value_check(tag + " pooled dc", got["dc"], gp64["dc"], gp32["dc"], keep=keep)
        value_check(tag + " pooled dr", got["dr"], gp64["dr"], gp32["dr"], keep=keep)
        a_pp = abs_bounds(spread)
        for k in ("dgamma", "dbeta", "dw1", "db1", "dw2", "db2"):
            o, ln = offs[k]
            ref = gp64[k].reshape(-1)
            sum_check("%s pooled %s" % (tag, k), got[k].reshape(-1), ref, CHUNK * U * a_pp[o:o + ln] + FLOOR * ref.abs().max())


def test_avgpool2_at_a_bench_stage_slice_and_its_refusals(ops):
    n, h, w, c = 2, 2400, 64, 32
    g = torch.Generator().manual_seed(4)
    x, dy = torch.randn(n, h, w, c, generator=g), torch.randn(n, h // 2, w // 2, c, generator=g)
    y = ops.avgpool2(dev(x))
    dx = ops.avgpool2_bwd(dev(dy), h, w)
    torch.cuda.synchronize()
    # measured (MI355X): err_gpu 7.4e-8 = err_ref forward (the same roundings), backward exact
    value_check("avgpool2 fwd", y, onet.avgpool2_nhwc(x.double()), onet.avgpool2_nhwc(x))
    spread = 0.25 * dy.double().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(d64(dx), spread), "avgpool2_bwd is exact in float32 (a multiplication by 0.25)"
    ref = F.avg_pool2d(x.double().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert float((onet.avgpool2_nhwc(x.double()) - ref).abs().max()) < 1e-14
    err = ops._lib.AdyoloHipError
    for hh, ww in ((7, 8), (8, 7)):
        with pytest.raises(err, match="avgpool2_fwd"):
            ops.avgpool2(dev(torch.zeros(1, hh, ww, 32)))
        with pytest.raises(err, match="avgpool2_bwd"):
            ops.avgpool2_bwd(dev(torch.zeros(1, 4, 4, 32)), hh, ww)


# ============================================================================================ small things
def test_maxpool3_propagates_nan(ops):
    """A NaN in a window comes out as NaN, never as an infinity (nn.MaxPool2d's rule; the kernel used to skip a NaN, ``v > best``
    from -inf, and an all-NaN window gave -inf); windows without a NaN are unchanged."""
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 6, 9, 8, generator=g)
    x[1, 2, 4, 3] = float("nan")
    x[0, :, :, 5] = float("nan")                       # every window of this channel holds only NaN
    y, arg = ops.maxpool3_fwd(dev(x))
    torch.cuda.synchronize()
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), kernel_size=3, stride=(1, 2), padding=1).permute(0, 2, 3, 1)
    y = y.cpu()
    assert not bool(torch.isinf(y).any()), "a NaN became an infinity"
    assert torch.equal(torch.isnan(y), torch.isnan(ref))
    assert bool(torch.isnan(y[0, :, :, 5]).all()) and bool(torch.isnan(y[1, 1:4, 2, 3]).all())
    ok = ~torch.isnan(ref)
    assert torch.equal(y[ok], ref[ok])
    assert int(arg.max()) <= 8


def test_dwconv3_wgrad_many_workgroups_matches_float64(ops):
    """B T = 4207 rows (65 rows per workgroup, T = 601 does not divide it: the taps cross workgroup and sample boundaries),
    C = 512 (two passes of the channel loop), dilation 2."""
    b, tt, c, d = 7, 601, 512, 2
    g = torch.Generator().manual_seed(12)
    x, dy = torch.randn(b, tt, c, generator=g), torch.randn(b, tt, c, generator=g)
    dw, db = ops.dwconv3_wgrad(dev(dy), dev(x), d)
    torch.cuda.synchronize()
    x64, dy64 = x.double(), dy.double()
    terms = [dy64[:, d:] * x64[:, :-d], dy64 * x64, dy64[:, :-d] * x64[:, d:]]
    ref = torch.stack([v.sum(dim=(0, 1)) for v in terms], dim=1)
    bound = torch.stack([onet.fp32_sum_bound(v.abs().sum(dim=(0, 1)), CHUNK) for v in terms], dim=1)
    # measured (MI355X): worst err / bound 4.5e-4 (dw), 3.3e-4 (db)
    sum_check("dwconv3_wgrad dw", dw, ref, bound)
    sum_check("dwconv3_wgrad db", db, dy64.sum(dim=(0, 1)), onet.fp32_sum_bound(dy64.abs().sum(dim=(0, 1)), CHUNK))
    # against autograd of the forward operator too (the tap order of the weight)
    w = torch.zeros(c, 1, 3, dtype=torch.float64, requires_grad=True)
    F.conv1d(x64.permute(0, 2, 1), w, None, padding=d, dilation=d, groups=c).backward(dy64.permute(0, 2, 1))
    assert float((w.grad[:, 0] - ref).abs().max()) < 1e-9
