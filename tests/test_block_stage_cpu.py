"""CPU tests of the float64 references and helpers behind tests/test_gpu_block_stage.py (oracle/seresnet.py): the
channels-last tail / BatchNorm formulas against the oracle's own SEBasicBlock and against autograd, the ReLU-mask bit layout
of csrc/common.hpp, the a-priori bound of a float32 sum, and the emulation of the one-pass variance that DESIGN.md quotes."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import seresnet as onet


def _block_sd(cin, c, down, seed):
    g = torch.Generator().manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, generator=g, dtype=torch.float64)
    sd = {"b.conv1.weight": rn(c, cin, 3, 3) / np.sqrt(9 * cin), "b.conv2.weight": rn(c, c, 3, 3) / np.sqrt(9 * c),
          "b.se.fc.0.weight": rn(c // 8, c) * 0.3, "b.se.fc.0.bias": rn(c // 8) * 0.1,
          "b.se.fc.2.weight": rn(c, c // 8) * 0.3, "b.se.fc.2.bias": rn(c) * 0.1}
    bns = ["bn1", "bn2"] + (["downsample.1"] if down else [])
    for bn in bns:
        sd["b.%s.weight" % bn] = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
        sd["b.%s.bias" % bn] = rn(c) * 0.2
        sd["b.%s.running_mean" % bn] = torch.zeros(c, dtype=torch.float64)
        sd["b.%s.running_var" % bn] = torch.ones(c, dtype=torch.float64)
    if down:
        sd["b.downsample.0.weight"] = rn(c, cin, 1, 1) / np.sqrt(cin)
    return sd


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def test_float64_tail_equals_the_oracle_block_tail():
    """oracle.seresnet.se_basic_block runs in float64 (it follows its state dict's dtype), and from conv2's output on it is
    what bn_train_nhwc + se_tail_nhwc compute in channels-last form: to 1e-12, identity and projection shortcut, with the
    pooled successor."""
    for cin, c, pool in ((16, 16, None), (8, 16, (2, 2))):
        down = cin != c
        sd = _block_sd(cin, c, down, seed=cin + c)
        g = torch.Generator().manual_seed(3)
        x = torch.randn(2, cin, 8, 12, generator=g, dtype=torch.float64).relu()
        ref = onet.se_basic_block(sd, "b", x, pool, training=True)
        assert ref.dtype == torch.float64
        p = F.avg_pool2d(x, 2, 2) if pool else x
        a = F.relu(F.conv2d(p, sd["b.conv1.weight"], None, padding=1))
        a_bn, _, _, _ = onet.bn_train_nhwc(_nhwc(a), sd["b.bn1.weight"], sd["b.bn1.bias"])
        cc = _nhwc(F.conv2d(a_bn.permute(0, 3, 1, 2), sd["b.conv2.weight"], None, padding=1))
        _, mean2, _, invstd2 = onet.bn_train_nhwc(cc)
        scale2 = sd["b.bn2.weight"] * invstd2
        shift2 = sd["b.bn2.bias"] - mean2 * scale2
        if down:
            q = _nhwc(F.conv2d(p, sd["b.downsample.0.weight"], None))
            _, meand, _, invstdd = onet.bn_train_nhwc(q)
            sc = sd["b.downsample.1.weight"] * invstdd
            r, raff = q, (sc, sd["b.downsample.1.bias"] - meand * sc)
        else:
            r, raff = _nhwc(p), None
        t = onet.se_tail_nhwc(cc, r, scale2, shift2, sd["b.se.fc.0.weight"], sd["b.se.fc.0.bias"], sd["b.se.fc.2.weight"],
                              sd["b.se.fc.2.bias"], r_affine=raff, pool=True)
        err = float((t["e"] - _nhwc(ref)).abs().max())
        assert err < 1e-12, "tail vs oracle block: %.2e" % err
        errp = float((t["out"] - _nhwc(F.avg_pool2d(ref, 2, 2))).abs().max())
        assert errp < 1e-12, "pooled tail vs avg_pool2d of the oracle block: %.2e" % errp


def test_bn_bwd_formula_equals_autograd_in_float64():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(3, 5, 4, 8, generator=g, dtype=torch.float64) * 2 + 0.5).relu()
    gamma = (torch.rand(8, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(8, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(3, 5, 4, 8, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    y, mean, var, invstd = onet.bn_train_nhwc(xr, gamma, beta)
    y.backward(dy)
    y_t = F.batch_norm(x.permute(0, 3, 1, 2), None, None, gamma.detach(), beta.detach(), training=True, eps=onet.BN_EPS)
    assert float((y.detach() - _nhwc(y_t)).abs().max()) < 1e-12
    dx, dgamma, dbeta = onet.bn_bwd_nhwc(dy, x, gamma.detach(), mean.detach(), invstd.detach())
    for got, ref in ((dx, xr.grad), (dgamma, gamma.grad), (dbeta, beta.grad)):
        assert float((got - ref).abs().max()) < 1e-12
    dxm, _, _ = onet.bn_bwd_nhwc(dy, x, gamma.detach(), mean.detach(), invstd.detach(), relu_mask=True)
    assert torch.equal(dxm, dx * (x > 0))
    rm, rv = onet.bn_running_update(torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64), mean.detach(),
                                    var.detach(), 60)
    rm_t, rv_t = torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64)
    F.batch_norm(x.permute(0, 3, 1, 2), rm_t, rv_t, None, None, training=True, momentum=onet.BN_MOM, eps=onet.BN_EPS)
    assert float((rm - rm_t).abs().max()) < 1e-12 and float((rv - rv_t).abs().max()) < 1e-12
    # one value per channel: the biased variance (0) goes into the buffer, no division by zero
    _, rv1 = onet.bn_running_update(torch.zeros(8), torch.ones(8), torch.zeros(8), torch.zeros(8), 1)
    assert torch.equal(rv1, torch.full((8,), 0.9))


def test_relu_bits_round_trip_and_hand_built_word():
    rng = np.random.default_rng(0)
    m = rng.random((2, 8, 16, 12)) > 0.5                      # 3072 elements = 12 groups of 64 float4
    words = onet.pack_relu_bits(m)
    assert words.dtype == np.int64 and words.shape == (12 * 4,)
    assert np.array_equal(onet.unpack_relu_bits(words, m.shape), m)
    # by hand: element o = 4 i + k of the flat tensor is bit (i & 63) of word (i >> 6) * 4 + k (csrc/common.hpp, mask_bit1)
    one = np.zeros(512, dtype=bool)
    for o in (0, 5, 255, 256 + 4 * 63 + 2):
        one[o] = True
    w = onet.pack_relu_bits(one).view(np.uint64)
    expect = np.zeros(8, dtype=np.uint64)
    expect[0] = 1                                             # o = 0: float4 0, component 0
    expect[1] = 1 << 1                                        # o = 5: float4 1, component 1
    expect[3] = 1 << 63                                       # o = 255: float4 63, component 3
    expect[4 + 2] = 1 << 63                                   # second group, float4 63, component 2
    assert np.array_equal(w, expect)
    for o in range(512):
        i = o >> 2
        assert bool((int(w[(i >> 6) * 4 + (o & 3)]) >> (i & 63)) & 1) == bool(one[o])
    # the top bit makes the int64 word negative: the view must not change it
    assert onet.pack_relu_bits(one)[3] == np.int64(-2 ** 63)


def test_fp32_sum_bound_on_a_hand_checked_case():
    # 3 terms of absolute sum 7: 3 * 2^-24 * 7
    assert onet.fp32_sum_bound(7.0, 3) == 21.0 / 16777216.0
    b = onet.fp32_sum_bound(torch.tensor([1.0, 2.0], dtype=torch.float64), 256)
    assert torch.equal(b, torch.tensor([2.0 ** -16, 2.0 ** -15], dtype=torch.float64))
    # it does bound a sequential float32 sum, and not by orders of magnitude more than the worst case needs:
    # 1 + 2^-24 + 2^-24 + ... loses every small term
    x = np.full(257, 2.0 ** -24, dtype=np.float32)
    x[0] = 1.0
    s = np.float32(0)
    for v in x:
        s = np.float32(s + v)
    err = abs(float(s) - float(x.astype(np.float64).sum()))
    assert err == 256 * 2.0 ** -24
    assert err <= onet.fp32_sum_bound(float(np.abs(x.astype(np.float64)).sum()), 257) < 2 * err


def test_onepass_variance_emulation_reproduces_the_documented_limit():
    """DESIGN.md, K6 / K9 LayerNorm paragraph, "Known limit": invstd from one-pass float32 sums is off by ~2e-6 at
    |mean| / std = 10 and ~2e-4 at 100; the emulation gives both within a factor of two, and grows with the ratio squared."""
    e1, e10, e100 = (onet.onepass_invstd_error(r, channels=4) for r in (1, 10, 100))
    print("one-pass invstd error: %.2e (1)  %.2e (10)  %.2e (100)" % (e1, e10, e100))
    assert 1e-6 <= e10 <= 4e-6
    assert 1e-4 <= e100 <= 4e-4
    assert e1 < 2e-7
