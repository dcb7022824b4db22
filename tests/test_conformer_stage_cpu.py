"""CPU tests of the references behind tests/test_gpu_conformer_stage.py (oracle/conformer.py): the block-wise online-softmax
attention against the materialised form, the hand-written backward against autograd, the max-pool tap numbers against
F.max_pool2d, and the NumPy restatement of the attention dropout hash: its statistics for the seeds the GPU module uses and
the seed mix against rng.DropoutStream.seed32."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conformer as oc

MASK_CASES = oc.ATTN_MASK_CASES     # (B, heads, T, p, seed): the dropout masks tests/test_gpu_conformer_stage.py relies on


def _qkv(b, t, heads, seed, gains=(1.0,)):
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(b, t, heads * 64, generator=g, dtype=torch.float64) for _ in range(4))
    for h in range(heads):
        q[:, :, h * 64:(h + 1) * 64] *= gains[h % len(gains)]
    return q, k, v, do


@pytest.mark.parametrize("b,t,heads,p", [(2, 1, 1, 0.0), (1, 33, 4, 0.0), (2, 131, 4, 0.2), (1, 257, 8, 0.5), (1, 64, 2, 0.9)])
def test_blockwise_attention_equals_materialised_in_float64(b, t, heads, p):
    """forward, lse2 and the three gradients (from the stored log-sum-exp) to 1e-12, ragged T, with and without a mask; the
    hand-written materialised backward equals autograd."""
    q, k, v, do = _qkv(b, t, heads, 100 + t, gains=(1.0, 4.0, 12.0))
    mask = torch.from_numpy(oc.attn_dropout_mask_np(b, heads, t, p, 99)).double() if p > 0 else None
    scale = 64 ** -0.5
    qa, ka, va = (z.clone().requires_grad_(True) for z in (q, k, v))
    ctx_m, lse_m = oc.attention_materialised(qa, ka, va, heads, scale, mask)
    (ctx_m * do).sum().backward()
    ctx_b, lse_b = oc.attention_blockwise(q, k, v, heads, scale, mask)
    dq, dk, dv, delta = oc.attention_blockwise_bwd(q, k, v, ctx_b, do, lse_b, heads, scale, mask)
    hq, hk, hv = oc.attention_materialised_bwd(q, k, v, do, heads, scale, mask)

    def rel(a, ref):
        return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1.0)        # (T = 1: dq = dk = 0)
    assert rel(ctx_b, ctx_m.detach()) < 1e-12 and rel(lse_b, lse_m.detach()) < 1e-12
    for got, hand, ref in ((dq, hq, qa.grad), (dk, hk, ka.grad), (dv, hv, va.grad)):
        assert rel(got, ref) < 1e-12 and rel(hand, ref) < 1e-12
    assert rel(delta, (oc._heads(do, heads) * oc._heads(ctx_m.detach(), heads)).sum(-1)) < 1e-12


def test_blockwise_attention_float32_is_a_float32_evaluation():
    """The float32 run of the block-wise form stays float32 throughout (it is the err_ref of the GPU module, not a float64 in disguise)."""
    q, k, v, _ = _qkv(1, 70, 2, 3)
    ctx, lse = oc.attention_blockwise(q.float(), k.float(), v.float(), 2, 0.125)
    assert ctx.dtype == torch.float32 and lse.dtype == torch.float32
    ref, _ = oc.attention_materialised(q, k, v, 2, 0.125)
    err = float((ctx.double() - ref).abs().max()) / float(ref.abs().max())
    assert 0 < err < 1e-5


def test_maxpool_taps_reproduce_torch_routing():
    """Ties (inputs after a ReLU, inputs of four distinct values), odd and even widths, W = 1 and the all -inf window: the tap
    numbers route a gradient exactly where autograd routes it."""
    g = torch.Generator().manual_seed(4)
    cases = [torch.relu(torch.randn(2, 9, w, 3, generator=g, dtype=torch.float64)) for w in (1, 2, 3, 5, 16, 33)]
    cases += [torch.randint(0, 4, (2, 2, w, 3), generator=g).double() for w in (2, 5, 16)]
    cases.append(torch.full((1, 3, 5, 1), -float("inf"), dtype=torch.float64))
    for x in cases:
        n, h, w, c = x.shape
        xa = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
        ya = F.max_pool2d(xa, 3, stride=(1, 2), padding=1)
        dy = torch.randint(-3, 4, ya.shape, generator=g).double()
        (ya * dy).sum().backward()
        y, tap = oc.maxpool3_taps(x)
        assert torch.equal(y, ya.detach().permute(0, 2, 3, 1))
        assert torch.equal(oc.maxpool3_bwd_from_taps(dy.permute(0, 2, 3, 1).contiguous(), tap, w), xa.grad.permute(0, 2, 3, 1))
    _, tap = oc.maxpool3_taps(cases[-1])
    assert tap[0, :, :, 0].tolist() == [[4, 3, 3], [1, 0, 0], [1, 0, 0]]
    dx = oc.maxpool3_bwd_from_taps(torch.ones(1, 3, 3, 1, dtype=torch.float64), tap, 5)
    assert dx[0, 0, :, 0].tolist() == [2.0, 2.0, 0.0, 2.0, 0.0]


def test_hash_restatement_known_values():
    """attn_hash is the 'lowbias32' finaliser: 0 -> 0, and one hand-evaluated value; the threshold of p is floor(fl32(p) 2^32)."""
    assert int(oc.attn_hash_np(np.uint32(0))) == 0
    x = 1
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(oc.attn_hash_np(np.uint32(1))) == x
    assert oc.drop_threshold_np(0.0) == 0 and oc.drop_threshold_np(0.5) == 1 << 31
    assert oc.drop_threshold_np(0.2) == int(float(np.float32(0.2)) * 2 ** 32)
    assert float(oc.keep_scale_np(0.5)) == 2.0


@pytest.mark.parametrize("b,heads,t,p,seed", MASK_CASES)
def test_numpy_dropout_mask_is_a_dropout_mask(b, heads, t, p, seed):
    """Keep share of the whole mask, of every row and of every column within z sqrt(p (1 - p) / n) of 1 - p, z from a union
    bound at 1e-6 over the rows and columns checked (z = 6.5 at 12800, normal approximation; n >= 257 at p = 0.9); no two
    (b, h) slabs equal; another seed gives another mask; the same seed the same."""
    keep = oc.attn_keep_np(b, heads, t, p, seed)
    z_all, z_row, z_col, count = oc.dropout_mask_statistics(keep, p)
    z = oc.union_z(count + 1)
    print("B %d H %d T %d p %.1f: z_all %.2f z_row %.2f z_col %.2f, bound %.2f over %d tests" % (b, heads, t, p, z_all, z_row, z_col, z, count + 1))
    assert max(z_all, z_row, z_col) <= z
    assert oc.slabs_distinct(keep)
    assert not np.array_equal(keep, oc.attn_keep_np(b, heads, t, p, seed + 1))
    assert np.array_equal(keep, oc.attn_keep_np(b, heads, t, p, seed))
    sub = oc.attn_keep_np(b, heads, t, p, seed, samples=[b - 1])
    assert np.array_equal(sub[0], keep[b - 1])
    m = oc.attn_dropout_mask_np(b, heads, t, p, seed)
    assert set(np.unique(m).tolist()) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}


def test_a_striped_or_repeated_mask_fails_the_statistics():
    """The bounds have teeth: a mask repeated per head fails ``slabs_distinct``; one that drops whole columns fails the column bound."""
    keep = oc.attn_keep_np(2, 4, 257, 0.2, 5)
    rep = keep.copy()
    rep[:, 1] = rep[:, 0]
    assert not oc.slabs_distinct(rep)
    striped = np.broadcast_to(keep[:, :, :1, :], keep.shape)
    _, _, z_col, count = oc.dropout_mask_statistics(striped, 0.2)
    assert z_col > oc.union_z(count + 1)


def test_union_z():
    assert 6.4 < oc.union_z(12800) < 6.6 and 4.8 < oc.union_z(1) < 5.0


def test_one_accumulator_convolutions_are_the_convolution():
    """conv_seq32_y / _dx / conv3x3_seq32_dw compute F.conv2d and its gradients (strided, padded, 7x7 .. 1x1), to float32 accuracy,
    and stay float32."""
    g = torch.Generator().manual_seed(0)
    for h, w, cin, cout, kh, kw, st, pd in [(40, 4, 16, 24, 3, 3, (1, 1), (1, 1)), (20, 16, 8, 12, 7, 7, (1, 2), (3, 3)),
                                            (20, 8, 16, 8, 1, 1, (1, 2), (0, 0)), (40, 1, 16, 16, 3, 3, (1, 1), (1, 1))]:
        x, wt = torch.randn(2, h, w, cin, generator=g), torch.randn(cout, cin, kh, kw, generator=g)
        xn = x.permute(0, 3, 1, 2).double()
        y = F.conv2d(xn, wt.double(), None, stride=st, padding=pd)
        dy = torch.randn(y.shape, generator=g).float()
        dx = torch.nn.grad.conv2d_input(xn.shape, wt.double(), dy.double(), stride=st, padding=pd)
        ys = oc.conv_seq32_y(x[0], wt, st, pd)
        dxs = oc.conv_seq32_dx(dy[0].permute(1, 2, 0), wt, st, pd, h, w)
        assert ys.dtype == dxs.dtype == torch.float32
        for got, ref in ((ys, y[0].permute(1, 2, 0)), (dxs, dx[0].permute(1, 2, 0))):
            assert got.shape == ref.shape and 0 < float((got.double() - ref).abs().max()) < 1e-5 * float(ref.abs().max())
        if (kh, st) == (3, (1, 1)):
            dw = torch.nn.grad.conv2d_weight(xn, wt.shape, dy.double(), padding=1)
            dws = oc.conv3x3_seq32_dw(x, dy.permute(0, 2, 3, 1).contiguous(), cout_keep=8, chunk=7)
            assert dws.dtype == torch.float32 and float((dws.double() - dw[:8]).abs().max()) < 1e-5 * float(dw.abs().max())


def test_seed32_restatement_equals_dropout_stream():
    import adyolo_amd  # noqa: F401  (import shim at the repo root)
    from adyolo_amd.rng import DropoutStream
    for seed, offs in ((100, (0, 1, 7, 2 ** 33 + 5)), (2 ** 63 + 12345, (0, 819200))):
        for off in offs:
            s = DropoutStream(0)
            s._seed, s.offset = seed, off
            assert s.seed32(4) == oc.seed32_np(seed, off)
            assert s.offset == off + 4
