"""GPU tests of the ResNet-Conformer stage (run with ``-m gpu`` on an MI355X): the flash-style attention kernels of
csrc/attention.hip, the elementwise / pooling / depthwise / softmax kernels of csrc/conformer.hip, and the stride-1 and
strided convolution routes of the Conformer's ResNet front end at the sizes the benchmark runs them -- each against plain
PyTorch in float64 on the CPU, starting from the float32 numbers the kernel sees (references: oracle/conformer.py, pinned on
the CPU by tests/test_conformer_stage_cpu.py).

Three kinds of bar, none taken from what a kernel returns (oracle/checks.py):

* value: err = max |q - q64| / max |q64| <= max(4 err_ref, 16 * 2^-24), err_ref the same error of a plain float32 PyTorch-CPU
  evaluation of the same formula on the same inputs.  Attention tensors are normalised per head (the inputs give the heads
  different scales) and take as err_ref the larger of two float32 evaluations: the materialised softmax(q k^T d^-1/2) v and
  the block-wise online-softmax algorithm the kernel's header documents, restated in PyTorch;
  convolutions likewise take the larger of PyTorch's float32 convolution and a plain loop that keeps ONE running float32 sum
  per output, as the matrix-core kernels do (``conv_value_check``);
* sums: the a-priori bound T * 2^-24 * sum |terms| of a float32 sum of T terms (``oracle.seresnet.fp32_sum_bound``);
* exact: masks, tap numbers, gradients that are copies or zeros, two paths that claim the same bits.

Every check prints its figures; the ones of an MI355X run stand next to the asserts and in DESIGN.md (K9 / K9a)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conformer as oc
from oracle import seresnet as onet
from oracle.checks import FLOOR, U, Collect, d64, sum_check, value_check, value_check_heads

pytestmark = pytest.mark.gpu

CHUNK = 512                       # terms bound of the float32 partial sums (as tests/test_gpu_block_stage.py)
D = 64
SCALE = D ** -0.5
GAINS = (1.0, 4.0, 12.0)          # per-head gains on q: scores up to about +-66, the softmax from flat to peaked
BENCH_B, BENCH_T, BENCH_H, BENCH_P = 32, 800, 4, 0.2
BENCH_PICK = [0, 17, BENCH_B - 1]
ROUTES = {}                       # route name -> geometries of this module that took it


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def dev(t):
    return t.to("cuda:0").contiguous()


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def worse_of(a, b, ref64):
    """Element by element the one of the two float32 evaluations that is further from float64: its error is the larger err_ref."""
    a, b, ref64 = d64(a), d64(b), d64(ref64)
    return torch.where((a - ref64).abs() >= (b - ref64).abs(), a, b)


# ====================================================================================================== 1a. attention
ATTN_T = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257)
# (B, T, heads, p): every length without dropout and with it, heads 1 / 4 / 8 and B 1 .. 3 in rotation; the training and the
# evaluation length (T = 2400: forward AND backward against float64, one sample)
ATTN_CASES = ([(1 + i % 3, t, (4, 1, 8)[i % 3], 0.0) for i, t in enumerate(ATTN_T)]
              + [(1 + (i + 1) % 3, t, (8, 4, 1)[i % 3], (0.2, 0.5, 0.9)[i % 3]) for i, t in enumerate(ATTN_T)]
              + [(2, 800, 4, 0.0), (2, 800, 4, 0.2), (1, 2400, 4, 0.0)])


def attn_inputs(b, t, heads, seed, kind="gains"):
    """q, k, v, dctx float32 [B][T][heads * 64].  ``gains``: head h of q scaled by GAINS[h % 3].  ``rising``: keys sorted by
    their score against a fixed direction every query points in, so the running maximum rises in every key block
    (alpha < 1 at every step).  ``last``: query row 5 has its maximum at the very last key (the ragged block)."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(b, t, heads * D, generator=g) for _ in range(4))
    qh, kh = q.view(b, t, heads, D), k.view(b, t, heads, D)
    if kind == "rising":
        u = torch.randn(heads, D, generator=g)
        u = u / u.norm(dim=-1, keepdim=True)
        order = (kh * u).sum(-1).argsort(dim=1)                                  # [B][T][heads]
        kh.copy_(torch.gather(kh.clone(), 1, order[..., None].expand(b, t, heads, D)))
        qh.copy_(16.0 * u + 0.02 * qh)
    else:
        if kind == "last":
            kh[:, t - 1] = 1.5 * qh[:, min(5, t - 1)]
        for h in range(heads):
            qh[:, :, h] *= GAINS[h % 3]
    return q, k, v, do


def attn_refs(q, k, v, do, heads, mask):
    """float64 (materialised) and the two float32 evaluations: {name: (ref64, (ref32 materialised, ref32 block-wise))}."""
    m64 = None if mask is None else mask.double()
    q64, k64, v64, do64 = (z.double() for z in (q, k, v, do))
    ctx64, lse64 = oc.attention_materialised(q64, k64, v64, heads, SCALE, m64)
    g64 = oc.attention_materialised_bwd(q64, k64, v64, do64, heads, SCALE, m64)
    ctx_a, lse_a = oc.attention_materialised(q, k, v, heads, SCALE, mask)
    g_a = oc.attention_materialised_bwd(q, k, v, do, heads, SCALE, mask)
    ctx_b, lse_b = oc.attention_blockwise(q, k, v, heads, SCALE, mask)
    g_b = oc.attention_blockwise_bwd(q, k, v, ctx_b, do, lse_b, heads, SCALE, mask)
    out = {"ctx": (ctx64, (ctx_a, ctx_b)), "lse2": (lse64, (lse_a, lse_b))}
    for i, n in enumerate(("dq", "dk", "dv")):
        out[n] = (g64[i], (g_a[i], g_b[i]))
    out["dv_allow"] = oc.attention_dv_recompute_allowance(q64, k64, do64, heads, SCALE, m64)
    return out


def attn_run(ops, q, k, v, do, heads, p, seed):
    qg, kg, vg, dg = (dev(z) for z in (q, k, v, do))
    ctx, lse = ops.attn_fwd(qg, kg, vg, heads, SCALE, p, seed)
    ctx_nolse, none = ops.attn_fwd(qg, kg, vg, heads, SCALE, p, seed, want_lse=False)
    grads = ops.attn_bwd(qg, kg, vg, ctx, dg, lse, heads, SCALE, p, seed)
    again = ops.attn_bwd(qg, kg, vg, ctx, dg, lse, heads, SCALE, p, seed)
    torch.cuda.synchronize()
    assert none is None and torch.equal(ctx, ctx_nolse), "want_lse=False changes ctx"
    for a, b_ in zip(grads, again):
        assert torch.equal(a, b_), "attn_bwd is not deterministic"
    return ctx.cpu(), lse.cpu(), tuple(z.cpu() for z in grads)


def attn_compare(tag, got, refs, heads, pick=None):
    """ctx, dq, dk: value bar per head.  lse2: value bar.  dv: value bar per head after the allowance of
    ``oracle.conformer.attention_dv_recompute_allowance`` (P recomputed in float32 from the stored log-sum-exp: up to
    2 ln2 2^-24 max |s2| of relative error in P, derived from the inputs) -- without it dv misses the bar where the CPU
    evaluations happen to have no such error: T = 1 and 2 (1.0e-6 .. 1.4e-6 against err_ref 0 .. 1.4e-7) and narrowly at
    2 x 32 x 8 heads, p = 0.2 (4.7e-6 against 4 x 1.1e-6), always in a head with gain 12 (max |s2| about 95).  At T = 1 the
    exact P is 1: the kernel's 1e-6 comes from attn_bwd_dkv_kernel scaling K where the forward scaled Q (its recomputed score
    rounds differently from the one the log-sum-exp was made of); scaling the Q tile there would remove it, at the price of
    changing what the training step computes.  dk needs no allowance (worst 7.9e-6 against 4 x 2.5e-6)."""
    ctx, lse, grads = got
    sel = (lambda z: z) if pick is None else (lambda z: z[pick])
    c = Collect()
    c(value_check_heads, tag + " ctx", sel(ctx), *refs["ctx"], heads)
    r64, (ra, rb) = refs["lse2"]
    c(value_check, tag + " lse2", sel(lse), r64, worse_of(ra, rb, r64))
    for n, gt in zip(("dq", "dk", "dv"), grads):
        c(value_check_heads, tag + " " + n, sel(gt), *refs[n], heads, allow=refs["dv_allow"] if n == "dv" else None)
    c.finish()


@pytest.mark.parametrize("b,t,heads,p", ATTN_CASES)
def test_attention_matches_float64(ops, b, t, heads, p):
    """ctx, lse2, dq, dk, dv at every tile edge (32-key block, 32-query wave, 128-query workgroup), per-head gains 1 / 4 / 12 on q,
    the float64 reference multiplied with the NumPy restatement of the dropout mask; want_lse=False gives the same ctx bits;
    the backward launched twice gives the same bits.
    Measured (MI355X, worst over the cases; err_gpu / err_ref / bar): ctx 2.0e-6 / 7.1e-7 / 2.9e-6 (T = 2400), lse2 4.6e-7 / 2.2e-7 /
    9.5e-7, dq 1.8e-6 / 8.6e-7 / 3.4e-6, dk 7.9e-6 / 2.5e-6 / 1.0e-5 (3 x 127 x 8 heads), dv 5.3e-6 raw, 4.9e-7 after the allowance of
    ``attn_compare`` (bar 9.5e-7)."""
    seed = 0xA77E + 13 * t + heads
    q, k, v, do = attn_inputs(b, t, heads, 7000 + 10 * t + heads + b)
    mask = torch.from_numpy(oc.attn_dropout_mask_np(b, heads, t, p, seed)) if p > 0 else None
    got = attn_run(ops, q, k, v, do, heads, p, seed)
    attn_compare("attn B%d T%d H%d p%.1f" % (b, t, heads, p), got, attn_refs(q, k, v, do, heads, mask), heads)


@pytest.mark.parametrize("kind,b,t,heads,p", [("rising", 2, 257, 4, 0.0), ("rising", 1, 800, 4, 0.2), ("rising", 2, 129, 1, 0.0),
                                              ("last", 2, 65, 4, 0.0), ("last", 1, 129, 8, 0.2), ("last", 3, 33, 1, 0.0)])
def test_attention_online_softmax_is_moved(ops, kind, b, t, heads, p):
    """``rising``: the running maximum rises in every key block for (nearly) every query, so alpha < 1 rescales both accumulators
    at every step; ``last``: a row's maximum sits in the last, ragged block.  The construction is checked in float64 first.
    Measured (MI355X; err_gpu / err_ref): every row rises in every block; ctx 3.0e-6 / 2.2e-6, dq 4.6e-6 / 2.5e-6, dk 2.3e-6 / 1.4e-6,
    lse2 2.0e-7 / 2.0e-7, dv 0 after the allowance."""
    seed = 4242 + t
    q, k, v, do = attn_inputs(b, t, heads, 9000 + t + heads, kind)
    s = oc._heads(q.double(), heads) @ oc._heads(k.double(), heads).transpose(-1, -2)
    if kind == "rising":
        nb = (t + 31) // 32
        pad = torch.full((b, heads, t, nb * 32 - t), -math.inf, dtype=torch.float64)
        bm = torch.cat([s, pad], -1).view(b, heads, t, nb, 32).amax(-1)
        rising = (bm[..., 1:] > bm[..., :-1]).all(-1).double().mean()
        print("rows whose block maximum rises in every one of %d blocks: %.3f" % (nb, float(rising)))
        assert float(rising) > 0.9
    else:
        assert bool((s[:, :, min(5, t - 1)].argmax(-1) == t - 1).all()) and (t - 1) % 32 != 31
    mask = torch.from_numpy(oc.attn_dropout_mask_np(b, heads, t, p, seed)) if p > 0 else None
    got = attn_run(ops, q, k, v, do, heads, p, seed)
    attn_compare("attn %s B%d T%d H%d p%.1f" % (kind, b, t, heads, p), got, attn_refs(q, k, v, do, heads, mask), heads)


def test_attention_at_the_benchmark_shape(ops):
    """B = 32, T = 800, 4 heads, p = 0.2: float64 for the first, a middle and the last sample (the operation is per sample; the
    NumPy mask of exactly those samples).
    Measured (MI355X; err_gpu / err_ref): ctx 9.5e-7 / 6.2e-7, lse2 3.3e-7 / 3.4e-7, dq 1.2e-6 / 5.1e-7, dk 9.7e-7 / 5.8e-7, dv 4.8e-6 raw
    / 2.4e-6 (9.5e-7 after the allowance)."""
    seed = 0xC0FFEE
    q, k, v, do = attn_inputs(BENCH_B, BENCH_T, BENCH_H, 32800)
    got = attn_run(ops, q, k, v, do, BENCH_H, BENCH_P, seed)
    mask = torch.from_numpy(oc.attn_dropout_mask_np(BENCH_B, BENCH_H, BENCH_T, BENCH_P, seed, samples=BENCH_PICK))
    refs = attn_refs(q[BENCH_PICK], k[BENCH_PICK], v[BENCH_PICK], do[BENCH_PICK], BENCH_H, mask)
    attn_compare("attn bench 32x800x4 p0.2", got, refs, BENCH_H, pick=BENCH_PICK)


def test_attention_autograd_node_is_the_ops_path(ops):
    """Fn.AttentionCoreFn returns the bits of ops.attn_fwd / attn_bwd, with and without dropout."""
    from adyolo_amd import functional as Fn
    for p, drop in ((0.0, None), (0.2, (0.2, 991))):
        q, k, v, do = attn_inputs(2, 131, 4, 55)
        ctx, lse, grads = attn_run(ops, q, k, v, do, 4, p, 991)
        qg, kg, vg = (dev(z).requires_grad_(True) for z in (q, k, v))
        out = Fn.AttentionCoreFn.apply(qg, kg, vg, 4, SCALE, drop)
        out.backward(dev(do))
        torch.cuda.synchronize()
        assert torch.equal(out.detach().cpu(), ctx)
        for a, b_ in zip((qg, kg, vg), grads):
            assert torch.equal(a.grad.cpu(), b_)


@pytest.mark.parametrize("b,t,heads,p", [(2, 33, 4, 0.2), (1, 129, 1, 0.0), (2, 1, 4, 0.0), (1, 257, 8, 0.5)])
def test_attention_never_reads_past_its_tensors(ops, b, t, heads, p):
    """Inputs taken as contiguous slices (starting at multiples of 4 floats: the kernels load float4) from the middle of one
    NaN-filled buffer: the clamped min(.., T - 1) loads never pull a guard value in -- every output finite and the bits of the
    run on separately allocated inputs."""
    q, k, v, do = attn_inputs(b, t, heads, 31 + t)
    n = q.numel()
    gap = heads * D + 256                               # more than one row (heads * 64 floats) and a float4, a multiple of 4
    big = torch.full((4 * (n + gap) + gap,), float("nan"), device="cuda:0")
    views = []
    for i, z in enumerate((q, k, v, do)):
        o = gap + i * (n + gap)
        assert o % 4 == 0
        big[o:o + n] = dev(z).view(-1)
        views.append(big[o:o + n].view(b, t, heads * D))
    assert all(z.is_contiguous() for z in views)
    qg, kg, vg, dg = views
    ctx, lse = ops.attn_fwd(qg, kg, vg, heads, SCALE, p, 77)
    grads = ops.attn_bwd(qg, kg, vg, ctx, dg, lse, heads, SCALE, p, 77)
    torch.cuda.synchronize()
    ref_ctx, ref_lse, ref_grads = attn_run(ops, q, k, v, do, heads, p, 77)
    for name, a, r in (("ctx", ctx, ref_ctx), ("lse2", lse, ref_lse)) + tuple(zip(("dq", "dk", "dv"), grads, ref_grads)):
        a = a.cpu()
        assert bool(torch.isfinite(a).all()), name + " pulled a guard value in"
        assert torch.equal(a, r), name + " differs from the run on separate tensors"
    assert bool(torch.isnan(big[:gap]).all()) and bool(torch.isnan(big[-gap:]).all())


def test_attention_nan_stays_in_its_sample_and_head(ops):
    """A NaN in one (sample, head) of v leaves every other (sample, head) of ctx bit-identical to the clean run."""
    b, t, heads = 3, 131, 4
    q, k, v, do = attn_inputs(b, t, heads, 404)
    clean, _ = ops.attn_fwd(dev(q), dev(k), dev(v), heads, SCALE, 0.2, 5)
    vb = v.clone()
    vb[1, 77, 2 * D + 9] = float("nan")
    dirty, _ = ops.attn_fwd(dev(q), dev(k), dev(vb), heads, SCALE, 0.2, 5)
    torch.cuda.synchronize()
    clean, dirty = clean.cpu().view(b, t, heads, D), dirty.cpu().view(b, t, heads, D)
    other = torch.ones(b, heads, dtype=torch.bool)
    other[1, 2] = False
    for bi in range(b):
        for h in range(heads):
            if other[bi, h]:
                assert torch.equal(clean[bi, :, h], dirty[bi, :, h]), "the NaN of (1, 2) reached (%d, %d)" % (bi, h)
    assert bool(torch.isnan(dirty[1, :, 2]).any())


# ---- dropout of the attention weights, independent of the code under test
MASK_CASES = oc.ATTN_MASK_CASES     # (B, heads, T, p, seed); the CPU module checks the NumPy hash's statistics for the same cases


@pytest.mark.parametrize("b,heads,t,p,seed", MASK_CASES)
def test_attention_dropout_mask_is_the_numpy_hash_and_a_dropout_mask(ops, b, heads, t, p, seed):
    """ops.attn_dropout_mask equals the NumPy restatement of attn_hash / attn_keep / drop_threshold bit for bit, and is a dropout
    mask: values in {0, fl(1 / (1 - p))}; keep share of the whole mask, of every row and of every column within
    z sqrt(p (1 - p) / n) of 1 - p, z from a union bound at 1e-6 over the rows and columns checked (z = 6.5 over 12801 tests at
    2 x 4 x 800, 6.3 .. 6.4 for the others: ``oracle.conformer.union_z``; tests/test_conformer_stage_cpu.py checks on the CPU that
    the hash meets them for these seeds: worst 4.3); no two (b, h) slabs equal, another seed another mask, the same seed the
    same bits."""
    like = torch.empty(1, device="cuda:0")
    m = ops.attn_dropout_mask(like, b, t, heads, p, seed)
    m2 = ops.attn_dropout_mask(like, b, t, heads, p, seed)
    m3 = ops.attn_dropout_mask(like, b, t, heads, p, seed + 1)
    torch.cuda.synchronize()
    assert torch.equal(m, m2) and not torch.equal(m, m3)
    m = m.cpu().numpy()
    assert np.array_equal(m, oc.attn_dropout_mask_np(b, heads, t, p, seed)), "the mask is not the documented hash"
    assert set(np.unique(m).tolist()) == {0.0, float(oc.keep_scale_np(p))}
    z_all, z_row, z_col, count = oc.dropout_mask_statistics(m > 0, p)
    z = oc.union_z(count + 1)
    print("mask B%d H%d T%d p%.1f: z_all %.2f z_row %.2f z_col %.2f, bound %.2f over %d tests" % (b, heads, t, p, z_all, z_row, z_col, z, count + 1))
    assert max(z_all, z_row, z_col) <= z
    assert oc.slabs_distinct(m > 0)


def test_attention_seed_from_the_device_gives_the_same_bits(ops):
    """A seed passed as the device tensor of ops.seed32_dev (what a recorded step uses) gives bit-identical ctx, dq, dk, dv to the
    host integer rng.DropoutStream.seed32 computes; both are the NumPy restatement's value."""
    from adyolo_amd.rng import DropoutStream
    base, off_host, off_dev = 0x1234ABCD5678EF01, 4096, 2 ** 33 + 77
    s = DropoutStream(0)
    s._seed, s.offset = base, off_host + off_dev
    host = s.seed32(10)
    counter = torch.tensor([off_dev], dtype=torch.int64, device="cuda:0")
    seed_dev = ops.seed32_dev(base, off_host, counter)
    torch.cuda.synchronize()
    assert host == oc.seed32_np(base, off_host + off_dev) == (int(seed_dev.cpu()[0]) & 0xFFFFFFFF)
    q, k, v, do = attn_inputs(2, 131, 4, 808)
    a = attn_run(ops, q, k, v, do, 4, 0.2, host)
    b_ = attn_run(ops, q, k, v, do, 4, 0.2, seed_dev)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])
    for x, y in zip(a[2], b_[2]):
        assert torch.equal(x, y)
    c = attn_run(ops, q, k, v, do, 4, 0.2, host + 1)
    assert not torch.equal(a[0], c[0])


def test_attention_refusals(ops):
    """D != 64, p >= 1 and B H T T >= 2^32 (the 32-bit row * T + key index of the dropout hash wraps there) raise before any
    launch, in attn_fwd, attn_bwd and attn_dropout_mask alike (torch.empty inputs: nothing is read)."""
    from adyolo_amd._lib import AdyoloHipError
    e = lambda *s: torch.empty(*s, device="cuda:0")                          # noqa: E731
    x = e(1, 8, 4 * 32)
    with pytest.raises(AdyoloHipError, match="head dimension"):
        ops.attn_fwd(x, x, x, 4, SCALE)
    with pytest.raises(AdyoloHipError, match="head dimension"):
        ops.attn_bwd(x, x, x, x, x, e(1, 4, 8), 4, SCALE)
    x = e(1, 8, 4 * D)
    for p in (1.0, 1.5):
        with pytest.raises(AdyoloHipError):
            ops.attn_fwd(x, x, x, 4, SCALE, p, 1)
        with pytest.raises(AdyoloHipError):
            ops.attn_bwd(x, x, x, x, x, e(1, 4, 8), 4, SCALE, p, 1)
        with pytest.raises(AdyoloHipError):
            ops.attn_dropout_mask(x, 1, 8, 4, p, 1)
    t = 32768                                                                # 1 * 4 * 32768^2 = 2^32
    x = e(1, t, 4 * D)
    with pytest.raises(AdyoloHipError, match="32-bit"):
        ops.attn_fwd(x, x, x, 4, SCALE, 0.2, 1)
    with pytest.raises(AdyoloHipError, match="32-bit"):
        ops.attn_bwd(x, x, x, x, x, e(1, 4, t), 4, SCALE, 0.2, 1)
    import ctypes
    one = e(1)                                                               # (the entry point refuses before it touches the buffer:
    with pytest.raises(AdyoloHipError, match="32-bit"):                      #  no 16 GiB mask is allocated for the refusal)
        ops._c("adyolo_attn_dropout_mask", ops._p(one), 1, t, 4, 0.2, ctypes.c_uint32(1), ops._stream())
    ok, _ = ops.attn_fwd(e(1, 8, 4 * D).zero_(), e(1, 8, 4 * D).zero_(), e(1, 8, 4 * D).zero_(), 4, SCALE)    # an ordinary call still runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ok).all())


# ====================================================================================================== 1b. conformer.hip
def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def pool_inputs(kind, seed, n, h, w, c):
    g = torch.Generator().manual_seed(seed)
    if kind == "relu":                                    # what the model feeds it: about half the values exactly 0 (ties everywhere)
        return torch.relu(torch.randn(n, h, w, c, generator=g))
    return torch.randint(0, 4, (n, h, w, c), generator=g).float() - 1.0     # four distinct values


def maxpool_check(ops, tag, x):
    n, h, w, c = x.shape
    y, arg = ops.maxpool3_fwd(dev(x))
    y64, tap = oc.maxpool3_taps(x.double())
    g = torch.Generator().manual_seed(h * 100 + w)
    dyi = torch.randint(-3, 4, y64.shape, generator=g).float()
    dyr = torch.randn(y64.shape, generator=g)
    dxi, dxr = ops.maxpool3_bwd(dev(dyi), arg, w), ops.maxpool3_bwd(dev(dyr), arg, w)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().double(), y64), tag + ": y"
    assert torch.equal(arg.cpu(), tap), tag + ": arg differs from F.max_pool2d's index in %d places" % int((arg.cpu() != tap).sum())
    refs = {}
    for dt in (torch.float64, torch.float32):
        for name, dy in (("i", dyi), ("r", dyr)):
            xa = nchw(x.to(dt)).requires_grad_(True)
            F.max_pool2d(xa, 3, stride=(1, 2), padding=1).backward(nchw(dy.to(dt)))
            refs[name, dt] = nhwc(xa.grad)
    assert torch.equal(dxi.cpu().double(), refs["i", torch.float64]), tag + ": dx for integer dy"
    value_check(tag + " dx", dxr, refs["r", torch.float64], refs["r", torch.float32])


@pytest.mark.parametrize("w", [1, 2, 3, 5, 16, 33])
def test_maxpool3_ties_and_edges(ops, w):
    """Widths 1 .. 33 (odd: the last window half in padding), heights 1, 2, 9, C = 3 and 64, inputs after a ReLU and inputs of
    four distinct values: y and arg equal F.max_pool2d(return_indices=True) in float64 exactly, dx equals autograd exactly for
    integer dy and holds the value bar for randn dy (up to six terms are added).
    Measured (MI355X): dx for randn dy 1.1e-7 (err_ref 6.2e-8, bar 9.5e-7)."""
    for h in (1, 2, 9):
        for c in (3, 64):
            for kind in ("relu", "four"):
                maxpool_check(ops, "maxpool3 %s 2x%dx%dx%d" % (kind, h, w, c), pool_inputs(kind, 10 * w + h + c, 2, h, w, c))


def test_maxpool3_grid_stride_and_autograd_node(ops):
    """2 x 130 x 256 x 64: 2.13 M outputs, above the 8192 x 256 threads of the largest grid; Fn.MaxPool3Fn is the ops path."""
    from adyolo_amd import functional as Fn
    x = pool_inputs("relu", 3, 2, 130, 256, 64)
    assert 2 * 130 * 128 * 64 > 8192 * 256
    maxpool_check(ops, "maxpool3 grid-stride 2x130x256x64", x)
    xg = dev(x[:1, :9, :33]).requires_grad_(True)
    y = Fn.MaxPool3Fn.apply(xg)
    dy = rnd(1, *y.shape)
    y.backward(dev(dy))
    y2, arg = ops.maxpool3_fwd(xg.detach())
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(xg.grad, ops.maxpool3_bwd(dev(dy), arg, 33))


def test_maxpool3_all_minus_inf_window_routes_like_torch(ops):
    """A window whose values are all -inf: forward stays -inf and the gradient goes to the window's first element inside the map,
    as F.max_pool2d routes it (the kernel used to name tap (0, 0), which is padding in the top row and the left column, and the
    backward dropped the gradient).  x = full(-inf, (1, 3, 5, 1)), dy = 1 -> dx[0] = [2, 2, 0, 2, 0]."""
    x = torch.full((1, 3, 5, 1), -math.inf)
    y, arg = ops.maxpool3_fwd(dev(x))
    dx = ops.maxpool3_bwd(dev(torch.ones(1, 3, 3, 1)), arg, 5)
    torch.cuda.synchronize()
    _, tap = oc.maxpool3_taps(x.double())
    assert bool((y.cpu() == -math.inf).all()) and torch.equal(arg.cpu(), tap)
    assert dx.cpu()[0, 0, :, 0].tolist() == [2.0, 2.0, 0.0, 2.0, 0.0]
    assert float(dx.sum()) == 9.0, "a window's gradient was dropped"
    x = pool_inputs("relu", 5, 2, 9, 16, 3)                # -inf regions inside an ordinary map, top row and left column included
    x[0, :3, :5] = -math.inf
    x[1, 4:, 9:] = -math.inf
    y, arg = ops.maxpool3_fwd(dev(x))
    torch.cuda.synchronize()
    y64, tap = oc.maxpool3_taps(x.double())
    assert torch.equal(y.cpu().double(), y64) and torch.equal(arg.cpu(), tap)


ACT_GRID = [0.0, 1e-30, 1.278, 10.0, 20.0, 87.0, 88.8, 104.0, 1e4]
TINY = 2.0 ** -126                # smallest normal float32: a result below it may be flushed to zero


def act_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 3
    grid = torch.tensor(ACT_GRID + [-a for a in ACT_GRID])
    pos = torch.randperm(n, generator=g)[:grid.numel()]
    x[pos] = grid
    keep = torch.ones(n, dtype=torch.bool)
    keep[pos] = False                                     # the randn part: the value bar is taken over it (its absmax, about 13)
    return x, pos, keep


def elementwise_check(tag, got, ref64, ref32, pos, factor):
    """The hand-placed arguments element by element: |got - ref64| <= 4 |ref32 - ref64| + 16 * 2^-24 |ref64| + 2^-126 |factor| -- the
    value bar with every element as its own scale (1e4 next to 1e-30 would hide everything else under one absmax).  The last
    term: a sigmoid below the smallest normal float32 may come out as 0 (1 / (1 + expf(-x)) with expf overflowing above 88.7 IS
    0: the documented form); ``factor`` is what the sigmoid is multiplied with."""
    got, ref64, ref32 = d64(got).reshape(-1)[pos], d64(ref64).reshape(-1)[pos], d64(ref32).reshape(-1)[pos]
    factor = d64(factor).reshape(-1)[pos].abs()
    assert bool(torch.isfinite(got).all()), "%s: not finite at %s" % (tag, pos[~torch.isfinite(got)].tolist())
    err, bar = (got - ref64).abs(), 4 * (ref32 - ref64).abs() + FLOOR * ref64.abs() + TINY * (factor + 1e-30)
    print("%-58s worst err / bar %.3e over %d hand-placed arguments" % (tag, float((err / bar).max()), pos.numel()))
    assert bool((err <= bar).all()), "%s: %s" % (tag, [(float(a), float(b)) for a, b in zip(got[err > bar], ref64[err > bar])])


@pytest.mark.parametrize("n", [1, 7, 1001, 8192 * 256 + 513])
def test_swish_matches_float64(ops, n):
    """randn * 3 plus +-{0, 1e-30, 1.278, 10, 20, 87, 88.8, 104, 1e4} (expf(-x) overflows above 88.7: the forms give 0 / x and a zero
    gradient, never NaN); n not a multiple of 4 or 256; one size above the largest grid.
    Measured (MI355X): forward 8.5e-8, backward 4.8e-7 (both = err_ref); hand-placed arguments 0.12 / 0.23 of their element-wise bar."""
    x, pos, keep = act_inputs(max(n, 18), n) if n >= 18 else (rnd(n, n) * 3, torch.zeros(0, dtype=torch.long), torch.ones(n, dtype=torch.bool))
    dy = rnd(n + 1, x.numel())
    y, dx = ops.swish_fwd(dev(x)), ops.swish_bwd(dev(dy), dev(x))
    torch.cuda.synchronize()

    def ref(dt):
        xa = x.to(dt).clone().requires_grad_(True)
        ya = xa * torch.sigmoid(xa)
        ya.backward(dy.to(dt))
        return ya.detach(), xa.grad
    (y64, dx64), (y32, dx32) = ref(torch.float64), ref(torch.float32)
    value_check("swish_fwd n=%d" % n, y.cpu()[keep], y64[keep], y32[keep])          # (the randn part under its own absmax)
    value_check("swish_bwd n=%d" % n, dx.cpu()[keep], dx64[keep], dx32[keep])
    if pos.numel():
        elementwise_check("swish_fwd grid n=%d" % n, y, y64, y32, pos, x)
        elementwise_check("swish_bwd grid n=%d" % n, dx, dx64, dx32, pos, dy * (1 + x.abs()))
        big = x.abs() >= 88.8
        yc, dxc = y.cpu(), dx.cpu()
        assert torch.equal(yc[big & (x > 0)], x[big & (x > 0)]) and bool((yc[big & (x < 0)] == 0).all())
        assert torch.equal(dxc[big & (x > 0)], dy[big & (x > 0)]) and bool((dxc[big & (x < 0)] == 0).all())


@pytest.mark.parametrize("r,c", [(1, 1), (3, 5), (1, 256), (3, 256), (25600, 256), (25600, 5), (3, 1)])
def test_glu_matches_float64(ops, r, c):
    """GLU over the channel axis, C = 1, 5, 256 and R = 1, 3, 25600 (the model's 32 x 800 rows), the gate drawn from randn * 3 plus
    the hand-placed arguments (saturated sigmoid: gradient of the gate exactly zero, never NaN); once through Fn.GLUFn.
    Measured (MI355X): forward 9.1e-8, value half 1.0e-7, gate half 8.7e-7 (all = err_ref); hand-placed arguments 0.25 of their bar."""
    from adyolo_amd import functional as Fn
    n = r * c
    a = rnd(r * 7 + c, r, c)
    if n >= 18:
        gate, pos, keep = act_inputs(n, r + c)
    else:
        gate, pos, keep = rnd(n, n) * 3, torch.zeros(0, dtype=torch.long), torch.ones(n, dtype=torch.bool)
    x = torch.cat([a, gate.view(r, c)], dim=1).contiguous()
    dy = rnd(n + 2, r, c)
    y, dx = ops.glu_fwd(dev(x)), ops.glu_bwd(dev(dy), dev(x))
    xg = dev(x).requires_grad_(True)
    yf = Fn.GLUFn.apply(xg)
    yf.backward(dev(dy))
    torch.cuda.synchronize()
    assert torch.equal(yf.detach(), y) and torch.equal(xg.grad, dx)

    def ref(dt):
        xa = x.to(dt).clone().requires_grad_(True)
        ya = F.glu(xa, dim=-1)
        ya.backward(dy.to(dt))
        return ya.detach(), xa.grad
    (y64, dx64), (y32, dx32) = ref(torch.float64), ref(torch.float32)
    tag = "glu %dx%d" % (r, c)
    k2 = keep.view(r, c)
    dxc = dx.cpu()
    value_check(tag + " fwd", y.cpu()[k2], y64[k2], y32[k2])
    value_check(tag + " bwd value half", dxc[:, :c][k2], dx64[:, :c][k2], dx32[:, :c][k2])
    value_check(tag + " bwd gate half", dxc[:, c:][k2], dx64[:, c:][k2], dx32[:, c:][k2])
    if pos.numel():
        elementwise_check(tag + " fwd grid", y, y64, y32, pos, a)
        elementwise_check(tag + " bwd value grid", dxc[:, :c].contiguous(), dx64[:, :c].contiguous(), dx32[:, :c].contiguous(), pos, dy)
        elementwise_check(tag + " bwd gate grid", dxc[:, c:].contiguous(), dx64[:, c:].contiguous(), dx32[:, c:].contiguous(), pos, dy * a)
        sat = (gate.abs() >= 88.8).view(r, c)
        assert bool((dx.cpu()[:, c:][sat] == 0).all()), "gate gradient of a saturated sigmoid is not zero"


# (B, T, C, dilation): dilations 1, 4, 16 and >= T (both side taps in padding everywhere), T = 1, 2, 40, 800, C = 5 .. 1024 (the
# c += 256 loop of the weight gradient), B T below 64, the model's 32 x 800 x 256
DW_CASES = [(2, 1, 5, 1), (3, 2, 5, 4), (1, 2, 256, 2), (1, 40, 256, 1), (2, 40, 512, 4), (1, 40, 1024, 16), (2, 40, 5, 64), (1, 40, 5, 16),
            (2, 800, 1024, 4), (32, 800, 256, 1), (32, 800, 256, 16), (3, 800, 512, 800)]


@pytest.mark.parametrize("b,t,c,d", DW_CASES)
def test_dwconv3_matches_float64(ops, b, t, c, d):
    """Forward (with bias and bias=None), the flip=True form against the float64 data gradient, the weight and bias gradients
    within T * 2^-24 * sum |terms| (T = 512 as test_dwconv3_wgrad_many_workgroups_matches_float64; a thread adds at most 127
    rows, the partials are joined by adyolo_colsum); once through Fn.DWConv3Fn.
    Measured (MI355X): forward 8.2e-8 (err_ref 9.0e-8), flip form 1.0e-7 (5.7e-8), dw 9.7e-3 and db 3.3e-3 of the bound."""
    from adyolo_amd import functional as Fn
    x, w, bias, dy = rnd(b + t, b, t, c), rnd(c + d, c, 1, 3), rnd(c, c), rnd(t + d, b, t, c)
    xg, wg, bg, dg = dev(x), dev(w), dev(bias), dev(dy)
    y = ops.dwconv3(xg, wg.view(c, 3), bg, d)
    y0 = ops.dwconv3(xg, wg.view(c, 3), None, d)
    dx = ops.dwconv3(dg, wg.view(c, 3), None, d, flip=True)
    dw, db = ops.dwconv3_wgrad(dg, xg, d)
    xa, wa, ba = xg.clone().requires_grad_(True), wg.clone().requires_grad_(True), bg.clone().requires_grad_(True)
    yf = Fn.DWConv3Fn.apply(xa, wa, ba, d)
    yf.backward(dg)
    torch.cuda.synchronize()
    assert torch.equal(yf.detach(), y) and torch.equal(xa.grad, dx) and torch.equal(wa.grad.view(c, 3), dw) and torch.equal(ba.grad, db)

    def ref(dt, with_bias):
        xr, wr = x.to(dt).clone().requires_grad_(True), w.to(dt)          # (clone: .to() of a float32 tensor is the tensor itself)
        yr = F.conv1d(xr.transpose(1, 2), wr, bias.to(dt) if with_bias else None, padding=d, dilation=d, groups=c).transpose(1, 2)
        yr.backward(dy.to(dt))
        return yr.detach(), xr.grad
    (y64, dx64), (y32, dx32) = ref(torch.float64, True), ref(torch.float32, True)
    tag = "dwconv3 %dx%dx%d d%d" % (b, t, c, d)
    value_check(tag + " fwd", y, y64, y32)
    value_check(tag + " fwd no bias", y0, ref(torch.float64, False)[0], ref(torch.float32, False)[0])
    value_check(tag + " flip (dx)", dx, dx64, dx32)
    x64, dy64 = x.double(), dy.double()
    z = torch.zeros(b, t, c, dtype=torch.float64)
    lo, hi = z.clone(), z.clone()
    if d < t:
        lo[:, d:] = dy64[:, d:] * x64[:, :-d]
        hi[:, :-d] = dy64[:, :-d] * x64[:, d:]
    terms = [lo, dy64 * x64, hi]
    ref_dw = torch.stack([v.sum(dim=(0, 1)) for v in terms], dim=1)
    bound = torch.stack([onet.fp32_sum_bound(v.abs().sum(dim=(0, 1)), CHUNK) for v in terms], dim=1)
    sum_check(tag + " dw", dw, ref_dw, bound)
    sum_check(tag + " db", db, dy64.sum(dim=(0, 1)), onet.fp32_sum_bound(dy64.abs().sum(dim=(0, 1)), CHUNK))
    if d >= t:
        assert float(dw[:, 0].abs().max()) == 0.0 and float(dw[:, 2].abs().max()) == 0.0


def test_dwconv3_wgrad_refuses_more_than_1024_channels(ops):
    from adyolo_amd._lib import AdyoloHipError
    x = torch.empty(1, 4, 1025, device="cuda:0")
    with pytest.raises(AdyoloHipError):
        ops.dwconv3_wgrad(x, x, 1)


@pytest.mark.parametrize("k", [1, 4, 5])
def test_avgpool1d_matches_float64_and_drops_the_tail(ops, k):
    """T in k, k + 1, 4 k - 1, 800: T % k != 0 drops the tail forward and writes exact zeros to it backward; the backward is the
    copy dy * fac / k (the two float32 roundings of the formula: exact); T < k is refused; once through Fn.AvgPool1dFn.
    Measured (MI355X): forward 1.1e-7 (= err_ref); backward exact."""
    from adyolo_amd import functional as Fn
    from adyolo_amd._lib import AdyoloHipError
    for t in sorted({k, k + 1, 4 * k - 1, 800}):
        for b, c, fac in ((2, 256, 2.0), (3, 5, 1.0)):
            x = rnd(t + c, b, t, c)
            to = t // k
            dy = rnd(t + k, b, to, c)
            y, dx = ops.avgpool1d(dev(x), k, fac), ops.avgpool1d_bwd(dev(dy), t, k, fac)
            xg = dev(x).requires_grad_(True)
            yf = Fn.AvgPool1dFn.apply(xg, k, fac)
            yf.backward(dev(dy))
            torch.cuda.synchronize()
            assert torch.equal(yf.detach(), y) and torch.equal(xg.grad, dx)
            ref = lambda dt: (F.avg_pool1d(x.to(dt).transpose(1, 2), k) * fac).transpose(1, 2)      # noqa: E731
            value_check("avgpool1d k%d %dx%dx%d" % (k, b, t, c), y, ref(torch.float64), ref(torch.float32))
            dxc = dx.cpu()
            want = torch.zeros(b, t, c)
            want[:, :to * k] = (dy * np.float32(fac) / np.float32(k)).repeat_interleave(k, dim=1)
            assert torch.equal(dxc, want), "avgpool1d_bwd k%d T%d" % (k, t)
            assert float(dxc[:, to * k:].abs().max() if t % k else 0.0) == 0.0
    if k > 1:
        with pytest.raises(AdyoloHipError):
            ops.avgpool1d(torch.empty(1, k - 1, 4, device="cuda:0"), k, 2.0)
        with pytest.raises(AdyoloHipError):
            ops.avgpool1d_bwd(torch.empty(1, 1, 4, device="cuda:0"), k - 1, k, 2.0)


@pytest.mark.parametrize("n", [4, 1028, 256 * 32769])          # (the last: C = 256 and more float4s than the 8192 x 256 threads of the largest grid)
def test_axpby_affine_relu_and_relu_bwd(ops, n):
    """axpby and affine_relu hold the value bar (a * x + b * z may be contracted into one fused multiply-add: not one rounding);
    with b = 0 axpby IS one rounding: exact; affine_relu's zeros are the float64 zeros wherever the float64 pre-activation is
    clearly on one side (|v| above the bar); relu_bwd is a masked copy: exact.  Fn.AxpbyFn hands dy on untouched for b = 1.
    Measured (MI355X): axpby 6.8e-8 (= err_ref), affine_relu 3.6e-8 (err_ref 7.2e-8)."""
    from adyolo_amd import functional as Fn
    x, z = rnd(n, n), rnd(n + 1, n)
    a, b = 0.5, 1.25
    y, y0 = ops.axpby(dev(x), dev(z), a, b), ops.axpby(dev(x), dev(z), 0.3, 0.0)
    torch.cuda.synchronize()
    value_check("axpby n=%d" % n, y, a * x.double() + b * z.double(), a * x + b * z)
    assert torch.equal(y0.cpu(), x * np.float32(0.3)), "axpby with b = 0 is not the single product"
    c = 4 if n == 4 else 256 if n % 256 == 0 else 4
    xs = x.view(-1, c)
    sc, sh = torch.rand(c, generator=torch.Generator().manual_seed(n)) + 0.5, rnd(n + 2, c) * 0.3
    r = ops.affine_relu(dev(xs), dev(sc), dev(sh))
    pre64 = xs.double() * sc.double() + sh.double()
    value_check("affine_relu n=%d" % n, r, pre64.relu(), (xs * sc + sh).relu())
    rc = r.cpu()
    clear = pre64.abs() > FLOOR * float(pre64.abs().max())
    assert torch.equal((rc > 0)[clear], (pre64 > 0)[clear])
    dy = rnd(n + 3, *xs.shape)
    dx = ops.relu_bwd(dev(dy), r)
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu(), torch.where(rc > 0, dy, torch.zeros(())))
    xg, zg = dev(x).requires_grad_(True), dev(z).requires_grad_(True)
    dyg = dev(dy.view(-1))
    Fn.AxpbyFn.apply(xg, zg, a, 1.0).backward(dyg)
    torch.cuda.synchronize()
    assert torch.equal(zg.grad, dyg) and torch.equal(xg.grad.cpu(), dy.view(-1) * np.float32(a))


def test_elementwise_refusals(ops):
    """n % 4 and C % 4: the float4 kernels refuse what they cannot address."""
    from adyolo_amd._lib import AdyoloHipError
    e = lambda *s: torch.empty(*s, device="cuda:0")                          # noqa: E731
    with pytest.raises(AdyoloHipError):
        ops.axpby(e(6), e(6), 1.0, 1.0)
    with pytest.raises(AdyoloHipError):
        ops.relu_bwd(e(6), e(6))
    with pytest.raises(AdyoloHipError):
        ops.affine_relu(e(2, 6), e(6), e(6))


@pytest.mark.parametrize("L", [1, 63, 64, 65, 800, 2400, 4096])
def test_row_softmax_matches_float64(ops, L):
    """softmax_fwd / _bwd (in the C ABI, used by no model path): R = 1, 3, 4, 5 (four rows per workgroup), scale 0.125, rows of randn
    scores, rows with scores up to +-66 after the scale and rows of equal scores.  P: value bar; rows sum to 1 within
    (ceil(L / 64) + 8) 2^-24 (a lane adds ceil(L / 64) terms, six shuffle adds, one reciprocal, one product: one rounding each; summed
    in float64 here); dS within scale P (T 2^-24 sum |dP P|) of the row dot, T = ceil(L / 64) + 6, plus four roundings of the
    difference and the two products.
    Measured (MI355X): P 1.5e-7 (= err_ref); |row sum - 1| 0.24 of its bound; dS 0.30 of its bound."""
    scale = 0.125
    for r in (1, 3, 4, 5):
        s = rnd(L * 10 + r, r, L)
        s[0] *= 66.0 / scale / max(float(s[0].abs().max()), 1e-9)           # scores up to +-66 after the scale
        if r >= 3:
            s[2] = 3.25                                                      # equal scores: P = 1 / L
        p = ops.softmax_fwd(dev(s), scale)
        dp = rnd(L + r, r, L)
        ds = ops.softmax_bwd(dev(dp), p, scale)
        torch.cuda.synchronize()
        tag = "softmax %dx%d" % (r, L)
        value_check(tag + " P", p, torch.softmax(s.double() * scale, -1), torch.softmax(s * scale, -1))
        p64 = d64(p)
        lane = -(-L // 64)
        dev_sum = float((p64.sum(-1) - 1.0).abs().max())
        print("%-58s |row sum - 1| %.3e  bound %.3e" % (tag, dev_sum, (lane + 8) * U))
        assert dev_sum <= (lane + 8) * U
        dp64 = dp.double()
        dot = (dp64 * p64).sum(-1, keepdim=True)
        ref = scale * p64 * (dp64 - dot)
        bound = scale * p64 * onet.fp32_sum_bound((dp64 * p64).abs().sum(-1, keepdim=True), lane + 6) + 4 * U * scale * p64 * (dp64.abs() + dot.abs())
        sum_check(tag + " dS", ds, ref, bound + TINY)


# ====================================================================================================== 1c. convolution routes
# The convolutions of the ResNet front end at the benchmark's Conformer input (conformer_bs32x20s: 32 x 7 x 800 x 64), (W, Cin,
# Cout) per stride-1 3x3 call of models.backbones.resnet_conformer._conv3x3_s1 and (KH, KW, W, Cin, Cout) per strided Fn.ConvFn
# call.  Read off the model: ``test_route_constants_are_the_models_geometries`` records them from one forward of the
# encoder (H and N do not enter: every stride is 1 along time) and compares.
S1_GEOMS = [(8, 64, 64), (4, 128, 128), (2, 256, 256), (1, 512, 512)]
STRIDED_GEOMS = [(7, 7, 64, 8, 64), (3, 3, 16, 64, 64), (1, 1, 16, 64, 64), (3, 3, 8, 64, 128), (1, 1, 8, 64, 128),
                 (3, 3, 4, 128, 256), (1, 1, 4, 128, 256), (3, 3, 2, 256, 512), (1, 1, 2, 256, 512)]
NAMED_ROUTES = ("Conv3x3S1Fn", "Conv3x3NarrowFn", "Conv3x1WinoFn", "ConvFn")
# (N, H, W, Cin, Cout) -> the form that has to run: training 32 x 800, evaluation 1 x 2400 (below wino1d_ok's 2048 rows), and
# H = 804 / 798 on the two narrow maps (H % 4 != 0 falls off the 1-D Winograd route)
S1_CASES = ([((32, 800) + g, r) for g, r in zip(S1_GEOMS, ("Conv3x3S1Fn", "Conv3x3NarrowFn", "Conv3x1WinoFn", "Conv3x1WinoFn"))]
            + [((1, 2400) + g, r) for g, r in zip(S1_GEOMS, ("Conv3x3S1Fn", "Conv3x3NarrowFn", "ConvFn", "ConvFn"))]
            + [((32, 804, 2, 256, 256), "Conv3x1WinoFn"), ((32, 798, 2, 256, 256), "ConvFn"),
               ((32, 804, 1, 512, 512), "Conv3x1WinoFn"), ((32, 798, 1, 512, 512), "ConvFn"),
               ((32, 800, 1, 96, 64), "ConvFn"), ((32, 800, 1, 64, 96), "ConvFn"), ((32, 800, 1, 64, 64), "Conv3x1WinoFn")])
CONV_PICK = [0, 13, 31]


def route_of(y):
    """The convolution's autograd node behind ``y`` (through the views of the folded forms)."""
    node = y.grad_fn
    while node is not None and not type(node).__name__.startswith("Conv"):
        node = node.next_functions[0][0]
    assert node is not None, "no convolution node behind the output"
    name = type(node).__name__
    return name[:-len("Backward")] if name.endswith("Backward") else name


def s1_run(n, h, w, cin, cout, seed):
    from adyolo_amd.models.backbones.resnet_conformer import _conv3x3_s1
    x = rnd(seed, n, h, w, cin)
    wt = rnd(seed + 1, cout, cin, 3, 3) / math.sqrt(9 * cin)
    dy = rnd(seed + 2, n, h, w, cout)
    xg, wg = dev(x).requires_grad_(True), dev(wt).requires_grad_(True)
    y = _conv3x3_s1(xg, wg)
    route = route_of(y)
    y.backward(dev(dy))
    torch.cuda.synchronize()
    return x, wt, dy, y.detach().cpu(), xg.grad.cpu(), wg.grad.cpu(), route


def conv_refs(x, wt, dy, pick, stride=(1, 1), padding=(1, 1)):
    """y and dx of the picked samples and dw of the whole batch, float64 and float32 (F.conv2d and its two gradients)."""
    out = []
    for dt in (torch.float64, torch.float32):
        xn, dyn, w_ = nchw(x.to(dt)), nchw(dy.to(dt)), wt.to(dt)
        y = F.conv2d(xn[pick], w_, None, stride=stride, padding=padding)
        dx = torch.nn.grad.conv2d_input(xn[pick].shape, w_, dyn[pick], stride=stride, padding=padding)
        dw = torch.nn.grad.conv2d_weight(xn, w_.shape, dyn, stride=stride, padding=padding)
        out.append((nhwc(y), nhwc(dx), dw))
    return out


def conv_value_check(tag, got, ref64, ref32, seq32, seq_slice):
    """The value bar with err_ref the larger of two float32 evaluations: PyTorch's own (``ref32``, the whole tensor) and the
    one-accumulator sum of ``oracle.conformer.conv_seq32_*`` (``seq32``: the part ``seq_slice`` of the tensor).  The kernels add
    the products of an output one after the other in one float32 MFMA accumulator; PyTorch's CPU convolution adds short blocked
    partial sums and is several times more accurate than ANY sum of that order (y: 2.1e-7 .. 3.6e-7 where the kernels have
    1.6e-6 .. 2.6e-6), so it alone is no measure of a float32 evaluation of the documented algorithm."""
    got, ref64, ref32 = d64(got), d64(ref64), d64(ref32)
    scale = float(ref64.abs().max())
    e_seq = float((d64(seq32) - ref64[seq_slice]).abs().max()) / scale
    e_pt = float((ref32 - ref64).abs().max()) / scale
    print("%-58s err_ref: PyTorch %.3e, one accumulator %.3e" % (tag, e_pt, e_seq))
    worse = ref32.clone()
    if e_seq > e_pt:
        worse[seq_slice] = d64(seq32)
    return value_check(tag, got, ref64, worse)


@pytest.mark.parametrize("geom,route", S1_CASES, ids=["x".join(map(str, g)) for g, _ in S1_CASES])
def test_conv3x3_s1_route_matches_float64(ops, geom, route):
    """The route the benchmark takes (and its evaluation / off-route neighbours): which form ran, then y and dx on three
    samples and dw over the whole batch against float64 F.conv2d(padding=1): value bar.  W == 1: the outer filter columns get
    exactly zero gradient.  (W == 2: every tap meets data -- kw = 0 through output bin 1, kw = 2 through output bin 0 -- so no
    tap is exactly zero there; a swapped block filter shows in all three tensors.)
    Measured (MI355X; worst y / dx / dw, err_ref in brackets): Conv3x3S1Fn 2.1e-6 (8.6e-7) / 2.1e-6 (1.0e-6) / 1.2e-6 (1.9e-6);
    Conv3x3NarrowFn 2.6e-6 (1.3e-6) / 2.5e-6 (1.3e-6) / 1.9e-6 (1.8e-6); Conv3x1WinoFn 2.6e-6 (1.4e-6) / 2.3e-6 (1.6e-6) / 6.6e-6 (2.8e-6);
    ConvFn 1.8e-6 (1.8e-6) / 2.0e-6 (1.3e-6) / 1.6e-6 (2.4e-6); worst err_gpu / bar 0.61."""
    n, h, w, cin, cout = geom
    x, wt, dy, y, dx, dw, took = s1_run(n, h, w, cin, cout, 17 * h + w + cin)
    ROUTES.setdefault(took, []).append(geom)
    assert took == route, "%s ran as %s, not %s" % (geom, took, route)
    assert ops.wino1d_ok(n, h, cin * w, cout * w) == (route == "Conv3x1WinoFn") or w > 2
    pick = sorted({p % n for p in CONV_PICK})
    (y64, dx64, dw64), (y32, dx32, dw32) = conv_refs(x, wt, dy, pick)
    tag = "conv3x3 s1 %s %s" % ("x".join(map(str, geom)), took)
    c = Collect()
    p0, one = pick[0], (1, 1)
    c(conv_value_check, tag + " y", y[pick], y64, y32, oc.conv_seq32_y(x[p0], wt, one, one), 0)
    c(conv_value_check, tag + " dx", dx[pick], dx64, dx32, oc.conv_seq32_dx(dy[p0], wt, one, one, h, w), 0)
    if took == "Conv3x1WinoFn":          # one GEMM over all N H / 4 tile rows in one accumulator (ops.wino1d_wgrad)
        c(conv_value_check, tag + " dw", dw, dw64, dw32, oc.conv3x3_seq32_dw(x, dy), slice(0, min(64, cout)))
    else:                                # (the other routes split the sum over slabs)
        c(value_check, tag + " dw", dw, dw64, dw32)
    if w == 1:
        assert float(dw[..., 0].abs().max()) == 0.0 and float(dw[..., 2].abs().max()) == 0.0
    c.finish()


@pytest.mark.parametrize("kh,kw,w,cin,cout", STRIDED_GEOMS)
def test_strided_conv_matches_float64(ops, kh, kw, w, cin, cout):
    """The 7x7 s(1,2) stem, the 3x3 s(1,2) and the 1x1 s(1,2) convolutions through Fn.ConvFn on two samples at H = 800.
    Measured (MI355X; worst of 7x7 / 3x3 / 1x1): y 9.4e-7 / 1.5e-6 / 5.7e-7, dx 1.6e-6 / 1.6e-6 / 9.3e-7, dw 5.4e-7 / 6.2e-7 / 6.3e-7; worst
    err_gpu / bar 0.40."""
    from adyolo_amd import functional as Fn
    n, h = 2, 800
    pad = (kh // 2, kw // 2)
    x = rnd(kh * 100 + w, n, h, w, cin)
    wt = rnd(kh * 100 + w + 1, cout, cin, kh, kw) / math.sqrt(kh * kw * cin)
    xg, wg = dev(x).requires_grad_(True), dev(wt).requires_grad_(True)
    y = Fn.ConvFn.apply(xg, wg, (1, 2), pad)
    dy = rnd(kh * 100 + w + 2, *y.shape)
    y.backward(dev(dy))
    torch.cuda.synchronize()
    ROUTES.setdefault(route_of(y), []).append((kh, kw, w, cin, cout))
    (y64, dx64, dw64), (y32, dx32, dw32) = conv_refs(x, wt, dy, [0, 1], (1, 2), pad)
    tag = "conv %dx%d s(1,2) W%d %d->%d" % (kh, kw, w, cin, cout)
    c = Collect()
    c(conv_value_check, tag + " y", y, y64, y32, oc.conv_seq32_y(x[0], wt, (1, 2), pad), 0)
    c(conv_value_check, tag + " dx", xg.grad, dx64, dx32, oc.conv_seq32_dx(dy[0], wt, (1, 2), pad, h, w), 0)
    c(value_check, tag + " dw", wg.grad, dw64, dw32)
    c.finish()


def _conformer_params():
    return {"args": {"device": "cuda:0", "encoder": "resnet-conformer", "loss": "adyolo"}, "data_config": {"nb_classes": 12},
            "train_config": {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
                             "loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
                             "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0}}


def test_route_constants_are_the_models_geometries(ops, monkeypatch):
    """One forward of the ResNet-Conformer encoder (64 mel bins like the benchmark's input; a short clip: the time axis is never
    strided) with _conv3x3_s1 and ops.conv_gemm recorded: the geometries are S1_GEOMS and STRIDED_GEOMS."""
    from adyolo_amd.models.backbones import resnet_conformer as rc
    from adyolo_amd.wrapper import WrapperModel
    s1, strided, state = set(), set(), {"inside": False}
    real_s1, real_gemm = rc._conv3x3_s1, ops.conv_gemm

    def rec_s1(x, w):
        s1.add((x.shape[2], x.shape[3], w.shape[0]))
        state["inside"] = True
        try:
            return real_s1(x, w)
        finally:
            state["inside"] = False

    def rec_gemm(mode, src, other, n, h, w, cin, cout, kh, kw, sh, sw, ph, pw):
        if not state["inside"]:
            assert (sh, sw) == (1, 2) and mode == 0
            strided.add((kh, kw, w, cin, cout))
        return real_gemm(mode, src, other, n, h, w, cin, cout, kh, kw, sh, sw, ph, pw)
    monkeypatch.setattr(rc, "_conv3x3_s1", rec_s1)
    monkeypatch.setattr(ops, "conv_gemm", rec_gemm)
    model = WrapperModel((1, 7, 32, 64), (), _conformer_params()).to("cuda:0").eval()
    with torch.no_grad():
        model.encoder(torch.randn(1, 7, 32, 64, device="cuda:0"))
    torch.cuda.synchronize()
    assert s1 == set(S1_GEOMS) and strided == set(STRIDED_GEOMS), (sorted(s1), sorted(strided))


def test_every_named_route_was_taken(ops):
    """Which form ran, at small channel counts and launched here so that the test stands alone: each of the four forms behind
    _conv3x3_s1 at least once, both sides of every clause of ops.wino1d_ok (rows, H % 4, Cin % 64, Cout % 64); what the other
    tests of the module logged are forms of the same table."""
    took = {}
    for geom in ((2, 16, 8, 64, 64), (2, 16, 4, 128, 128), (32, 256, 2, 32, 32), (32, 256, 1, 64, 64), (32, 252, 1, 64, 64),
                 (32, 254, 1, 64, 64), (32, 256, 1, 32, 64), (32, 256, 1, 64, 32), (2, 16, 3, 128, 128), (2, 16, 4, 24, 24)):
        took[geom] = s1_run(*geom, seed=5)[-1]
    print(took)
    assert took[(2, 16, 8, 64, 64)] == "Conv3x3S1Fn" and took[(2, 16, 4, 128, 128)] == took[(2, 16, 3, 128, 128)] == "Conv3x3NarrowFn"
    assert took[(32, 256, 2, 32, 32)] == took[(32, 256, 1, 64, 64)] == "Conv3x1WinoFn"          # 2048 rows exactly
    assert took[(32, 252, 1, 64, 64)] == "ConvFn"                                                 # 2016 rows
    assert took[(32, 254, 1, 64, 64)] == took[(32, 256, 1, 32, 64)] == took[(32, 256, 1, 64, 32)] == "ConvFn"
    assert took[(2, 16, 4, 24, 24)] == "ConvFn"
    assert set(took.values()) == set(NAMED_ROUTES)
    if ROUTES:                           # the benchmark-size cases ran in this session: they too took every form
        assert set(ROUTES) == set(NAMED_ROUTES), sorted(ROUTES)
