"""Oracle (test infrastructure): ResNet-Conformer encoder, PyTorch-CPU float32, functional over a reference-shaped
state_dict.  Restates /root/reference/src/models/backbones/resnet_conformer.py: MultiHeadAttention :25-85,
ConformerConvModule :154-178, FeedForwardModule :181-212, ConformerBlock :215-282, PoolingModule :285-297,
ResnetConformer :342-447.  The residual blocks of the front end are torchvision==0.11 ``BasicBlock``s
(README.md:20; not vendored in /root/reference): their published definition (conv3x3(stride) -> BN -> ReLU -> conv3x3 ->
BN, + identity or downsample(x), ReLU) is restated here -- PARITY UNPINNED for that block beyond the stub used to
generate tests/golden/conformer.npz.  Dropout (p = 0.2) is omitted: goldens are generated with dropout disabled.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

LAYER_BLOCKS = (3, 4, 5, 3)          # layer3 has 5 blocks, not 6 (resnet_conformer.py:373-384)
LAYER_WIDTHS = (64, 128, 256, 512)


def _bn(sd, p, x, training):
    rm, rv = sd[p + ".running_mean"].clone(), sd[p + ".running_var"].clone()
    return F.batch_norm(x, rm, rv, sd[p + ".weight"], sd[p + ".bias"], training=training, momentum=0.1, eps=1e-5)


def basic_block(sd, p, x, stride, training):
    out = F.conv2d(x, sd[p + ".conv1.weight"], None, stride=stride, padding=1)
    out = F.relu(_bn(sd, p + ".bn1", out, training))
    out = _bn(sd, p + ".bn2", F.conv2d(out, sd[p + ".conv2.weight"], None, padding=1), training)
    if (p + ".downsample.0.weight") in sd:
        idn = _bn(sd, p + ".downsample.1", F.conv2d(x, sd[p + ".downsample.0.weight"], None, stride=stride), training)
    else:
        idn = x
    return F.relu(out + idn)


def _ln(sd, p, x):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], 1e-5)


def _swish(x):
    return x * torch.sigmoid(x)


def feed_forward(sd, p, x):
    y = _ln(sd, p + ".sequential.0", x)
    y = _swish(F.linear(y, sd[p + ".sequential.1.weight"], sd[p + ".sequential.1.bias"]))
    return F.linear(y, sd[p + ".sequential.4.weight"], sd[p + ".sequential.4.bias"])


def attention(sd, p, x, heads=4):
    b, t, e = x.shape
    d = e // heads
    q, k, v = (F.linear(x, sd[p + "." + n + ".weight"], sd[p + "." + n + ".bias"]).view(b, t, heads, d).transpose(1, 2)
               for n in ("query", "key", "value"))
    w = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1)
    ctx = (w @ v).transpose(1, 2).reshape(b, t, e)
    return F.linear(ctx, sd[p + ".linear.weight"], sd[p + ".linear.bias"])


def conv_module(sd, p, x, dilation, training):
    y = _ln(sd, p + ".conv.0", x).transpose(1, 2)
    y = F.conv1d(y, sd[p + ".conv.2.weight"], sd[p + ".conv.2.bias"])
    y = F.glu(_bn(sd, p + ".conv.3", y, training), dim=1)
    y = F.conv1d(y, sd[p + ".conv.5.weight"], sd[p + ".conv.5.bias"], padding=dilation, dilation=dilation, groups=y.shape[1])
    y = _swish(_bn(sd, p + ".conv.6", y, training))
    return F.conv1d(y, sd[p + ".conv.8.weight"], sd[p + ".conv.8.bias"]).transpose(1, 2)


def conformer_block(sd, p, x, dilation, training):
    x = feed_forward(sd, p + ".sequential.0.module", x) * 0.5 + x
    x = attention(sd, p + ".sequential.1.module.1", _ln(sd, p + ".sequential.1.module.0", x)) * 0.5 + x
    x = conv_module(sd, p + ".sequential.2.module", x, dilation, training) + x
    x = feed_forward(sd, p + ".sequential.3.module", x) * 0.5 + x
    return _ln(sd, p + ".sequential.4", x)


def encoder_forward(sd, x, training=False, taps=None):
    """resnet_conformer.py:419-447.  x (B,7,T,64) -> (B, T//4, 256)."""
    y = F.conv2d(x, sd["conv1.weight"], None, stride=(1, 2), padding=3)
    y = _bn(sd, "bn1", F.relu(y), training)
    y = F.max_pool2d(y, 3, stride=(1, 2), padding=1)
    if taps is not None:
        taps["stem"] = y
    for li, nblk in enumerate(LAYER_BLOCKS, start=1):
        for bi in range(nblk):
            y = basic_block(sd, "layer%d.%d" % (li, bi), y, (1, 2) if bi == 0 else 1, training)
    if taps is not None:
        taps["layer4"] = y
    y = y.permute(0, 2, 1, 3).squeeze(-1)
    y = F.linear(y, sd["bottleneck.weight"])
    for i in range(8):
        y = conformer_block(sd, "conformer.encoder_module.%d" % i, y, 2 ** i, training)
        if taps is not None and i == 0:
            taps["block0"] = y
    y = y.transpose(1, 2)
    y = (F.avg_pool1d(y, 4) + F.avg_pool1d(y, 4)).transpose(1, 2)
    return _ln(sd, "t_pooling.norm", y)


# ================================================================================================ kernel-level references
# What tests/test_gpu_conformer_stage.py compares csrc/attention.hip and csrc/conformer.hip with (pinned on the CPU by
# tests/test_conformer_stage_cpu.py).  Every function follows the dtype of its inputs: float64 for the reference, float32 for
# the "plain float32 evaluation" the value bar is scaled by.
LOG2E = 1.4426950408889634
ATTN_BLOCK = 32                      # keys per step of the online softmax (csrc/attention.hip)
# (B, heads, T, p, seed) of the dropout masks the GPU module relies on; the CPU module checks their statistics (n >= 257 at p = 0.9:
# the normal approximation of the bound)
ATTN_MASK_CASES = [(2, 4, 800, 0.2, 0xC0FFEE + 800), (3, 4, 131, 0.2, 0xC0FFEE + 131), (2, 8, 257, 0.5, 12345), (2, 4, 257, 0.9, 7)]


def _heads(x, heads):
    b, t, e = x.shape
    return x.view(b, t, heads, e // heads).transpose(1, 2)              # [B][H][T][D]


def _merge(x):
    b, h, t, d = x.shape
    return x.transpose(1, 2).reshape(b, t, h * d)


def attention_materialised(q, k, v, heads, scale, mask=None):
    """dropout(softmax(scale q k^T)) v per head with the scores materialised (resnet_conformer.py:57-85); q, k, v [B][T][heads * D],
    mask [B][heads][T][T] holding 0 or 1 / (1 - p), or None.  -> (ctx [B][T][E], lse2 [B][heads][T] = log2 sum_k 2^(scale log2e s_k))."""
    qh, kh, vh = (_heads(z, heads) for z in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * scale
    w = torch.softmax(s, dim=-1)
    if mask is not None:
        w = w * mask.to(w.dtype)
    return _merge(w @ vh), torch.logsumexp(s, dim=-1) * LOG2E


def attention_materialised_bwd(q, k, v, dctx, heads, scale, mask=None):
    """The gradients of ``attention_materialised``'s ctx written out by hand: P_d = P mask, dV = P_d^T dO, dP = (dO V^T) mask,
    dS = P (dP - sum_k dP P) scale, dQ = dS K, dK = dS^T Q."""
    qh, kh, vh, doh = (_heads(z, heads) for z in (q, k, v, dctx))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    m = 1.0 if mask is None else mask.to(p.dtype)
    dv = (p * m).transpose(-1, -2) @ doh
    dp = (doh @ vh.transpose(-1, -2)) * m
    ds = p * (dp - (dp * p).sum(-1, keepdim=True)) * scale
    return _merge(ds @ kh), _merge(ds.transpose(-1, -2) @ qh), _merge(dv)


def attention_blockwise(q, k, v, heads, scale, mask=None, block=ATTN_BLOCK):
    """The algorithm csrc/attention.hip documents, in plain PyTorch: keys in blocks of ``block``, running maximum m and sum l in
    base 2 with q pre-scaled by scale * log2 e, the accumulator rescaled by alpha = 2^(m_old - m_new) at every block, the
    dropout mask applied to the probabilities that go into the product only, one division by l at the end.
    -> (ctx, lse2 = m + log2 l)."""
    qh, kh, vh = (_heads(z, heads) for z in (q, k, v))
    b, h, t, d = qh.shape
    sl = torch.tensor(scale, dtype=q.dtype) * torch.tensor(LOG2E, dtype=q.dtype)
    qs = qh * sl
    m = torch.full((b, h, t), -math.inf, dtype=q.dtype)
    l = torch.zeros((b, h, t), dtype=q.dtype)
    o = torch.zeros((b, h, t, d), dtype=q.dtype)
    for k0 in range(0, t, block):
        k1 = min(k0 + block, t)
        s = qs @ kh[:, :, k0:k1].transpose(-1, -2)
        m_new = torch.maximum(m, s.amax(dim=-1))
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(s - m_new[..., None])
        l = l * alpha + p.sum(-1)
        if mask is not None:
            p = p * mask[:, :, :, k0:k1].to(p.dtype)
        o = o * alpha[..., None] + p @ vh[:, :, k0:k1]
        m = m_new
    return _merge(o * (1.0 / l)[..., None]), m + torch.log2(l)


def attention_blockwise_bwd(q, k, v, ctx, dctx, lse2, heads, scale, mask=None, block=ATTN_BLOCK):
    """Backward as the kernels do it: P recomputed block by block as 2^(s - lse2) from the stored log-sum-exp,
    delta = sum_d dO O, dS = P (dP mask - delta) scale.  -> (dq, dk, dv, delta [B][heads][T])."""
    qh, kh, vh, oh, doh = (_heads(z, heads) for z in (q, k, v, ctx, dctx))
    t = qh.shape[2]
    sl = torch.tensor(scale, dtype=q.dtype) * torch.tensor(LOG2E, dtype=q.dtype)
    qs = qh * sl
    delta = (doh * oh).sum(-1)
    dq, dk, dv = torch.zeros_like(qh), torch.zeros_like(kh), torch.zeros_like(vh)
    for k0 in range(0, t, block):
        k1 = min(k0 + block, t)
        p = torch.exp2(qs @ kh[:, :, k0:k1].transpose(-1, -2) - lse2[..., None])
        m = 1.0 if mask is None else mask[:, :, :, k0:k1].to(p.dtype)
        dp = doh @ vh[:, :, k0:k1].transpose(-1, -2)
        ds = p * (dp * m - delta[..., None]) * scale
        dv[:, :, k0:k1] = (p * m).transpose(-1, -2) @ doh
        dk[:, :, k0:k1] = ds.transpose(-1, -2) @ qh
        dq += ds @ kh[:, :, k0:k1]
    return _merge(dq), _merge(dk), _merge(dv), delta


def attention_dv_recompute_allowance(q, k, dctx, heads, scale, mask=None):
    """What a float32 recomputation of P from a stored log-sum-exp may cost dV, derived from the inputs (float64 in).
    P = 2^(s2 - lse2) with s2 = scale log2e q.k and lse2 both float32 numbers of magnitude up to S = max |s2| of that (sample, head):
    whatever the order of the 64-term product before, the last operation that produced each of them rounds it by up to 2^-24 S,
    and the exponential turns an absolute error d of its argument into a relative error ln2 d of P.  So |dP| <= 2 ln2 2^-24 S P and
    |d dV[key]| <= 2 ln2 2^-24 S sum_query P_d[query][key] |dO[query]|.  (At T = 1 and 2 the CPU evaluations recompute s2 bit for
    bit as the forward made it and have no such error at all, while attn_bwd_dkv_kernel scales K instead of Q.)"""
    qh, kh, doh = (_heads(z, heads) for z in (q, k, dctx))
    s = qh @ kh.transpose(-1, -2) * scale
    p = torch.softmax(s, dim=-1)
    if mask is not None:
        p = p * mask.to(p.dtype)
    smax = (s.abs() * LOG2E).amax(dim=(-1, -2), keepdim=True)
    return _merge(2.0 * math.log(2.0) * 2.0 ** -24 * smax * (p.transpose(-1, -2) @ doh.abs()))


# ---- dropout of the attention weights: NumPy (uint32) restatement of attn_hash / attn_keep / drop_threshold / seed32_dev
def attn_hash_np(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def drop_threshold_np(p):
    """floor(p 2^32) of the float32 ``p``, saturated; 0 = no dropout."""
    p = float(np.float32(p))
    if p <= 0.0:
        return 0
    return int(min(p * 4294967296.0, 4294967295.0))


def keep_scale_np(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def attn_keep_np(b, heads, t, p, seed, samples=None):
    """bool [len(samples)][heads][T][T]: weight (b, h, query, key) is kept iff hash((((b H + h) T + query) T + key) * 0x9E3779B1 + seed)
    >= threshold, all in 32-bit unsigned arithmetic.  ``samples``: the batch indices wanted (default: all ``b``)."""
    samples = list(range(b)) if samples is None else list(samples)
    assert b * heads * t * t < 2 ** 32
    bi = np.asarray(samples, dtype=np.uint32)[:, None, None, None]
    hi = np.arange(heads, dtype=np.uint32)[None, :, None, None]
    qi = np.arange(t, dtype=np.uint32)[None, None, :, None]
    ki = np.arange(t, dtype=np.uint32)[None, None, None, :]
    with np.errstate(over="ignore"):
        row = (bi * np.uint32(heads) + hi) * np.uint32(t) + qi
        x = (row * np.uint32(t) + ki) * np.uint32(0x9E3779B1) + np.uint32(seed & 0xFFFFFFFF)
    return attn_hash_np(x) >= np.uint32(drop_threshold_np(p))


def attn_dropout_mask_np(b, heads, t, p, seed, samples=None):
    """float32 mask: 0 or fl(1 / (1 - p)) (``adyolo_attn_dropout_mask``)."""
    keep = attn_keep_np(b, heads, t, p, seed, samples)
    return np.where(keep, keep_scale_np(p), np.float32(0.0)).astype(np.float32)


def seed32_np(seed, offset):
    """``rng.DropoutStream.seed32`` / ``seed32_dev_kernel``: splitmix64 finaliser of seed ^ (offset * golden ratio), low 32 bits."""
    m64 = (1 << 64) - 1
    x = (seed ^ ((offset * 0x9E3779B97F4A7C15) & m64)) & m64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m64
    return (x ^ (x >> 31)) & 0xFFFFFFFF


def union_z(tests, prob=1e-6):
    """z with 2 * tests * Q(z) <= prob (normal approximation, two-sided, union bound over ``tests`` tests)."""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if tests * math.erfc(mid / math.sqrt(2.0)) > prob:
            lo = mid
        else:
            hi = mid
    return hi


def dropout_mask_statistics(keep, p):
    """keep: bool [B][H][T][T].  Deviation of the keep share from 1 - p in standard deviations sqrt(p (1 - p) / n): of the whole
    mask, the worst row (n = T keys) and the worst column (n = T queries) -> (z_all, z_row, z_col, rows + columns checked)."""
    keep = np.asarray(keep)
    t = keep.shape[-1]
    q = 1.0 - float(np.float32(p))
    sd = lambda n: math.sqrt(q * (1.0 - q) / n)                         # noqa: E731
    z_all = abs(float(keep.mean()) - q) / sd(keep.size)
    z_row = float(np.abs(keep.mean(axis=-1) - q).max()) / sd(t)
    z_col = float(np.abs(keep.mean(axis=-2) - q).max()) / sd(t)
    return z_all, z_row, z_col, 2 * keep.size // t


def slabs_distinct(keep):
    """No two (b, h) slabs of the mask are equal."""
    flat = np.asarray(keep).reshape(-1, keep.shape[-2] * keep.shape[-1])
    packed = np.packbits(flat, axis=1)
    return len({r.tobytes() for r in packed}) == flat.shape[0]


# ---- max-pool 3 x 3, stride (1, 2), padding 1 with the tap number of the maximum
def maxpool3_taps(x_nhwc):
    """-> (y [N][H][Wo][C], tap uint8 = kh * 3 + kw of the element F.max_pool2d routes the gradient to: the first maximum in
    row-major order of the window's in-map elements, the first in-map element for an all -inf window, a NaN if there is one)."""
    n, h, w, c = x_nhwc.shape
    y, idx = F.max_pool2d(x_nhwc.permute(0, 3, 1, 2), 3, stride=(1, 2), padding=1, return_indices=True)
    wo = y.shape[-1]
    hh, ww = idx // w, idx % w
    kh = hh - (torch.arange(h).view(1, 1, h, 1) - 1)
    kw = ww - (2 * torch.arange(wo).view(1, 1, 1, wo) - 1)
    assert bool(((kh >= 0) & (kh < 3) & (kw >= 0) & (kw < 3)).all())
    return y.permute(0, 2, 3, 1).contiguous(), (kh * 3 + kw).permute(0, 2, 3, 1).contiguous().to(torch.uint8)


def maxpool3_bwd_from_taps(dy_nhwc, tap, w):
    """dx [N][H][W][C]: every window's gradient added to the element its tap names."""
    n, h, wo, c = dy_nhwc.shape
    dx = torch.zeros(n, h, w, c, dtype=dy_nhwc.dtype)
    t = tap.long()
    hh = torch.arange(h).view(1, h, 1, 1) - 1 + t // 3
    ww = 2 * torch.arange(wo).view(1, 1, wo, 1) - 1 + t % 3
    ni = torch.arange(n).view(n, 1, 1, 1).expand_as(t)
    ci = torch.arange(c).view(1, 1, 1, c).expand_as(t)
    dx.index_put_((ni, hh.expand_as(t), ww.expand_as(t), ci), dy_nhwc, accumulate=True)
    return dx


# ---- convolutions summed in ONE float32 accumulator per output, the order the matrix-core kernels document
def conv_seq32_y(x_hwc, wt, stride, padding):
    """Forward convolution of one sample x [H][W][Cin] with wt [Cout][Cin][KH][KW] in float32, every output one running sum over
    the KH KW Cin products in the order (kh, kw, ci) of the implicit GEMM (k = (kh KW + kw) Cin + ci) -- what 4 err_ref should
    reflect for a kernel that adds its products one after the other, where PyTorch's own float32 convolution adds short
    blocked partial sums.  -> [Ho][Wo][Cout]."""
    cout, cin, kh, kw = wt.shape
    (sh, sw), (ph, pw) = stride, padding
    h, w, _ = x_hwc.shape
    ho, wo = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    xp = F.pad(x_hwc.float().permute(2, 0, 1), (pw, pw, ph, ph))
    wt = wt.float()
    acc = torch.zeros(cout, ho, wo)
    for a in range(kh):
        for b in range(kw):
            xs = xp[:, a:a + (ho - 1) * sh + 1:sh, b:b + (wo - 1) * sw + 1:sw]
            if not bool(xs.any()):
                continue                                   # a tap that only meets padding adds exact zeros
            for ci in range(cin):
                acc.addcmul_(wt[:, ci, a, b].view(cout, 1, 1), xs[ci].unsqueeze(0))
    return acc.permute(1, 2, 0).contiguous()


def conv_seq32_dx(dy_hwc, wt, stride, padding, h, w):
    """Data gradient of one sample, dy [Ho][Wo][Cout] -> dx [H][W][Cin], in float32 with one running sum per element over the
    KH KW Cout products, order (kh, kw, co)."""
    cout, cin, kh, kw = wt.shape
    (sh, sw), (ph, pw) = stride, padding
    ho, wo, _ = dy_hwc.shape
    dyc = dy_hwc.float().permute(2, 0, 1)
    wt = wt.float()
    acc = torch.zeros(cin, h + 2 * ph + kh, w + 2 * pw + kw)
    for a in range(kh):
        for b in range(kw):
            view = acc[:, a:a + (ho - 1) * sh + 1:sh, b:b + (wo - 1) * sw + 1:sw]
            for co in range(cout):
                view.addcmul_(wt[co, :, a, b].view(cin, 1, 1), dyc[co].unsqueeze(0))
    return acc[:, ph:ph + h, pw:pw + w].permute(1, 2, 0).contiguous()


def conv3x3_seq32_dw(x, dy, cout_keep=64, tile=4, chunk=256):
    """Weight gradient of a stride-1 3x3 convolution (padding 1), x [N][H][W][Cin], dy [N][H][W][Cout], in float32 with one running
    sum per entry over the N H / tile tile rows (a tile row's own products are added first), the order of a GEMM whose contraction
    runs over the tile rows in one accumulator (``ops.wino1d_wgrad``).  For the first ``cout_keep`` output channels
    -> [cout_keep][Cin][3][3]."""
    n, h, w, cin = x.shape
    co = min(cout_keep, dy.shape[-1])
    assert h % tile == 0
    rows = n * h // tile
    xp = F.pad(x.float(), (0, 0, 1, 1, 1, 1))
    dyr = dy.float()[..., :co].reshape(rows, tile * w, co)
    out = torch.zeros(co, cin, 3, 3)
    for a in range(3):
        for b in range(3):
            xs = xp[:, a:a + h, b:b + w].reshape(rows, tile * w, cin)
            acc = torch.zeros(co, cin)
            for r0 in range(0, rows, chunk):
                part = dyr[r0:r0 + chunk].transpose(1, 2) @ xs[r0:r0 + chunk]              # [chunk][co][cin]
                for r in range(part.shape[0]):             # (a plain loop: torch.cumsum accumulates float32 in double on the CPU)
                    acc += part[r]
            out[:, :, a, b] = acc
    return out
