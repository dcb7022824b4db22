"""Oracle (test infrastructure): cases, inputs, float64 references, the checker and a float32 emulation for the tests of the
implicit-GEMM convolution (K7, ``adyolo_conv_gemm`` in csrc/gemm.hip: ``gemm_kernel<false,false,1>`` for the forward and the data
gradient, ``gemm_kernel<true,true,2>`` for the weight gradient).  tests/test_conv_gemm_stage_cpu.py pins everything here on the CPU,
tests/test_gpu_conv_gemm_stage.py compares the kernels with it.  Imports no project code.

A case is ``(n, h, w, cin, cout, kh, kw, sh, sw, ph, pw)``; it runs in the three modes of the entry point, mode 2 with every
``splits`` of ``SPLITS``.  ``plan`` mirrors the host decisions (the GPU module asserts it against ``adyolo_conv_gemm_plan``) and
names the form the kernel takes:

    modes 0 / 1   pixel operand  "GA"     descriptor gather: tap in the scalar offset, base moved back by the tap bias
                                 "carry"  (c, kh, kw) carried from K tile to K tile, general loads
                                 "div"    (c, kh, kw) by division from k; a K tile may straddle taps
                  filter         "descriptor" (K % 32 == 0) or "general" (K tail zero-filled)
    mode 2        pixel triple   "fastp"  (x, y, n) of a K row carried, started from kbeg under split-K
                                 "div"    by division from k

``build`` embeds the gathered source in NaN (in front: at least the tap bias + 64 floats, which is where a descriptor moved back
by the bias points), the other operand and the slab workspace in NaN, the output in the sentinel ``SENT``.  ``check`` wants

    |got - ref| <= (K + S + 4) * u * (|A| |B|),        u = 2^-24,

per element, with float64 references from explicit tap loops, K the contraction length of the mode and S the effective number
of splits: the derivation of oracle/gemm_stage.py (any-order summation, one rounding per operation, S - 1 more in the slab sum).
No margin.  An element whose float64 sum has no term (rows of dx no output touches, taps that only ever meet padding) has bound
0 and must be exactly 0.  Every float outside the output window must keep its bits.

``emulate`` is a float32 NumPy model of the staging, tile by tile and split by split through the kernel's index arithmetic on
the same embedded buffers, with the plantable faults of ``FAULTS``."""
import functools

import numpy as np

U = 2.0 ** -24
GBM, GBN, GBK = 128, 64, 32
FETCH_LIMIT = (1 << 29) - 64
SENT = np.float32(-777.25)
PRE, POST = 16, 64
F32 = np.float32
SPLITS = (1, 2, 3, 7, 64)
MODES = (0, 1, 2)

# (n, h, w, cin, cout, kh, kw, sh, sw, ph, pw)
CASES = (
    (2, 9, 4, 32, 64, 3, 3, 1, 1, 1, 1),        # 36 pixels per sample
    (3, 7, 5, 64, 68, 3, 3, 1, 1, 1, 1),
    (2, 37, 1, 32, 32, 3, 1, 1, 1, 1, 0),       # Wo = 1
    (1, 1, 40, 32, 4, 1, 3, 1, 1, 0, 1),        # H = 1; data gradient with K = 12
    (2, 10, 6, 32, 64, 3, 3, 2, 2, 1, 1),       # a dx row and column that no output touches
    (2, 9, 8, 64, 32, 3, 3, 1, 2, 1, 1),
    (2, 11, 7, 32, 32, 1, 1, 2, 2, 0, 0),       # stride > kernel: whole dx rows and columns exactly zero
    (2, 12, 9, 32, 64, 3, 3, 3, 2, 0, 1),
    (2, 6, 6, 16, 16, 2, 2, 1, 1, 1, 1),        # a K tile straddles taps
    (2, 6, 6, 16, 48, 2, 2, 2, 2, 0, 0),
    (1, 20, 16, 8, 64, 7, 7, 1, 2, 3, 3),       # the stem's form; K = 392
    (2, 8, 4, 48, 40, 3, 3, 1, 1, 1, 1),        # Ho = 32 / Wo exactly
    (2, 9, 5, 12, 20, 3, 3, 2, 1, 1, 1),        # Kp = 108
    (3, 13, 3, 4, 4, 1, 1, 1, 1, 0, 0),         # K = 4
    (1, 16, 8, 32, 132, 3, 3, 1, 1, 1, 1),      # M = 128; Cout = 132
    (2, 5, 5, 32, 32, 3, 3, 1, 1, 2, 2),        # padding k - 1
    (5, 5, 5, 32, 32, 3, 3, 1, 1, 1, 1),        # M = 125
    (2, 33, 2, 32, 32, 3, 3, 1, 2, 1, 1),
    (2, 3, 64, 32, 32, 1, 3, 1, 1, 0, 1),       # Wo = 64
    (2, 2, 16, 32, 32, 3, 3, 1, 1, 1, 1),       # Wo = 16 with Ho = 2 exactly
    # what the coverage assertions of the CPU module missed in the list above
    (1, 16, 2, 8, 8, 3, 3, 1, 1, 1, 1),         # Wo = 2 with Ho = 16 exactly
    (1, 34, 1, 4, 8, 3, 1, 1, 1, 0, 0),         # Wo = 1 with Ho = 32 exactly
    (3, 4, 8, 8, 8, 3, 3, 1, 1, 1, 1),          # Wo = 8 with Ho = 4 exactly
    (3, 1, 32, 8, 8, 1, 3, 1, 1, 0, 1),         # Wo = 32 with Ho = 1 exactly
    (2, 1, 16, 8, 12, 1, 3, 1, 1, 0, 1),        # Wo = 16 with Ho = 1: fastp refused
    (2, 7, 6, 8, 8, 5, 3, 2, 1, 2, 1),          # 5 x 3 taps, stride (2, 1)
)


def cdiv(a, b):
    return -(-a // b)


def name(case):
    return "n%d_%dx%d_c%d_%d_k%dx%d_s%d%d_p%d%d" % tuple(case)


def out_hw(case):
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw = case
    return (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1


def geometry(case, mode):
    """The GEMM and the gather of a mode as ``adyolo_conv_gemm`` sets them up: M, Nn, K, source map [Hs][Ws][Cs], pixel grid
    [Hm][Wm] of the GEMM index that runs over pixels, dgrad, ldo (leading dimension of the packed filter, modes 0 / 1)."""
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw = case
    ho, wo = out_hw(case)
    kp, kq = cdiv(kh * kw * cin, 4) * 4, cdiv(kh * kw * cout, 4) * 4
    if mode == 0:
        return {"M": n * ho * wo, "Nn": cout, "K": kp, "Hs": h, "Ws": w, "Cs": cin, "Hm": ho, "Wm": wo, "dgrad": 0, "ldo": kp,
                "kreal": kh * kw * cin}
    if mode == 1:
        return {"M": n * h * w, "Nn": cin, "K": kq, "Hs": ho, "Ws": wo, "Cs": cout, "Hm": h, "Wm": w, "dgrad": 1, "ldo": kq,
                "kreal": kh * kw * cout}
    return {"M": cout, "Nn": kp, "K": n * ho * wo, "Hs": h, "Ws": w, "Cs": cin, "Hm": ho, "Wm": wo, "dgrad": 0, "ldo": 0,
            "kreal": kh * kw * cin}


def plan(case, mode, splits=1):
    """Mirror of the host entry.  -> dict M, Nn, K, klen, splits (effective), last (length of the last K slice), fastg, fastk,
    fastp, pixel ("GA" / "carry" / "div" in modes 0 / 1, "fastp" / "div" in mode 2), filter ("descriptor" / "general"; mode 2:
    None -- its plain operand dy is transposed and always takes the general fetch)."""
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw = case
    g = geometry(case, mode)
    m, nn, k = g["M"], g["Nn"], g["K"]
    splits = max(1, int(splits)) if mode == 2 else 1
    klen = cdiv(cdiv(k, splits), GBK) * GBK
    eff = cdiv(k, klen)
    if mode == 2:
        ea, eb = (k - 1) * cout + m, (k - 1) * 4 + 4
    else:
        ea, eb = 3 * 4 + k, (nn - 1) * g["ldo"] + k
    fastg = 3 if (k % GBK == 0 and ea < FETCH_LIMIT and eb < FETCH_LIMIT) else 0
    fastg &= 1 if mode == 2 else 2
    fastk = int(mode != 2 and g["Cs"] % GBK == 0)
    fastp = int(mode == 2 and GBK % g["Wm"] == 0 and g["Hm"] >= GBK // g["Wm"])
    if (fastg and mode != 2 and fastk and (mode == 0 or (sh == 1 and sw == 1))
            and n * g["Hs"] * g["Ws"] * g["Cs"] + (kh * g["Ws"] + kw) * g["Cs"] < (1 << 29)):
        fastg |= 4
    if mode == 2:
        pixel, filt = ("fastp" if fastp else "div"), None
    else:
        pixel = "GA" if fastg & 4 else ("carry" if fastk else "div")
        filt = "descriptor" if fastg & 2 else "general"
    return {"M": m, "Nn": nn, "K": k, "klen": klen, "splits": eff, "last": k - (eff - 1) * klen, "fastg": fastg, "fastk": fastk,
            "fastp": fastp, "pixel": pixel, "filter": filt}


def plan_row(case, mode, splits=1):
    """``plan`` as the eight integers of ``adyolo_conv_gemm_plan``."""
    p = plan(case, mode, splits)
    return [p["M"], p["Nn"], p["K"], p["klen"], p["splits"], p["fastg"], p["fastk"], p["fastp"]]


# every form a mode can take at sizes below the 2^29 switch.  Not feasible, by the kernel's own code: "GA" or "carry" with the
# general filter fetch (source channels % 32 == 0 makes K a multiple of 32); "carry" in mode 0 (fastk and whole K tiles give bit 2)
FEASIBLE = {0: (("GA", "descriptor"), ("div", "descriptor"), ("div", "general")),
            1: (("GA", "descriptor"), ("carry", "descriptor"), ("div", "descriptor"), ("div", "general")),
            2: (("fastp", None), ("div", None))}


def form_of(case, mode):
    p = plan(case, mode)
    return (p["pixel"], p["filter"])


def runs():
    """Every (case, mode, splits) the modules run."""
    return [(c, m, s) for c in CASES for m in MODES for s in (SPLITS if m == 2 else (1,))]


# ----------------------------------------------------------------------------------------------------------------- inputs
def _seed(case):
    s = 17
    for v in case:
        s = (s * 131 + v) % (2 ** 31 - 1)
    return s


def _spike(rng, t):
    """A few large isolated values in the first and last row and column of every sample of t [n][H][W][C]."""
    n, hh, ww, c = t.shape
    for b in range(n):
        for (ys, xs) in (((0,), range(ww)), ((hh - 1,), range(ww)), (range(hh), (0,)), (range(hh), (ww - 1,))):
            ys, xs = list(ys), list(xs)
            for _ in range(2):
                y, x, ch = ys[rng.integers(len(ys))], xs[rng.integers(len(xs))], rng.integers(c)
                t[b, y, x, ch] = F32(rng.choice((-1.0, 1.0)) * rng.uniform(8.0, 16.0))


@functools.lru_cache(maxsize=None)
def tensors(case):
    """x [N][H][W][Cin], w [Cout][Cin][KH][KW], dy [N][Ho][Wo][Cout] (float32, seeded by the case; shared by the three modes)."""
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw = case
    ho, wo = out_hw(case)
    rng = np.random.default_rng(_seed(case))
    x = rng.standard_normal((n, h, w, cin)).astype(F32)
    wt = (rng.standard_normal((cout, cin, kh, kw)) / np.sqrt(kh * kw * cin)).astype(F32)
    dy = rng.standard_normal((n, ho, wo, cout)).astype(F32)
    _spike(rng, x)
    _spike(rng, dy)
    for t in (x, wt, dy):
        t.setflags(write=False)
    return x, wt, dy


def pack_wk(w):
    """w [Cout][Cin][KH][KW] -> [Cout][roundup4(KH KW Cin)], k = (kh KW + kw) Cin + ci, zeros behind."""
    cout, cin, kh, kw = w.shape
    out = np.zeros((cout, cdiv(kh * kw * cin, 4) * 4), dtype=w.dtype)
    out[:, :kh * kw * cin] = w.transpose(0, 2, 3, 1).reshape(cout, -1)
    return out


def unpack_wk(wk, cout, cin, kh, kw):
    return np.ascontiguousarray(wk[:, :kh * kw * cin].reshape(cout, kh, kw, cin).transpose(0, 3, 1, 2))


def _taps(case, x64, w64, dy64):
    """y, dx, dw by explicit tap loops on zero-padded float64 arrays."""
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw = case
    ho, wo = out_hw(case)
    xp = np.zeros((n, h + 2 * ph, w + 2 * pw, cin))
    xp[:, ph:ph + h, pw:pw + w] = x64
    y = np.zeros((n, ho, wo, cout))
    dxp = np.zeros_like(xp)
    dw = np.zeros((cout, cin, kh, kw))
    for a in range(kh):
        for b in range(kw):
            ys, xs = slice(a, a + sh * (ho - 1) + 1, sh), slice(b, b + sw * (wo - 1) + 1, sw)
            y += xp[:, ys, xs] @ w64[:, :, a, b].T
            dxp[:, ys, xs] += dy64 @ w64[:, :, a, b]
            dw[:, :, a, b] = np.einsum("nyxo,nyxi->oi", dy64, xp[:, ys, xs])
    return y, dxp[:, ph:ph + h, pw:pw + w], dw


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> {mode: (ref, mag, terms)}: float64 result in the GEMM's output layout, the same on absolute values, and the number of
    terms of every element's sum (a tap that meets padding is no term)."""
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw = case
    x, wt, dy = (t.astype(np.float64) for t in tensors(case))
    ref = _taps(case, x, wt, dy)
    mag = _taps(case, np.abs(x), np.abs(wt), np.abs(dy))
    cnt = _taps(case, np.ones_like(x), np.ones_like(wt), np.ones_like(dy))

    def lay(t3):
        y, dx, dw = t3
        return {0: y.reshape(-1, cout), 1: dx.reshape(-1, cin), 2: pack_wk(dw)}
    r, m, c = lay(ref), lay(mag), lay(cnt)
    return {mode: (r[mode], m[mode], c[mode]) for mode in MODES}


def tap_bias(case, mode):
    """Floats by which the descriptor of the gathered operand is moved back (form GA)."""
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw = case
    g = geometry(case, mode)
    return ((kh - 1) * g["Ws"] + (kw - 1)) * g["Cs"] if g["dgrad"] else (ph * g["Ws"] + pw) * g["Cs"]


def build(case, mode, splits=1):
    """-> dict: srcbuf / src0 (the gathered operand at float offset src0 of a NaN-filled buffer, src0 a multiple of 4 and at
    least the tap bias + 64), othbuf / oth0 (filter or dy, NaN around), outbuf / out0 (SENT around a SENT-filled window), slabbuf
    / slab0 (mode 2: NaN-filled workspace for the effective splits), ref, bound, terms (float64, [M][Nn])."""
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw = case
    g = geometry(case, mode)
    x, wt, dy = tensors(case)
    src = (x, dy, x)[mode].reshape(-1)
    oth = (pack_wk(wt), pack_wk(np.ascontiguousarray(wt.transpose(1, 0, 2, 3))), dy)[mode].reshape(-1)
    front = cdiv(max(tap_bias(case, 0), tap_bias(case, 1)) + 64, 4) * 4
    back = (kh * g["Ws"] + kw) * g["Cs"] + POST
    srcbuf = np.full(front + src.size + back, np.nan, dtype=F32)
    srcbuf[front:front + src.size] = src
    othbuf = np.full(PRE + oth.size + POST, np.nan, dtype=F32)
    othbuf[PRE:PRE + oth.size] = oth
    p = plan(case, mode, splits)
    m, nn = g["M"], g["Nn"]
    outbuf = np.full(PRE + m * nn + POST, SENT, dtype=F32)
    slabbuf = np.full(PRE + p["splits"] * m * nn + POST, np.nan, dtype=F32) if mode == 2 else None
    ref, mag, terms = reference(case)[mode]
    return {"srcbuf": srcbuf, "src0": front, "othbuf": othbuf, "oth0": PRE, "outbuf": outbuf, "out0": PRE, "slabbuf": slabbuf,
            "slab0": PRE, "ref": ref, "bound": (g["K"] + p["splits"] + 4) * U * mag, "terms": terms, "plan": p}


def check(case, mode, inp, out_buffer):
    """out_buffer: the whole output buffer after the call.  -> worst err / bound over the elements with a term."""
    tag = "%s mode %d" % (name(case), mode)
    out = np.asarray(out_buffer, dtype=F32).reshape(-1)
    assert out.shape == inp["outbuf"].shape, "%s: output buffer of %d floats, expected %d" % (tag, out.size, inp["outbuf"].size)
    m, nn = inp["ref"].shape
    o0 = inp["out0"]
    inside = np.zeros(out.size, dtype=bool)
    inside[o0:o0 + m * nn] = True
    changed = (out.view(np.int32) != inp["outbuf"].view(np.int32)) & ~inside
    assert not changed.any(), "%s: %d floats outside the output window changed (first at float offset %d)" % (
        tag, int(changed.sum()), int(np.argmax(changed)))
    got32 = out[o0:o0 + m * nn].reshape(m, nn)
    assert np.isfinite(got32).all(), "%s: %d results are not finite" % (tag, int((~np.isfinite(got32)).sum()))
    assert not (got32 == SENT).any(), "%s: %d elements of the window keep the sentinel" % (tag, int((got32 == SENT).sum()))
    got = got32.astype(np.float64)
    empty = inp["terms"] == 0
    assert (got[empty] == 0.0).all(), "%s: %d elements without a term are not exactly 0" % (tag, int((got[empty] != 0.0).sum()))
    err = np.abs(got - inp["ref"])
    ratio = np.where(empty, 0.0, err / np.where(empty, 1.0, inp["bound"]))
    worst = float(ratio.max())
    assert (err <= inp["bound"]).all(), "%s: %d of %d elements over the bound, worst err / bound %.3f (err %.3e)" % (
        tag, int((err > inp["bound"]).sum()), err.size, worst, float(err.max()))
    return worst


# -------------------------------------------------------------------------------------------------------------- emulation
FAULTS = ("no_row_mask", "no_col_mask", "no_divisibility_test", "no_tap_flip", "no_kw_carry", "no_sample_carry",
          "fastp_from_zero", "no_ktail_zero_fill", "drop_last_split", "bias_off_by_one_pixel")


def _tdiv(a, b):
    """Integer division that truncates toward zero, as in C."""
    return np.sign(a) * (np.abs(a) // b)


def _inside(v, size, dropped):
    """0 <= v < size, or everywhere when the fault drops the mask."""
    return ((v >= 0) & (v < size)) | dropped


def _read(buf, idx, ok, stats, key):
    vals = buf[np.clip(idx, 0, buf.size - 1)]
    if stats is not None:
        stats[key] = stats.get(key, 0) + int(ok.sum())
    return np.where(ok, vals, F32(0)).astype(F32)


def _emulate_g1(case, mode, inp, fault, stats):
    """gemm_kernel<false,false,1>: A gathered [M][K], B = the packed filter [Nn][K]."""
    n, h, w, cin, cout, kh_, kw_, sh, sw, ph, pw = case
    g, p = geometry(case, mode), inp["plan"]
    m_, nn_, k_, hs, ws, cs, hm, wm, dgrad = g["M"], g["Nn"], g["K"], g["Hs"], g["Ws"], g["Cs"], g["Hm"], g["Wm"], g["dgrad"]
    src, s0, oth, o0 = inp["srcbuf"], inp["src0"], inp["othbuf"], inp["oth0"]
    m = np.arange(m_)[:, None]
    x_, t_ = m % wm, m // wm
    y_, n_ = t_ % hm, t_ // hm
    gy = y_ + ph if dgrad else y_ * sh - ph
    gx = x_ + pw if dgrad else x_ * sw - pw
    gb = n_ * hs * ws
    col = np.arange(GBK)[None, :]
    fastk, form = p["fastk"], p["pixel"]
    c_run = kh_run = kw_run = 0
    acc = np.zeros((m_, nn_), dtype=F32)
    nrow = np.arange(nn_)[:, None]
    kend = k_
    no_row, no_col = fault == "no_row_mask", fault == "no_col_mask"
    for k0 in range(0, k_, GBK):
        k = k0 + col
        if fastk:
            c, kh, kw = c_run + col, kh_run, kw_run
            c_run += GBK
            if c_run >= cs:
                c_run = 0
                kw_run += 1
                if kw_run == kw_ and fault != "no_kw_carry":
                    kw_run = 0
                    kh_run += 1
        else:
            tap = k // cs
            c, kh = k - tap * cs, tap // kw_
            kw = tap - kh * kw_
        if fault == "no_tap_flip" and dgrad:
            kh, kw = kh_ - 1 - kh, kw_ - 1 - kw
        if form == "GA":
            bias = tap_bias(case, mode)
            base = s0 - (bias - cs if fault == "bias_off_by_one_pixel" else bias)          # where the descriptor points
            if dgrad:
                pix = gb + (gy - (kh_ - 1)) * ws + gx - (kw_ - 1)
                so = ((kh_ - 1 - kh) * ws + (kw_ - 1 - kw)) * cs
                sy, sx = gy - kh, gx - kw
            else:
                pix = gb + gy * ws + gx
                so = (kh * ws + kw) * cs
                sy, sx = gy + kh, gx + kw
            voff = pix * cs + bias + col                                                # vector offset incl. the lane's column
            records = hs * ws * cs * n + bias
            ok = _inside(sy, hs, no_row) & _inside(sx, ws, no_col) & (voff >= 0) & (voff < records)               # the range check sees the vector offset alone
            at = _read(src, base + voff + so + (c - col), ok, stats, "a_reads")         # c - col: c_run of this tile
        else:
            kok = ((k < kend) & (k < g["kreal"])) | (fault == "no_ktail_zero_fill")
            if dgrad:
                ty, tx = gy - kh, gx - kw
                sy, sx = _tdiv(ty, sh), _tdiv(tx, sw)
                exact = ((sy * sh == ty) & (sx * sw == tx)) | (fault == "no_divisibility_test")
                ok = kok & (ty >= 0) & (tx >= 0) & exact
                if no_row or no_col:
                    ok = kok & exact & ((ty >= 0) | no_row) & ((tx >= 0) | no_col)
            else:
                sy, sx = gy + kh, gx + kw
                ok = kok
            ok = ok & _inside(sy, hs, no_row) & _inside(sx, ws, no_col)
            at = _read(src, s0 + (gb + sy * ws + sx) * cs + c, ok, stats, "a_reads")
        okb = (k < kend) | (fault == "no_ktail_zero_fill") | np.zeros((nn_, 1), dtype=bool)
        bt = _read(oth, o0 + nrow * g["ldo"] + k, okb, stats, "b_reads")
        acc = (acc + at @ bt.T).astype(F32)
    return acc


def _emulate_g2(case, inp, fault, stats):
    """gemm_kernel<true,true,2> and the slab sum: A = dy^T [K pixels][M = Cout], B gathered [K pixels][Nn = (kh, kw, c)]."""
    n, h, w, cin, cout, kh_, kw_, sh, sw, ph, pw = case
    g, p = geometry(case, 2), inp["plan"]
    m_, nn_, k_, hs, ws, cs, hm, wm = g["M"], g["Nn"], g["K"], g["Hs"], g["Ws"], g["Cs"], g["Hm"], g["Wm"]
    src, s0, oth, o0 = inp["srcbuf"], inp["src0"], inp["othbuf"], inp["oth0"]
    nn = np.arange(nn_)[None, :]
    tap = nn // cs
    bc, bkh = nn - tap * cs, tap // kw_
    bkw = tap - bkh * kw_
    row = np.arange(GBK)[:, None]
    mcol = np.arange(m_)[None, :]
    slabs = []
    for z in range(p["splits"]):
        kbeg, kend = z * p["klen"], min(k_, (z + 1) * p["klen"])
        k_start = 0 if fault == "fastp_from_zero" else kbeg
        px, py, pn = (k_start + row) % wm, ((k_start + row) // wm) % hm, ((k_start + row) // wm) // hm
        acc = np.zeros((m_, nn_), dtype=F32)
        for k0 in range(kbeg, kend, GBK):
            k = k0 + row
            kok = (k < kend) | (fault == "no_ktail_zero_fill")
            if p["fastp"]:
                x_, y_, n_ = px, py.copy(), pn.copy()
                py = py + GBK // wm
                carry = py >= hm
                py = np.where(carry, py - hm, py)
                if fault != "no_sample_carry":
                    pn = pn + carry
            else:
                x_, t_ = k % wm, k // wm
                y_, n_ = t_ % hm, t_ // hm
            sy, sx = y_ * sh - ph + bkh, x_ * sw - pw + bkw
            ok = kok & _inside(sy, hs, fault == "no_row_mask") & _inside(sx, ws, fault == "no_col_mask")
            bt = _read(src, s0 + ((n_ * hs + sy) * ws + sx) * cs + bc, ok, stats, "b_reads")
            at = _read(oth, o0 + k * cout + mcol, kok | np.zeros((1, m_), dtype=bool), stats, "a_reads")
            acc = (acc + at.T @ bt).astype(F32)
        slabs.append(acc)
    if p["splits"] == 1:
        return slabs[0]
    slabbuf = inp["slabbuf"].copy()
    for z, sl in enumerate(slabs):
        slabbuf[inp["slab0"] + z * m_ * nn_:inp["slab0"] + (z + 1) * m_ * nn_] = sl.reshape(-1)
    total = np.zeros(m_ * nn_, dtype=F32)
    for z in range(p["splits"] - (fault == "drop_last_split")):
        total = (total + slabbuf[inp["slab0"] + z * m_ * nn_:inp["slab0"] + (z + 1) * m_ * nn_]).astype(F32)
    return total.reshape(m_, nn_)


def emulate(case, mode, splits=1, fault=None, stats=None, inp=None):
    """float32 model of the launch (and of gemm_slab_reduce_kernel under split-K) -> the output buffer after the call.
    stats (a dict) receives "a_reads" / "b_reads": the operand elements actually fetched (not zero-filled)."""
    assert fault is None or fault in FAULTS
    inp = build(case, mode, splits) if inp is None else inp
    res = _emulate_g2(case, inp, fault, stats) if mode == 2 else _emulate_g1(case, mode, inp, fault, stats)
    out = inp["outbuf"].copy()
    out[inp["out0"]:inp["out0"] + res.size] = res.reshape(-1)
    return out
