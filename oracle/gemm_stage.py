"""Oracle (test infrastructure): cases, inputs, float64 references and the checker of the GEMM-family tests (K7, csrc/gemm.hip;
tests/test_gemm_stage_cpu.py pins everything here on the CPU, tests/test_gpu_gemm_stage.py compares the kernels with it).

``plan`` mirrors the host decisions of ``adyolo_gemm`` (klen, effective splits, the fastg bits, the fetch each operand takes,
the epilogue that runs); the GPU module asserts it against ``adyolo_gemm_plan``.

A case is a dict of plain numbers; ``build`` turns it into NumPy buffers.  Every operand is a view into a larger buffer
filled with NaN -- floats before and after it, the ``ld - cols`` gap columns, rows past the last -- so that any read outside
the logical operand that reaches the matrix core shows in the result.  The output is a view into a buffer filled with the
finite sentinel ``SENT``; ``check`` wants every float outside the M x N windows bitwise unchanged and, per element,

    |got - ref| <= (K + S + 4) * u * ( |alpha| * (|A| |B|)[m,n] + |bias[n]| + |C0[m,n]| ),       u = 2^-24,

with float64 references, S the effective number of splits and C0 the old content under ``accumulate``: the any-order summation
bound with one rounding per operation (a term of the sum meets at most K roundings on its way through the K products and
additions, S - 1 more in the slab sum, one each for alpha, the bias and C0; (K + S + 4) u covers gamma_{K+S+2} for K < 2^20).
It needs no margin.

``emulate`` is a float32 NumPy model of the tiled kernel (tile by tile, split by split, fetching through the same index
arithmetic from the same NaN-embedded buffers) with plantable faults: the CPU module shows that ``check`` passes the honest
emulation on every case and catches every fault of ``FAULTS`` on at least one -- but for "no_row_zero_fill", which cannot
change C (a row past M feeds only accumulator rows that are never stored): there the module shows equal bits and that the
emulation's record of its fetches (``stats``) sees the reads."""
import functools
import itertools
import random

import numpy as np

U = 2.0 ** -24
GBM, GBN, GBK = 128, 64, 32
FETCH_LIMIT = (1 << 29) - 64          # floats: an operand of this extent or more takes the general fetch
SENT = np.float32(-777.25)
PRE, POST = 16, 64                    # floats in front of an aligned operand (64 bytes) and behind the last row
F32 = np.float32


def cdiv(a, b):
    return -(-a // b)


def plan(m, n, k, lda, ldb, ta, tb, splits=1, ldc=None, c_ptr=0, bias_ptr=None):
    """The host decisions of ``adyolo_gemm`` and the kernel's choice of epilogue.  c_ptr / bias_ptr: byte addresses (only their
    low four bits matter; bias_ptr None = no bias).  -> dict klen, splits, fastg, last (length of the last K slice), fetch_a,
    fetch_b ("descriptor" / "general"), epilogue ("vector" / "scalar" / "slabs")."""
    splits = max(1, int(splits))
    klen = cdiv(cdiv(k, splits), GBK) * GBK
    eff = cdiv(k, klen)
    ea = (k - 1) * lda + m if ta else (m - 1) * lda + k
    eb = (k - 1) * ldb + n if tb else (n - 1) * ldb + k
    fastg = 3 if (k % GBK == 0 and klen % GBK == 0 and ea < FETCH_LIMIT and eb < FETCH_LIMIT) else 0
    ldc = n if ldc is None else ldc
    if eff > 1:
        epi = "slabs"
    elif (not ta and n % 4 == 0 and ldc % 4 == 0 and c_ptr % 16 == 0 and (bias_ptr is None or bias_ptr % 16 == 0)):
        epi = "vector"
    else:
        epi = "scalar"
    return {"klen": klen, "splits": eff, "fastg": fastg, "last": k - (eff - 1) * klen,
            "fetch_a": "descriptor" if (fastg & 1 and not ta) else "general",
            "fetch_b": "descriptor" if (fastg & 2 and not tb) else "general", "epilogue": epi}


def case_plan(cs):
    """``plan`` of a plain case with the pointers ``build`` gives it (allocations are 16-byte aligned)."""
    oa, ob, obias, oc = cs["offs"]
    return plan(cs["m"], cs["n"], cs["k"], cs["lda"], cs["ldb"], cs["ta"], cs["tb"], cs["splits"], cs["ldc"],
                4 * (PRE + oc), 4 * (PRE + obias) if cs["bias"] else None)


def form_of(cs):
    p = case_plan(cs)
    return (cs["ta"], cs["tb"], p["fetch_a"], p["fetch_b"], p["epilogue"], cs["acc"], cs["bias"])


def feasible_forms():
    """Every (TA, TB, fetch A, fetch B, epilogue, accumulate, bias) the kernel can take.  Left out, each by the kernel's own
    code: a descriptor on a transposed operand (fastA / fastB need a k-major operand); a descriptor on one k-major operand
    with the general fetch on the other k-major one (the host's fastg is 3 or 0); the vector epilogue with a transposed A
    (VEPI = !TA)."""
    out = []
    for ta, tb, fa, fb, epi, acc, bias in itertools.product((False, True), (False, True), ("descriptor", "general"),
                                                            ("descriptor", "general"), ("vector", "scalar", "slabs"),
                                                            (False, True), (False, True)):
        if (ta and fa == "descriptor") or (tb and fb == "descriptor"):
            continue
        if not ta and not tb and fa != fb:
            continue
        if ta and epi == "vector":
            continue
        out.append((ta, tb, fa, fb, epi, acc, bias))
    return out


# ------------------------------------------------------------------------------------------------------------------ cases
def make_case(name, m, n, k, ta, tb, gap_a=0, gap_b=0, ldc_extra=0, splits=1, bias=False, acc=False, offs=(0, 0, 0, 0), seed=0):
    return {"kind": "plain", "name": name, "m": m, "n": n, "k": k, "ta": bool(ta), "tb": bool(tb),
            "lda": (m if ta else k) + gap_a, "ldb": (n if tb else k) + gap_b, "ldc": n + ldc_extra, "splits": splits,
            "bias": bool(bias), "acc": bool(acc), "offs": tuple(offs), "alpha": 1.0, "seed": seed}


def variant(cs, **kw):
    """The same case (same seed, same logical numbers) with other strides / offsets / flags."""
    out = dict(cs)
    for key in ("gap_a", "gap_b"):
        if key in kw:
            ld, cont = ("lda", cs["m"] if cs["ta"] else cs["k"]) if key == "gap_a" else ("ldb", cs["n"] if cs["tb"] else cs["k"])
            out[ld] = cont + kw.pop(key)
    if "ldc_extra" in kw:
        out["ldc"] = cs["n"] + kw.pop("ldc_extra")
    out.update(kw)
    out["name"] = cs["name"] + "/" + ",".join("%s=%s" % kv for kv in sorted(kw.items())) if kw else cs["name"]
    return out


M_VALUES = (4, 31, 32, 33, 128, 129, 260)
N_VALUES = (4, 8, 63, 64, 68, 132)
K_VALUES = (4, 28, 32, 36, 64, 96, 100, 160)
LDC_EXTRA = (0, 4, 1)                 # ldc = N, N + 4, N + 1 (the last forces the scalar epilogue)
SPLITS = (1, 2, 3, 7, 64)
GAPS = (0, 4)                         # lda / ldb: compact, or four NaN columns after every row
TRANS = ((False, False), (False, True), (True, False), (True, True))
_FACTORS = (TRANS, M_VALUES, N_VALUES, K_VALUES, LDC_EXTRA, SPLITS, GAPS)


def _valid(c):
    (ta, tb), m, n = c[0], c[1], c[2]
    return not (ta and m % 4) and not (tb and n % 4)        # the contiguous axis of an operand is a multiple of 4 (K always is)


@functools.lru_cache(maxsize=None)
def pairwise_rows():
    """A pairwise-covering list over (TA TB, M, N, K, ldc, splits, gap): every pair of values of two factors that a valid
    case can hold occurs in one row at least.  Seeded greedy; the CPU module asserts the coverage and the size."""
    rng = random.Random(7)
    nf = len(_FACTORS)
    need = set()
    for i, j in itertools.combinations(range(nf), 2):
        for vi in _FACTORS[i]:
            for vj in _FACTORS[j]:
                if i == 0 and j in (1, 2):
                    (ta, tb) = vi
                    if (j == 1 and ta and vj % 4) or (j == 2 and tb and vj % 4):
                        continue
                need.add((i, vi, j, vj))
    rows = []
    while need:
        i, vi, j, vj = min(need, key=repr)
        best, gain = None, -1
        for _ in range(40):
            c = [rng.choice(f) for f in _FACTORS]
            c[i], c[j] = vi, vj
            if not _valid(c):
                continue
            g = sum(1 for a, b in itertools.combinations(range(nf), 2) if (a, c[a], b, c[b]) in need)
            if g > gain:
                best, gain = tuple(c), g
        assert best is not None
        rows.append(best)
        for a, b in itertools.combinations(range(nf), 2):
            need.discard((a, best[a], b, best[b]))
    return tuple(rows)


def pairwise_cases():
    """Section 1: the pairwise rows, each with and without bias, with and without accumulate."""
    out = []
    for i, ((ta, tb), m, n, k, ldx, s, gap) in enumerate(pairwise_rows()):
        for bias, acc in itertools.product((False, True), (False, True)):
            name = "pw%03d_%s%s_m%d_n%d_k%d_ldc+%d_s%d_gap%d_b%d_a%d" % (i, "FT"[ta], "FT"[tb], m, n, k, ldx, s, gap, bias, acc)
            out.append(make_case(name, m, n, k, ta, tb, gap, gap, ldx, s, bias, acc, seed=1000 + i))
    return out


def form_base(ta, tb, fa, fb, epi):
    """One small shape per (TA, TB, fetch, fetch, epilogue): 36 x 68, K = 64 where an operand goes through a descriptor and
    36 (one whole tile and a tail of 4) where none does; ldc = N + 4 / N + 1 / two splits for vector / scalar / slabs."""
    k = 64 if "descriptor" in (fa, fb) else 36
    return make_case("form_%s%s_%s_%s_%s" % ("FT"[ta], "FT"[tb], fa[:4], fb[:4], epi), 36, 68, k, ta, tb,
                     ldc_extra={"vector": 4, "scalar": 1, "slabs": 4}[epi], splits=2 if epi == "slabs" else 1,
                     seed=2000 + 16 * ta + 8 * tb + 4 * (fa == "general") + 2 * (fb == "general")
                     + ("vector", "scalar", "slabs").index(epi))


def form_cases():
    """Every feasible form once (with the four accumulate / bias combinations)."""
    out, seen = [], set()
    for ta, tb, fa, fb, epi, acc, bias in feasible_forms():
        base = form_base(ta, tb, fa, fb, epi)
        cs = variant(base, acc=acc, bias=bias)
        assert form_of(cs) == (ta, tb, fa, fb, epi, acc, bias), cs["name"]
        if cs["name"] not in seen:
            seen.add(cs["name"])
            out.append(cs)
    return out


def alignment_bases():
    """Section 2: per (TA, TB) one shape whose k-major operands go through descriptors (K = 64) and one general-fetch shape
    (K = 36); bias on, ldc = N + 4, M and N past one tile edge each."""
    out = []
    for ta, tb in TRANS:
        for k in (64, 36):
            out.append(make_case("align_%s%s_k%d" % ("FT"[ta], "FT"[tb], k), 132, 68, k, ta, tb, ldc_extra=4, bias=True,
                                 seed=3000 + 8 * ta + 4 * tb + (k == 36)))
    return out


# float offsets of (A, B, bias, C) inside their allocations: each at 1, 2 and 3 with the others aligned, then all together
ALIGN_OFFSETS = tuple(tuple(o if i == j else 0 for j in range(4)) for i in range(4) for o in (1, 2, 3)) + (
    (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (1, 2, 3, 1))


def batched_case(name, m, n, k, lda, ldb, ldc, ta, tb, outer, inner, oa, ia, ob, ib, oc, ic, alpha=1.0, acc=False, seed=0,
                 bias=False, gpu=True):
    return {"kind": "batched", "name": name, "m": m, "n": n, "k": k, "lda": lda, "ldb": ldb, "ldc": ldc, "ta": bool(ta),
            "tb": bool(tb),
            "outer": outer, "inner": inner, "strides": (oa, ia, ob, ib, oc, ic), "alpha": float(alpha), "acc": bool(acc),
            "bias": bool(bias), "splits": 1, "offs": (0, 0, 0, 0), "seed": seed, "gpu": gpu}


def batched_cases():
    """Section 4.  The two forms of the 1-D Winograd path (``ops.wino1d_conv``: FF, M rows x N cout x K cin; ``ops.wino1d_wgrad``:
    TT, M cout x N cin x K rows; outer 6, inner 1) and a general one: outer 3, inner 2, A shared over inner (iA = 0),
    oC > M ldc (sentinel gaps between the problems), alpha = 0.125, accumulate."""
    out = []
    rows, cin, cout = 40, 64, 68
    out.append(batched_case("wino1d_conv_FF", rows, cout, cin, cin, cin, cout, False, False, 6, 1,
                            rows * cin, 0, cout * cin, 0, rows * cout, 0, seed=4000))
    for r in (5, 20, 33):
        out.append(batched_case("wino1d_wgrad_TT_rows%d" % r, cout, cin, r, cout, cin, cin, True, True, 6, 1,
                                r * cout, 0, r * cin, 0, cout * cin, 0, seed=4001 + r))
    m, n, k, lda, ldb, ldc = 33, 68, 36, 40, 36, 72
    out.append(batched_case("general_o3_i2", m, n, k, lda, ldb, ldc, False, False, 3, 2,
                            m * lda + 8, 0, 2 * (n * ldb + 4), n * ldb + 4, 2 * (m * ldc + 12) + 4, m * ldc + 12,
                            alpha=0.125, acc=True, seed=4100))
    # CPU only: alpha together with a bias, which the kernel's epilogue handles (v = acc * alpha + bias) and no entry point passes
    out.append(batched_case("alpha_and_bias_cpu_only", 8, 8, 36, 36, 36, 8, False, False, 2, 1, 8 * 36, 0, 8 * 36, 0, 64, 0,
                            alpha=0.125, bias=True, seed=4200, gpu=False))
    return out


def all_cases(gpu_only=False):
    out = pairwise_cases() + form_cases()
    out += [variant(b, offs=o) for b in alignment_bases() for o in ((0, 0, 0, 0),) + ALIGN_OFFSETS]
    out += [c for c in batched_cases() if c["gpu"] or not gpu_only]
    return out


# ----------------------------------------------------------------------------------------------------------------- inputs
def _embed(mat, ld, first, fill):
    """mat [rows][cols] at float offset ``first`` of a new buffer filled with ``fill``, row stride ld; two more rows and POST
    floats of fill behind it."""
    rows, cols = mat.shape
    buf = np.full(first + (rows + 2) * ld + POST, fill, dtype=F32)
    _window(buf, first, rows, cols, ld)[...] = mat
    return buf


def _window(buf, first, rows, cols, ld):
    assert first >= 0 and first + (rows - 1) * ld + cols <= buf.size
    return np.lib.stride_tricks.as_strided(buf[first:], (rows, cols), (buf.itemsize * ld, buf.itemsize))


def problems(cs):
    """-> [(a0, b0, c0)]: float offsets of every problem's operands in their buffers."""
    oa_, ob_, _, oc_ = cs["offs"]
    if cs["kind"] == "plain":
        return [(PRE + oa_, PRE + ob_, PRE + oc_)]
    oa, ia, ob, ib, oc, ic = cs["strides"]
    return [(PRE + zo * oa + zi * ia, PRE + zo * ob + zi * ib, PRE + zo * oc + zi * ic)
            for zo in range(cs["outer"]) for zi in range(cs["inner"])]


def build(cs):
    """-> dict: abuf, bbuf, biasbuf (or None), cbuf (float32 buffers: NaN around the operands, SENT around the output; under
    accumulate the windows hold C0), bias0 (float offset of the bias), probs [(a0, b0, c0)], A / B / C0 (per problem: the
    logical stored matrices, float32), ref / bound (per problem, float64)."""
    rng = np.random.default_rng(cs["seed"])
    m, n, k, ta, tb = cs["m"], cs["n"], cs["k"], cs["ta"], cs["tb"]
    ashape, bshape = ((k, m) if ta else (m, k)), ((k, n) if tb else (n, k))
    probs = problems(cs)
    amats, bmats = {}, {}
    for a0, b0, _ in probs:                                     # an operand shared by several problems is one matrix
        if a0 not in amats:
            amats[a0] = rng.standard_normal(ashape).astype(F32)
        if b0 not in bmats:
            bmats[b0] = rng.standard_normal(bshape).astype(F32)
    asize = max(amats) + (ashape[0] + 2) * cs["lda"] + POST
    bsize = max(bmats) + (bshape[0] + 2) * cs["ldb"] + POST
    abuf, bbuf = np.full(asize, np.nan, dtype=F32), np.full(bsize, np.nan, dtype=F32)
    for a0, mat in amats.items():
        _window(abuf, a0, ashape[0], ashape[1], cs["lda"])[...] = mat
    for b0, mat in bmats.items():
        _window(bbuf, b0, bshape[0], bshape[1], cs["ldb"])[...] = mat
    bias, biasbuf, bias0 = None, None, PRE + cs["offs"][2]
    if cs["bias"]:
        bias = rng.standard_normal(n).astype(F32)
        biasbuf = np.full(bias0 + n + POST, np.nan, dtype=F32)
        biasbuf[bias0:bias0 + n] = bias
    cbuf = np.full(max(c for _, _, c in probs) + (m + 2) * cs["ldc"] + POST, SENT, dtype=F32)
    c0s, refs, bounds = [], [], []
    eff = plan(m, n, k, cs["lda"], cs["ldb"], ta, tb, cs["splits"])["splits"]
    for a0, b0, c0 in probs:
        a64 = (amats[a0].T if ta else amats[a0]).astype(np.float64)
        b64 = (bmats[b0] if tb else bmats[b0].T).astype(np.float64)             # [k][n]
        c_old = rng.standard_normal((m, n)).astype(F32) if cs["acc"] else np.zeros((m, n), dtype=F32)
        if cs["acc"]:
            _window(cbuf, c0, m, n, cs["ldc"])[...] = c_old
        ref = cs["alpha"] * (a64 @ b64) + c_old.astype(np.float64)
        mag = abs(cs["alpha"]) * (np.abs(a64) @ np.abs(b64)) + np.abs(c_old.astype(np.float64))
        if bias is not None:
            ref = ref + bias.astype(np.float64)[None, :]
            mag = mag + np.abs(bias.astype(np.float64))[None, :]
        c0s.append(c_old)
        refs.append(ref)
        bounds.append((k + eff + 4) * U * mag)
    return {"abuf": abuf, "bbuf": bbuf, "biasbuf": biasbuf, "bias0": bias0, "cbuf": cbuf, "probs": probs, "A": amats, "B": bmats,
            "C0": c0s, "ref": refs, "bound": bounds}


def check(cs, inp, out_buffer):
    """out_buffer: the whole output buffer after the call (float32, the size of inp["cbuf"]).  Every float outside the windows
    bitwise unchanged, every element of a window within its bound.  -> worst err / bound."""
    out = np.asarray(out_buffer, dtype=F32).reshape(-1)
    assert out.shape == inp["cbuf"].shape, "%s: output buffer of %d floats, expected %d" % (
        cs["name"], out.size, inp["cbuf"].size)
    m, n, ldc = cs["m"], cs["n"], cs["ldc"]
    inside = np.zeros(out.size, dtype=bool)
    for _, _, c0 in inp["probs"]:
        _window(inside, c0, m, n, ldc)[...] = True
    changed = (out.view(np.int32) != inp["cbuf"].view(np.int32)) & ~inside
    assert not changed.any(), "%s: %d floats outside the output window changed (first at float offset %d)" % (
        cs["name"], int(changed.sum()), int(np.argmax(changed)))
    worst = 0.0
    for (_, _, c0), ref, bound in zip(inp["probs"], inp["ref"], inp["bound"]):
        got = _window(out, c0, m, n, ldc).astype(np.float64)
        assert np.isfinite(got).all(), "%s: %d results are not finite" % (cs["name"], int((~np.isfinite(got)).sum()))
        err = np.abs(got - ref)
        ratio = float((err / bound).max())
        assert (err <= bound).all(), "%s: %d of %d elements over the bound, worst err / bound %.3f (err %.3e)" % (
            cs["name"], int((err > bound).sum()), err.size, ratio, float(err.max()))
        worst = max(worst, ratio)
    return worst


# -------------------------------------------------------------------------------------------------------------- emulation
FAULTS = ("drop_last_tile", "no_row_zero_fill", "no_ktail_zero_fill", "bias_per_split", "alpha_on_bias", "ignore_accumulate",
          "column_past_n", "next_problem_offsets")


def _stage(buf, first, ld, trans, r0, rows_valid, tile_rows, k0, kend, fault, stats):
    """One operand tile [tile_rows][GBK] as the kernel stages it: element (r, kk) from buf[first + ...] where the row is below
    rows_valid and k below kend, zero elsewhere.  The faults drop one of the two conditions: the read then goes wherever the
    index arithmetic points (clipped to the buffer, whose end is NaN).  stats["outside_reads"] counts the elements fetched
    from outside the operand's rows and K slice."""
    r = r0 + np.arange(tile_rows)[:, None]
    kk = k0 + np.arange(GBK)[None, :]
    idx = first + (kk * ld + r if trans else r * ld + kk)
    ok_r = (r < rows_valid) | (fault == "no_row_zero_fill")
    ok_k = (kk < kend) | (fault == "no_ktail_zero_fill")
    vals = buf[np.clip(idx, 0, buf.size - 1)]
    if stats is not None:
        stats["outside_reads"] = stats.get("outside_reads", 0) + int((ok_r & ok_k & ((r >= rows_valid) | (kk >= kend))).sum())
    return np.where(ok_r & ok_k, vals, F32(0)).astype(F32)


def emulate(cs, inp, fault=None, stats=None):
    """float32 model of gemm_kernel (+ gemm_slab_reduce_kernel): -> the output buffer after the call.  stats (a dict):
    receives "outside_reads", the operand elements fetched from outside the logical operand."""
    assert fault is None or fault in FAULTS
    m, n, k, ta, tb, lda, ldb, ldc = cs["m"], cs["n"], cs["k"], cs["ta"], cs["tb"], cs["lda"], cs["ldb"], cs["ldc"]
    p = plan(m, n, k, lda, ldb, ta, tb, cs["splits"])
    klen, splits = p["klen"], p["splits"]
    alpha = F32(cs["alpha"])
    out = inp["cbuf"].copy()
    bias = None if inp["biasbuf"] is None else inp["biasbuf"][inp["bias0"]:inp["bias0"] + n + 1]
    probs = inp["probs"]
    mp, np_ = cdiv(m, GBM) * GBM, cdiv(n, GBN) * GBN
    for z, (a0, b0, c0) in enumerate(probs):
        if fault == "next_problem_offsets" and z + 1 < len(probs):
            a0, b0 = probs[z + 1][0], probs[z + 1][1]
        slabs = []
        for s in range(splits):
            kbeg, kend = s * klen, min(k, (s + 1) * klen)
            acc = np.zeros((mp, np_), dtype=F32)
            tiles = list(range(kbeg, kend, GBK))
            if fault == "drop_last_tile" and s == splits - 1:
                tiles = tiles[:-1]
            for k0 in tiles:
                at = _stage(inp["abuf"], a0, lda, ta, 0, m, mp, k0, kend, fault, stats)
                bt = _stage(inp["bbuf"], b0, ldb, tb, 0, n, np_, k0, kend, fault, stats)
                acc = (acc + at @ bt.T).astype(F32)
            slabs.append(acc)
        ncol = n + 1 if fault == "column_past_n" else n
        win = _window(out, c0, m, ncol, ldc)
        old = win.copy()
        if splits > 1:
            v = np.zeros((mp, np_), dtype=F32)
            for i, sl in enumerate(slabs):
                v = (v + sl).astype(F32)
                if bias is not None and fault == "bias_per_split" and i > 0:
                    v[:, :n] = v[:, :n] + bias[None, :n]
        else:
            v = (slabs[0] * alpha).astype(F32)
        v = np.concatenate([v, np.zeros((mp, 1), dtype=F32)], axis=1)[:m, :ncol]       # (column N of a full tile: zero-filled B)
        if bias is not None:
            bb = np.nan_to_num(bias[None, :ncol], nan=0.0).astype(F32)
            v = (v + (bb * alpha if fault == "alpha_on_bias" else bb)).astype(F32)
        if cs["acc"] and fault != "ignore_accumulate":
            v = (v + old).astype(F32)
        win[...] = v
    return out


# ----------------------------------------------------------------------------------------------------------------- colsum
COLSUM_R = (1, 3, 4, 5, 63, 64, 65, 129, 65601)
COLSUM_C = (1, 5, 63, 64, 65, 100)


def colsum_rows_per_block(r):
    """Rows one workgroup of colsum_partial_kernel sums (adyolo_colsum: at most 1024 workgroups of at least 64 rows)."""
    nblk = min(1024, cdiv(r, 64))
    return cdiv(r, nblk)


def colsum_cases():
    return [(r, c) for r in COLSUM_R for c in COLSUM_C]


def colsum_inputs(r, c, gap=3, seed=51):
    """a [R][C] float32 as a view (row stride C + gap) of a NaN-filled buffer, old out [C].  -> buf, first, ld, a, old."""
    rng = np.random.default_rng(seed + 7 * r + c)
    a = rng.standard_normal((r, c)).astype(F32)
    ld = c + gap
    buf = _embed(a, ld, 5, np.nan)
    return buf, 5, ld, a, rng.standard_normal(c).astype(F32)


def colsum_bound(a):
    """(ceil(rows_per_block / 4) + 5) u sum_r |a[r, c]|: a lane adds every fourth row of its block, three additions join the four
    lanes, the blocks are summed in double and rounded once."""
    r = a.shape[0]
    return (cdiv(colsum_rows_per_block(r), 4) + 5) * U * np.abs(a.astype(np.float64)).sum(axis=0)


# ----------------------------------------------------------------------------------------------------------------- linear
LINEAR_N = (13, 39, 117, 40)
LINEAR_RK = tuple((r, k) for r in (70, 129) for k in (64, 256))


def linear_inputs(r, k, n, seed=61):
    rng = np.random.default_rng(seed + r + k + n)
    return {"x": rng.standard_normal((r, k)).astype(F32), "w": (rng.standard_normal((n, k)) / np.sqrt(k)).astype(F32),
            "b": rng.standard_normal(n).astype(F32), "dy": rng.standard_normal((r, n)).astype(F32)}


def linear_reference(li, splits_dw=1):
    """float64 y, dx, dw, db and their bounds: the bound of ``check`` with the contraction lengths K, n and R (the zeros that
    pad n to a multiple of 4 add nothing to a sum, so dx keeps the bound of n terms)."""
    x, w, b, dy = (li[key].astype(np.float64) for key in ("x", "w", "b", "dy"))
    r, k = x.shape
    n = w.shape[0]
    ax, aw, ady = np.abs(x), np.abs(w), np.abs(dy)
    return {"y": (x @ w.T + b, (k + 1 + 4) * U * (ax @ aw.T + np.abs(b))),
            "dx": (dy @ w, (n + 1 + 4) * U * (ady @ aw)),
            "dw": (dy.T @ x, (r + splits_dw + 4) * U * (ady.T @ ax)),
            "db": (dy.sum(axis=0), colsum_bound(li["dy"]))}
