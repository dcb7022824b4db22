"""GPU: the detection stage of evaluation against float64 at its edges -- ``yolo_decode_kernel`` (csrc/loss.hip, K8b),
``yolo_select_kernel`` / ``select_scan_kernel`` / ``select_compact_kernel`` (csrc/select.hip, K8c) and the class-wise count /
write kernels (K8e).  The float64 statements and the input builders are oracle/select_stage.py; tests/test_select_stage_cpu.py
holds every case used here to its conditions (no candidate pair near the unify threshold, K and N, vote norm, coverage).

Bars, none taken from the kernels:
* decode, and xyz of a row written alone: ``checks.value_check``, err <= max(4 err_ref, 16 * 2^-24) of the float64 absmax, err_ref
  the error of the NumPy float32 evaluation (``oracle.postprocess.decode``; the host rows of ``postprocess.nms_decoded``);
* xyz of a voted row: |x - x64| <= (16 e_max + K_cluster + 16) * 2^-24 / norm per component (``select_stage.vote_bound``);
* frames, classes, counts, order, and every class-wise row: equal (the class-wise rows bit for bit).
Every check prints its figures (run with -s)."""
import numpy as np
import pytest
import torch

from oracle import postprocess as opost
from oracle import select_stage as S
from oracle.checks import Collect, d64, value_check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------------------ decode
def _decode(ops, logit, geom):
    gaz, gel, a, c, gs, ov = geom
    got = ops.yolo_decode(torch.from_numpy(logit).cuda(), c, (gaz, gel), a, gs, ov)
    ref64, u_raw, v_raw = S.decode64(logit, c, (gaz, gel), a, gs, ov)
    with np.errstate(over="ignore"):
        ref32 = opost.decode(logit, c, (gaz, gel), a, gs, ov)
    assert tuple(got.shape) == ref64.shape == ref32.shape
    return got.cpu().numpy(), ref64, ref32, u_raw, v_raw


DECODE_CASES = [(g, f) for g in S.DECODE_GEOMS for f in S.DECODE_FRAMES] + [(S.DECODE_LARGE[1], S.DECODE_LARGE[0])]


@pytest.mark.parametrize("geom,frames", DECODE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_decode_against_float64(ops, geom, frames):
    """conf and the class scores together, U and V apart (scales 1, 180, 90), against ``decode64`` with the NumPy float32 decode
    as the float32 evaluation: N(0, 2) logits with +-17, +-30, +-88, +-104 and +-inf planted in every channel of the first and
    last anchor of the first and last cell; 1 and 7 frames, and 6554 frames x 160 anchors, past the grid cap of 4096 x 256
    threads (the grid-stride loop).  U within 1e-3 degree of +-180 before the wrap and V within 1e-3 of +-90 before the clamp are
    left out (``branch_keep``), at most 0.1 % of the drawn elements.
    Measured on the MI355X, the worst of the nine cases: conf / class err 1.7e-7 (err_ref 3.0e-8, bar 9.5e-7), U 6.6e-8 of 180
    (err_ref 8.6e-8), V 5.9e-8 of 90 (err_ref 9.1e-8); share left out 7.2e-6 in the large case, 0 elsewhere."""
    gaz, gel, a, c, gs, ov = geom
    logit, planted = S.decode_logits(frames, c, (gaz, gel), a, seed=5 if frames > 7 else frames + c)
    got, ref64, ref32, u_raw, v_raw = _decode(ops, logit, geom)
    keep_u, keep_v = S.branch_keep(u_raw, v_raw, logit.reshape(ref64.shape))
    share, n17, only17 = S.decode_share(keep_u, keep_v, planted, logit.reshape(ref64.shape))
    print("share left out %.2e, planted +-17 left out %d" % (share, n17))
    assert share <= 1e-3 and only17
    t = torch.from_numpy
    col = Collect()
    what = "decode %dx%dx%d C=%d ov=%.2f T=%d" % (gaz, gel, a, c, ov, frames)
    col(value_check, what + " conf+class", t(got[..., :c + 1]), t(ref64[..., :c + 1]), t(ref32[..., :c + 1]))
    col(value_check, what + " U", t(got[..., -2]), t(ref64[..., -2]), t(ref32[..., -2]), keep=t(keep_u))
    col(value_check, what + " V", t(got[..., -1]), t(ref64[..., -1]), t(ref32[..., -1]), keep=t(keep_v))
    col.finish()
    assert got[..., -1].max() <= np.float32(90.0 - 1e-7) and got[..., -1].min() >= -90.0
    assert got[..., -2].max() < 180.0 and got[..., -2].min() >= -180.0
    assert got[..., :c + 1].min() >= 0.0 and got[..., :c + 1].max() <= 1.0


@pytest.mark.parametrize("geom", S.DECODE_GEOMS, ids=lambda v: str(v).replace(" ", ""))
def test_decode_decisions_are_exact_where_they_are_exact(ops, geom):
    """Frame k holds PLANTED[k] in every channel of the first and last anchor of the first and last cell.  From |x| = 30 on tanh
    is exactly +-1 in float32 and float64, every term is exactly representable, and U and V must EQUAL the float64 statement:
    g_overlap 0 gives U = 180 in the last azimuth cell, which wraps to -180, and -180 in the first, which stays; 0.5 gives
    202.5 -> -157.5 and -202.5 -> 157.5; V clamps to float32(90 - 1e-7) and to -90.  conf and the class scores are exactly 1
    and 0 under +-inf.  +-17 saturates in float32 alone: those U and V follow the float32 evaluation to 16 * 2^-24 of the
    scale."""
    gaz, gel, a, c, gs, ov = geom
    logit = S.saturated_logits(c, (gaz, gel), a)
    got, ref64, ref32, u_raw, v_raw = _decode(ops, logit, geom)
    pos = S.plant_positions((gaz, gel), a)
    for k, val in enumerate(S.PLANTED):
        for gi, gj, an in pos:
            g, r64, r32 = got[k, gi, gj, an], ref64[k, gi, gj, an], ref32[k, gi, gj, an]
            if abs(val) >= 30.0:
                assert g[-2] == r64[-2] and g[-1] == r64[-1], (val, gi, gj, an, g[-2:], r64[-2:])
            else:
                assert abs(float(g[-2]) - float(r32[-2])) <= 180 * 16 * S.U24 and abs(float(g[-1]) - float(r32[-1])) <= 90 * 16 * S.U24
            if np.isinf(val):
                want = 1.0 if val > 0 else 0.0
                assert (g[:c + 1] == want).all(), (val, g)
    sat = [k for k, val in enumerate(S.PLANTED) if val >= 30.0]
    neg = [k for k, val in enumerate(S.PLANTED) if val <= -30.0]
    last, first = got[:, gaz - 1, gel - 1, a - 1], got[:, 0, 0, 0]
    assert (last[sat, -1] == np.float32(90.0 - 1e-7)).all() and (first[neg, -1] == -90.0).all()
    if (gaz, gs[0], ov) == (8, 45.0, 0.0):
        assert (last[sat, -2] == -180.0).all() and (first[neg, -2] == -180.0).all()
    if (gaz, gs[0], ov) == (8, 45.0, 0.5):
        assert (last[sat, -2] == -157.5).all() and (first[neg, -2] == 157.5).all()


# --------------------------------------------------------------------------------------------------------- selection
def _select_case(ops, name, dec, info, thresholds=S.THRESHOLDS, modes=S.NMS):
    """One case through ``ops.yolo_select`` for every mode and threshold against ``select64``: frame, class, count and order
    columns, the per-frame counts and the total equal; xyz under the bars.  -> {(nms, threshold): device rows (R, 5)}."""
    from adyolo_amd import postprocess as P
    dev = torch.from_numpy(np.ascontiguousarray(dec)).cuda()
    c, un = info["C"], info.get("unify", 0.5)
    col, out = Collect(), {}
    for th in thresholds:
        for nms in modes:
            what = "%s %s t=%r" % (name, nms, th)
            ref, diag = S.select64(dec, c, th, th, un, nms)
            host = S.flat_rows(P.nms_decoded(dec, c, th, th, un, nms))
            rows, counts = ops.yolo_select(dev, c, th, th, un, nms)
            rows_full, counts_full = ops.yolo_select(dev, c, th, th, un, nms, trim=False)
            got, cnt = d64(rows).numpy(), counts.cpu().numpy()
            assert counts.dtype == torch.int32 and cnt.shape == (dec.shape[0],)
            np.testing.assert_array_equal(cnt, np.bincount(ref[:, 0].astype(np.int64), minlength=dec.shape[0]), err_msg=what)
            assert len(got) == len(ref) == int(cnt.sum()), "%s: %d rows, float64 statement %d" % (what, len(got), len(ref))
            np.testing.assert_array_equal(counts_full.cpu().numpy(), cnt, err_msg=what)
            assert torch.equal(rows_full[:len(got)], rows), what
            S.check_rows(what, got, ref, diag, host, collect=col)
            out[(nms, th)] = got
    col.finish()
    return out


@pytest.mark.parametrize("k,n", S.WORD_EDGES)
def test_chain_at_the_lane_word_edges(ops, k, n):
    """2 frames x 2 classes (one slot empty), K candidates among N anchors on a chain of step 0.3 degree under unify 0.5, ranks
    permuted against the positions: K and N at 64, 65, 128, 1023 and 1024 put the last candidate in the last bit of a lane
    word, alone in a new word, and in the 16th word; conn-merge grows one component per slot over all the words, the greedy
    modes seed across them.
    Measured on the MI355X: voted rows worst err / bound 0.040, rows written alone err 1.4e-7 (err_ref 1.4e-7, bar 9.5e-7)."""
    name = "chain K=%d N=%d" % (k, n)
    dec, info = S.cases()[name]()
    got = _select_case(ops, name, dec, info)
    for th in S.THRESHOLDS:
        assert len(got[("conn-merge", th)]) == 3
        assert k <= 2 or len(got[("soft-merge", th)]) == len(got[("default", th)]) > 3


@pytest.mark.parametrize("k,n", S.WORD_EDGES)
def test_single_candidates_at_the_lane_word_edges(ops, k, n):
    """The same K as one candidate in each of K classes (``_single``, K = 1 in every slot), at scattered anchors of N.
    Measured on the MI355X: err 1.7e-7 (err_ref 1.7e-7, bar 9.5e-7)."""
    name = "singles K=%d N=%d" % (k, n)
    dec, info = S.cases()[name]()
    got = _select_case(ops, name, dec, info)
    assert all(len(r) == k for r in got.values())


@pytest.mark.parametrize("name", ["deep K=200 step 0.8", "deep K=200 step 0.3"])
def test_deep_breadth_first_growth(ops, name):
    """K = 200 at scattered anchors of N = 1024 under unify 1.  Step 0.8: a row reaches its two neighbours only, 124 to 176
    generations of one or two rows through the two frontier lists that alias the sort keys.  Step 0.3: three neighbours on
    either side, 43 to 62 generations with frontiers of up to six rows that come from three or four of the four lane words
    (``growth64``; asserted by tests/test_select_stage_cpu.py).
    Measured on the MI355X: voted rows worst err / bound 0.022, rows written alone err 1.5e-7 (err_ref 1.4e-7, bar 9.5e-7)."""
    dec, info = S.cases()[name]()
    got = _select_case(ops, name, dec, info)
    assert all(len(got[("conn-merge", th)]) == 3 for th in S.THRESHOLDS)
    assert all(g[1] == (2 if "0.8" in name else 6) for g in S.growth64(dec, 2, 0.5, 0.5, info["unify"]))


def test_square_cluster_membership_shows_in_xyz(ops):
    """Four rows at the corners of a 4 degree square under unify 5, confidences 0.58 .. 0.62: conn-merge votes over all four,
    soft-merge over a seed and its two neighbours, and one member more or less moves the float64 vote by more than 100 x the
    bound (tests/test_select_stage_cpu.py), so here the membership is pinned by xyz, not only by the counts.
    Measured on the MI355X: voted rows worst err / bound 0.016, rows written alone err 1.9e-8."""
    dec, info = S.square()
    got = _select_case(ops, "square", dec, info)
    for th in S.THRESHOLDS:
        assert [len(got[(nms, th)]) for nms in S.NMS] == [2, 4, 4]


@pytest.mark.parametrize("k,n,block", S.TIES)
def test_ties_rank_in_anchor_order(ops, k, n, block):
    """Class confidences equal in runs of ``block`` candidates that straddle every 64-row boundary (block = 1024: all equal, at
    the saturated 1.0), directions farther apart than unify: every mode writes one row per candidate in rank order, which inside
    a run is the anchor order -- checked on xyz against the single-row direction of the anchor that must stand there.  Up to
    1024 rows go into one slot: the compaction's stride loop and the slot's last float.
    Measured on the MI355X: voted rows worst err / bound 0.045, rows written alone err 1.3e-7 (err_ref 1.3e-7, bar 9.5e-7)."""
    name = "ties K=%d N=%d block=%d" % (k, n, block)
    dec, info = S.cases()[name]()
    got = _select_case(ops, name, dec, info)
    want = S.xyz64(dec[0, info["order"], -2], dec[0, info["order"], -1])
    cand = np.flatnonzero(dec[0, :, 0] > 0.5)
    every = S.xyz64(dec[0, cand, -2], dec[0, cand, -1])
    for key, rows in got.items():
        assert len(rows) == k, key
        np.testing.assert_array_equal(cand[np.argmax(rows[:, 2:].astype(np.float64) @ every.T, axis=1)], info["order"], err_msg=str(key))
        assert float(np.abs(rows[:, 2:] - want).max()) < 1e-5, key
    for th in S.THRESHOLDS:
        assert len(got[("conn-merge", th)]) == len(got[("soft-merge", th)])


def test_triple_tells_the_three_modes_apart(ops):
    """Rows A, B, C of one class, A-B and B-C within unify, A-C not, in all six rank orders: conn-merge one row; with an end
    ranked first soft-merge votes {first, B} and then {B, other end} -- B was removed and is counted again -- and default
    writes the two ends; with B first every mode writes one row.  Dropping or adding one member moves the float64 vote by more
    than 100 x the bound (tests/test_select_stage_cpu.py), so a vote over another set fails here.
    Measured on the MI355X: voted rows worst err / bound 0.016, rows written alone err 2.2e-8."""
    dec, info = S.triple()
    got = _select_case(ops, "triple", dec, info)
    for th in S.THRESHOLDS:
        for nms in S.NMS:
            np.testing.assert_array_equal(np.bincount(got[(nms, th)][:, 0].astype(np.int64), minlength=6),
                                          [len(e) for e in info["expect"][nms]], err_msg=nms)


def test_rows_at_the_thresholds(ops):
    """Objectness and class confidence at float32(t), one float32 below and one above, t = 0.3 and 0.5, with the threshold a
    Python float, a float32 and a float64 NumPy scalar (``np_f32_threshold``): strict >, and the float64 scalar 0.3 lets the
    rows AT float32(0.3) pass.
    Measured on the MI355X: voted rows worst err / bound 0.028, rows written alone err 9.2e-8 (bar 9.5e-7)."""
    dec, info = S.at_threshold()
    counts = []
    for t in (0.3, np.float32(0.3), np.float64(0.3), 0.5, np.float32(0.5), np.float64(0.5)):
        got = _select_case(ops, "at_threshold %s" % type(t).__name__, dec, info, thresholds=(t,))
        assert len({len(r) for r in got.values()}) == 1
        counts.append(len(got[("default", t)]))
    assert counts == [8, 8, 10, 2, 2, 2], counts


@pytest.mark.parametrize("pattern", S.PATTERNS)
@pytest.mark.parametrize("frames,c,n", S.SCAN_SHAPES)
def test_scan_and_compaction_of_the_adyolo_slots(ops, frames, c, n, pattern):
    """4098 slots (1366 frames x 3 classes: ``select_scan_kernel`` with chunks of 5 slots, a ragged last chunk and threads whose
    chunk is empty, the frame-count loop past 1024 frames, the compaction's grid stride past 4096 slots) and 1025 slots (chunks
    of 2), a slot that is switched on holding 1 + slot % 4 rows: all empty, only the first, only the last, alternating, all full.
    Measured on the MI355X: voted rows worst err / bound 0.045, rows written alone err 1.4e-7 (err_ref 1.4e-7, bar 9.5e-7)."""
    name = "slots %dx%dx%d %s" % (frames, c, n, pattern)
    dec, info = S.slots(frames, c, n, pattern)
    got = _select_case(ops, name, dec, info)
    for rows in got.values():
        assert len(rows) == int(info["counts"].sum())
        slot = (rows[:, 0] * c + rows[:, 1]).astype(np.int64)
        np.testing.assert_array_equal(np.bincount(slot, minlength=frames * c), info["counts"])


# ------------------------------------------------------------------------------------------------ class-wise path (K8e)
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _classwise_equal(ops, rec, c, loss, conf, unify, what):
    """``ops.classwise_select`` on the records against ``postprocess.classwise_select``: counts, frames, classes and the bits
    of xyz.  -> number of rows."""
    from adyolo_amd import postprocess as P
    want = P.classwise_select(rec, loss, conf, unify)
    rows, counts = ops.classwise_select(torch.from_numpy(rec).cuda(), c, loss, conf, unify)
    got, cnt = rows.cpu().numpy(), counts.cpu().numpy()
    frames = rec.shape[0]
    np.testing.assert_array_equal(cnt, [len(want.get(f, ())) for f in range(frames)], err_msg=what)
    assert len(got) == int(cnt.sum()), what
    flat = np.asarray([[fr] + list(r) for fr, rr in want.items() for r in rr], dtype=np.float32).reshape(-1, 5)
    np.testing.assert_array_equal(got[:, :2], flat[:, :2], err_msg=what)
    np.testing.assert_array_equal(_bits(got[:, 2:]), _bits(flat[:, 2:]), err_msg=what)
    return len(got)


@pytest.mark.parametrize("pattern", S.PATTERNS)
@pytest.mark.parametrize("frames,c", [(1, 1), (1023, 1), (1024, 1), (1025, 1), (2047, 1), (2049, 1), (4097, 1), (3000, 13)])
def test_scan_through_the_classwise_path(ops, frames, c, pattern):
    """seddoa and accdoa records give 0 or 1 row per slot: slot counts 1, 1023, 1024, 1025 (the first chunk of 2), 2047, 2049,
    4097 and 3000 x 13 under the five count patterns, bit for bit the rows of the host statement."""
    rec = S.classwise_records(frames, c, pattern, seed=frames + c)
    on = int(S.pattern_mask(frames * c, pattern).sum())
    for loss in ("seddoa", "accdoa"):
        assert _classwise_equal(ops, rec, c, loss, 0.5, None, "%s %dx%d %s" % (loss, frames, c, pattern)) == on
        _classwise_equal(ops, rec, c, loss, 0.3, None, "%s %dx%d %s t=0.3" % (loss, frames, c, pattern))


@pytest.mark.parametrize("conf,unify", [(0.5, 15.0), (1.0, 30.0)])
def test_adpit_every_combination(ops, conf, unify):
    """Hand-built ADPIT records in which each of the 64 combinations of the three track activities (above conf or not) and
    the three pair tests (distance below unify or not) occurs three times, for conf below 1 and conf >= 1 (where the
    reference's second test on the boolean keeps no lone track): bit for bit the rows of the host statement."""
    rec = S.adpit_records(conf, unify, seed=3)
    code = S.adpit_codes(rec, conf, unify)
    assert (np.bincount(code.reshape(-1), minlength=64) == 3).all()
    n = _classwise_equal(ops, rec, 1, "adpit", conf, unify, "adpit conf %.1f" % conf)
    assert n > 0
    wide = np.ascontiguousarray(rec.reshape(-1, 3, 16))                                # the same records as 3 classes
    _classwise_equal(ops, wide, 3, "adpit", conf, unify, "adpit conf %.1f, 3 classes" % conf)
