"""GPU: the device data path at batch scale -- every one-workgroup scan past 1024 elements (a chunk of more than one element a
thread, the carry between threads, partial and empty chunks) and the capped grids, on the cases tests/test_pipeline_scale_cpu.py
builds and pins; every comparison against the project's host definition of the stage, bit for bit (the SELD scorer by the rule
of tests/test_gpu_seld_score.py).  Batch 16 x 20 s chunks (3200 frames, 3200 / 6400 label lanes) is what the default run uses.

Sizes run (the whole module: 55 tests, 10.0 s wall on one MI355X; scan chunk = ceil(scanned size / 1024)):
  AD-YOLO labels   (B, max_events) (3, 341) (4, 256) (5, 205) (3, 683) (16, 200) x plain / mates / yaw / mates + yaw: 1023 to 3200
                   lanes, 2046 to 6400 with mates (chunk 1 to 7); rows grid: cap 266 240 and 16 x 16 385 lanes (260 / 257 blocks,
                   4 trips), cap 1 052 672 and 16 x 65 537 lanes (the 1024-block cap, 5 trips; scan chunk 1025)
  class-wise       600 + 530 events in one 8-frame tile (cache of 512), T' 9; C = 256, T' 9, B 2; C = 257 refused; 3 formats x
                   plain / mates
  TTA pool         1025 and 2049 frames x 2 classes x 2 views, P = 4 (collect chunk 2, 3; merge chunk 3, 5)
  tracking         (clips, T', C) (5, 205, 2) (1, 2049, 1) (16, 200, 3) (257, 256, 1): chunk 2, 3, 4, 65; 65 792 frames wrap the
                   65 536-block emit grid; track_run: 1100 run frames in two segments + hold, then 200 with the carry
  SELD scoring     5 x 205, 16 x 200 and 3 x 360 frames (chunk 2, 4, 2), the last also as one run of three segments
  CSV bytes        1025, 2049, 2050, 3200 frames x 0-3 rows, 7 files (chunk 2, 3, 3, 4); 1100 x 240 rows = 1032 tiles (chunk 2)"""
import numpy as np
import pytest
import torch

import test_pipeline_scale_cpu as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OVERFLOW, BAD_ITEM, BAD_CLASS = 1, 2, 4                        # ops.CORPUS_STATUS


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------ 1. AD-YOLO labels
def _yolo_run(ops, case, mix, yaw, cap, items=None, mates=None):
    """One call: the workspace -77, the target 7.0, count -7; guard words behind the workspace and the target must stay.
    -> (target on the host, count, status)"""
    from adyolo_amd.augmentations import COMBINATIONS
    from adyolo_amd.datasets import YoloLabelEncoder
    enc = YoloLabelEncoder()
    bounds = torch.from_numpy(np.concatenate([enc.az_lb, enc.az_ub, enc.el_lb, enc.el_ub]).astype(np.float64)).to(DEV)
    items = case["items"] if items is None else items
    mates = case["mates"] if mates is None else mates
    b, me = case["B"], case["max_events"]
    words = ops.corpus_labels_workspace_words(b, me, mix=mix)
    assert words == b * me * (2 if mix else 1)
    ws = torch.full((words + 16,), -77, dtype=torch.int32, device=DEV)
    buf = torch.full((cap * 7 + 64,), 7.0, device=DEV)
    target = buf[:cap * 7].view(cap, 7)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.corpus_yolo_labels(case["events"].to(DEV), items.to(DEV), me, case["t"], bounds, (len(enc.az_lb), len(enc.el_lb)),
                           ops.corpus_rot_table(COMBINATIONS), ws, target, count, status, mates=mates.to(DEV) if mix else None,
                           yaw=yaw)
    torch.cuda.synchronize()
    assert bool((buf[cap * 7:] == 7.0).all()) and bool((ws[words:] == -77).all())
    return target.cpu(), int(count.item()), int(status.item())


def _yolo_check(got, want, cap, status=0):
    target, count, st = got
    m = want.shape[0]
    assert st == status and count == m, (st, count, m)
    k = min(m, cap)
    assert torch.equal(_bits(target[:k]), _bits(want[:k]))
    assert bool((target[k:, 0] == -1).all()) and not bool(target[k:, 1:].any())      # the b = -1 tail, exact
    assert not bool((_bits(target[k:, 1:]) != 0).any())                              # (+0.0, not -0.0)


@pytest.mark.parametrize("variant", cases.YOLO_VARIANTS, ids=["plain", "mates", "yaw", "mates-yaw"])
@pytest.mark.parametrize("size", cases.YOLO_SIZES, ids=lambda s: "%dx%d" % s)
def test_yolo_labels_at_scale(ops, size, variant):
    mix, yaw = variant
    case = cases.yolo_case(*size)
    want = cases.yolo_reference(case, mix, yaw)
    total = want.shape[0]
    print("lanes %d, chunk %d, rows %d" % (size[0] * size[1] * (2 if mix else 1), cases.chunk_of(size[0] * size[1] * (2 if mix else 1)),
                                           total))
    _yolo_check(_yolo_run(ops, case, mix, yaw, total + 257), want, total + 257)
    # the capacity one below, at and one above the total: the overflow bit for the first only, the true total in all three
    for cap in (total - 1, total, total + 1):
        _yolo_check(_yolo_run(ops, case, mix, yaw, cap), want, cap, status=OVERFLOW if cap < total else 0)
    # one bad item (more events than max_events) whose lanes lie outside thread 0's chunk: no rows for it, the others unchanged
    b = cases.yolo_bad_item(case, mix)
    items = case["items"].clone()
    items[b, 3] = case["max_events"] + 1
    less = cases.yolo_reference(case, mix, yaw, skip={b})
    _yolo_check(_yolo_run(ops, case, mix, yaw, total + 257, items=items), less, total + 257, status=BAD_ITEM)
    if mix:                                                       # the same through the mate's row
        j = b if case["labels"][b][1] is not None else b - 1
        mates = case["mates"].clone()
        mates[j, 3] = case["max_events"] + 1
        less = cases.yolo_reference(case, mix, yaw, skip={j})
        _yolo_check(_yolo_run(ops, case, mix, yaw, total + 257, mates=mates), less, total + 257, status=BAD_ITEM)


def test_yolo_rows_fill_wraps_the_grid(ops):
    """The six-event chunks of tests/test_gpu_time_mix.py into a capacity past the rows kernel's largest grid (262 144
    threads), and past four times that, where the 1024-block cap is reached: the b = -1 fill loops."""
    import test_gpu_time_mix as tm
    events, rows = tm._event_table()
    pairs = tm.BATCHES[1]
    items, mates = tm._label_rows(pairs, rows)
    want = tm._yolo_want(pairs, 20)
    for cap in (cases.ROWS_WRAP_CAP, cases.ROWS_CAPPED_CAP):
        got = tm._yolo_run(ops, events, items, mates, 20, cap)
        _yolo_check(got, want, cap)


@pytest.mark.parametrize("max_events", [cases.ROWS_WRAP_EVENTS, cases.ROWS_CAPPED_EVENTS])
def test_yolo_lane_loop_wraps_the_grid(ops, max_events):
    case = cases.yolo_wide_case(max_events)
    want = cases.yolo_reference(case, False, False)
    _yolo_check(_yolo_run(ops, case, False, False, 256), want, 256)
    mates = case["mates"].clone()                                 # the mates form: item 15 takes item 14's row as its mate
    mates[15] = case["items"][14]
    mates[15, 6] = cases._gain_word(0.5)
    both = dict(case, mates=mates, labels=case["labels"][:15] + [(case["labels"][15][0], case["labels"][14][0])])
    want = cases.yolo_reference(both, True, False)
    assert want.shape[0] > cases.yolo_reference(case, True, False).shape[0]
    _yolo_check(_yolo_run(ops, both, True, False, 256), want, 256)


# ------------------------------------------------------------------------------------------------------ 2. class-wise labels
def _cw_run(ops, case, loss, nb_classes, t, max_events, mix, events=None):
    """One call: the target 7.0 with guard words behind it, every element written.  -> (target on the host, status)"""
    from adyolo_amd.corpus import xyz_table
    events = case["events"] if events is None else events
    xyz = torch.from_numpy(xyz_table(events[:, 2].numpy(), events[:, 3].numpy())).to(DEV)
    shape = ops.corpus_classwise_shape(loss, case["items"].shape[0], t, nb_classes)
    n = int(np.prod(shape))
    buf = torch.full((n + 97,), 7.0, device=DEV)
    target = buf[:n].view(shape)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.corpus_classwise_labels(events.to(DEV), case["items"].to(DEV), xyz, max_events, t, nb_classes, loss, target, status,
                                mates=case["mates"].to(DEV) if mix else None)
    torch.cuda.synchronize()
    assert bool((buf[n:] == 7.0).all())
    return target.cpu(), int(status.item())


@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mates"])
@pytest.mark.parametrize("loss", cases.CW_LOSSES)
def test_classwise_event_cache(ops, loss, mix):
    """600 (and with the mate 530 more) events in one tile of 8 label frames: the classes past the first 512 of a source come
    from memory, the first three of a class and its last event on both sides of that line."""
    case = cases.classwise_cache_case()
    want = cases.classwise_reference(case, loss, cases.CW_C, cases.CW_T, mix)
    target, status = _cw_run(ops, case, loss, cases.CW_C, cases.CW_T, cases.CW_MAX_EVENTS, mix)
    assert status == 0
    for j, w in enumerate(want):
        assert torch.equal(_bits(target[j]), _bits(w)), (loss, mix, j)
    # an event past position 512 with a class outside [0, C): dropped, the bad-class bit
    f, i = 7, cases.CW_BAD_AT - sum(cases.CW_TILE_ITEM[:7])
    want = cases.classwise_reference(case, loss, cases.CW_C, cases.CW_T, mix, drop=(0, 0, f, i))
    for cls in (cases.CW_C, -1):
        changed = case["events"].clone()
        changed[int(case["items"][0, 2]) + cases.CW_BAD_AT, 1] = cls
        target, status = _cw_run(ops, case, loss, cases.CW_C, cases.CW_T, cases.CW_MAX_EVENTS, mix, events=changed)
        assert status == BAD_CLASS
        for j, w in enumerate(want):
            assert torch.equal(_bits(target[j]), _bits(w)), (loss, mix, cls, j)


@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mates"])
@pytest.mark.parametrize("loss", cases.CW_LOSSES)
def test_classwise_most_classes(ops, loss, mix):
    from adyolo_amd._lib import AdyoloHipError
    case = cases.classwise_wide_case()
    C = cases.CW_MAX_CLASSES
    want = cases.classwise_reference(case, loss, C, cases.CW_T, mix)
    target, status = _cw_run(ops, case, loss, C, cases.CW_T, cases.CW_WIDE_MAX_EVENTS, mix)
    assert status == 0
    for j, w in enumerate(want):
        assert torch.equal(_bits(target[j]), _bits(w)), (loss, mix, j)
    # one class more is refused before any launch: the target and the status keep their fill
    from adyolo_amd.corpus import xyz_table
    xyz = torch.from_numpy(xyz_table(case["events"][:, 2].numpy(), case["events"][:, 3].numpy())).to(DEV)
    fill = torch.full(ops.corpus_classwise_shape(loss, 2, cases.CW_T, C + 1), 7.0, device=DEV)
    st = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(AdyoloHipError, match="at most %d" % C) as err:
        ops.corpus_classwise_labels(case["events"].to(DEV), case["items"].to(DEV), xyz, cases.CW_WIDE_MAX_EVENTS, cases.CW_T, C + 1,
                                    loss, fill, st, mates=case["mates"].to(DEV) if mix else None)
    assert "rc=-2" in str(err.value)                              # ADYOLO_ENOSUP
    torch.cuda.synchronize()
    assert bool((fill == 7.0).all()) and int(st.item()) == -7


# ------------------------------------------------------------------------------------------------------------ 3. TTA pool
def _tta_merge(ops, per_view, min_views, pad_rows):
    """``tta_collect`` of both views and ``tta_merge``; the pool NaN, the counts -7, the workspace NaN, guard words behind the
    pool and the merged rows (``tta_buffers`` sizes them exactly: the guards sit in buffers of the test's own)."""
    from adyolo_amd.augmentations import view_matrix
    from adyolo_amd.postprocess import tta_cos
    frames = len(per_view[0][1])
    buf = ops.tta_buffers(DEV, len(cases.TTA_VIEWS), frames, cases.TTA_CLASSES, cases.TTA_POOL, min_views)
    guarded = {}
    for key, fill in (("pool", float("nan")), ("pool_counts", -7), ("rows", float("nan")), ("counts", -7), ("ws", float("nan"))):
        t = buf[key]
        whole = torch.full((t.numel() + 64,), fill, dtype=t.dtype, device=DEV)
        guarded[key] = (whole, t.numel(), fill)
        buf[key] = whole[:t.numel()].view(t.shape)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k, (rows, counts) in enumerate(per_view):
        padded = np.concatenate([rows, np.full((pad_rows if k == 0 else 5, 5), 9.0, dtype=np.float32)])
        ops.tta_collect(torch.from_numpy(padded).to(DEV), torch.from_numpy(counts).to(DEV), k, view_matrix(cases.TTA_VIEWS[k]),
                        cases.TTA_CLASSES, buf["pool"], buf["pool_counts"], status, buf["ws"])
    rows, counts = ops.tta_merge(buf["pool"], buf["pool_counts"], cases.TTA_CLASSES, tta_cos(cases.TTA_UNIFY), min_views, status,
                                 buf["ws"], buf["rows"], buf["counts"])
    torch.cuda.synchronize()
    for key, (whole, n, fill) in guarded.items():
        tail = whole[n:]
        assert bool(torch.isnan(tail).all() if fill != fill else (tail == fill).all()), key
    assert int(buf["counts"][frames]) == rows.shape[0]
    return rows.cpu().numpy(), counts.cpu().numpy(), int(status.cpu()[0])


@pytest.mark.parametrize("frames", cases.TTA_FRAMES)
def test_tta_pool_at_scale(ops, frames):
    from adyolo_amd.postprocess import TTA_BAD_ROWS, TTA_ROWS_OVERFLOW, merge_view_rows
    per_view, bad, short = cases.tta_case(frames)
    for min_views in (1, 2):
        for views, ref, pad, bits in ((per_view, per_view, 5, 0), (bad, short, 0, TTA_BAD_ROWS)):
            (want_rows, want_counts), want_status = merge_view_rows(ref, cases.TTA_VIEWS, cases.TTA_UNIFY, min_views,
                                                                    max_rows_per_frame=cases.TTA_POOL)
            rows, counts, status = _tta_merge(ops, views, min_views, pad)
            print("frames %d, min_views %d: %d rows, status %d" % (frames, min_views, len(want_rows), status))
            assert status == want_status | bits and want_status == TTA_ROWS_OVERFLOW
            assert np.array_equal(counts, want_counts)
            assert rows.shape == want_rows.shape and np.array_equal(rows.view(np.int32), want_rows.view(np.int32))


# ------------------------------------------------------------------------------------------------------------- 4. tracking
def _opts(corner):
    return {"gate_deg": cases.TRACK_GATE, "max_gap": corner[0], "min_len": corner[1], "smooth": corner[2]}


def _track(ops, rows, counts, n_clips, C, opts, junk):
    """``ops.track_rows``: the workspace and rows NaN, ids and counts -7, ``junk`` rows of 9.0 behind the counted ones, guard
    words behind every buffer of ``track_buffers``."""
    frames = len(counts)
    buf = ops.track_buffers(DEV, frames, C)
    guarded = {}
    for key, fill in (("ws", float("nan")), ("rows", float("nan")), ("ids", -7), ("counts", -7)):
        t = buf[key]
        whole = torch.full((t.numel() + 64,), fill, dtype=t.dtype, device=DEV)
        guarded[key] = (whole, t.numel(), fill)
        buf[key] = whole[:t.numel()].view(t.shape)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    padded = np.concatenate([rows.reshape(-1, 5), np.full((junk, 5), 9.0, dtype=np.float32)])
    got = ops.track_rows(torch.from_numpy(padded).to(DEV), torch.from_numpy(counts).to(DEV), n_clips, C, opts, buf=buf,
                         status=status)
    torch.cuda.synchronize()
    for key, (whole, n, fill) in guarded.items():
        tail = whole[n:]
        assert bool(torch.isnan(tail).all() if fill != fill else (tail == fill).all()), key
    assert int(buf["counts"][frames]) == got[0].shape[0] == got[2].shape[0]
    return got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy(), int(status.cpu()[0])


def _same_tracks(got, want):
    (want_rows, want_counts), want_ids, want_status = want
    rows, counts, ids, status = got
    assert status == want_status
    assert np.array_equal(counts, want_counts)
    assert rows.shape == want_rows.shape and np.array_equal(rows.view(np.int32), want_rows.view(np.int32))
    assert np.array_equal(ids, want_ids)


@pytest.mark.parametrize("corner", cases.TRACK_CORNERS, ids=["identity", "defaults"])
@pytest.mark.parametrize("shape", cases.TRACK_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_track_rows_at_scale(ops, shape, corner):
    n_clips, T, C = shape
    case = cases.track_case(shape)
    want = cases.track_want(shape, corner)
    print("clips %d, T' %d, C %d, corner %s: %d rows in, %d out, status %d" % (n_clips, T, C, corner, len(case["rows"]),
                                                                               len(want[0][0]), want[2]))
    _same_tracks(_track(ops, case["rows"], case["counts"], n_clips, C, _opts(corner), junk=7), want)
    # a negative count beyond frame 1024 (junk behind the rows: a frame that starts early must not reach it), and a last
    # frame that runs past the rows (nothing behind them: nothing may be read there)
    for kind, junk in (("neg", 7), ("past", 0)):
        _same_tracks(_track(ops, case["rows"], case["bad"][kind][0], n_clips, C, _opts(corner), junk=junk),
                     cases.track_want(shape, corner, bad=kind))


@pytest.mark.parametrize("corner", cases.TRACK_CORNERS, ids=["identity", "defaults"])
def test_track_run_at_scale(ops, corner):
    from test_gpu_track_windows import device_step
    from test_track_windows_cpu import host_step, run_plan
    rows, counts, start, parts, plan, hold = cases.track_run_case(corner)
    want = run_plan(host_step(cases.TRACK_RUN_C, *corner, hold), rows, counts, plan, cases.TRACK_RUN_BOUNDS)
    got = run_plan(device_step(ops, cases.TRACK_RUN_C, _opts(corner), hold), rows, counts, plan, cases.TRACK_RUN_BOUNDS)
    assert len(got) == len(want) == 2
    for p, (((g_rows, g_counts), g_ids, g_status), ((w_rows, w_counts), w_ids, w_status)) in enumerate(zip(got, want)):
        print("pass %d: %d frames emitted, %d rows, status %d" % (p, len(w_counts), len(w_rows), w_status))
        assert g_status == w_status and np.array_equal(g_counts, w_counts) and np.array_equal(g_ids, w_ids)
        assert len(w_rows) > 0 and g_rows.tobytes() == w_rows.tobytes()


# ------------------------------------------------------------------------------------------------------------- 6. CSV bytes
@pytest.mark.parametrize("frames", cases.CSV_FRAMES)
def test_csv_bytes_at_scale(ops, frames):
    from adyolo_amd.postprocess import CSV_BAD_COUNTS
    from test_gpu_csv_format import _check, _device_format
    rows, counts, table, ids, bad = cases.csv_case(frames)
    for with_ids in (None, ids):
        want = _check(ops, rows, counts, table, with_ids, spare=5, garbage=0xffc12345)
        assert len(want) > 0
    got, seg, status, whole = _device_format(ops, rows, bad, table, ids)
    assert status == CSV_BAD_COUNTS and not seg.any() and (whole == 0xAB).all()


def test_csv_tile_scan_at_scale(ops):
    """264 000 rows are 1032 tiles: the tile scan takes two tiles a thread; then a byte short of the total."""
    from adyolo_amd.postprocess import CSV_OVERFLOW, format_rows
    from test_gpu_csv_format import _device_format
    rows, counts, table = cases.csv_tiles_case()
    want, want_seg = format_rows(rows, counts, table)
    assert len(want) > 0 and len(want_seg) == 5
    got, seg, status, whole = _device_format(ops, rows, counts, table, n_bytes=len(want))
    assert status == 0 and seg.tolist() == want_seg.tolist() and got == want
    assert (whole[len(want):] == 0xAB).all() and len(whole) >= len(want) + 64
    got, seg, status, whole = _device_format(ops, rows, counts, table, n_bytes=len(want) - 1)
    assert status == CSV_OVERFLOW and seg.tolist() == want_seg.tolist() and (whole == 0xAB).all()


# ------------------------------------------------------------------------------------------------------------ 5. SELD scoring
SELD_BAD_ROWS = 4                                              # ops.SELD_STATUS


def _seld_acc(table, fill=0.0):
    """The accumulators [files][9 C + 3] float64 with guard words behind them -> (acc, the whole buffer, its length)"""
    n = table.n_files * (9 * cases.SELD_C + 3)
    whole = torch.full((n + 64,), 7.0, dtype=torch.float64, device=DEV)
    whole[:n] = fill
    return whole[:n].view(table.n_files, 9 * cases.SELD_C + 3), whole, n


def _seld_same(got, want):
    """The rule of tests/test_gpu_seld_score.py: counts exactly (the draw is robust), the float sums within rtol 1e-12."""
    C = cases.SELD_C
    de = slice(5 * C, 6 * C)                                            # total_DE: a float sum
    exact = np.r_[0:5 * C, 6 * C:9 * C + 3]
    np.testing.assert_array_equal(got[:, exact], want[:, exact])
    np.testing.assert_allclose(got[:, de], want[:, de], rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape", cases.SELD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_seld_score_at_scale(ops, shape, tmp_path):
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    case = cases.seld_case(shape, str(tmp_path))
    assert case["margin"] > cases.SELD_MARGIN
    sc = DeviceSELDScorer(cases.SELD_PRM, case["ref_dir"], DEV)
    table = sc.table
    ids = [sc._lookup(n) for n in case["names"]]
    file_ids = torch.tensor(ids, dtype=torch.int32, device=DEV)
    junk = np.full((5, 5), 9.0, dtype=np.float32)                       # rows behind the counted ones: not read
    rows = torch.from_numpy(np.concatenate([case["rows"], junk])).to(DEV)
    counts = torch.from_numpy(case["counts"]).to(DEV)
    acc, whole, n = _seld_acc(table)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.seld_score(rows, counts, table, file_ids, shape[1], acc, status)
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and bool((whole[n:] == 7.0).all())
    got = acc.cpu().numpy()[ids]
    print("clips %d x %d frames: %d rows, margin %.3g degrees" % (shape + (len(case["rows"]), case["margin"])))
    _seld_same(got, case["want"])
    # a negative count beyond frame 1024, and a total one row above the rows given (nothing behind them): the bit, and
    # nothing is added
    neg, past = cases.seld_bad_counts(case)
    for bad, r in ((neg, rows), (past, torch.from_numpy(case["rows"]).to(DEV))):
        acc, whole, n = _seld_acc(table, fill=1.5)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.seld_score(r, torch.from_numpy(bad).to(DEV), table, file_ids, shape[1], acc, status)
        torch.cuda.synchronize()
        assert int(status.item()) == SELD_BAD_ROWS and bool((acc == 1.5).all()) and bool((whole[n:] == 7.0).all())
    if shape != cases.SELD_RUN_SHAPE:
        return
    # the same frames as ONE stitched run of three segments: the bits of the whole-clip call
    (seg, seg_blocks, seg_ids), = sc.segment_tables(case["names"], [shape[1]] * shape[0], [0, shape[0] * shape[1]])
    assert tuple(seg.shape) == (3, 8) and seg_ids == ids
    run, whole, n = _seld_acc(table)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.seld_score_runs(rows, counts, table, seg, seg_blocks, run, status)
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and bool((whole[n:] == 7.0).all())
    run_h = run.cpu().numpy()[ids]
    _seld_same(run_h, case["want"])
    assert np.array_equal(run_h.view(np.int64), got.view(np.int64))
    for bad, r in ((neg, rows), (past, torch.from_numpy(case["rows"]).to(DEV))):
        acc, whole, n = _seld_acc(table, fill=1.5)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.seld_score_runs(r, torch.from_numpy(bad).to(DEV), table, seg, seg_blocks, acc, status)
        torch.cuda.synchronize()
        assert int(status.item()) == SELD_BAD_ROWS and bool((acc == 1.5).all()) and bool((whole[n:] == 7.0).all())
