"""CPU: the cases of tests/test_gpu_pipeline_scale.py -- the device data path at batch scale -- built and pinned.

Every stage of the device data path ends in a one-workgroup scan of 1024 threads: thread t sums the ``chunk = ceil(n / 1024)``
consecutive elements from ``t * chunk`` on, the chunk sums are scanned, and the thread writes the offsets of its own chunk.  Up
to n = 1024 every thread owns one element or none and the carry ``part[t] - sum`` between threads is the whole scan; above it
the loop over a chunk runs more than once.  This module builds the inputs that take each stage past that size, and asserts
what makes them tell a wrong scan from a right one: the chunk is longer than one element, one thread holds a partial chunk and
one an empty one, a scan that dropped the carry between threads (or the run inside a chunk) would give other offsets, every
planted bad element lies outside thread 0's chunk, every reference result has rows, and the SELD draws are robust.

"The elements of every chunk from the second on are not all zero, and neither is the prefix in front of them" holds as written
for the inputs whose counts are drawn here for the purpose (``dense_counts``: the CSV frames).  The AD-YOLO label lanes must
hold whole items without events, and the tracking, TTA and SELD generators of the existing tests keep stretches of empty
frames on purpose; for those ``assert_discriminating`` asserts the property the sentence is there for: the offsets of a scan
without the carry, and of a scan without the run inside a chunk, differ from the true ones at elements that have rows, and
at least 32 chunks behind the first hold rows behind rows.  (With the carry of every other wave of threads off by one for
chunk > 1, every GPU test of a size above 1024 fails and every other one passes.)  A partial and an empty chunk are asserted
over the sizes of a stage (``assert_partial_and_empty``): 2048 lanes have neither."""
import os

import numpy as np
import pytest
import torch

import adyolo_amd  # noqa: F401

SCAN_THREADS = 1024            # csrc/corpus.hip:352 CORPUS_SCAN_THREADS, track.hip:36 TRK_SCAN_THREADS, seld.hip:356 and
#                                select.hip:232 SCAN_THREADS, csv.hip:26 CSV_SCAN_THREADS
ROWS_GRID_THREADS = 1024 * 256  # csrc/corpus.hip:825 ``gx > 1024 ? 1024 : gx`` blocks of (line 826) 256 threads
ROWS_GRID_ELEMS = 4            # csrc/corpus.hip:824 ``cdiv(work, 256L * 4)``: the grid is sized for four elements a thread, so
#                                the loops of corpus_rows_kernel wrap from 4 elements a thread on; the 1024-block cap itself is
#                                reached past 1024 * 256 * 4 elements
EMIT_GRID_BLOCKS = 65536       # csrc/track.hip:353 ``n_frames < 65536 ? n_frames : 65536``
CW_EV_CACHE = 512              # csrc/corpus.hip:454
CW_MAX_CLASSES = 256           # csrc/corpus.hip:453
CW_FRAMES = 8                  # csrc/corpus.hip:452
CW_THREADS = 256               # csrc/corpus.hip:451
CSV_TILE = 256                 # csrc/csv.hip:25

N_EDGES = (1023, 1024, 1025, 2049, 3200)


# ------------------------------------------------------------------------------------------------------------- the work split
def chunk_of(n):
    return -(-n // SCAN_THREADS)


def split(n):
    """(chunk, threads with a full chunk, length of the partial chunk or 0, threads with an empty chunk)"""
    chunk = chunk_of(n)
    full, part = divmod(n, chunk)
    return chunk, full, part, SCAN_THREADS - full - (part > 0)


def scan_facts(counts):
    """What the exclusive scan of ``counts`` (negative ones count as they are) asks of the work split -> dict.  ``no_carry``:
    elements with rows whose offset a scan that forgot ``part[t] - sum`` would get wrong; ``no_run``: the same for a scan
    that gave every element of a chunk the chunk's first offset; ``live_chunks``: chunks from the second on with a non-zero
    element behind a non-zero prefix; ``chunks``: non-empty chunks from the second on; ``last_live``: the last non-empty chunk
    is such a chunk."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    n = len(c)
    chunk = chunk_of(n)
    true = np.cumsum(c) - c
    first = (np.arange(n) // chunk) * chunk                      # the first element of each element's chunk
    in_chunk = true - true[first]                                 # the offsets without the carry
    has = c != 0
    starts = np.arange(chunk, n, chunk)
    live = [bool(c[s:s + chunk].any() and true[s] != 0) for s in starts]
    return {"chunk": chunk, "no_carry": int((has & (in_chunk != true)).sum()), "no_run": int((has & (true[first] != true)).sum()),
            "chunks": len(starts), "live_chunks": int(sum(live)), "last_live": bool(live[-1]) if live else False}


def assert_discriminating(counts, every_chunk=False):
    """The assertions of the module docstring on one scanned array longer than 1024."""
    n = len(counts)
    chunk, full, part, empty = split(n)
    facts = scan_facts(counts)
    assert n > SCAN_THREADS and chunk >= 2 and facts["chunk"] == chunk
    assert facts["no_carry"] > 0 and facts["no_run"] > 0, facts
    assert facts["live_chunks"] >= 32, facts
    if every_chunk:
        assert facts["live_chunks"] == facts["chunks"] and facts["last_live"], facts
    return facts


def test_the_edges_split_as_documented():
    assert [split(n) for n in N_EDGES] == [(1, 1023, 0, 1), (1, 1024, 0, 0), (2, 512, 1, 511), (3, 683, 0, 341), (4, 800, 0, 224)]
    # 1025: thread 512 holds one element, threads 513 .. 1023 none; 2049: the last non-empty thread is 682, all chunks full
    # (2049 = 683 * 3) -- the partial chunk at chunk 3 needs 2050 -- so the CSV frames also run 2050, and the label lanes and
    # the TTA merge reach it through their mates and classes (2 * 1025 = 2050 lanes or slots).
    assert split(2050) == (3, 683, 1, 340)
    assert scan_facts([1] * 1025)["live_chunks"] == 512 and scan_facts([1] * 1025)["last_live"]
    assert scan_facts([0] * 1024 + [1])["no_carry"] == 0          # the check does see a case that shows nothing


def assert_partial_and_empty(sizes):
    """Among the scanned sizes of a stage: one in which a thread holds a partial chunk, one in which a thread holds none."""
    big = [split(n) for n in sizes if n > SCAN_THREADS]
    assert big and all(s[0] >= 2 for s in big)
    assert any(s[2] >= 1 for s in big) and any(s[3] >= 1 for s in big), (sizes, big)


def dense_counts(rng, n, high=4):
    """Counts 0 .. high - 1 with no chunk of the scan all zero and a row in front of the second chunk."""
    c = rng.integers(0, high, n)
    chunk = chunk_of(n)
    c[0] = max(c[0], 1)
    for s in range(0, n, chunk):
        if not c[s:s + chunk].any():
            c[min(n - 1, s + chunk - 1)] = 1
    return c


# ------------------------------------------------------------------------------------------------------ 1. AD-YOLO labels
YOLO_SIZES = ((3, 341), (4, 256), (5, 205), (3, 683), (16, 200))        # (B, max_events): the lanes are N_EDGES
YOLO_VARIANTS = ((False, False), (True, False), (False, True), (True, True))      # (mates, yaw): the four kernel instances
YOLO_T = 200                                                             # label frames of a 20 s chunk
# the ``special`` list of test_corpus_cpu._events (local to that function): az +-180, el +-90, 179.999
SPECIAL = ((180.0, 0.0), (-180.0, 12.5), (0.0, 90.0), (45.0, -90.0), (179.999, 89.9), (-0.25, -45.0), (90.0, 22.5))
NO_MATE = (-1, 0, 0, 0, -1, 0, 0, 0)


def _gain_word(g):
    return int(np.float32(g).view(np.uint32))


def _source(rng, n, t):
    """n events, frame-sorted, over frames [0, t + 6): some lie past the label frames -> {frame: [[cls, src, az, el], ...]}"""
    label = {}
    for f in np.sort(rng.integers(0, t + 6, n)).tolist():
        az, el = SPECIAL[int(rng.integers(len(SPECIAL)))] if rng.random() < 0.3 else \
            (float(rng.uniform(-180, 180)), float(rng.uniform(-90, 90)))
        label.setdefault(int(f), []).append([int(rng.integers(13)), 0, az, el])
    return label


def _n_events(label):
    return sum(len(v) for v in label.values())


def yolo_case(B, max_events, seed=None, t=YOLO_T):
    """A batch of B items and mates.  Items hold 0, 1, exactly ``max_events`` and random numbers of events; item 1 has no
    mate, item 2's mate is full as well.  -> dict: 'labels' [(item label, mate label or None)], 'events' float64 (E, 4),
    'items' / 'mates' int64 (B, 8) (every row with a combination in -1 .. 15 and a yaw in [-180, 180))."""
    rng = np.random.default_rng(1000 * B + max_events if seed is None else seed)
    n_item = [0, 1, max_events] + rng.integers(0, max_events + 1, max(0, B - 3)).tolist()
    n_mate = [int(rng.integers(1, max_events + 1)), None, max_events] + rng.integers(0, max_events + 1, max(0, B - 3)).tolist()
    labels, ev = [], []
    items, mates = torch.zeros(B, 8, dtype=torch.int64), torch.zeros(B, 8, dtype=torch.int64)
    for j in range(B):
        pair = []
        for k, n in enumerate((n_item[j], n_mate[j])):
            if n is None:
                pair.append(None)
                mates[j] = torch.tensor(NO_MATE)
                continue
            label = _source(rng, n, t)
            f_off, lo = 10 * (2 * j + k) + 3, len(ev)
            ev += [[float(f + f_off), float(e[0]), e[2], e[3]] for f, evs in label.items() for e in evs]
            row = torch.tensor([16 * (2 * j + k), f_off, lo, n, int(rng.integers(-1, 16)), 0, _gain_word(0.5) if k else 0,
                                int(rng.integers(-180, 180))])
            (mates if k else items)[j] = row
            pair.append(label)
        labels.append(tuple(pair))
    return {"B": B, "max_events": max_events, "t": t, "labels": labels, "items": items, "mates": mates,
            "events": torch.tensor(ev, dtype=torch.float64).reshape(-1, 4)}


def _moved(label, row, yaw):
    from adyolo_amd.augmentations import rotate_labels, yaw_labels
    comb = int(row[4])
    out = label if comb < 0 else rotate_labels(label, comb)
    return yaw_labels(out, int(row[7])) if yaw else out


def yolo_merged(case, j, mix, yaw):
    """The labels of item j as the host path forms them: each source moved by its own row, then ``merge_labels``."""
    from adyolo_amd.augmentations import merge_labels
    a, m = case["labels"][j]
    return merge_labels(_moved(a, case["items"][j], yaw), {} if m is None or not mix else _moved(m, case["mates"][j], yaw))


def yolo_reference(case, mix, yaw, skip=()):
    """-> (M, 7) float32: ``get_yolo_label`` + ``collate_fn``, as ``_yolo_want`` of tests/test_gpu_time_mix.py and of
    tests/test_gpu_yaw_rotation.py."""
    from adyolo_amd.datasets import YoloLabelEncoder, collate_fn
    enc = YoloLabelEncoder()
    labels = [[] if j in skip else enc.get_yolo_label(yolo_merged(case, j, mix, yaw), case["t"]) for j in range(case["B"])]
    if not any(labels):
        return torch.zeros(0, 7)
    return collate_fn([(np.zeros(1, dtype=np.float32), r) for r in labels])[1]


def yolo_lane_counts(case, mix, yaw):
    """The row count of every place of the workspace, in the order the scan sees them: per item the events of the merged label
    in its order (an event past the label frames gives no row), the places without an event behind them."""
    from adyolo_amd.datasets import YoloLabelEncoder
    enc = YoloLabelEncoder()
    per = (2 if mix else 1) * case["max_events"]
    out = np.zeros((case["B"], per), dtype=np.int64)
    for j in range(case["B"]):
        evs = [(f, e) for f, lst in yolo_merged(case, j, mix, yaw).items() for e in lst]
        if not evs:
            continue
        rows = enc.encode_events(np.arange(len(evs)), [e[0] for _, e in evs], [e[2] for _, e in evs], [e[3] for _, e in evs])
        n = np.bincount(rows[:, 0].astype(np.int64), minlength=len(evs))
        n[[f >= case["t"] for f, _ in evs]] = 0
        out[j, :len(evs)] = n
    return out.reshape(-1)


def yolo_bad_item(case, mix):
    """The item to spoil: the last one -- its lanes begin behind thread 0's chunk."""
    per = (2 if mix else 1) * case["max_events"]
    b = case["B"] - 1
    assert b * per >= chunk_of(case["B"] * per)
    return b


@pytest.mark.parametrize("size", YOLO_SIZES, ids=lambda s: "%dx%d" % s)
def test_yolo_cases(size):
    B, me = size
    assert B * me in N_EDGES
    case = yolo_case(B, me)
    n = [_n_events(a) for a, _ in case["labels"]]
    assert n[:3] == [0, 1, me] and case["labels"][1][1] is None and _n_events(case["labels"][2][1]) == me
    assert int(case["items"][:, 3].max()) == me and len(case["events"]) == int(case["items"][:, 3].sum() + case["mates"][:, 3].sum())
    for a, m in case["labels"]:
        for label in (a, m):
            if label:
                assert list(label) == sorted(label)                                  # frame-sorted
    assert any(f >= case["t"] for a, _ in case["labels"] for f in a)                 # events past the label frames
    assert any(set(a) & set(m) for a, m in case["labels"] if m)                      # frames shared by item and mate
    angles = {(e[2], e[3]) for a, _ in case["labels"] for evs in a.values() for e in evs}
    assert set(SPECIAL) <= angles
    for mix, yaw in YOLO_VARIANTS:
        want = yolo_reference(case, mix, yaw)
        lanes = yolo_lane_counts(case, mix, yaw)
        assert len(lanes) == B * me * (2 if mix else 1) and int(lanes.sum()) == want.shape[0] > 0
        if len(lanes) > SCAN_THREADS:
            assert_discriminating(lanes)
        b = yolo_bad_item(case, mix)
        less = yolo_reference(case, mix, yaw, skip={b})
        assert 0 < less.shape[0] < want.shape[0]                                     # the bad item did have rows
    # the mates double the lanes: 1025 -> 2050 lanes is the partial chunk at chunk 3, 2049 -> 4098 a partial chunk at chunk 5
    assert split(2 * 1025)[2] == 1 and split(2 * 2049) == (5, 819, 3, 204)
    assert_partial_and_empty([b * m * k for b, m in YOLO_SIZES for k in (1, 2)])


# the grid of corpus_rows_kernel: cdiv(max(cap, lanes), 1024) blocks, at most 1024
ROWS_WRAP_CAP = ROWS_GRID_THREADS + 4096                # past the largest grid: 260 blocks, the b = -1 fill makes 4 trips
ROWS_WRAP_EVENTS = 16385                                # B = 16: 262 160 lanes, 257 blocks, the lane loop makes 4 trips
ROWS_CAPPED_CAP = ROWS_GRID_THREADS * ROWS_GRID_ELEMS + 4096   # 1024 blocks (capped): the fill makes 5 trips
ROWS_CAPPED_EVENTS = 65537                              # B = 16: 1 048 592 lanes, 1024 blocks (capped): 5 trips


def yolo_wide_case(max_events, B=16, t=20):
    """B items of which only the last two have events, ``max_events`` each, and only the last five of those lie in the item's
    window: the others are earlier events of the recording (a window-relative frame below 0 gives no row), so the rows come
    from the last lanes of the last items.  Both items read one range of the table under different combinations.
    -> the case (as ``yolo_case``; every mate row is the no-mate row)"""
    f_off = 1000
    tail = {0: [[3, 0, 170.0, 10.0]], 3: [[1, 0, -180.0, -20.0], [2, 0, 179.999, 89.9]], 7: [[4, 0, 90.0, 45.0]],
            19: [[5, 0, -90.0, 0.0]]}
    n_fill = max_events - 5
    ev = np.zeros((max_events, 4))
    ev[:n_fill, 0] = np.arange(n_fill) * (f_off - 1) // n_fill                       # ascending, all below f_off
    ev[:n_fill, 1] = np.arange(n_fill) % 13
    ev[:n_fill, 2] = (np.arange(n_fill) * 37) % 360 - 180.0
    ev[n_fill:] = [[float(f + f_off), float(e[0]), e[2], e[3]] for f, evs in tail.items() for e in evs]
    assert (np.diff(ev[:, 0]) >= 0).all() and ev[n_fill - 1, 0] < f_off
    items = torch.zeros(B, 8, dtype=torch.int64)
    items[:, 0] = 16 * torch.arange(B)
    items[:, 1] = f_off
    items[:, 4] = torch.arange(B) % 17 - 1
    items[B - 2:, 3] = max_events
    mates = torch.tensor(NO_MATE).repeat(B, 1)
    labels = [({}, None)] * (B - 2) + [(tail, None)] * 2
    return {"B": B, "max_events": max_events, "t": t, "labels": labels, "items": items, "mates": mates,
            "events": torch.from_numpy(ev)}


def test_yolo_grid_cases():
    blocks = lambda work: min(1024, -(-work // (256 * ROWS_GRID_ELEMS)))             # noqa: E731  (corpus.hip:824-825)
    trips = lambda work: -(-work // (blocks(work) * 256))                            # noqa: E731
    assert blocks(ROWS_WRAP_CAP) == 260 and trips(ROWS_WRAP_CAP) == 4
    assert 16 * ROWS_WRAP_EVENTS == 262160 > ROWS_GRID_THREADS and blocks(262160) == 257 and trips(262160) == 4
    assert blocks(ROWS_CAPPED_CAP) == 1024 and trips(ROWS_CAPPED_CAP) == 5
    assert blocks(16 * ROWS_CAPPED_EVENTS) == 1024 and trips(16 * ROWS_CAPPED_EVENTS) == 5
    for me in (ROWS_WRAP_EVENTS, ROWS_CAPPED_EVENTS):
        case = yolo_wide_case(me)
        want = yolo_reference(case, False, False)
        lanes = yolo_lane_counts(case, False, False)          # (the host labels hold the window's events only: five places)
        assert want.shape[0] == int(lanes.sum()) > 0 and set(want[:, 0].tolist()) == {14.0, 15.0}
        assert not torch.equal(want[want[:, 0] == 14][:, 5], want[want[:, 0] == 15][:, 5])     # two combinations
        # on the device the five events are lanes max_events - 5 .. max_events - 1 of items 14 and 15
        first = 14 * me + me - 5
        assert first >= blocks(16 * me) * 256 * (trips(16 * me) - 2)                 # reached on a late trip of the loop
        assert first // chunk_of(16 * me) >= 1


# ------------------------------------------------------------------------------------------------------------ 3. TTA pool
TTA_FRAMES = (1025, 2049)
TTA_CLASSES, TTA_VIEWS, TTA_POOL, TTA_UNIFY = 2, [0, 5], 4, 15.0


def tta_case(frames):
    """``random_views`` of tests/test_tta_cpu.py (frame 1 holds a crowd, view 1 has P rows in frame 0 and P + 1 in the last
    one) -> (per_view, and per_view with a bad count: view 0's last frame -- in the last non-empty thread's chunk -- claims
    three rows more than the rows given hold; with no row behind them it gives none: 'short' is what the host merges)."""
    from test_tta_cpu import random_views
    per_view, redrawn = random_views(900 + frames, frames, TTA_CLASSES, TTA_VIEWS, TTA_UNIFY, rows_cap=TTA_POOL)
    assert redrawn <= frames // 100
    rows0, counts0 = per_view[0]
    n_last = int(counts0[-1])
    bad_counts = counts0.copy()
    bad_counts[-1] = n_last + 3
    short_counts = counts0.copy()
    short_counts[-1] = 0
    bad = [(rows0, bad_counts), per_view[1]]
    short = [(rows0[:len(rows0) - n_last], short_counts), per_view[1]]
    return per_view, bad, short


@pytest.mark.parametrize("frames", TTA_FRAMES)
def test_tta_cases(frames):
    from adyolo_amd.postprocess import TTA_ROWS_OVERFLOW, merge_view_rows
    per_view, bad, short = tta_case(frames)
    assert per_view[1][1][0] == TTA_POOL and per_view[1][1][-1] == TTA_POOL + 1          # a frame with P + 1 rows
    for rows, counts in per_view:                                                        # tta_collect scans the frame counts
        assert len(counts) == frames and int(counts.sum()) == len(rows)
        assert_discriminating(counts)
    assert (frames - 1) // chunk_of(frames) >= 1                                          # the bad frame: not thread 0's
    for min_views in (1, 2):
        (rows, counts), status = merge_view_rows(per_view, TTA_VIEWS, TTA_UNIFY, min_views, max_rows_per_frame=TTA_POOL)
        assert status == TTA_ROWS_OVERFLOW and len(rows) > 0
        (s_rows, s_counts), s_status = merge_view_rows(short, TTA_VIEWS, TTA_UNIFY, min_views, max_rows_per_frame=TTA_POOL)
        assert s_status == TTA_ROWS_OVERFLOW and (min_views == 2 or int(per_view[0][1][-1]) == 0 or len(s_rows) <= len(rows))
        slots = np.zeros((frames, TTA_CLASSES), dtype=np.int64)                           # tta_merge scans (frame, class)
        np.add.at(slots, (rows[:, 0].astype(int), rows[:, 1].astype(int)), 1)
        assert_discriminating(slots.reshape(-1))
    assert_partial_and_empty(list(TTA_FRAMES) + [f * TTA_CLASSES for f in TTA_FRAMES])


# ------------------------------------------------------------------------------------------------------------- 4. tracking
TRACK_SHAPES = ((5, 205, 2), (1, 2049, 1), (16, 200, 3), (257, 256, 1))      # (clips, frames, classes): 1025, 2049, 3200, 65 792
TRACK_CORNERS = ((0, 1, 1.0), (2, 3, 0.5))
TRACK_GATE = 20.0
_track_cache = {}


def track_case(shape):
    """``random_tracks`` of tests/test_track_cpu.py at one shape -> {'rows', 'counts', 'bad': {'neg': (counts, frame), 'past':
    (counts, frame)}}: a negative count in a frame beyond frame 1024 (the frames behind it start two rows early, as the
    definition has it), and the last frame claiming three rows more than there are."""
    from test_track_cpu import random_tracks
    if shape not in _track_cache:
        n_clips, T, C = shape
        case = random_tracks(300 + T + n_clips, n_clips, T, C)
        counts = case["counts"]
        n = len(counts)
        f = min(n - 1, 1024 + n // 9)
        neg, past = counts.copy(), counts.copy()
        neg[f] = -2
        past[-1] += 3
        case["bad"] = {"neg": (neg, f), "past": (past, n - 1)}
        _track_cache[shape] = case
    return _track_cache[shape]


def track_want(shape, corner, bad=None):
    from adyolo_amd.postprocess import track_rows
    key = (shape, corner, bad)
    if key not in _track_cache:
        case = track_case(shape)
        counts = case["counts"] if bad is None else case["bad"][bad][0]
        _track_cache[key] = track_rows(case["rows"], counts, shape[0], shape[2], TRACK_GATE, *corner)
    return _track_cache[key]


@pytest.mark.parametrize("shape", TRACK_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_track_cases(shape):
    from adyolo_amd.postprocess import TRACK_BAD_ROWS
    n_clips, T, C = shape
    n = n_clips * T
    case = track_case(shape)
    assert n > SCAN_THREADS and len(case["counts"]) == n and int(case["counts"].sum()) == len(case["rows"])
    assert_discriminating(case["counts"])                                   # track_scan_kernel<true>: the frame counts
    for kind, (counts, f) in case["bad"].items():
        assert f >= 1024 and f // chunk_of(n) >= 1                          # the 1025th frame or a later one: not thread 0's
        offs = np.cumsum(counts) - counts
        assert counts[f] < 0 if kind == "neg" else offs[f] + counts[f] == len(case["rows"]) + 3
    for corner in TRACK_CORNERS:
        (rows, counts), ids, status = track_want(shape, corner)
        assert len(rows) > 0 and len(counts) == n and not status & TRACK_BAD_ROWS
        assert_discriminating(counts)                                       # track_scan_kernel<false>: the emitted counts
        for kind in case["bad"]:
            (b_rows, b_counts), _, b_status = track_want(shape, corner, bad=kind)
            assert b_status & TRACK_BAD_ROWS and len(b_rows) > 0
            assert not np.array_equal(b_counts, counts) or not np.array_equal(b_rows, rows)
    if n > EMIT_GRID_BLOCKS:                                                # the frame loop of track_emit_kernel wraps
        assert -(-n // EMIT_GRID_BLOCKS) == 2 and track_want(shape, TRACK_CORNERS[0])[0][1][EMIT_GRID_BLOCKS:].sum() > 0


def test_track_shapes_cover_the_split():
    assert [c * t for c, t, _ in TRACK_SHAPES] == [1025, 2049, 3200, 65792]
    assert_partial_and_empty([c * t for c, t, _ in TRACK_SHAPES])


TRACK_RUN_LENGTHS, TRACK_RUN_BOUNDS, TRACK_RUN_C = (700, 600), (0, 1100, 1300), 2


def track_run_case(corner):
    """Two recordings of 700 and 600 frames in two passes: the first holds recording 0 whole and 400 frames of recording 1,
    which stays open (1100 run frames + the hold > 1024); the second takes the carry.  -> (rows, counts, start, parts, plan, hold)"""
    from adyolo_amd.corpus import plan_track
    from adyolo_amd.postprocess import track_hold
    from test_track_windows_cpu import stream_of_recordings
    hold = track_hold(corner[0], corner[1])
    rows, counts, start, parts = stream_of_recordings(820, TRACK_RUN_LENGTHS, TRACK_RUN_C)
    return rows, counts, start, parts, plan_track(start, TRACK_RUN_BOUNDS, hold), hold


@pytest.mark.parametrize("corner", TRACK_CORNERS)
def test_track_run_case(corner):
    from test_track_windows_cpu import by_recording, host_step, run_plan, whole
    rows, counts, start, parts, plan, hold = track_run_case(corner)
    seg = [s.tolist() for s in plan["segments_host"]]
    assert seg == [[[0, 700, 0, 0], [700, 400, 0, 1]], [[0, 200, 1, 0]]]
    assert 1100 + hold > SCAN_THREADS and chunk_of(1100) == 2
    assert_discriminating(counts[:1100])                                    # the first pass's frame counts
    results = run_plan(host_step(TRACK_RUN_C, *corner, hold), rows, counts, plan, TRACK_RUN_BOUNDS)
    emitted = np.zeros(1100 + hold, dtype=np.int64)
    emitted[:len(results[0][0][1])] = results[0][0][1]
    assert_discriminating(emitted)                                          # the emitted counts: hold + run frames are scanned
    got, status = by_recording(results, plan, start)
    for r, (r_rows, r_counts) in enumerate(parts):                          # the host definition of the carried form is the whole one
        (w_rows, w_counts), w_ids, _ = whole(r_rows, r_counts, TRACK_RUN_C, *corner)
        assert len(w_rows) > 0 and got[r][0].tobytes() == w_rows.tobytes() and np.array_equal(got[r][1], w_counts)
        assert np.array_equal(got[r][2], w_ids)


# ------------------------------------------------------------------------------------------------------------- 6. CSV bytes
CSV_FRAMES = (1025, 2049, 2050, 3200)                  # 2050: the partial chunk at chunk 3 (2049 = 683 x 3 has none)
CSV_TILES_FRAMES, CSV_TILES_ROWS = 1100, 240           # 264 000 rows = 1032 tiles of 256: csv_scan_kernel takes chunk 2


def csv_case(frames):
    """0 to 3 rows per frame (no chunk of the scan without a row), a table of several files, track ids.
    -> (rows, counts, table, ids, counts with a negative one beyond frame 1024)"""
    from test_gpu_csv_format import _rows
    rng = np.random.default_rng(60 + frames)
    counts = dense_counts(rng, frames)
    rows = _rows(rng, counts)
    ids = rng.integers(0, 30, len(rows)).astype(np.int32)
    cuts = sorted(rng.choice(np.arange(1, frames), 5, replace=False).tolist())
    table = np.asarray([[0, 0], [cuts[0], 0], [cuts[1], 7], [cuts[1], 0], [cuts[2], 990], [cuts[3], 0], [cuts[4], 0]], dtype=np.int32)
    bad = counts.copy()
    bad[min(frames - 1, 1024 + frames // 9)] = -1
    return rows, counts, table, ids, bad


def csv_tiles_case():
    from adyolo_amd.postprocess import csv_segments_clips
    from test_gpu_csv_format import _rows
    rng = np.random.default_rng(77)
    counts = np.full(CSV_TILES_FRAMES, CSV_TILES_ROWS)
    return _rows(rng, counts), counts, csv_segments_clips(4, CSV_TILES_FRAMES // 4)


@pytest.mark.parametrize("frames", CSV_FRAMES)
def test_csv_cases(frames):
    from adyolo_amd.postprocess import format_rows
    rows, counts, table, ids, bad = csv_case(frames)
    assert counts.min() == 0 and counts.max() == 3 and len(table) == 7
    assert_discriminating(counts, every_chunk=True)
    f = int(np.flatnonzero(bad < 0)[0])
    assert f >= 1024 and f // chunk_of(frames) >= 1               # the 1025th frame or a later one
    data, seg = format_rows(rows, counts, table, ids)
    assert len(data) > 0 and len(seg) == 8 and (np.diff(seg) >= 0).all() and seg[3] == seg[2]      # an empty file among them
    with pytest.raises(ValueError):
        format_rows(rows, bad, table, ids)


def test_csv_sizes_cover_the_split():
    assert_partial_and_empty(CSV_FRAMES)
    n_rows = CSV_TILES_FRAMES * CSV_TILES_ROWS
    tiles = -(-n_rows // CSV_TILE)
    assert n_rows == 264000 and tiles == 1032 and split(tiles) == (2, 516, 0, 508)
    assert split(CSV_TILES_FRAMES) == (2, 550, 0, 474)
    from adyolo_amd.postprocess import format_rows
    rows, counts, table = csv_tiles_case()
    data, seg = format_rows(rows, counts, table)
    assert len(rows) == n_rows and len(data) > 0 and len(seg) == 5 and (np.diff(seg) > 0).all()      # every tile holds bytes


# ------------------------------------------------------------------------------------------------------ 2. class-wise labels
CW_C, CW_T, CW_MAX_EVENTS = 13, 9, 700                 # 9 label frames: a tile of 8 and a tile of one
CW_TILE_ITEM, CW_TILE_MATE = (85,) * 6 + (60, 30), (85,) * 6 + (15, 5)     # events per frame of the first tile: 600 and 530
CW_TRIPLE = (10, 11)                                   # the class of the three events at tile positions 511 .. 513, per source
CW_LAST = 12                                           # a class of frame 7 with two events, both past position 512
CW_BAD_AT = 585                                        # the item's event that the bad-class run spoils (a filler of frame 7)
CW_LOSSES = ("seddoa", "accdoa", "adpit")


def _cw_source(rng, sizes, triple):
    """{frame: events}: frames 0 .. 7 with ``sizes`` events of classes 0 .. 9, frame 6 holding ``triple`` at the tile's
    positions 511 .. 513 and frame 7 ``CW_LAST`` first and last; 12 events in frame 8 and 4 in frame 9 (past the frames)."""
    def ev(cls):
        return [int(cls), 0, float(rng.integers(-180, 181)), float(rng.integers(-90, 91))]
    label, at = {}, 0
    for f, n in enumerate(tuple(sizes) + (12, 4)):
        evs = [ev(rng.integers(0, 10)) for _ in range(n)]
        for k in range(n):
            if at + k in (511, 512, 513):
                evs[k] = ev(triple)
        if f == 7:
            evs[0], evs[-1] = ev(CW_LAST), ev(CW_LAST)
        label[f] = evs
        at += n
    return label


def _cw_table(sources, combs):
    """sources [(label or None)] -> (events (E, 4) float64, rows int64 (len, 8): the no-mate row for None)"""
    ev, rows = [], []
    for k, (label, comb) in enumerate(zip(sources, combs)):
        if label is None:
            rows.append(list(NO_MATE))
            continue
        f_off, lo = 11 * k + 2, len(ev)
        ev += [[float(f + f_off), float(e[0]), e[2], e[3]] for f, evs in label.items() for e in evs]
        rows.append([16 * k, f_off, lo, len(ev) - lo, comb, 0, _gain_word(1.0) if k % 2 else 0, 0])
    return torch.tensor(ev, dtype=torch.float64).reshape(-1, 4), torch.tensor(rows, dtype=torch.int64)


def classwise_cache_case():
    """Item 0: 600 events in its first tile of 8 label frames, its mate 530; item 1: a dozen events, no mate.
    -> {'labels' [(item, mate or None)], 'events', 'items', 'mates', 'combs'}"""
    rng = np.random.default_rng(512)
    big, mate = _cw_source(rng, CW_TILE_ITEM, CW_TRIPLE[0]), _cw_source(rng, CW_TILE_MATE, CW_TRIPLE[1])
    small = {f: [[int(rng.integers(0, CW_C)), 0, float(rng.integers(-180, 181)), float(rng.integers(-90, 91))]
                 for _ in range(int(rng.integers(1, 4)))] for f in (0, 3, 7, 8, 9)}
    combs = (5, 12, -1, -1)
    events, rows = _cw_table([big, mate, small, None], combs)
    return {"labels": [(big, mate), (small, None)], "events": events, "items": rows[0::2].contiguous(),
            "mates": rows[1::2].contiguous(), "combs": combs}


def classwise_reference(case, loss, nb_classes, t, mix, drop=None):
    """The host encoder on each item's merged labels -> [target per item]; drop = (item, source, frame, index): without that
    event."""
    from adyolo_amd.augmentations import merge_labels, rotate_labels
    from adyolo_amd.datasets import CLASSWISE_LABELS, ClasswiseLabelEncoder
    enc = ClasswiseLabelEncoder(nb_classes)
    out = []
    for j, pair in enumerate(case["labels"]):
        moved = []
        for k, label in enumerate(pair):
            if label is None or (k == 1 and not mix):
                moved.append({})
                continue
            if drop is not None and drop[:2] == (j, k):
                label = {f: [e for i, e in enumerate(evs) if (f, i) != drop[2:]] for f, evs in label.items()}
            comb = int((case["mates"] if k else case["items"])[j, 4])
            moved.append(label if comb < 0 else rotate_labels(label, comb))
        out.append(getattr(enc, CLASSWISE_LABELS[loss])(merge_labels(*moved), t))
    return out


def test_classwise_cache_case():
    case = classwise_cache_case()
    for k, (label, sizes) in enumerate(zip(case["labels"][0], (CW_TILE_ITEM, CW_TILE_MATE))):
        flat = [(f, e) for f, evs in label.items() for e in evs]
        tile = [x for x in flat if x[0] < CW_FRAMES]
        assert len(tile) == sum(sizes) > CW_EV_CACHE and len(flat) <= CW_MAX_EVENTS
        assert [e[0] for _, e in flat[511:514]] == [CW_TRIPLE[k]] * 3 and {f for f, _ in flat[511:514]} == {6}
        assert sum(e[0] == CW_TRIPLE[k] for e in label[6]) == 3                       # ADPIT: exactly these three
        assert CW_EV_CACHE - 1 in (511, 512, 513) and CW_EV_CACHE in (511, 512, 513)   # the pick straddles the cache
        last = [i for i, (f, e) in enumerate(flat) if f == 7 and e[0] == CW_LAST]
        assert len(last) == 2 and min(last) > CW_EV_CACHE and label[7][0][2:] != label[7][-1][2:]
        assert any(f == CW_T - 1 for f, _ in flat) and any(f >= CW_T for f, _ in flat)  # the second tile; past the frames
    assert all(e[0] != CW_TRIPLE[0] for e in case["labels"][0][1][6]) and all(e[0] != CW_TRIPLE[1] for e in case["labels"][0][0][6])
    f, i = 7, CW_BAD_AT - sum(CW_TILE_ITEM[:7])
    assert CW_BAD_AT > CW_EV_CACHE and 0 < i < CW_TILE_ITEM[7] - 1 and case["labels"][0][0][f][i][0] < 10
    assert float(case["events"][int(case["items"][0, 2]) + CW_BAD_AT, 1]) == case["labels"][0][0][f][i][0]
    assert int(case["items"][0, 3]) == 616 and int(case["mates"][0, 3]) == 546 and -(-CW_T // CW_FRAMES) == 2
    for loss in CW_LOSSES:
        for mix in (False, True):
            want = classwise_reference(case, loss, CW_C, CW_T, mix)
            assert all(bool(w.any()) for w in want)
            dropped = classwise_reference(case, loss, CW_C, CW_T, mix, drop=(0, 0, f, i))
            assert len(dropped) == 2
        # the mate changes item 0, and the triple lands in ADPIT's slots 3 .. 5 of frame 6
        assert not torch.equal(classwise_reference(case, loss, CW_C, CW_T, False)[0], classwise_reference(case, loss, CW_C, CW_T, True)[0])
    adpit = classwise_reference(case, "adpit", CW_C, CW_T, True)[0]
    assert bool((adpit[6, 3:, 0, CW_TRIPLE[0]] == 1).all()) and bool((adpit[6, 3:, 0, CW_TRIPLE[1]] == 1).all())


CW_WIDE_MAX_EVENTS = 96


def classwise_wide_case(nb_classes=CW_MAX_CLASSES):
    """B = 2 with mates at the largest class count: every frame holds the classes 0 and C - 1, a pair and a triple of one
    class each, and random ones."""
    rng = np.random.default_rng(256)

    def source():
        label = {}
        for f in range(CW_T + 1):
            cls = [0, nb_classes - 1] + rng.integers(0, nb_classes, 2).tolist()
            pair, triple = (int(v) for v in rng.choice(np.arange(1, nb_classes - 1), 2, replace=False))
            cls += [pair] * 2 + [triple] * 3
            label[f] = [[int(c), 0, float(rng.integers(-180, 181)), float(rng.integers(-90, 91))] for c in rng.permutation(cls)]
        return label
    sources = [source() for _ in range(4)]
    combs = (3, -1, 15, 8)
    events, rows = _cw_table(sources, combs)
    return {"labels": [(sources[0], sources[1]), (sources[2], sources[3])], "events": events, "items": rows[0::2].contiguous(),
            "mates": rows[1::2].contiguous(), "combs": combs}


def test_classwise_wide_case():
    case = classwise_wide_case()
    assert int(max(case["items"][:, 3].max(), case["mates"][:, 3].max())) <= CW_WIDE_MAX_EVENTS
    assert 24 * CW_MAX_CLASSES == 6144 == 24 * CW_THREADS and CW_FRAMES * CW_MAX_CLASSES * 4 * 4 == 32768     # passes; LDS bytes
    for loss in CW_LOSSES:
        for mix in (False, True):
            for w in classwise_reference(case, loss, CW_MAX_CLASSES, CW_T, mix):
                assert bool(w.any()) and w.shape[0] == CW_T
    adpit = classwise_reference(case, "adpit", CW_MAX_CLASSES, CW_T, True)[0]
    assert bool(adpit[:, 0, 0, CW_MAX_CLASSES - 1].any() | adpit[:, 1, 0, CW_MAX_CLASSES - 1].any()) and bool(adpit[:, 3:, 0].any())


# ------------------------------------------------------------------------------------------------------------ 5. SELD scoring
SELD_PRM = {"data_config": {"nb_classes": 12, "sr": 24000, "label_hop_len_s": 0.1}}
SELD_C = 12
SELD_SHAPES = ((5, 205), (16, 200), (3, 360))          # (clips, frames): 1025 and 3200 frames; 1080, also scored as ONE run
SELD_RUN_SHAPE = (3, 360)                               # ... of three segments, one per file
SELD_SEEDS = (31, 32, 33, 34, 35, 36, 37, 38)           # the draws of a shape, tried in this order: the first robust one is used
SELD_MARGIN = 1e-9                                      # degrees from the 20-degree threshold (tests/test_gpu_seld_score.py)


def seld_case(shape, root):
    """``_synthetic_split`` of tests/test_gpu_seld_score.py (sparse) at one shape, its reference and prediction CSV folders
    written under ``root``, scored per file by the host ``SELDScorer``.  A draw with a track average within ``SELD_MARGIN`` of
    the threshold is drawn again under the next pinned seed.
    -> {'names', 'ref_dir', 'want' (files, 9 C + 3), 'rows' (N, 5) float32, 'counts' (clips * frames,) int32, 'margin',
    'draws'}"""
    from adyolo_amd.postprocess import write_seld_output_file
    from adyolo_amd.seld_metrics import ComputeSELDResults, SELDScorer
    from test_gpu_seld_score import _synthetic_split, _track_averages
    n_files, t_clip = shape
    names = ["f%02d" % k for k in range(n_files)]
    for draw, seed in enumerate(SELD_SEEDS):
        refs, preds = _synthetic_split(np.random.default_rng(1000 * seed + t_clip), n_files, t_clip, False)
        ref_dir, pred_dir = os.path.join(root, "ref_%d" % draw), os.path.join(root, "pred_%d" % draw)
        os.makedirs(ref_dir), os.makedirs(pred_dir)
        for name, ref, pred in zip(names, refs, preds):
            with open(os.path.join(ref_dir, name + ".csv"), "w") as f:
                for r in ref:
                    f.write("%d,%d,%d,%d,%d\n" % tuple(r))
            write_seld_output_file(os.path.join(pred_dir, name + ".csv"), pred)
        host = ComputeSELDResults(SELD_PRM, ref_dir)
        want, avgs = [], []
        for name in names:
            labels = host._pred_labels(pred_dir, name + ".csv")
            sc = SELDScorer(SELD_C, 20.0)
            sc.update(labels, host._ref[name + ".csv"][0])
            want.append(sc.accumulator())
            avgs += _track_averages(labels, host._ref[name + ".csv"][0], SELD_C)
        margin = min(abs(a - 20.0) for a in avgs)
        if margin > SELD_MARGIN:
            break
    rows, counts = [], np.zeros((n_files, t_clip), dtype=np.int32)
    for k, pred in enumerate(preds):                               # float32 rows in frame order, as yolo_select leaves them
        for fr in sorted(pred):
            counts[k, fr] = len(pred[fr])
            rows += [[k * t_clip + fr] + r for r in pred[fr]]
    return {"names": names, "ref_dir": ref_dir, "want": np.asarray(want), "margin": margin, "draws": draw + 1, "tracks": len(avgs),
            "rows": np.asarray(rows, dtype=np.float32).reshape(-1, 5), "counts": counts.reshape(-1)}


def seld_bad_counts(case):
    """-> (counts with a negative one beyond frame 1024, counts that total one row above the rows)"""
    n = len(case["counts"])
    neg, past = case["counts"].copy(), case["counts"].copy()
    neg[min(n - 1, 1024 + n // 9)] = -1
    past[-1] += 1
    return neg, past


@pytest.mark.parametrize("shape", SELD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_seld_cases(shape, tmp_path):
    case = seld_case(shape, str(tmp_path))
    n = shape[0] * shape[1]
    assert case["margin"] > SELD_MARGIN and case["tracks"] > 50, case["margin"]      # the final draw is robust
    assert case["draws"] == 1                                                        # (pinned: the first seed is)
    assert n > SCAN_THREADS and len(case["counts"]) == n and int(case["counts"].sum()) == len(case["rows"]) > 0
    assert_discriminating(case["counts"])
    neg, past = seld_bad_counts(case)
    f = int(np.flatnonzero(neg < 0)[0])
    assert f >= 1024 and f // chunk_of(n) >= 1 and int(past.sum()) == len(case["rows"]) + 1
    want, C = case["want"], SELD_C
    assert want[:, 0:C].sum() > 0 and want[:, C:2 * C].sum() > 0 and want[:, 3 * C:4 * C].sum() > 0     # TP, FP and FN
    if shape == SELD_RUN_SHAPE:
        from adyolo_amd.seld_metrics import run_segments
        seg, = run_segments([shape[1]] * 3, [0, n])
        assert seg.tolist() == [[0, 0, 0, 360, 1], [1, 0, 360, 360, 1], [2, 0, 720, 360, 1]]


def test_seld_sizes_cover_the_split():
    assert [c * t for c, t in SELD_SHAPES] == [1025, 3200, 1080]
    assert_partial_and_empty([c * t for c, t in SELD_SHAPES])
