"""CPU: tracks carried across runs -- the host definition ``postprocess.track_run`` against ``postprocess.track_rows`` on whole
recordings (every cut position, random partitions, runs of several recordings), the hold bound ``track_hold`` and its guard, the
window plan (``corpus.plan_track`` / ``_WindowCorpus.track_plan``), the scorer's segments on the emitted bounds and the C ABI's
declarations.  ``stream_case`` / ``feed`` / ``cut_sets`` are what the GPU test (test_gpu_track_windows.py) feeds to the kernels."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import adyolo_amd  # noqa: F401
from adyolo_amd import _lib
from adyolo_amd.corpus import _WindowCorpus, plan_track
from adyolo_amd.postprocess import track_hold, track_rows, track_run
from adyolo_amd.seld_metrics import run_segments
from test_track_cpu import direction, pack, random_tracks

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 20.0
GRID = [(g, m) for g in range(4) for m in range(1, 5)]           # max_gap 0..3 x min_len 1..4
SMOOTH = {1: 1.0, 2: 0.5, 3: 0.5, 4: 0.25}                       # by min_len: the identity weight and two smoothing ones
T_STREAM, C_STREAM, SEED = 70, 3, 170                            # one recording: frames 0 .. 69, a cut at 64 among all cuts


def stream_case(seed, T, C):
    """One recording's selected rows: ``random_tracks`` (for T >= 60 the 64- and 65-row frames, the zero and the NaN vector, the
    pairs of lone detections, the pair that is filled and pruned) -> (rows, counts)."""
    case = random_tracks(seed, 1, T, C)
    return case["rows"], case["counts"]


def whole(rows, counts, C, max_gap, min_len, smooth, trace=None):
    return track_rows(rows, counts, 1, C, GATE, max_gap, min_len, smooth, trace=trace)


def feed(step, rows, counts, cuts, open_end=False):
    """One recording fed in runs cut at ``cuts`` (ascending frames inside it), one segment per run: step(rows, counts, segments
    (1, 4)) -> ((rows', counts'), ids, status) per run, the carry kept by ``step``.  -> the runs' results concatenated on the
    emitted axis: (rows, counts, ids, status)."""
    T = len(counts)
    bounds = [0] + list(cuts) + [T]
    offs = np.concatenate([[0], np.cumsum(counts)])
    out_rows, out_counts, out_ids, status, emitted = [], [], [], 0, 0
    for k, (lo, hi) in enumerate(zip(bounds, bounds[1:])):
        seg = np.asarray([[0, hi - lo, int(k > 0), int(hi < T or open_end)]], dtype=np.int32)
        (r, c), i, st = step(rows[offs[lo]:offs[hi]], counts[lo:hi], seg)
        r = r.copy()
        r[:, 0] += emitted
        emitted += len(c)
        out_rows.append(r), out_counts.append(c), out_ids.append(i)
        status |= st
    return np.concatenate(out_rows), np.concatenate(out_counts), np.concatenate(out_ids), status


def host_step(C, max_gap, min_len, smooth, hold, trace=None):
    """``feed``'s step on the host definition; trace sums what every call counted."""
    state = {"carry": None}

    def step(rows, counts, seg):
        seen = {}
        got, ids, status, state["carry"] = track_run(rows, counts, seg, C, GATE, max_gap, min_len, smooth, hold, state["carry"],
                                                     trace=seen)
        if trace is not None:
            for k, v in seen.items():
                trace[k] = trace.get(k, 0) + v
        return got, ids, status
    return step


def cut_sets(T, seed, n_random=6):
    """Every single cut, and random partitions that hold one-frame runs."""
    rng = np.random.default_rng(seed)
    sets = [[t] for t in range(1, T)]
    for _ in range(n_random if T > 2 else 0):
        cuts = set(rng.choice(np.arange(1, T), size=int(rng.integers(2, min(T - 1, 12) + 1)), replace=False).tolist())
        t = int(rng.integers(1, T - 1))
        cuts |= {t, t + 1}                                                           # a run of one frame
        sets.append(sorted(c for c in cuts if 0 < c < T))
    return sets


def same(got, want):
    (rows, counts), ids, status = want
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    assert np.array_equal(got[1], counts) and np.array_equal(got[2], ids) and got[3] == status
    assert got[0].tobytes() == rows.tobytes()


# ------------------------------------------------------------------------------------------------------------ the hold bound
def test_track_hold_is_the_reach_of_the_parameters():
    assert track_hold(2, 3) == 7 and track_hold(0, 1) == 0 and track_hold(3, 1) == 3 and track_hold(3, 5) == 17
    for g, m in GRID:
        assert track_hold(g, m) == (g if m == 1 else (m - 1) * (g + 1) + 1)
    for bad in ((-1, 1), (0, 0)):
        with pytest.raises(ValueError):
            track_hold(*bad)


@pytest.fixture(scope="module")
def recording():
    return stream_case(SEED, T_STREAM, C_STREAM)


@pytest.mark.parametrize("max_gap,min_len", GRID)
def test_any_cut_gives_the_whole_recordings_bits(recording, max_gap, min_len):
    rows, counts = recording
    smooth, hold = SMOOTH[min_len], track_hold(max_gap, min_len)
    want = whole(rows, counts, C_STREAM, max_gap, min_len, smooth)
    assert len(want[0][0]) > 0
    trace = {}
    for cuts in cut_sets(T_STREAM, 7 + max_gap * 4 + min_len):
        same(feed(host_step(C_STREAM, max_gap, min_len, smooth, hold, trace), rows, counts, cuts), want)
    # the inputs reach the carried paths: a fill into a frame held by an earlier call, an erasure of such a frame
    if max_gap > 0:
        assert trace["carried_fills"] > 0
    if min_len > 1:
        assert trace["carried_prunes"] > 0
    # a larger hold (the scorer's block) changes nothing
    for cuts in ([1], [64], [9, 10, 30]):
        same(feed(host_step(C_STREAM, max_gap, min_len, smooth, -(-hold // 10) * 10), rows, counts, cuts), want)


def test_the_recording_holds_what_the_issue_names(recording):
    rows, counts = recording
    frame = np.repeat(np.arange(T_STREAM), counts)
    per = np.bincount(frame * C_STREAM + rows[:, 1].astype(int), minlength=T_STREAM * C_STREAM)
    assert (per == 64).any() and (per == 65).any()
    with np.errstate(all="ignore"):
        norm = np.sqrt((rows[:, 2:] * rows[:, 2:]).sum(1))
    assert (norm == 0).any() and np.isnan(norm).any() and T_STREAM > 64
    trace = {}
    whole(rows, counts, C_STREAM, 2, 3, 0.5, trace=trace)
    assert trace["filled"] > 0 and trace["pruned"] > 0 and trace["pruned_fills"] > 0 and trace["reused"] > 0


def planted_reach(max_gap, min_len):
    """A track whose closing write reaches back exactly H frames: min_len - 1 hits max_gap + 1 frames apart, erased when it
    expires (min_len > 1); two hits max_gap + 1 frames apart, the gap between them filled (min_len 1)."""
    d = direction(15, 5)
    hits = [k * (max_gap + 1) for k in range(max(2, min_len) - 1 + (min_len == 1))]
    T = hits[-1] + max_gap + 3
    return pack([(f, 0, d) for f in hits], T)


@pytest.mark.parametrize("max_gap,min_len", [gm for gm in GRID if track_hold(*gm) > 0])
def test_one_frame_less_hold_trips_the_guard(max_gap, min_len):
    rows, counts = planted_reach(max_gap, min_len)
    H = track_hold(max_gap, min_len)
    want = whole(rows, counts, 1, max_gap, min_len, 1.0)
    T = len(counts)
    for cuts in ([], [1], [T - 1], [T // 2]):
        same(feed(host_step(1, max_gap, min_len, 1.0, H), rows, counts, [c for c in cuts if 0 < c < T]), want)
        with pytest.raises(AssertionError, match="hold"):
            feed(host_step(1, max_gap, min_len, 1.0, H - 1), rows, counts, [c for c in cuts if 0 < c < T])


def test_arguments_are_checked():
    rows, counts = planted_reach(2, 3)
    T = len(counts)
    ok = dict(nb_classes=1, gate_deg=GATE, max_gap=2, min_len=3, smooth=0.5, hold=7, carry=None)
    track_run(rows, counts, [[0, T, 0, 0]], **ok)
    for seg in ([[0, T - 1, 0, 0]], [[1, T - 1, 0, 0]], [[0, 2, 0, 0], [3, T - 3, 0, 0]], [[0, 2, 0, 0], [1, T - 1, 0, 0]],
                [[0, 2, 0, 1], [2, T - 2, 0, 0]], [[0, 2, 0, 0], [2, T - 2, 1, 0]], [[0, 0, 0, 0], [0, T, 0, 0]],
                [[0, T, 2, 0]], np.zeros((0, 4))):
        with pytest.raises(ValueError):
            track_run(rows, counts, seg, **ok)
    for kw in (dict(hold=-1), dict(max_gap=-1), dict(min_len=0), dict(smooth=0.0), dict(gate_deg=90.0)):
        with pytest.raises(ValueError):
            track_run(rows, counts, [[0, T, 0, 0]], **dict(ok, **kw))
    *_, carry = track_run(rows, counts, [[0, T, 0, 1]], **ok)
    assert carry["walked"] == T and carry["held"] == 7
    with pytest.raises(ValueError):
        track_run(rows, counts, [[0, T, 1, 0]], **dict(ok, hold=10, carry=carry))
    # a closed last segment leaves an empty carry, and continuing from it is starting fresh
    *_, carry = track_run(rows, counts, [[0, T, 0, 0]], **ok)
    assert carry["walked"] == 0 and carry["held"] == 0 and not carry["cells"]
    fresh = track_run(rows, counts, [[0, T, 0, 0]], **ok)
    again = track_run(rows, counts, [[0, T, 1, 0]], **dict(ok, carry=carry))
    assert again[0][0].tobytes() == fresh[0][0].tobytes() and np.array_equal(again[1], fresh[1])


# -------------------------------------------------------------------------------- runs that hold several recordings: the plan
LENGTHS = (1, 9, 0, 63, 64, 3, 65, 130, 2, 0)                    # label frames per recording, two of them without any


def stream_of_recordings(seed, lengths, C):
    """The recordings' rows (``stream_case`` each) laid end to end -> (rows, counts, frame_start, per recording (rows, counts))."""
    parts = [stream_case(seed + r, n, C) if n else (np.zeros((0, 5), dtype=F32), np.zeros(0, dtype=np.int32))
             for r, n in enumerate(lengths)]
    start = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]).astype(np.int32), start, parts)


def run_plan(step, rows, counts, plan, bounds):
    """Every pass's frames through step(rows, counts, segments) -> per pass ((rows', counts'), ids, status)."""
    offs = np.concatenate([[0], np.cumsum(counts)])
    return [step(rows[offs[lo]:offs[hi]], counts[lo:hi], plan["segments_host"][p])
            for p, (lo, hi) in enumerate(zip(bounds, bounds[1:]))]


def by_recording(results, plan, start):
    """The passes' emitted rows put on every recording's own axis -> per recording (rows, counts, ids), and the status."""
    n = len(start) - 1
    rows, ids, status = [[] for _ in range(n)], [[] for _ in range(n)], 0
    counts = [np.zeros(int(start[r + 1] - start[r]), dtype=np.int32) for r in range(n)]
    for p, ((r_p, c_p), i_p, st) in enumerate(results):
        status |= st
        assert len(c_p) == plan["pass_frames"][p]
        ends = np.cumsum(c_p)
        for f in np.flatnonzero(c_p).tolist():
            g = plan["pass_base"][p] + f
            r = int(np.searchsorted(start, g, "right")) - 1
            part = r_p[ends[f] - c_p[f]:ends[f]].copy()
            assert (part[:, 0] == f).all()
            part[:, 0] = g - start[r]
            rows[r].append(part), ids[r].append(i_p[ends[f] - c_p[f]:ends[f]])
            counts[r][g - start[r]] = c_p[f]
    return [(np.concatenate(rows[r]) if rows[r] else np.zeros((0, 5), dtype=F32), counts[r],
             np.concatenate(ids[r]) if ids[r] else np.zeros(0, dtype=np.int32)) for r in range(n)], status


def pass_bound_sets(total, seed):
    rng = np.random.default_rng(seed)
    sets = [[0, total], list(range(0, total, 40)) + [total], list(range(0, total, 7)) + [total]]
    for _ in range(3):
        cuts = rng.choice(np.arange(1, total), size=int(rng.integers(3, 15)), replace=False)
        sets.append([0] + sorted(cuts.tolist()) + [total])
    return sets


@pytest.mark.parametrize("max_gap,min_len,smooth,block", [(0, 1, 1.0, 1), (2, 3, 0.5, 1), (2, 3, 0.5, 10), (3, 5, 0.5, 1)])
def test_runs_of_several_recordings_give_every_recordings_bits(max_gap, min_len, smooth, block):
    C = 3
    rows, counts, start, parts = stream_of_recordings(300, LENGTHS, C)
    hold = -(-track_hold(max_gap, min_len) // block) * block
    want, want_status = [], 0
    for r, (r_rows, r_counts) in enumerate(parts):
        if not len(r_counts):
            want.append(None)
            continue
        (w_rows, w_counts), w_ids, st = whole(r_rows, r_counts, C, max_gap, min_len, smooth)
        want.append((w_rows, w_counts, w_ids))
        want_status |= st
    several = 0
    for bounds in pass_bound_sets(int(start[-1]), 11):
        plan = plan_track(start, bounds, hold)
        several += sum(len(s) > 2 and s[0, 2] == 1 and s[-1, 3] == 1 for s in plan["segments_host"])
        got, status = by_recording(run_plan(host_step(C, max_gap, min_len, smooth, hold), rows, counts, plan, bounds), plan, start)
        assert status == want_status
        for r, w in enumerate(want):
            if w is None:
                assert len(got[r][1]) == 0
                continue
            assert got[r][0].tobytes() == w[0].tobytes() and np.array_equal(got[r][1], w[1]) and np.array_equal(got[r][2], w[2])
    assert several > 0                       # closed segments between a continuing and an open one, in one run


# ---------------------------------------------------------------------------------------------------------------- the plan
def test_the_plan_moves_inner_bounds_back_by_the_hold_and_clamps():
    start = np.asarray([0, 4, 4, 104, 110, 330])                 # recordings of 4, 0, 100, 6 and 220 frames
    bounds = [0, 50, 106, 112, 115, 300, 330]
    plan = plan_track(start, bounds, 10)
    # 50: inside recording 2 -> 40; 106: inside recording 3 (6 frames, starts at 104) -> clamped to 104; 112 and 115: inside
    # recording 4 (starts at 110) -> both clamped to 110: the pass [112, 115) emits nothing; 300 -> 290
    assert plan["bounds"].tolist() == [0, 40, 104, 110, 110, 290, 330] and plan["hold"] == 10
    assert plan["pass_base"] == [0, 40, 104, 110, 110, 290] and plan["pass_frames"] == [40, 64, 6, 0, 180, 40]
    assert (np.diff(plan["bounds"]) >= 0).all()
    seg = [s.tolist() for s in plan["segments_host"]]
    assert seg[0] == [[0, 4, 0, 0], [4, 46, 0, 1]]                # the recording without a frame has no row
    assert seg[1] == [[0, 54, 1, 0], [54, 2, 0, 1]] and seg[2] == [[0, 4, 1, 0], [4, 2, 0, 1]]
    assert seg[3] == [[0, 3, 1, 1]] and seg[4] == [[0, 185, 1, 1]] and seg[5] == [[0, 30, 1, 0]]
    assert all(s.dtype == np.int32 for s in plan["segments_host"])
    # what a pass emits is what track_run emits: the held frames in, the run, the newly held frames out
    held = 0
    for p, s in enumerate(plan["segments_host"]):
        n_run = bounds[p + 1] - bounds[p]
        walked = (bounds[p] - int(start[np.searchsorted(start, bounds[p], "right") - 1])) if s[0][2] else 0
        assert held == min(10, walked)
        out = min(10, (walked if len(s) == 1 else 0) + int(s[-1][1])) if s[-1][3] else 0
        assert plan["pass_frames"][p] == held + n_run - out
        held = out
    assert plan_track(start, bounds, 0)["bounds"].tolist() == bounds
    for bad in ([0, 50], [1, 330], [0, 50, 50, 330], [0, 330, 400]):
        with pytest.raises(ValueError):
            plan_track(start, bad, 10)
    with pytest.raises(ValueError):
        plan_track(start, bounds, -1)


class _Plan(_WindowCorpus):
    def __init__(self, label_frames, pass_bounds, hold_block):
        self.frame_start = np.concatenate([[0], np.cumsum(label_frames)]).astype(np.int64)
        self.pass_base, self.hold_block, self.device = list(pass_bounds[:-1]), hold_block, "cpu"


def test_the_corpus_plan_rounds_the_hold_to_the_scorers_block_and_the_scorer_finds_every_recordings_end():
    opts = {"gate_deg": 20.0, "max_gap": 2, "min_len": 3, "smooth": 0.5}
    label_frames = [30, 0, 500, 7, 0, 200, 0]                    # a recording shorter than D, recordings without a frame
    bounds = [0, 30, 190, 350, 530, 537, 697, 737]               # inside a recording: whole blocks of 10 from its start
    plan = _Plan(label_frames, bounds, 10).track_plan(opts)
    assert plan["hold"] == 10 and _Plan(label_frames, bounds, 1).track_plan(opts)["hold"] == 7
    assert _Plan(label_frames, bounds, 10).track_plan(dict(opts, max_gap=3, min_len=5))["hold"] == 20
    assert _Plan(label_frames, bounds, 10).track_plan(dict(opts, max_gap=0, min_len=1))["hold"] == 0
    corpus = _Plan(label_frames, bounds, 10)
    assert corpus.track_plan(opts) is corpus.track_plan(dict(opts))                  # built once
    assert [tuple(t.shape) for t in plan["segments"]] == [s.shape for s in plan["segments_host"]]
    start = np.concatenate([[0], np.cumsum(label_frames)])
    e = plan["bounds"]
    assert e.tolist() == [0, 30, 180, 340, 530, 537, 687, 737]
    for x in e.tolist():                                         # block-aligned on the recording's own axis, or its end
        r = int(np.searchsorted(start, x, "right")) - 1
        assert x in start or (x - start[r]) % 10 == 0
    runs = run_segments(label_frames, sorted(set(e.tolist())))
    last = np.concatenate([s[s[:, 4] == 1, 0] for s in runs])
    assert sorted(last.tolist()) == list(range(len(label_frames)))                   # exactly one last row each
    for s in runs:
        inner = s[(s[:, 4] == 0)]
        assert ((inner[:, 1] + inner[:, 3]) % 10 == 0).all() and (s[:, 1] % 10 == 0).all()
    # a pass that emits nothing drops out of the scorer's runs
    plan = plan_track(start, [0, 30, 33, 36, 737], 10)
    assert plan["pass_frames"] == [30, 0, 0, 707] and sorted(set(plan["bounds"].tolist())) == [0, 30, 737]


# -------------------------------------------------------------------------------------------------------------------- ABI
def test_the_abi_declares_the_carried_entry_points():
    from adyolo_amd import ops, postprocess, test as atest
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adyolo_hip.h")).read(), flags=re.S)
    assert "#define ADYOLO_ABI_VERSION 4" in hdr
    lib = _lib.load()
    I, L, F, P = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    ctype = {"int": I, "long": L, "float": F}
    for name in ("adyolo_track_carry_words", "adyolo_track_run_workspace_words", "adyolo_track_run"):
        m = re.search(r"\b(long|int)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        args = [P if "*" in a else ctype[a.split()[-2]] for a in m.group(2).split(",")]
        assert _lib.SIGNATURES[name] == (ctype[m.group(1)], args), name
        assert getattr(lib, name) is not None
    assert lib.adyolo_track_carry_words(0, 7) == 0 and lib.adyolo_track_carry_words(3, -1) == 0
    assert lib.adyolo_track_carry_words(3, 0) == 3 * (4 + 8 * 8)                     # heads and slots, no held frame
    assert lib.adyolo_track_carry_words(13, 10) == 13 * (4 + 8 * 8) + 10 * 13 * 8 * 4
    assert lib.adyolo_track_run_workspace_words(0, 3, 7) == 0 and lib.adyolo_track_run_workspace_words(5, 3, -1) == 0
    assert lib.adyolo_track_run_workspace_words(10, 3, 7) >= 17 * 3 * 8 * 4 + 10 * 3 * 3 * 64 + lib.adyolo_track_carry_words(3, 7)
    for fn in (ops.track_run, ops.track_run_buffers, ops.track_carry, postprocess.LabelPostProcessor.track_device_run,
               postprocess.track_run, postprocess.track_hold, atest._RunTracker.reset):
        assert callable(fn)
    for fn in (atest.test_epoch_windows, atest.sweep_conf_thresh_windows, atest.infer_epoch_corpus):
        assert inspect.signature(fn).parameters["tracking"].default is None and "Tracking" in fn.__doc__
        assert "track_run" in fn.__doc__
    assert "tracking" not in inspect.signature(atest.test_epoch_audio).parameters
