"""CPU: tracks across frames -- the host definition ``postprocess.track_rows`` on hand-built clips and at each of its edge
rules, the configuration keys (``augmentations.track_options``), the CSV writer's track column and the C ABI's declarations.
``random_tracks`` is the generator the GPU test (test_gpu_track.py) feeds to the kernels; here the host definition runs on it."""
import math
import os
import re

import numpy as np
import pytest

import adyolo_amd  # noqa: F401
from adyolo_amd import _lib
from adyolo_amd.augmentations import track_options
from adyolo_amd.postprocess import (TRACK_BAD_ROWS, TRACK_BAD_VECTOR, TRACK_DET_OVERFLOW, TRACK_MAX_DET, TRACK_SLOT_OVERFLOW,
                                    TRACK_SLOTS, group_rows, track_cos, track_groups, track_rows, write_seld_output_file)

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def direction(az, el):
    a, e = math.radians(az), math.radians(el)
    return np.array([math.cos(a) * math.cos(e), math.sin(a) * math.cos(e), math.sin(e)])


def angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return math.degrees(math.acos(max(-1.0, min(1.0, float(a @ b) / float(np.linalg.norm(a) * np.linalg.norm(b))))))


def pack(cells, n_frames):
    """[(frame, class, vector), ...] in any frame order (the order within a frame is kept) -> (rows (N, 5) float32, counts)."""
    cells = sorted(cells, key=lambda r: r[0])
    rows = np.asarray([[f, c] + list(v) for f, c, v in cells], dtype=F32).reshape(-1, 5)
    counts = np.bincount([r[0] for r in cells], minlength=n_frames).astype(np.int32)
    return rows, counts


def run(cells, n_frames, n_clips=1, C=2, gate=20.0, max_gap=2, min_len=3, smooth=0.5, trace=None):
    rows, counts = pack(cells, n_frames)
    (out, out_counts), ids, status = track_rows(rows, counts, n_clips, C, gate, max_gap, min_len, smooth, trace=trace)
    assert out.dtype == np.float32 and out.shape == (len(ids), 5) and ids.dtype == np.int32
    assert out_counts.dtype == np.int32 and out_counts.shape == counts.shape and out_counts.sum() == len(out)
    assert np.array_equal(out[:, 0], np.repeat(np.arange(n_frames), out_counts))     # the frame column: the counts' axis
    return out, ids, status


def cells_of(out):
    return sorted((int(r[0]), int(r[1])) for r in out)


# --------------------------------------------------------------------------------------------------------- the semantics
def test_flicker_is_repaired_and_false_alarms_are_dropped_on_a_hand_built_clip():
    T, max_gap = 50, 2
    src = {"a": (0, direction(30, 10), range(2, 45)), "b": (0, direction(-120, -20), range(10, 40)),
           "c": (1, direction(80, 40), range(5, 30))}
    short, long_ = set(range(20, 20 + max_gap)), set(range(30, 30 + max_gap + 1))    # dropouts of source a
    cells, clean = [], {}
    for name, (cls, d, frames) in src.items():
        for f in frames:
            clean[(f, cls, name)] = d
            if name == "a" and (f in short or f in long_):
                continue
            if name == "c" and f in (12, 13):
                continue
            cells.append((f, cls, d * (1.0 + 0.1 * (f % 3))))                        # any length: the stage normalises
    for f, cls, az in ((1, 0, 170), (15, 1, -60), (33, 0, 100), (47, 1, -150), (48, 0, -30)):
        cells.append((f, cls, direction(az, -50)))                                   # lone false alarms, far from everything
    out, ids, status = run(cells, T, max_gap=max_gap)
    assert status == 0
    want = sorted((f, c) for (f, c, n) in clean if not (n == "a" and f in long_))    # the long dropout stays a hole
    assert cells_of(out) == want
    by_source = {}
    for r, tid in zip(out, ids):
        f, c = int(r[0]), int(r[1])
        near = [n for (ff, cc, n), d in clean.items() if ff == f and cc == c and angle_deg(d, r[2:5]) < 1.0]
        assert len(near) == 1, (f, c)
        assert np.abs(r[2:5] - clean[(f, c, near[0])].astype(F32)).max() <= 1e-6     # a few float32 ulps of normalisation
        by_source.setdefault(near[0], {}).setdefault("late" if near[0] == "a" and f > 31 else "early", set()).add(int(tid))
    # one id per source, in opening order within the class, the pruned false alarm of frame 1 counted (it was id 0)
    assert by_source["b"] == {"early": {2}} and by_source["c"] == {"early": {0}}
    assert by_source["a"] == {"early": {1}, "late": {3}}                             # the long dropout splits the track


def test_a_filled_direction_of_a_moving_source_lies_between_its_hits():
    a, b = direction(0, 0), direction(12, 0)
    cells = [(0, 0, direction(-4, 0)), (1, 0, a), (4, 0, b), (5, 0, direction(16, 0))]
    out, ids, status = run(cells, 6, smooth=1.0, min_len=1)
    assert status == 0 and cells_of(out) == [(f, 0) for f in range(6)] and set(ids.tolist()) == {0}
    for f in (2, 3):
        v = out[f, 2:5]
        assert abs(np.linalg.norm(v.astype(np.float64)) - 1) < 1e-6
        assert abs(angle_deg(a, v) + angle_deg(v, b) - 12) < 1e-3 and 0 < angle_deg(a, v) < 12
    assert angle_deg(a, out[2, 2:5]) < angle_deg(a, out[3, 2:5])


# -------------------------------------------------------------------------------------------------------- the edge rules
def test_min_len_keeps_exactly_min_len_hits_and_prunes_one_fewer_with_its_fills():
    d = direction(10, 10)
    trace = {}
    out, ids, _ = run([(0, 0, d), (2, 0, d), (4, 0, d)], 8, min_len=3, trace=trace)
    assert cells_of(out) == [(f, 0) for f in range(5)] and trace["pruned"] == 0 and trace["filled"] == 2
    out, ids, _ = run([(0, 0, d), (2, 0, d)], 8, min_len=3, trace=trace)
    assert len(out) == 0 and trace["pruned"] == 1 and trace["pruned_fills"] == 1


def test_a_gap_of_max_gap_is_bridged_and_one_frame_more_is_not():
    d = direction(-40, 5)
    for max_gap in (0, 1, 3):
        out, ids, _ = run([(0, 0, d), (max_gap + 1, 0, d)], 12, max_gap=max_gap, min_len=1)
        assert cells_of(out) == [(f, 0) for f in range(max_gap + 2)] and set(ids.tolist()) == {0}
        out, ids, _ = run([(0, 0, d), (max_gap + 2, 0, d)], 12, max_gap=max_gap, min_len=1)
        assert cells_of(out) == [(0, 0), (max_gap + 2, 0)] and ids.tolist() == [0, 1]


def test_the_ninth_simultaneous_direction_is_dropped():
    dirs = [direction(40 * k, 0) for k in range(9)]
    out, ids, status = run([(0, 0, d) for d in dirs], 1, C=1, min_len=1)
    assert status == TRACK_SLOT_OVERFLOW and len(out) == TRACK_SLOTS and ids.tolist() == list(range(8))
    for k in range(8):
        assert angle_deg(out[k, 2:5], dirs[k]) < 1e-3                               # the ninth in row order is the one missing


def test_the_65th_row_of_a_frame_and_class_is_not_considered():
    d = direction(5, 5)
    out, ids, status = run([(0, 0, d)] * TRACK_MAX_DET, 1, C=1, min_len=1)
    assert status == TRACK_SLOT_OVERFLOW and len(out) == 8                          # 64 rows: no detection overflow
    far = direction(-170, -60)
    out, ids, status = run([(0, 0, d)] * TRACK_MAX_DET + [(0, 0, far)], 1, C=1, min_len=1)
    assert status == TRACK_SLOT_OVERFLOW | TRACK_DET_OVERFLOW
    assert all(angle_deg(r[2:5], d) < 1e-3 for r in out)
    out, ids, status = run([(0, 0, far)] + [(0, 0, d)] * TRACK_MAX_DET, 1, C=1, min_len=1)
    assert status & TRACK_DET_OVERFLOW and angle_deg(out[0, 2:5], far) < 1e-3


def test_zero_and_nan_vectors_are_dropped():
    d = direction(0, 30)
    out, ids, status = run([(0, 0, np.zeros(3)), (0, 0, d), (0, 0, np.array([np.nan, 0, 1])), (0, 1, np.array([np.inf, 0, 0]))],
                           1, min_len=1)
    assert status == TRACK_BAD_VECTOR and cells_of(out) == [(0, 0)] and ids.tolist() == [0]


def test_a_slot_is_closed_and_reused_in_the_same_frame():
    a, b = direction(0, 0), direction(180, 0)
    trace = {}
    out, ids, status = run([(0, 0, a), (2, 0, b)], 4, max_gap=0, min_len=1, trace=trace)
    assert trace["reused"] == 1 and cells_of(out) == [(0, 0), (2, 0)] and ids.tolist() == [0, 1]
    out, ids, status = run([(0, 0, a), (1, 0, b)], 4, max_gap=0, min_len=1, trace=trace)
    assert trace["reused"] == 0 and ids.tolist() == [0, 1]                           # (frame 1: slot 0 is still open)


def test_state_does_not_cross_a_clip_boundary():
    d = direction(77, -7)
    out, ids, status = run([(3, 0, d), (4, 0, d)], 8, n_clips=2, min_len=1)
    assert cells_of(out) == [(3, 0), (4, 0)] and ids.tolist() == [0, 0]
    out, ids, status = run([(3, 0, d), (4, 0, d)], 8, n_clips=2, min_len=2)         # ... so neither reaches two hits
    assert len(out) == 0
    out, ids, status = run([(3, 0, d), (4, 0, d)], 8, n_clips=1, min_len=2)
    assert ids.tolist() == [0, 0] and len(out) == 2


def test_the_lower_slot_takes_a_detection_equidistant_from_two_tracks():
    lo, hi, mid = np.array([1.0, 0.25, 0.0]), np.array([1.0, -0.25, 0.0]), np.array([1.0, 0.0, 0.0])
    for first, second in ((lo, hi), (hi, lo)):
        out, ids, status = run([(0, 0, first), (0, 0, second), (1, 0, mid)], 2, min_len=1, smooth=1.0)
        assert len(out) == 3 and ids.tolist() == [0, 1, 0]                           # the same dot to both: slot 0 wins
    # the largest dot wins over the slot order
    out, ids, status = run([(0, 0, lo), (0, 0, hi), (1, 0, np.array([1.0, -0.2, 0.0]))], 2, min_len=1)
    assert ids.tolist() == [0, 1, 1]


def test_identity_parameters_return_the_input_cells_normalised():
    rng = np.random.default_rng(5)
    cells = [(f, int(rng.integers(3)), rng.normal(size=3) * 3) for f in range(12) for _ in range(int(rng.integers(0, 4)))]
    out, ids, status = run(cells, 12, C=3, max_gap=0, min_len=1, smooth=1.0)
    assert status == 0 and cells_of(out) == sorted((f, c) for f, c, _ in cells)
    want = sorted([f, c] + (v / np.linalg.norm(v)).tolist() for f, c, v in cells)
    for r in out:                                                                   # every input vector comes back, unit length
        k = next(i for i, w in enumerate(want) if w[0] == r[0] and w[1] == r[1] and np.abs(np.asarray(w[2:]) - r[2:5]).max() < 1e-6)
        want.pop(k)
    assert not want


def test_a_track_open_at_the_clips_end_is_closed_and_pruned_like_any_other():
    d = direction(20, 20)
    out, ids, status = run([(6, 0, d), (7, 0, d)], 8, min_len=3)
    assert len(out) == 0
    out, ids, status = run([(5, 0, d), (6, 0, d), (7, 0, d)], 8, min_len=3)
    assert cells_of(out) == [(5, 0), (6, 0), (7, 0)]


def test_bad_rows_are_reported_and_skipped():
    d = direction(1, 2)
    rows = np.asarray([[0, 0] + d.tolist(), [0, 5] + d.tolist(), [1, 0.5] + d.tolist(), [1, 1] + d.tolist()], dtype=F32)
    (out, oc), ids, status = track_rows(rows, [2, 2], 1, 2, 20.0, 0, 1, 1.0)
    assert status == TRACK_BAD_ROWS and cells_of(out) == [(0, 0), (1, 1)]
    for counts in ([2, 3], [-1, 2], [5, 0]):
        (out, oc), ids, status = track_rows(rows, counts, 1, 2, 20.0, 0, 1, 1.0)
        assert status & TRACK_BAD_ROWS
    for kw in (dict(gate_deg=0.0), dict(gate_deg=90.0), dict(max_gap=-1), dict(min_len=0), dict(smooth=0.0), dict(smooth=1.5)):
        args = dict(gate_deg=20.0, max_gap=2, min_len=3, smooth=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            track_rows(rows, [2, 2], 1, 2, **args)
    assert track_cos(20.0) == F32(math.cos(math.radians(20.0)))


# ------------------------------------------------------------------------------------------------------ options and writer
def test_track_options_parse_their_keys():
    assert track_options({}) is None and track_options({"test_config": {"track": False}}) is None
    assert track_options({"test_config": {"track_max_gap": 4}}) is None               # only ``track: true`` switches it on
    assert track_options({"test_config": {"track": True}}) == {"gate_deg": 20.0, "max_gap": 2, "min_len": 3, "smooth": 0.5}
    got = track_options({"train_config": {"track": True, "track_gate_deg": 10, "track_max_gap": 0, "track_min_len": 1,
                                          "track_smooth": 1}})
    assert got == {"gate_deg": 10.0, "max_gap": 0, "min_len": 1, "smooth": 1.0}      # the train_config fallback
    both = {"test_config": {"track": True, "track_min_len": 5}, "train_config": {"track": False, "track_min_len": 9,
                                                                                 "track_max_gap": 7}}
    assert track_options(both) == {"gate_deg": 20.0, "max_gap": 7, "min_len": 5, "smooth": 0.5}
    assert track_options({"test_config": {"track": False}, "train_config": {"track": True}}) is None
    for key, bad in (("track", 1), ("track", "yes"), ("track_gate_deg", 0), ("track_gate_deg", 90), ("track_gate_deg", "20"),
                     ("track_gate_deg", True), ("track_gate_deg", float("nan")), ("track_max_gap", -1), ("track_max_gap", 1.5),
                     ("track_max_gap", True), ("track_min_len", 0), ("track_min_len", 2.0), ("track_smooth", 0),
                     ("track_smooth", 1.01), ("track_smooth", "0.5"), ("track_smooth", float("inf"))):
        cfg = {"track": True}
        cfg[key] = bad
        with pytest.raises(ValueError, match=r"test_config\.%s\b" % key):
            track_options({"test_config": cfg})


def test_the_writer_keeps_its_bytes_and_writes_ids_that_reload_and_score_the_same(tmp_path):
    from adyolo_amd.seld_metrics import ComputeSELDResults, load_output_format_file
    cells = [(f, 0, direction(30, 10)) for f in range(0, 9)] + [(f, 1, direction(-90, 0)) for f in range(3, 12)] \
        + [(f, 0, direction(120, -30)) for f in range(5, 14)]
    rows, counts = pack(cells, 20)
    (out, oc), ids, status = track_rows(rows, counts, 1, 2, 20.0, 2, 3, 0.5)
    output, tracks = group_rows(out, oc)[0], track_groups(ids, oc)[0]
    assert list(output) == list(tracks) and all(len(output[f]) == len(tracks[f]) for f in output)
    plain, zero, tracked = (str(tmp_path / n) for n in ("plain", "zero", "tracked"))
    for d in (plain, zero, tracked):
        os.makedirs(d)
    write_seld_output_file(os.path.join(plain, "a.csv"), output)
    write_seld_output_file(os.path.join(zero, "a.csv"), output, tracks=None)
    write_seld_output_file(os.path.join(tracked, "a.csv"), output, tracks)
    want = "".join("{},{},{},{},{},{}\n".format(int(f), int(c), 0, float(x), float(y), float(z))
                   for f in output for c, x, y, z in output[f])                      # the writer as it was
    assert open(os.path.join(plain, "a.csv")).read() == want == open(os.path.join(zero, "a.csv")).read()
    back = load_output_format_file(os.path.join(tracked, "a.csv"))
    assert [r[1] for f in back for r in back[f]] == ids.tolist() and set(ids.tolist()) == {0, 1}
    assert [r[0] for f in back for r in back[f]] == out[:, 1].astype(int).tolist()
    with pytest.raises(ValueError):
        write_seld_output_file(str(tmp_path / "b.csv"), output, {f: [] for f in output})
    ref = str(tmp_path / "ref")
    os.makedirs(ref)
    with open(os.path.join(ref, "a.csv"), "w") as f:
        for t in range(14):
            f.write("%d,0,0,30,10\n" % t)
            f.write("%d,1,0,-80,0\n" % t)
    prm = {"data_config": {"nb_classes": 2, "sr": 24000, "label_hop_len_s": 0.1}}
    a = ComputeSELDResults(prm, ref).get_SELD_Results(zero)
    b = ComputeSELDResults(prm, ref).get_SELD_Results(tracked)
    assert [float(v) for v in a[:5]] == [float(v) for v in b[:5]] and np.array_equal(np.asarray(a[5]), np.asarray(b[5]))


# -------------------------------------------------------------------------------------------------------------------- ABI
def test_the_abi_declares_the_entry_points_and_the_constants():
    from adyolo_amd import ops, postprocess, test as atest
    import ctypes
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adyolo_hip.h")).read(), flags=re.S)
    assert "#define ADYOLO_ABI_VERSION 4" in hdr
    lib = _lib.load()
    I, L, F, P = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    ctype = {"int": I, "long": L, "float": F}
    for name in ("adyolo_track_workspace_words", "adyolo_track_rows"):
        m = re.search(r"\b(long|int)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        args = [P if "*" in a else ctype[a.split()[-2]] for a in m.group(2).split(",")]
        assert _lib.SIGNATURES[name] == (ctype[m.group(1)], args), name
        assert getattr(lib, name) is not None
    for name, value in (("SLOTS", 8), ("MAX_DET", 64), ("DET_OVERFLOW", 1), ("SLOT_OVERFLOW", 2), ("BAD_VECTOR", 4),
                        ("BAD_ROWS", 8)):
        assert re.search(r"#define ADYOLO_TRACK_%s\s+%d\b" % (name, value), hdr), name
        assert getattr(postprocess, "TRACK_" + name) == value
    assert ops.TRACK_SLOTS == 8 and ops.TRACK_BAD_ROWS == 8 and [b for b, _ in ops.TRACK_STATUS] == [1, 2, 4, 8]
    assert lib.adyolo_track_workspace_words(0, 13) == 0 and lib.adyolo_track_workspace_words(5, 0) == 0
    assert lib.adyolo_track_workspace_words(10, 3) >= 10 * 3 * (8 * 4 + 3 * 64)       # the cell grid and the candidate lists
    assert callable(ops.track_rows) and callable(ops.track_buffers) and callable(ops.track_status_check)
    assert callable(postprocess.LabelPostProcessor.track_device_rows)
    import inspect
    for fn in (atest.test_epoch_corpus, atest.sweep_conf_thresh_corpus):
        assert inspect.signature(fn).parameters["track"].default is None
    for fn in (atest.test_epoch_windows, atest.sweep_conf_thresh_windows, atest.infer_epoch_corpus, atest.test_epoch_audio):
        assert "track" not in inspect.signature(fn).parameters and "Tracking" in fn.__doc__
    with pytest.warns(UserWarning):
        ops.track_status_check(1 | 2 | 4)
    with pytest.raises(_lib.AdyoloHipError):
        ops.track_status_check(8)
    ops.track_status_check(0)


# ------------------------------------------------------------------------------------- random cases (also for the GPU test)
def random_tracks(seed, n_clips, T, C):
    """Random selected rows of n_clips clips of T frames: persistent sources that drift slowly, with dropouts, jitter and false
    alarms, rows of any length, the rows of a frame in shuffled order.  Planted where the clip has room for them: a (frame,
    class) with exactly 64 rows and one with 65 (many more directions than slots), a zero and a NaN vector, an isolated pair
    of hits one frame apart (filled, then pruned when min_len > 2), pairs of lone detections 2, 4 and 7 frames apart (slot 0
    expires in the frame it is taken again, for max_gap 0, 2 and 5), whole 64-frame blocks without a row of one class and one
    direction on both sides of a clip boundary.
    -> {'rows' (N, 5) float32, 'counts' (n_clips * T,) int32, 'clean': [(frame, class, source, unit vector), ...] the sources'
    true cells}."""
    rng = np.random.default_rng(seed)

    def rand_dir():
        v = rng.normal(size=3)
        return v / np.linalg.norm(v)

    def turned(d, deg):
        v = d + math.tan(math.radians(deg)) * rand_dir()
        return v / np.linalg.norm(v)

    per_frame = [[] for _ in range(n_clips * T)]
    clean = []
    source = 0
    for clip in range(n_clips):
        for c in range(C):
            for _ in range(int(rng.choice([0, 1, 1, 2, 3]))):
                start = int(rng.integers(0, T))
                d, vel = rand_dir(), rand_dir()
                for t in range(start, min(T, start + int(rng.integers(1, max(2, T // 2))))):
                    d = turned(d + 0.01 * vel, 0.0)                                  # about half a degree a frame
                    clean.append((clip * T + t, c, source, d.astype(F32)))
                    if rng.random() > 0.2:
                        per_frame[clip * T + t].append([c] + (turned(d, 2.0) * rng.uniform(0.5, 2.0)).tolist())
                source += 1
            for t in np.flatnonzero(rng.random(T) < 0.04).tolist():
                per_frame[clip * T + t].append([c] + (rand_dir() * rng.uniform(0.5, 2.0)).tolist())
    def only(f, c, keep):
        per_frame[f] = [r for r in per_frame[f] if r[0] != c] + [[c] + v for v in keep]

    if T >= 30:                                  # class 0 of frames 2 .. 47 of clip 0 holds nothing but what is planted here
        for f in range(2, min(T, 48)):
            only(f, 0, [])
        only(2, 0, [[0.0, 0.0, 0.0], [float("nan"), 1.0, 0.0]])
        lone = direction(10, 60)
        plant = [(3, direction(0, 0)), (5, direction(90, 0)), (13, direction(180, 0)), (17, direction(270, 0)), (25, lone),
                 (27, lone)]
        if T >= 48:
            plant += [(36, direction(45, -60)), (43, direction(-135, -60))]
        for f, d in plant:
            only(f, 0, [d.tolist()])
    if T >= 60:                                  # a stretch nothing happens in
        for f in range(54, 60):
            per_frame[f] = []
    dense = [(0, TRACK_MAX_DET + 1)] if T < 3 else [(50 if T >= 60 else T - 4, TRACK_MAX_DET),
                                                    (51 if T >= 60 else T - 3, TRACK_MAX_DET + 1)]
    for f, n in dense:
        only(f, C - 1, [rand_dir().tolist() for _ in range(n)])
    if T >= 129 and C >= 3 and n_clips >= 2:     # 64-frame blocks of silence, with a detection in the first frame behind them
        for f in range(T, T + 64):
            only(f, 1, [])
        only(T + 64, 1, [rand_dir().tolist()])
        for f in range(57, 128):
            only(f, 2, [])
        only(128, 2, [rand_dir().tolist()])
    if n_clips >= 2:
        edge = rand_dir().tolist()
        for f in (T - 1, T):
            only(f, 0, [edge])
    rows = []
    for f, lst in enumerate(per_frame):
        for k in rng.permutation(len(lst)).tolist():
            rows.append([f] + lst[k])
    return {"rows": np.asarray(rows, dtype=F32).reshape(-1, 5),
            "counts": np.asarray([len(lst) for lst in per_frame], dtype=np.int32), "clean": clean}


TRACK_CONFIGS = ((1, 1, 1), (1, 70, 1), (3, 37, 13), (2, 129, 3))
TRACK_CORNERS = ((0, 1, 1.0), (2, 3, 0.5), (5, 8, 0.25))


def track_features(case, n_clips, T, C, max_gap, min_len, smooth):
    """What one random case exercises, from its inputs and the host definition's result and trace."""
    rows, counts = case["rows"], case["counts"]
    trace = {}
    (out, oc), ids, status = track_rows(rows, counts, n_clips, C, 20.0, max_gap, min_len, smooth, trace=trace)
    frame = np.repeat(np.arange(len(counts)), counts)
    per_cell = np.bincount((frame * C + rows[:, 1].astype(int)), minlength=len(counts) * C) if len(rows) else np.zeros(1, int)
    boundary = False
    for clip in range(1, n_clips):
        a, b = rows[frame == clip * T - 1], rows[frame == clip * T]
        boundary |= any(ra[1] == rb[1] and angle_deg(ra[2:], rb[2:]) < 1e-3 for ra in a for rb in b)
    # a 64-frame block of a (clip, class) without rows, behind a block without rows (or first): stepped over as a whole
    quiet = (per_cell.reshape(len(counts), C) if len(rows) else np.zeros((len(counts), C), int)).reshape(n_clips, T, C) == 0
    blocks = [quiet[:, b:b + 64].all(axis=1) for b in range(0, T, 64)]
    silent = any((blk & (blocks[i - 1] if i else True)).any() for i, blk in enumerate(blocks))
    return {"silent_block": bool(silent), "empty_frames": bool((counts == 0).any()), "rows_64": bool((per_cell == TRACK_MAX_DET).any()),
            "rows_65": bool((per_cell == TRACK_MAX_DET + 1).any()) and bool(status & TRACK_DET_OVERFLOW),
            "ninth_track": bool(status & TRACK_SLOT_OVERFLOW), "pruned_with_fills": trace["pruned_fills"] > 0,
            "slot_reuse": trace["reused"] > 0, "clip_boundary": bool(boundary), "bad_vector": bool(status & TRACK_BAD_VECTOR),
            "filled": trace["filled"] > 0, "rows_out": len(out) > 0}


def test_the_random_cases_reach_every_rule():
    seen = {}
    for n_clips, T, C in TRACK_CONFIGS:
        case = random_tracks(100 + T, n_clips, T, C)
        assert case["counts"].shape == (n_clips * T,) and case["counts"].sum() == len(case["rows"])
        for corner in TRACK_CORNERS:
            feat = track_features(case, n_clips, T, C, *corner)
            if corner[1] == 1:
                assert feat["rows_out"]
            for k, v in feat.items():
                seen[k] = seen.get(k, False) or v
            if T >= 30:
                assert feat["rows_64"] and feat["rows_65"] and feat["ninth_track"] and feat["bad_vector"]
                assert feat["slot_reuse"] or (T < 48 and corner[0] == 5), (T, corner)
                assert feat["pruned_with_fills"] == (corner[1] > 2), (T, corner)
            if T >= 60:
                assert feat["empty_frames"]
            if T >= 129:
                assert feat["silent_block"]
            if n_clips > 1:
                assert feat["clip_boundary"]
    assert all(seen.values()), seen
