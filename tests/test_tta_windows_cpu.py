"""CPU: what rotation test-time augmentation through windows rests on.  The view merge (``postprocess.merge_view_rows``) is
defined per (frame, class), so merging the views run by run -- at bounds that fall inside recordings, as the window passes'
do -- and laying the results end to end gives the bytes of one merge over the whole axis; and ``postprocess.track_run`` over
those merged runs, with the carry, gives ``postprocess.track_rows`` on each merged whole recording.  The two invariances
compose: merge, then link, run by run, is merge, then link, on whole recordings.  Last, the three windowed loops take ``tta=``."""
import inspect

import numpy as np
import pytest

import adyolo_amd  # noqa: F401
from adyolo_amd.corpus import plan_track
from adyolo_amd.postprocess import merge_view_rows, track_hold
from test_track_windows_cpu import by_recording, host_step, run_plan, whole
from test_tta_cpu import random_views, seen_by

F32 = np.float32
LENGTHS = (0, 12, 30, 45, 110)                     # label frames per recording: the MIXED split of the GPU tests
C, VIEWS, UNIFY = 3, [0, 5, 10], 15.0
START = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)              # 0, 0, 12, 42, 87, 197
TOTAL = int(START[-1])
# run bounds: the windowed passes' shape (a run ends inside the 45- and the 110-frame recording), one-frame runs, one run
BOUNDS = ([0, 42, 62, 102, 132, 162, TOTAL], [0, 5, 6, 7, 13, 41, 43, 86, 88, 196, TOTAL], [0, TOTAL])
CORNERS = ((0, 1, 1.0), (2, 3, 0.5), (3, 5, 0.5))  # (max_gap, min_len, smooth): the corners of test_gpu_track_windows.py


def moving_sources(seed, per_view):
    """Rows added to ``random_views``' (whose frames are drawn one by one, so that hardly anything links across them): in every
    recording three sources that drift a few degrees per frame and drop out for a frame or two now and then, each seen by
    most views with a jitter inside the merge's threshold -- tracks long enough to survive every corner's ``min_len``, with
    gaps to fill, across the run bounds.  Every view's rows of a frame stay in class order."""
    rs = np.random.RandomState(seed)
    frames = [[[] for _ in range(TOTAL)] for _ in VIEWS]
    for k, (rows, counts) in enumerate(per_view):
        offs = np.concatenate([[0], np.cumsum(counts)])
        for f in range(TOTAL):
            frames[k][f] = rows[offs[f]:offs[f + 1], 1:].tolist()

    def turned(d, deg):
        w = rs.randn(3)
        w -= (w @ d) * d
        w /= np.linalg.norm(w)
        t = np.radians(rs.uniform(0, deg))
        return np.cos(t) * d + np.sin(t) * w
    for r, n in enumerate(LENGTHS):
        for _ in range(3 if n else 0):
            cls, d = int(rs.randint(C)), rs.randn(3)
            d /= np.linalg.norm(d)
            for f in range(int(START[r]), int(START[r + 1])):
                d = turned(d, 4.0)
                if rs.rand() < 0.15:                                 # not seen by any view: a gap
                    continue
                for k, v in enumerate(VIEWS):
                    if rs.rand() < 0.9:
                        frames[k][f].append([float(cls)] + seen_by(v, turned(d, 3.0) * rs.uniform(0.6, 1.4)).tolist())
    out = []
    for k in range(len(VIEWS)):
        rows, counts = [], np.zeros(TOTAL, dtype=np.int32)
        for f in range(TOTAL):
            here = sorted(frames[k][f], key=lambda row: row[0])
            rows += [[float(f)] + row for row in here]
            counts[f] = len(here)
        out.append((np.asarray(rows, dtype=F32).reshape(-1, 5), counts))
    return out


@pytest.fixture(scope="module")
def views():
    per_view = moving_sources(78, random_views(77, TOTAL, C, VIEWS, UNIFY)[0])
    assert all(len(c) == TOTAL and int(c.sum()) == len(r) for r, c in per_view)
    return per_view


def _cut(per_view, lo, hi):
    """Frames [lo, hi) of every view's selection, the frame column counted from lo."""
    out = []
    for rows, counts in per_view:
        offs = np.concatenate([[0], np.cumsum(counts)])
        part = rows[offs[lo]:offs[hi]].copy()
        part[:, 0] -= lo
        out.append((part, counts[lo:hi].copy()))
    return out


def _merged_runs(per_view, bounds, min_views):
    """The views merged run by run -> (rows, counts) laid end to end on the whole axis, the status bits of all runs."""
    rows, counts, status = [], [], 0
    for lo, hi in zip(bounds, bounds[1:]):
        (r, c), st = merge_view_rows(_cut(per_view, lo, hi), VIEWS, UNIFY, min_views)
        assert r.dtype == np.float32 and c.dtype == np.int32 and len(c) == hi - lo
        r = r.copy()
        r[:, 0] += lo
        rows.append(r), counts.append(c)
        status |= st
    return np.concatenate(rows), np.concatenate(counts), status


@pytest.mark.parametrize("min_views", [1, 2, 3])
def test_the_merge_does_not_depend_on_where_the_axis_is_cut(views, min_views):
    (want_rows, want_counts), want_status = merge_view_rows(views, VIEWS, UNIFY, min_views)
    assert len(want_rows) > 0 and len(want_counts) == TOTAL
    for bounds in BOUNDS:
        assert any(b not in START.tolist() for b in bounds[1:-1]) or len(bounds) == 2      # cuts inside recordings
        rows, counts, status = _merged_runs(views, bounds, min_views)
        assert status == want_status
        assert np.array_equal(counts, want_counts) and rows.tobytes() == want_rows.tobytes()


@pytest.mark.parametrize("corner", CORNERS, ids=["identity", "defaults", "reach17"])
def test_merged_runs_tracked_with_the_carry_equal_merged_whole_recordings_tracked(views, corner):
    max_gap, min_len, smooth = corner
    (m_rows, m_counts), _ = merge_view_rows(views, VIEWS, UNIFY, 1)
    offs = np.concatenate([[0], np.cumsum(m_counts)])
    want, want_status, n_out = [], 0, 0
    for r, n in enumerate(LENGTHS):                                  # the definition: each merged recording whole
        if not n:
            want.append(None)
            continue
        lo, hi = int(START[r]), int(START[r + 1])
        rec_rows = m_rows[offs[lo]:offs[hi]].copy()
        rec_rows[:, 0] -= lo
        (w_rows, w_counts), w_ids, st = whole(rec_rows, m_counts[lo:hi], C, max_gap, min_len, smooth)
        want.append((w_rows, w_counts, w_ids))
        want_status |= st
        n_out += len(w_rows)
    assert n_out > 0
    for block in (1, 10):                                            # the hold as it is, and rounded up to the scorer's block
        hold = -(-track_hold(max_gap, min_len) // block) * block
        for bounds in BOUNDS:
            plan = plan_track(START, bounds, hold)
            rows, counts, _ = _merged_runs(views, bounds, 1)         # merged run by run, then linked run by run
            got, status = by_recording(run_plan(host_step(C, max_gap, min_len, smooth, hold), rows, counts, plan, bounds), plan,
                                       START)
            assert status == want_status
            for r, w in enumerate(want):
                if w is None:
                    assert len(got[r][1]) == 0
                    continue
                assert got[r][0].tobytes() == w[0].tobytes() and np.array_equal(got[r][1], w[1])
                assert np.array_equal(got[r][2], w[2])


def test_the_windowed_loops_take_views():
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import EvalWindowCorpus, InferDeviceCorpus, _WindowCorpus
    for fn in (atest.test_epoch_windows, atest.sweep_conf_thresh_windows, atest.infer_epoch_corpus):
        prm = inspect.signature(fn).parameters
        assert "tta" in prm and prm["tta"].default is None, fn.__name__
    assert list(inspect.signature(_WindowCorpus.launch_view).parameters) == ["self", "p", "comb", "audio_out"]
    assert EvalWindowCorpus.launch_view is InferDeviceCorpus.launch_view is _WindowCorpus.launch_view
