"""CPU: the host half of labelled windowed evaluation (ad-yolo_amd/corpus.py ``plan_windows``, ``window_items``,
``EvalWindowCorpus``'s refusals; ad-yolo_amd/seld_metrics.py ``run_segments``): the invariants of the segment plan over every
length 0..200 in small folders, the constructor's refusals before anything is uploaded, the event sub-range of every window
against a brute-force filter, and the new symbols.  The scorer's block is 10 label frames throughout."""
import os
import re

import numpy as np
import pytest

import adyolo_amd  # noqa: F401
from adyolo_amd import _lib
from adyolo_amd import corpus as C
from adyolo_amd.seld_metrics import run_segments

from test_eval_corpus_cpu import eval_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP, FPB = 2400, 10
PLANS = ((30, 10), (20, 0), (200, 20))
BATCHES = (1, 3, 8)


def _folders(f):
    """Small folders around a recording of ``f`` label frames: neighbours of other lengths, recordings without a frame in
    front, in the middle and at the end."""
    return ([f, 37, f, 10], [0, f, 0, 45, 0], [110, f, 12], [f, 0])


def _plan(frames, wf, mf, batch):
    lengths = [v * HOP + (77 if k % 2 else 0) for k, v in enumerate(frames)]
    rec_start = np.concatenate([[0], np.cumsum([(n + 15) // 16 * 16 for n in lengths])])
    return C.plan_windows(frames, lengths, rec_start, HOP, wf * HOP, wf, mf, batch), lengths, rec_start


@pytest.mark.parametrize("wf,mf", PLANS)
@pytest.mark.parametrize("batch", BATCHES)
def test_segments_tile_every_recording_on_block_boundaries(wf, mf, batch):
    checked = 0
    for f in range(0, 201):
        for frames in _folders(f):
            if not any(frames):
                continue
            plan, _, _ = _plan(frames, wf, mf, batch)
            total = int(plan["frame_start"][-1])
            assert total == sum(frames) and len(plan["pass_base"]) == plan["n_passes"] >= 1
            bounds = plan["pass_base"] + [total]
            assert [b - a for a, b in zip(bounds, bounds[1:])] == plan["pass_frames"]       # the runs tile the common axis
            segs = run_segments(frames, bounds)
            assert len(segs) == plan["n_passes"]
            nb = [-(-v // FPB) + 2 for v in frames]                  # the file's blocks: two past its audio (trailing FN blocks)
            pos_f, pos_b, lasts = [0] * len(frames), [0] * len(frames), [0] * len(frames)
            for p, seg in enumerate(segs):
                run = plan["pass_frames"][p]
                assert seg.shape[1] == 5 and len(seg) >= 1
                end = 0
                for r, f0, r0, n, last in seg.tolist():
                    assert lasts[r] == 0                             # nothing of a recording follows its last segment
                    assert f0 % FPB == 0 and n >= 0 and (last or (f0 + n) % FPB == 0), (frames, p, seg)
                    assert f0 == pos_f[r] and f0 // FPB == pos_b[r], (frames, p, seg)       # in order, exactly once
                    assert r0 >= end and r0 + n <= run, (frames, p, seg)                    # disjoint, inside the run
                    assert r0 == int(plan["frame_start"][r]) + f0 - bounds[p]               # where the stitch puts the frames
                    end = r0 + n
                    pos_f[r] = f0 + n
                    pos_b[r] = nb[r] if last else (f0 + n) // FPB
                    lasts[r] += last
                    assert last == (pos_f[r] == frames[r])
            assert pos_f == frames and pos_b == nb and lasts == [1] * len(frames), (frames, wf, mf, batch)
            # every window's kept frames lie in the segment of its recording in its pass
            table = plan["table"].reshape(plan["n_passes"], batch, -1)
            for p in range(plan["n_passes"]):
                by_rec = {row[0]: row for row in segs[p].tolist()}
                for off, valid, src_lo, dst, cnt, r, _, _ in table[p].tolist():
                    if r < 0:
                        assert cnt == 0 and p == plan["n_passes"] - 1
                        continue
                    _, f0, r0, n, _ = by_rec[r]
                    lo = dst - int(plan["frame_start"][r])
                    assert f0 <= lo and lo + cnt <= f0 + n and dst - bounds[p] == r0 + lo - f0
            checked += 1
    assert checked > 700


def test_run_segments_places_recordings_without_frames():
    # [0, 0) [0, 25) [25, 25) [25, 65) [65, 65): runs cut at 20 and 50
    segs = [s.tolist() for s in run_segments([0, 25, 0, 40, 0], [0, 20, 50, 65])]
    assert segs == [[[0, 0, 0, 0, 1], [1, 0, 0, 20, 0]],
                    [[1, 20, 0, 5, 1], [2, 0, 5, 0, 1], [3, 0, 5, 25, 0]],
                    [[3, 25, 0, 15, 1], [4, 0, 15, 0, 1]]]
    assert [s.tolist() for s in run_segments([7], [0, 7])] == [[[0, 0, 0, 7, 1]]]
    for frames, bounds in (([10, 5], [0, 10]), ([10], [1, 10]), ([10], [0, 5, 5, 10]), ([10], [0])):
        with pytest.raises(ValueError):
            run_segments(frames, bounds)


def _host_split(lengths, events=None):
    hc = C.HostCorpus(C.HostCorpus.EVAL, ["rec%d" % k for k in range(len(lengths))], lengths, HOP, "test")
    if events is not None:
        hc.set_events(events)
        hc.max_events = max(len(e) for e in events)
    return hc


def test_constructor_refuses_windows_off_the_block_grid_and_empty_splits():
    prm = eval_params("unused")
    hc = _host_split([48000, 72000])
    # nothing is uploaded before the refusal: the device does not exist here
    with pytest.raises(ValueError, match="block"):
        C.EvalWindowCorpus(hc, prm, "cuda:0", window_s=2.0, margin_s=0.4)            # (Wf, Mf) = (20, 4)
    with pytest.raises(ValueError, match="block"):
        C.EvalWindowCorpus(hc, prm, "cuda:0", window_s=2.5, margin_s=0.0)            # (25, 0)
    with pytest.raises(ValueError, match="no window"):
        C.EvalWindowCorpus(_host_split([1000, 0, 2399]), prm, "cuda:0", window_s=2.0, margin_s=0.0)
    with pytest.raises(ValueError, match="label hop"):                               # InferDeviceCorpus's rules hold too
        C.EvalWindowCorpus(hc, prm, "cuda:0", window_s=2.05, margin_s=0.0)
    with pytest.raises(ValueError, match="margins"):
        C.EvalWindowCorpus(hc, prm, "cuda:0", window_s=2.0, margin_s=1.0)
    infer = C.infer_split_from_arrays(["a"], [np.zeros((48000, 4), dtype=np.int16)], prm)
    with pytest.raises(ValueError, match="load_eval_split"):
        C.EvalWindowCorpus(infer, prm, "cuda:0", window_s=2.0, margin_s=0.0)


@pytest.mark.parametrize("wf,mf", [(30, 10), (20, 0)])
def test_item_rows_hold_the_events_of_their_window(wf, mf):
    rs = np.random.RandomState(23)
    frames = [0, 12, 30, 45, 110, 31]
    events = []
    for f in frames:
        # about two events per frame, some frames empty, and rows past the label frames (a CSV longer than its audio)
        fr = np.sort(rs.randint(0, f + 15, size=2 * f + 3))
        ev = np.zeros((len(fr), 5))
        ev[:, 0], ev[:, 1] = fr, rs.randint(0, 12, size=len(fr))
        events.append(ev)
    plan, lengths, rec_start = _plan(frames, wf, mf, 3)
    ev_start = np.concatenate([[0], np.cumsum([len(e) for e in events])])
    all_frames = np.concatenate(events, 0)[:, 0]
    items = C.window_items(plan, frames, wf, ev_start, all_frames)
    assert items.shape == (plan["n_passes"] * 3, 8)
    assert plan["n_windows"] == sum(len(C.window_plan(f, wf, mf)) for f in frames if f) and plan["n_windows"] % 3
    seen = 0
    for w, row in enumerate(items.tolist()):
        if w >= plan["n_windows"]:
            assert row == [0, 0, 0, 0, -1, 0, 0, 0]                  # an empty window: no events, not a bad item
            continue
        r, start = int(plan["table"][w, 5]), int(plan["starts"][w])
        assert row[0] == int(rec_start[r]) + start * HOP == int(plan["table"][w, 0]) and row[1] == start
        assert row[4:] == [-1, r, 0, 0]
        end = min(start + wf, frames[r])
        want = [int(ev_start[r]) + k for k, f in enumerate(events[r][:, 0].tolist()) if start <= f < end]
        assert list(range(row[2], row[2] + row[3])) == want, (w, row)
        seen += len(want)
    assert seen > 100


def test_new_symbols_are_declared_bound_and_wrapped():
    from adyolo_amd import ops, test as atest
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adyolo_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("adyolo_seld_score_runs", "adyolo_seld_score_runs_workspace_words"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
        assert getattr(lib, name) is not None
    assert "#define ADYOLO_SELD_RUN_WORDS 8" in hdr and ops.SELD_RUN_WORDS == 8
    assert re.search(r"#define ADYOLO_SELD_BAD_RUN\s+32\b", hdr) and ops.SELD_BAD_RUN == 32
    assert "#define ADYOLO_ABI_VERSION 4" in hdr
    assert lib.adyolo_seld_score_runs_workspace_words(3, 40, 5, 13) == 2 * 3 * 5 * 13 * 11 + 40
    assert lib.adyolo_seld_score_runs_workspace_words(0, 40, 5, 13) == 0
    assert callable(ops.seld_score_runs) and callable(atest.test_epoch_windows) and callable(atest.sweep_conf_thresh_windows)
    assert callable(C.EvalWindowCorpus) and callable(DeviceSELDScorer.add_run) and callable(DeviceSELDScorer.segment_tables)
