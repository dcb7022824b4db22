"""CPU: the host half of streaming inference (ad-yolo_amd/corpus.py ``stream_plan``, the ring of ``StreamDeviceCorpus`` restated
in NumPy, the ABI of ``adyolo_stream_gather_windows``): the plan's invariants over random parameters and random push partitions,
its relation to ``window_plan`` at the default hop, its refusals; the ring ``ring[s % capacity]`` against linear slicing, and
the rule that says how much a push may take, at the smallest ring, against a model that remembers which sample every ring
place holds.  test_gpu_stream.py reuses the restatement."""
import os
import random
import re

import numpy as np
import pytest

import adyolo_amd  # noqa: F401
from adyolo_amd import _lib
from adyolo_amd import corpus as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(x):
    """The gather's arithmetic in NumPy float32: x / 32768 + 1e-8."""
    return np.asarray(x, dtype=np.float32) / np.float32(32768.0) + np.float32(1e-8)


# ------------------------------------------------------------------------------------------------- the ring, in NumPy
def ring_push(ring, head, pcm):
    """``pcm`` (k, 4) appended to a stream of ``head`` samples: sample s lands at ring[s % capacity] -> the new head."""
    cap = ring.shape[0]
    idx = (head + np.arange(pcm.shape[0])) % cap
    ring[idx] = pcm
    return head + pcm.shape[0]


def ring_window(ring, off, valid, n):
    """The int16 frames [off, off + valid) of the stream read out of the ring, then n - valid frames of int16 zero."""
    out = np.zeros((n, 4), dtype=np.int16)
    out[:valid] = ring[(off + np.arange(valid)) % ring.shape[0]]
    return out


def ring_gather(ring, head, rows, n):
    """``adyolo_stream_gather_windows`` without a view, restated: float32 (W, n, 4); a bad window is all +0."""
    cap = ring.shape[0]
    out = np.empty((len(rows), n, 4), dtype=np.float32)
    for w, row in enumerate(rows):
        off, valid = int(row[0]), int(row[1])
        if valid == 0:
            out[w] = _f32(0)
        elif off < 0 or off & 1 or valid < 0 or valid > n or off + valid > head or off < head - cap:
            out[w] = 0
        else:
            out[w] = _f32(ring_window(ring, off, valid, n))
    return out


def random_cuts(rnd, total, k):
    """A partition of ``total`` samples into pushes: the sizes."""
    cuts = sorted(rnd.randint(0, total) for _ in range(k)) + [total]
    return [b - a for a, b in zip([0] + cuts[:-1], cuts)]


# --------------------------------------------------------------------------------------------------------------- the plan
def _random_case(rnd):
    wf = rnd.randint(3, 30)
    mf = rnd.randint(1, (wf - 1) // 2)
    hf = rnd.randint(1, wf - 2 * mf)
    hop = rnd.choice([1, 3, 2400])
    return wf, mf, hf, hop, rnd.randint(0, 6 * wf * hop)


def _incremental(wf, mf, hf, hop, pushes):
    planned, head, rows = 0, 0, []
    for k in pushes:
        head += k
        new = C.stream_plan(wf, mf, hf, hop, planned, head, False)
        if new:
            planned = new[-1][3] + new[-1][4]
        rows += new
    return rows + C.stream_plan(wf, mf, hf, hop, planned, head, True)


def test_stream_plan_tiles_in_order_with_context_over_random_parameters_and_partitions():
    rnd = random.Random(20)
    for _ in range(4000):
        wf, mf, hf, hop, total = _random_case(rnd)
        one = C.stream_plan(wf, mf, hf, hop, 0, total, True)
        assert _incremental(wf, mf, hf, hop, random_cuts(rnd, total, rnd.randint(0, 8))) == one, (wf, mf, hf, hop, total)
        f, pos, n = total // hop, 0, wf * hop
        if f == 0:
            assert one == []
            continue
        for i, row in enumerate(one):
            off, valid, lo, dst, cnt = row[:5]
            assert len(row) == 8 and row[5:] == (0, 0, 0) and all(isinstance(v, int) for v in row)
            assert dst == pos and cnt > 0 and off % hop == 0 and off // hop + lo == dst          # exact tiling, in order
            assert 0 <= lo and lo + cnt <= wf and 0 <= valid <= n and off + valid <= total
            closing = i == len(one) - 1
            if not closing:                                          # a step: window k at k Hf, whole, Mf of context on the right
                assert off == i * hf * hop and valid == n and wf - (lo + cnt) >= mf
                assert (lo, cnt) == ((0, wf - mf) if i == 0 else (wf - mf - hf, hf))
                assert i * hf + wf <= f
            if i > 0:
                assert lo >= mf                                      # Mf of context on the left
            pos += cnt
        assert pos == f
        steps = len(one) - 1
        assert steps * hf + wf > f                                   # every runnable step ran
        if steps == 0:                                               # F <= Wf and no step ran: the sub-frame remainder is fed
            assert f < wf and one == [(0, min(total, n), 0, 0, f, 0, 0, 0)]
        else:                                                        # the closing window is tail-aligned and whole
            assert one[-1][0] == (f - wf) * hop and one[-1][1] == n and one[-1][2] + one[-1][4] == wf
        # latency: frame q is kept by a window that ends at most Mf + Hf frames after it (the closing window apart)
        for off, _, lo, dst, cnt in (r[:5] for r in one[:-1]):
            assert off // hop + wf - dst <= mf + hf + (wf - mf - hf if dst == 0 else 0)


def test_stream_plan_is_window_plan_at_the_default_hop():
    rnd = random.Random(21)
    same = dup = 0
    for _ in range(3000):
        wf, mf, _, hop, total = _random_case(rnd)
        hf, f = wf - 2 * mf, total // hop
        if f == 0:
            continue
        one = C.stream_plan(wf, mf, hf, hop, 0, total, True)
        want = C.window_plan(f, wf, mf)
        start_of = {q: s for s, lo, d, cnt in want for q in range(d, d + cnt)}
        for off, _, lo, dst, cnt in (r[:5] for r in one):            # every frame from a window with the same start
            assert all(start_of[q] == off // hop for q in range(dst, dst + cnt))
        got = [(r[0] // hop, r[2], r[3], r[4]) for r in one]
        if f < wf or (f - wf) % hf:
            assert got == want
            same += 1
        else:                                                        # the last start ran as a step and runs again on close
            assert len(got) == len(want) + 1 and one[-1][0] == one[-2][0] and got[:-2] == want[:-1]
            dup += 1
    assert same > 100 and dup > 100
    # the shapes of the GPU tests: Wf 20, Mf 4, Hf 12
    assert C.stream_plan(20, 4, 12, 2400, 0, 44 * 2400, True) == [
        (0, 48000, 0, 0, 16, 0, 0, 0), (28800, 48000, 4, 16, 12, 0, 0, 0), (57600, 48000, 4, 28, 12, 0, 0, 0),
        (57600, 48000, 16, 40, 4, 0, 0, 0)]
    assert C.stream_plan(20, 4, 12, 2400, 0, 10 * 2400 + 77, True) == [(0, 24077, 0, 0, 10, 0, 0, 0)]
    assert C.stream_plan(20, 4, 12, 2400, 0, 60000, True) == [(0, 48000, 0, 0, 16, 0, 0, 0), (12000, 48000, 11, 16, 9, 0, 0, 0)]
    assert C.stream_plan(20, 4, 12, 2400, 0, 1000, True) == [] and C.stream_plan(20, 4, 12, 2400, 0, 1000, False) == []
    assert C.stream_plan(20, 4, 12, 2400, 16, 60000, False) == []    # nothing new while open


def test_stream_plan_refusals():
    for wf, mf, hf in ((20, 0, 12), (20, 4, 13), (20, 4, 0), (20, 4, -1), (8, 4, 1), (2, 1, 1)):
        with pytest.raises(ValueError):
            C.stream_plan(wf, mf, hf, 2400, 0, 48000, False)
    assert len(C.stream_plan(3, 1, 1, 2400, 0, 3 * 2400, False)) == 1
    with pytest.raises(ValueError):
        C.stream_plan(20, 4, 12, 2400, 17, 60 * 2400, False)        # 17 is not where a step stops
    with pytest.raises(ValueError):
        C.stream_plan(20, 4, 12, 2400, 0, -1, False)
    with pytest.raises(ValueError):
        C.stream_plan(20, 4, 12, 0, 0, 100, False)


# --------------------------------------------------------------------------------------------------------------- the ring
def test_ring_restatement_agrees_with_linear_slicing():
    rs, rnd = np.random.RandomState(3), random.Random(3)
    n, cap = 480, 480 + 7 * 24
    stream = rs.randint(-32768, 32768, size=(5 * cap + 131, 4)).astype(np.int16)
    ring, head = np.full((cap, 4), 12345, dtype=np.int16), 0
    for k in random_cuts(rnd, stream.shape[0], 40):
        k0 = head
        while k0 < head + k:                                         # a push larger than the ring goes in ring-sized pieces
            take = min(cap, head + k - k0)
            assert ring_push(ring, k0, stream[k0:k0 + take]) == k0 + take
            k0 += take
        head += k
        if head < n:
            continue
        even = head - (head & 1)                                     # offsets are even: the newest, the oldest, short ones
        oldest = max(0, head - cap)
        rows = [(off, valid, 0, 0, 0, 0, 0, 0) for off, valid in
                ((even - n, n), (even - n, 77), (oldest + (oldest & 1), n), (even - 2, 1), (0, 0))]
        want = np.empty((len(rows), n, 4), dtype=np.float32)
        for w, (off, valid) in enumerate((r[0], r[1]) for r in rows):
            want[w, :valid] = _f32(stream[off:off + valid])
            want[w, valid:] = _f32(0)
        assert np.array_equal(ring_gather(ring, head, rows, n).view(np.int32), want.view(np.int32)), head
    # what the kernel calls a bad window: all zeros
    bad = [(head - n + 1, n, 0, 0, 0, 0, 0, 0), (head - n + 2, n, 0, 0, 0, 0, 0, 0), (head - cap - 2, 10, 0, 0, 0, 0, 0, 0)]
    assert not ring_gather(ring, head - (head & 1), bad, n).view(np.int32).any()


def stream_passes(wf, mf, hf, hop, cap, batch, pushes, on_take=None, on_window=None):
    """``StreamDeviceCorpus``'s rule with ``StreamInference.push``'s loop, restated: a push takes min(n, low + capacity - head)
    samples, ``low`` the start of the last launched window (0 before the first); after every slice the runnable windows are
    launched in passes of up to ``batch``; the stream is closed after the last push -> the passes, each a list of plan rows.
    on_take(head, take) / on_window(head, off, valid): called for every slice taken and every window launched."""
    head = planned = low = 0
    passes, pending = [], []

    def run(closing):
        nonlocal planned, low
        new = C.stream_plan(wf, mf, hf, hop, planned, head, closing)
        if new:
            planned = new[-1][3] + new[-1][4]
        pending.extend(new)
        ran = 0
        while pending:
            rows = pending[:batch]
            del pending[:batch]
            for row in rows:
                if on_window is not None:
                    on_window(head, row[0], row[1])
            low = rows[-1][0]
            passes.append(rows)
            ran += 1
        return ran

    for k in pushes:
        left = k
        while True:
            take = min(left, low + cap - head)
            if on_take is not None:
                on_take(head, take)
            head += take
            left -= take
            ran = run(False)
            if not left:
                break
            assert take or ran                                       # the ring is never stuck
    run(True)
    return passes


@pytest.mark.parametrize("batch,extra_hops", [(1, 0), (3, 0), (3, 2), (2, 5)])
def test_the_smallest_ring_never_loses_a_sample_a_window_reads(batch, extra_hops):
    """At the smallest ring (a window and a hop) and above, every window launched finds every sample it reads still in the
    ring, whatever the pushes: a model that remembers which absolute sample each ring place holds."""
    rnd = random.Random(7 + batch)
    for _ in range(150):
        wf, mf, hf, hop, total = _random_case(rnd)
        hop = min(hop, 3)
        total = rnd.randint(0, 6 * wf * hop)
        cap = (wf + hf + extra_hops * hf) * hop
        held = np.full(cap, -1, dtype=np.int64)

        def on_take(head, take):
            held[(head + np.arange(take)) % cap] = head + np.arange(take)

        def on_window(head, off, valid):
            assert off + valid <= head and off >= head - cap
            assert np.array_equal(held[(off + np.arange(valid)) % cap], off + np.arange(valid))

        passes = stream_passes(wf, mf, hf, hop, cap, batch, random_cuts(rnd, total, rnd.randint(0, 6)), on_take, on_window)
        assert [r for rows in passes for r in rows] == C.stream_plan(wf, mf, hf, hop, 0, total, True)
        assert all(1 <= len(rows) <= batch for rows in passes)


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_stream_symbols_are_declared_bound_and_wrapped():
    from adyolo_amd import ops, test as atest
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adyolo_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    name = "adyolo_stream_gather_windows"
    assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr) and getattr(lib, name) is not None
    assert len(_lib.SIGNATURES[name][1]) == 12
    assert callable(ops.stream_gather_windows) and callable(C.StreamDeviceCorpus) and callable(atest.StreamInference)


def test_output_file_rows_can_be_appended(tmp_path):
    from adyolo_amd.postprocess import write_seld_output_file
    rows = {0: [[1, 0.5, 0.25, -0.125]], 3: [[2, 1.0, 0.0, 0.0], [4, 0.0, 1.0, 0.0]], 9: [[0, 0.1, 0.2, 0.3]]}
    ids = {0: [1], 3: [2, 3], 9: [1]}
    whole, parts = str(tmp_path / "whole.csv"), str(tmp_path / "parts.csv")
    write_seld_output_file(whole, rows, ids)
    open(parts, "wb").close()
    for keys in ((0,), (), (3, 9)):
        write_seld_output_file(parts, {k: rows[k] for k in keys}, {k: ids[k] for k in keys}, mode="a")
    assert open(parts, "rb").read() == open(whole, "rb").read() and len(open(whole, "rb").read()) > 0
