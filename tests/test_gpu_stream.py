"""GPU: streaming inference (``corpus.StreamDeviceCorpus``, ``test.StreamInference``, csrc/corpus.hip
``adyolo_stream_gather_windows``).  The ring gather against the NumPy restatement of test_stream_cpu.py bit for bit, after the
ring has wrapped, at the seam, under views in both audio formats, with its bad rows and refusals; recordings streamed in
pieces against the CSV file ``infer_epoch_corpus`` writes for them, byte for byte -- eager, through one recorded graph, tracked,
under test-time augmentation, with the lines formatted on the device; a smaller hop and a larger batch against a restatement
that forms the same passes on the host; ``reset()``.  The shapes are those of test_gpu_infer_windows.py: 2 s windows (48 000
samples, 20 label frames), a 0.4 s margin (4 frames), so a default hop of 12 frames."""
import os
import random
import warnings

import numpy as np
import pytest
import torch

from test_infer_windows_cpu import infer_params
from test_stream_cpu import _f32, random_cuts, ring_gather, ring_push, stream_passes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, WF, MF, HF, HOP = 48000, 20, 4, 12, 2400
CAP = N + HF * HOP
BAD_ITEM = 2
# 70 frames + 401 samples, exactly one window, half a window + 77 samples, Wf + 2 Hf (the last start runs twice), no frame
RECORDINGS = (("s0_long", 70 * HOP + 401), ("s1_one", 20 * HOP), ("s2_short", 10 * HOP + 77), ("s3_dup", 44 * HOP),
              ("s4_none", 1000))
PARTITIONS = ("one", "hops", "cycle", "random")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _status():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


# ------------------------------------------------------------------------------------------------------------ the gather
@pytest.fixture(scope="module")
def wrapped():
    """A stream of 2.5 rings pushed into a ring of CAP samples in uneven pieces -> (stream, ring, head); head is odd."""
    rs = np.random.RandomState(9)
    head = 2 * CAP + CAP // 2 + 1201
    stream = rs.randint(-32768, 32768, size=(head, 4)).astype(np.int16)
    ring, at = np.full((CAP, 4), 30000, dtype=np.int16), 0
    for k in random_cuts(random.Random(9), head, 9):
        for a in range(at, at + k, CAP):
            ring_push(ring, a, stream[a:min(a + CAP, at + k)])
        at += k
    return stream, ring, head


def _seam(head):
    """The newest absolute sample that lies at ring place 0."""
    return head // CAP * CAP


def _rows(head):
    """The window rows of the first test, all legal: -> (rows, what each is)."""
    seam = _seam(head)
    assert head - CAP <= seam - N // 2 and seam + 1200 < head
    rows = [(seam - N // 2, N, 0, 0, 0, 0, 0, 0),               # straddles the seam
            (seam - N // 2, N // 2, 0, 0, 0, 0, 0, 0),          # its last valid frame is the last before the seam
            (seam - 4320, 4321, 0, 0, 0, 0, 0, 0),              # valid odd, one frame past the seam
            (seam - 1000, 999, 0, 0, 0, 0, 0, 0),               # valid odd, all before the seam; the padding crosses it
            (head - 1201, 1200, 0, 0, 0, 0, 0, 0),              # valid < n, up to the last even sample
            (head - 1201 - N + 2, N, 0, 0, 0, 0, 0, 0),         # ends one sample short of the head
            (-7, 0, 0, 0, 0, -1, 0, 0)]                         # valid = 0: a filler, its offset is not looked at
    return rows


def test_stream_gather_equals_the_ring_restatement_bit_for_bit(ops, wrapped):
    stream, ring, head = wrapped
    rows = _rows(head)
    want = ring_gather(ring, head, rows, N)
    linear = np.empty_like(want)                                # the restatement itself is linear slicing of the stream
    for w, (off, valid) in enumerate((r[0], r[1]) for r in rows):
        linear[w, :valid] = _f32(stream[off:off + valid]) if valid else 0
        linear[w, valid:] = _f32(0)
    assert np.array_equal(want.view(np.int32), linear.view(np.int32)) and want[6, 0, 0] == np.float32(1e-8)
    dring, table = torch.from_numpy(ring).to(DEV), torch.tensor(rows, dtype=torch.int64, device=DEV)
    out = torch.full((len(rows), N, 4), -5.0, dtype=torch.float32, device=DEV)
    status = _status()
    assert ops.stream_gather_windows(dring, head, table, out, status) is out and int(status.item()) == 0
    assert np.array_equal(_bits(out), want.view(np.int32))
    # and what the linear gather makes of the same rows on the stream laid out linearly
    dstream = torch.from_numpy(np.concatenate([stream, np.zeros((16 - head % 16, 4), dtype=np.int16)])).to(DEV)
    lin = ops.corpus_gather_windows(dstream[:head], table, torch.empty_like(out), status)
    assert int(status.item()) == 0 and torch.equal(lin.view(torch.int32), out.view(torch.int32))
    # W = 3 with a filler row, as a pass of three with two runnable windows
    three = torch.tensor([rows[0], rows[2], (0, 0, 0, 16, 0, -1, 0, 0)], dtype=torch.int64, device=DEV)
    out3 = ops.stream_gather_windows(dring, head, three, torch.empty((3, N, 4), device=DEV), status)
    assert int(status.item()) == 0 and np.array_equal(_bits(out3), want[[0, 2, 6]].view(np.int32))


@pytest.mark.parametrize("fmt", ["foa", "mic"])
def test_stream_gather_views_equal_the_linear_view_gather(ops, wrapped, fmt):
    from adyolo_amd.augmentations import COMBINATIONS, MIC_SWAP_COMBS, mic_swap_source
    stream, ring, head = wrapped
    rows = _rows(head)
    dring, table = torch.from_numpy(ring).to(DEV), torch.tensor(rows, dtype=torch.int64, device=DEV)
    dstream = torch.from_numpy(np.concatenate([stream, np.zeros((16 - head % 16, 4), dtype=np.int16)])).to(DEV)[:head]
    rot = ops.corpus_rot_table(COMBINATIONS)
    mic = ops.corpus_mic_table({k: mic_swap_source(k) for k in MIC_SWAP_COMBS}) if fmt == "mic" else None
    combs = [0] + ([c for c in MIC_SWAP_COMBS if c][:2] if fmt == "mic" else [5, 10])
    assert len(combs) == 3
    plain = ops.stream_gather_windows(dring, head, table, torch.empty((len(rows), N, 4), device=DEV), _status())
    seen = []
    for comb in combs:
        status = _status()
        want = ops.corpus_gather_windows_view(dstream, table, comb, rot, torch.empty((len(rows), N, 4), device=DEV), status,
                                              mic_src=mic)
        got = ops.stream_gather_windows(dring, head, table, torch.full((len(rows), N, 4), -5.0, device=DEV), status, comb=comb,
                                        rot=rot, mic_src=mic)
        assert int(status.item()) == 0 and torch.equal(got.view(torch.int32), want.view(torch.int32)), comb
        assert torch.equal(got.view(torch.int32), plain.view(torch.int32)) == (comb == 0)
        seen.append(got)
    assert not torch.equal(seen[1], seen[2])
    if fmt == "mic":                                            # a combination that is no symmetry of the array: every window bad
        none = [c for c in range(1, 16) if c not in MIC_SWAP_COMBS][0]
        status = _status()
        got = ops.stream_gather_windows(dring, head, table, torch.full((len(rows), N, 4), -5.0, device=DEV), status, comb=none,
                                        rot=rot, mic_src=mic)
        assert int(status.item()) == BAD_ITEM and not _bits(got).any()


def test_stream_gather_bad_rows_zero_fill_and_set_the_status_bit(ops, wrapped):
    from adyolo_amd import _lib
    from adyolo_amd.augmentations import COMBINATIONS
    stream, ring, head = wrapped
    dring = torch.from_numpy(ring).to(DEV)
    seam = _seam(head)
    good = (seam - 1200, 2400, 0, 0, 0, 0, 0, 0)
    want = _f32(stream[seam - 1200:seam + 1200])
    n = 2400
    oldest = head - CAP + 1                                     # (head is odd: the oldest even sample still there)
    for bad in ((seam + 1, 10, 0, 0, 0, 0, 0, 0),               # an odd offset
                (-2, 10, 0, 0, 0, 0, 0, 0),                     # a negative offset
                (head - 9, 10, 0, 0, 0, 0, 0, 0),               # offset + valid > head: not pushed yet
                (head + 1, 1, 0, 0, 0, 0, 0, 0),
                (oldest - 2, 10, 0, 0, 0, 0, 0, 0),             # older than head - capacity: overwritten
                (0, 10, 0, 0, 0, 0, 0, 0),
                (seam, n + 1, 0, 0, 0, 0, 0, 0),                # more valid samples than the window holds
                (seam, -1, 0, 0, 0, 0, 0, 0)):
        status = _status()
        out = torch.full((3, n, 4), -5.0, dtype=torch.float32, device=DEV)
        ops.stream_gather_windows(dring, head, torch.tensor([good, bad, good], dtype=torch.int64, device=DEV), out, status)
        assert int(status.item()) == BAD_ITEM, bad
        host = out.cpu().numpy()
        assert np.array_equal(host[0].view(np.int32), want.view(np.int32)), bad
        assert np.array_equal(host[2].view(np.int32), want.view(np.int32)) and not host[1].view(np.int32).any(), bad
    for edge, first in (((oldest, 10, 0, 0, 0, 0, 0, 0), stream[oldest]),      # the oldest sample, the newest one: legal
                        ((head - 11, 11, 0, 0, 0, 0, 0, 0), stream[head - 11])):
        status = _status()
        out = ops.stream_gather_windows(dring, head, torch.tensor([edge], dtype=torch.int64, device=DEV),
                                        torch.empty((1, n, 4), device=DEV), status)
        assert int(status.item()) == 0 and np.array_equal(_bits(out[0, 0]), _f32(first).view(np.int32))
    # EINVAL before any launch
    status, table = _status(), torch.tensor([good], dtype=torch.int64, device=DEV)
    rot = ops.corpus_rot_table(COMBINATIONS)
    out = torch.empty((1, n, 4), device=DEV)
    odd_ring = torch.zeros((CAP + 1, 4), dtype=torch.int16, device=DEV)
    for call in (lambda: ops.stream_gather_windows(odd_ring[:CAP + 1], head, table, out, status),          # capacity odd
                 lambda: ops.stream_gather_windows(dring[:n - 2], head, table, out, status),               # capacity < n
                 lambda: ops.stream_gather_windows(dring, head, table, out, status, comb=16, rot=rot),     # comb >= 16
                 lambda: ops.stream_gather_windows(dring, head, table, out, status, comb=3),               # a view without a table
                 lambda: ops.stream_gather_windows(dring[1:], head, table, out, status),                   # ring 8 bytes off 16
                 lambda: ops.stream_gather_windows(dring, head, table, out.view(-1)[1:1 + (n - 1) * 4].view(1, n - 1, 4), status),
                 lambda: ops.stream_gather_windows(dring, head, table, torch.empty((2, n, 4), device=DEV), status)):
        with pytest.raises(_lib.AdyoloHipError):
            call()
    assert int(status.item()) == 0


# ----------------------------------------------------------------------------------------------------- the whole pipeline
_CHAINS, _WANT = {}, {}


def _chain(loss, nb_classes):
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.wrapper import WrapperModel
    if loss not in _CHAINS:
        prm = infer_params("unused", loss=loss, nb_classes=nb_classes, device=DEV)
        torch.manual_seed(8)
        model = WrapperModel((1, 7, 80, 64), (), prm).to(DEV).eval()
        _CHAINS[loss] = (prm, model, FeatureExtractor(None, DEV), LabelPostProcessor(prm))
    return _CHAINS[loss]


def _arrays():
    rs = np.random.RandomState(23)
    return [rs.randint(-8000, 8000, size=(n, 4)).astype(np.int16) for _, n in RECORDINGS]


def _track_opts():
    from adyolo_amd.augmentations import track_options
    return track_options({"test_config": {"track": True}})


def _file_path(loss, nb_classes, tmp_path_factory, tracking=None, tta=None):
    """The CSV bytes ``infer_epoch_corpus`` writes for every recording at batch_size 1, once per (loss, tracking, tta)."""
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import InferDeviceCorpus, infer_split_from_arrays
    key = (loss, tracking is not None, tta is not None)
    if key not in _WANT:
        prm, model, fx, post = _chain(loss, nb_classes)
        names = [n for n, _ in RECORDINGS]
        corpus = InferDeviceCorpus(infer_split_from_arrays(names, _arrays(), prm), prm, DEV, window_s=2, margin_s=0.4, batch_size=1)
        out = str(tmp_path_factory.mktemp("file_path"))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            atest.infer_epoch_corpus(corpus, model, fx, post, out, tracking=tracking, tta=tta)
        _WANT[key] = {n: open(os.path.join(out, n + ".csv"), "rb").read() for n in names}
        assert all(len(_WANT[key][n]) > 0 for n in names[:4]) and _WANT[key]["s4_none"] == b""
    return _WANT[key]


def _pushes(kind, total, seed=0):
    if kind == "one":
        return [total]
    if kind == "hops":
        return [HF * HOP] * (total // (HF * HOP)) + ([total % (HF * HOP)] if total % (HF * HOP) else [])
    if kind == "cycle":
        out, k = [], 0
        while sum(out) < total:
            out.append(min((1, 999, 4801, 23999)[k % 4], total - sum(out)))
            k += 1
        return out
    return random_cuts(random.Random(100 + seed), total, 7)


def _lines(rows, ids, path):
    from adyolo_amd.postprocess import write_seld_output_file
    write_seld_output_file(path, rows, ids)
    return open(path, "rb").read()


def _stream(session, audio, pushes, hold=None):
    """``audio`` pushed in ``pushes`` and closed -> the union of what came back; the properties every stream has."""
    session.reset()
    rows, ids, at, final = {}, ({} if session.tracker is not None else None), 0, 0
    for k in pushes + [None]:
        got, got_ids = session.close() if k is None else session.push(audio[at:at + (k or 0)])
        at += k or 0
        assert list(got) == sorted(got) and (not got or not rows or min(got) > max(rows))    # ascending, never revised
        assert (got_ids is None) == (ids is None) and (ids is None or list(got_ids) == list(got))
        assert session.frames_final >= final and (not got or max(got) < session.frames_final)
        if hold is not None and k is not None and got:                       # no frame before it is ``hold`` frames old
            assert max(got) < at // HOP - hold
        final = session.frames_final
        rows.update(got)
        if ids is not None:
            ids.update(got_ids)
    assert at == audio.shape[0] and final == audio.shape[0] // HOP
    return rows, ids


@pytest.mark.parametrize("partition", PARTITIONS)
@pytest.mark.parametrize("loss,nb_classes", [("adyolo", 12), ("adpit", 13)])
def test_streamed_recordings_equal_the_file_path(ops, tmp_path, tmp_path_factory, loss, nb_classes, partition):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import StreamDeviceCorpus
    want = _file_path(loss, nb_classes, tmp_path_factory)
    prm, model, fx, post = _chain(loss, nb_classes)
    corpus = StreamDeviceCorpus(prm, DEV, window_s=2, margin_s=0.4, batch_size=1)
    assert (corpus.window_frames, corpus.margin_frames, corpus.hop_frames, corpus.capacity, corpus.min_capacity) == \
        (WF, MF, HF, CAP, CAP)
    out = str(tmp_path / "live.csv")
    session = atest.StreamInference(corpus, model, fx, post, output_file=out)
    for r, ((name, total), audio) in enumerate(zip(RECORDINGS, _arrays())):
        if partition == "one" and r == 0:
            assert total > corpus.capacity                                   # one push larger than the ring
        rows, ids = _stream(session, audio, _pushes(partition, total, r))
        assert open(out, "rb").read() == want[name], (name, partition)
        assert ids is None and _lines(rows, None, str(tmp_path / "union.csv")) == want[name]
        corpus.check()
        steps = max(0, (total // HOP - WF) // HF + 1) if total // HOP >= WF else 0
        assert corpus.n_windows == corpus.n_passes == steps + (1 if total // HOP else 0)


@pytest.mark.parametrize("loss,nb_classes", [("adyolo", 12), ("adpit", 13)])
def test_streamed_recordings_through_one_recorded_graph(ops, tmp_path, tmp_path_factory, loss, nb_classes):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import StreamDeviceCorpus
    from adyolo_amd.graph import ForwardGraphs
    want = _file_path(loss, nb_classes, tmp_path_factory)
    prm, model, fx, post = _chain(loss, nb_classes)
    corpus = StreamDeviceCorpus(prm, DEV, window_s=2, margin_s=0.4, batch_size=1)
    fg = ForwardGraphs(model, fx, post, warm_calls=0)
    out = str(tmp_path / "live.csv")
    session = atest.StreamInference(corpus, model, fx, post, forward=fg, output_file=out)
    passes = 0
    for r, ((name, total), audio) in enumerate(zip(RECORDINGS, _arrays())):
        _stream(session, audio, _pushes(("cycle", "random", "one", "hops", "one")[r], total, r))
        assert open(out, "rb").read() == want[name], name
        passes += corpus.n_passes
    assert fg.captures == 1 and len(fg.entries) == 1 and fg.evictions == 0 and fg.replays == passes
    assert fg.static_input((1, N, 4)) is not None


@pytest.mark.parametrize("mode", ["track", "tta", "tta-track", "csv", "csv-tta-track"])
@pytest.mark.parametrize("loss,nb_classes", [("adyolo", 12), ("adpit", 13)])
def test_tracked_merged_and_device_formatted_streams_equal_the_file_path(ops, tmp_path, tmp_path_factory, loss, nb_classes, mode):
    from adyolo_amd import test as atest
    from adyolo_amd.augmentations import tta_options
    from adyolo_amd.corpus import StreamDeviceCorpus
    from adyolo_amd.postprocess import track_hold
    prm, model, fx, post = _chain(loss, nb_classes)
    tracking = _track_opts() if "track" in mode else None
    # (the untrained AD-YOLO head selects hundreds of rows per frame: the pool of test_gpu_tta_windows.py; two views)
    cfg = {"tta_views": [5], "tta_min_views": 1 if loss == "adyolo" else 2, "tta_max_rows_per_frame": 340 if loss == "adyolo" else 64}
    tta = tta_options(dict(prm, test_config=cfg), postprocessor=post) if "tta" in mode else None
    assert tta is None or tta["views"] == [0, 5]
    assert tracking is None or (tracking["max_gap"], tracking["min_len"]) == (2, 3)
    hold = track_hold(tracking["max_gap"], tracking["min_len"]) if tracking else None
    want = _file_path(loss, nb_classes, tmp_path_factory, tracking, tta)
    if tracking is not None:                                                 # the ids are there, and tracking changed the rows
        plain = _file_path(loss, nb_classes, tmp_path_factory, None, tta)
        assert want["s0_long"] != plain["s0_long"] and any(line.split(b",")[2] != b"0" for line in want["s0_long"].splitlines())
    if tta is not None:
        assert want["s0_long"] != _file_path(loss, nb_classes, tmp_path_factory, tracking, None)["s0_long"]
    corpus = StreamDeviceCorpus(prm, DEV, window_s=2, margin_s=0.4, batch_size=1)
    out = str(tmp_path / "live.csv")
    session = atest.StreamInference(corpus, model, fx, post, tracking=tracking, tta=tta, device_csv="csv" in mode, output_file=out)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                      # (the tracker's caps only warn)
        for r, ((name, total), audio) in enumerate(zip(RECORDINGS, _arrays())):
            for partition in ("cycle", "random") if r in (0, 3) else ("hops",):
                rows, ids = _stream(session, audio, _pushes(partition, total, r), hold)
                assert open(out, "rb").read() == want[name], (name, partition)
                if "csv" in mode:
                    assert rows == {} and ids in ({}, None)                  # the lines go to the file only
                else:
                    assert _lines(rows, ids, str(tmp_path / "union.csv")) == want[name]


def _restated(ops, audio, passes, batch, model, fx, post, path):
    """The stream's CSV restated: the passes of ``stream_passes``, every window materialised on the host with int16 zero
    fill, the eager forward + ``decode_device`` on the batch, the stitch as NumPy slices, ``select_device_rows`` on the run."""
    from adyolo_amd.postprocess import group_rows, write_seld_output_file
    found = {}
    with torch.no_grad():
        for rows in passes:
            pcm = np.zeros((batch, N, 4), dtype=np.int16)
            for k, (off, valid) in enumerate((r[0], r[1]) for r in rows):
                pcm[k, :valid] = audio[off:off + valid]
            dev = ops.pcm16_to_f32(torch.from_numpy(pcm).to(DEV).contiguous()).view(batch, N, 4)
            host = post.decode_device(model(fx(dev, channels_last8=True), channels_last8=True)).cpu().numpy()
            host = host.reshape((batch, WF) + host.shape[1:])
            run = np.concatenate([host[k, r[2]:r[2] + r[4]] for k, r in enumerate(rows)], 0)
            sel, counts = post.select_device_rows(torch.from_numpy(run).to(DEV).contiguous(), 1)
            for f, vals in group_rows(sel.cpu().numpy(), counts.cpu().numpy(), 1)[0].items():
                found[rows[0][3] + f] = vals
    write_seld_output_file(path, found)
    return open(path, "rb").read()


@pytest.mark.parametrize("loss,nb_classes", [("adyolo", 12), ("adpit", 13)])
def test_a_smaller_hop_and_a_larger_batch_equal_the_restatement(ops, tmp_path, loss, nb_classes):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import StreamDeviceCorpus
    prm, model, fx, post = _chain(loss, nb_classes)
    hf, batch = 3, 3
    corpus = StreamDeviceCorpus(prm, DEV, window_s=2, margin_s=0.4, hop_s=0.3, batch_size=batch)
    assert (corpus.hop_frames, corpus.min_capacity, corpus.capacity) == (hf, N + hf * HOP, N + batch * hf * HOP)
    out = str(tmp_path / "live.csv")
    session = atest.StreamInference(corpus, model, fx, post, output_file=out)
    audio, total = _arrays()[0], RECORDINGS[0][1]
    sizes = set()
    for partition in ("one", "cycle", "random"):
        pushes = _pushes(partition, total, 4)
        passes = stream_passes(WF, MF, hf, HOP, corpus.capacity, batch, pushes)
        sizes |= {len(rows) for rows in passes}
        want = _restated(ops, audio, passes, batch, model, fx, post, str(tmp_path / "want.csv"))
        assert len(want) > 0
        rows, _ = _stream(session, audio, pushes)
        assert (corpus.n_passes, corpus.n_windows) == (len(passes), sum(len(r) for r in passes))
        assert open(out, "rb").read() == want and _lines(rows, None, str(tmp_path / "union.csv")) == want, partition
        corpus.check()
    assert {1, 3} <= sizes <= {1, 2, 3}                                      # full catch-up passes and filler windows


def test_reset_starts_a_fresh_stream_and_the_ids_again(ops, tmp_path, tmp_path_factory):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import StreamDeviceCorpus
    prm, model, fx, post = _chain("adyolo", 12)
    want = _file_path("adyolo", 12, tmp_path_factory, _track_opts(), None)
    corpus = StreamDeviceCorpus(prm, DEV, window_s=2, margin_s=0.4, batch_size=1)
    out = str(tmp_path / "live.csv")
    session = atest.StreamInference(corpus, model, fx, post, tracking=_track_opts(), output_file=out)
    arrays = _arrays()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        session.push(arrays[0][:50 * HOP + 17])                              # a stream left open, its carry full: abandoned
        assert corpus.head == 50 * HOP + 17 and session.frames_final > 0
        for r in (3, 0):                                                     # _stream resets first
            _, ids = _stream(session, arrays[r], _pushes("cycle", RECORDINGS[r][1]))
            assert open(out, "rb").read() == want[RECORDINGS[r][0]]
            assert ids and all(len(v) > 0 for v in ids.values())             # (the bytes hold the ids: they started again)
    with pytest.raises(ValueError):
        session.push(arrays[1])                                              # closed: reset() starts a new stream
    session.reset()
    assert (corpus.head, corpus.planned, session.frames_final, open(out, "rb").read()) == (0, 0, 0, b"")


def test_stream_corpus_refusals(ops):
    from adyolo_amd.corpus import StreamDeviceCorpus
    prm = infer_params("unused")
    for kw in (dict(margin_s=0.0), dict(hop_s=1.3), dict(hop_s=0.0), dict(hop_s=0.25), dict(window_s=2.05),
               dict(capacity_s=3.1), dict(capacity_s=(CAP + 1) / 24000.0), dict(batch_size=0)):
        with pytest.raises(ValueError):
            StreamDeviceCorpus(prm, DEV, **dict(dict(window_s=2, margin_s=0.4), **kw))
    corpus = StreamDeviceCorpus(prm, DEV, window_s=2, margin_s=0.4, capacity_s=3.2)
    assert corpus.capacity == CAP and corpus.free == CAP and corpus.runnable() == 0
    for bad in (np.zeros((10, 3), dtype=np.int16), np.zeros((10, 4), dtype=np.float32), np.zeros(10, dtype=np.int16)):
        with pytest.raises(ValueError):
            corpus.append(bad)
    with pytest.raises(ValueError):
        corpus.launch()                                                      # nothing is runnable
    assert corpus.append(np.zeros((0, 4), dtype=np.int16)) == 0
    assert corpus.append(np.zeros((CAP + 5, 4), dtype=np.int16)) == CAP and corpus.free == 0 and corpus.runnable() == 2
