"""GPU: windowed inference from an HBM-resident folder (``corpus.InferDeviceCorpus``, ``test.infer_epoch_corpus``, csrc/corpus.hip
``adyolo_corpus_gather_windows`` / ``adyolo_decode_stitch``).  The two kernels against NumPy bit for bit; a recording of exactly
one window against ``test_epoch_audio(device_select=True)`` on the same file, byte for byte; a folder of mixed lengths against a
restatement that forms the same passes on the host, byte for byte.  The model is the small one of test_gpu_eval_corpus.py:
2 s windows (48 000 samples, 20 label frames), here with a 0.4 s margin (4 frames).

The stitch cases: the AD-YOLO record of this grid (8 x 4 cells x 5 anchors) is 2560 floats with 13 classes and 2400 with 12 --
both whole float4 runs -- so the 4-byte path is taken by the class-wise ADPIT record (13 classes x 15 = 195 floats) and by a
one-cell AD-YOLO record of 12 classes (15 floats); ACCDOA (13 x 4 = 52 floats) is a second class-wise record on the float4 path."""
import os

import numpy as np
import pytest
import torch

from test_infer_windows_cpu import SR, infer_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, WF, MF, HOP = 48000, 20, 4, 2400
BAD_ITEM = 2
# samples per recording: shorter than a window, one window, two windows, one window plus a tail below a label hop, six windows,
# and one below a label hop (no frame at all: no window, an empty CSV)
FOLDER = (("r0_short", 24000 + 77), ("r1_one", 48000), ("r2_two", 72000), ("r3_tail", 48000 + 401), ("r4_long", 168000),
          ("r5_none", 1000))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _f32(x):
    """The gather's arithmetic in NumPy float32: x / 32768 + 1e-8."""
    return np.asarray(x, dtype=np.float32) / np.float32(32768.0) + np.float32(1e-8)


def _status():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------------------ the gather
@pytest.mark.parametrize("n", [9602, 9603])                  # three workgroups per window; an even and an odd window length
def test_gather_windows_equals_numpy_bit_for_bit(ops, n):
    rs = np.random.RandomState(5)
    valids = [0, 1, 4321, n - 1, n, n - 2, 2]
    # every recording holds exactly its window's valid samples; everything else of the stream -- the alignment gaps, the
    # neighbours -- is loud, so that one frame read past a valid count shows
    stream = np.full((16 * 8000, 4), 30000, dtype=np.int16)
    rows, pos = [], 32
    for v in valids:
        stream[pos:pos + v] = rs.randint(-32768, 32768, size=(v, 4)).astype(np.int16)
        rows.append((pos, v, 0, 0, 0, 0, 0, 0))
        pos += (v + 15) // 16 * 16 + 16
    rows[0] = (-7, 0, 0, 0, 0, 0, 0, 0)                                     # an empty window: its offset is not looked at
    assert pos <= stream.shape[0]
    want = np.empty((len(rows), n, 4), dtype=np.float32)
    for w, (off, v) in enumerate((r[0], r[1]) for r in rows):
        want[w, :v] = _f32(stream[off:off + v]) if v else 0
        want[w, v:] = _f32(0)
    assert want[0, 0, 0] == np.float32(1e-8)
    pcm, table = torch.from_numpy(stream).to(DEV), torch.tensor(rows, dtype=torch.int64, device=DEV)
    out = torch.full((len(rows), n, 4), -5.0, dtype=torch.float32, device=DEV)
    status = _status()
    got = ops.corpus_gather_windows(pcm, table, out, status)
    assert got is out and int(status.item()) == 0
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    # the full windows are what the plain gather makes of the same offsets
    items = torch.tensor([(rows[4][0], 0, 0, 0, -1, 0, 0, 0)], dtype=torch.int64, device=DEV)
    from adyolo_amd.augmentations import COMBINATIONS
    plain = ops.corpus_gather(pcm, items, ops.corpus_rot_table(COMBINATIONS), torch.empty((1, n, 4), device=DEV), status)
    assert torch.equal(plain[0].view(torch.int32), out[4].view(torch.int32))


def test_gather_windows_bad_items_zero_fill_and_set_the_status_bit(ops):
    n, total = 1200, 4800
    stream = np.full((total, 4), 30000, dtype=np.int16)
    pcm = torch.from_numpy(stream).to(DEV)
    good = (1200, 1200, 0, 0, 0, 0, 0, 0)
    for bad in ((1201, 10, 0, 0, 0, 0, 0, 0),            # an odd offset
                (-2, 10, 0, 0, 0, 0, 0, 0),              # a negative offset
                (total - 8, 10, 0, 0, 0, 0, 0, 0),       # offset + valid beyond the stream
                (total + 2, 1, 0, 0, 0, 0, 0, 0),
                (0, n + 1, 0, 0, 0, 0, 0, 0),            # more valid samples than the window holds
                (0, -1, 0, 0, 0, 0, 0, 0)):
        status = _status()
        out = torch.full((2, n, 4), -5.0, dtype=torch.float32, device=DEV)
        ops.corpus_gather_windows(pcm, torch.tensor([good, bad], dtype=torch.int64, device=DEV), out, status)
        assert int(status.item()) == BAD_ITEM, bad
        host = out.cpu().numpy()
        assert np.array_equal(host[0].view(np.int32), _f32(stream[1200:2400]).view(np.int32))
        assert not host[1].view(np.int32).any(), bad                        # zeros, bit for bit
    status = _status()
    edge = (total - 10, 10, 0, 0, 0, 0, 0, 0)                               # ends with the stream: legal
    out = torch.empty((1, n, 4), dtype=torch.float32, device=DEV)
    ops.corpus_gather_windows(pcm, torch.tensor([edge], dtype=torch.int64, device=DEV), out, status)
    assert int(status.item()) == 0 and float(out[0, 9, 0]) == float(_f32(30000)) and float(out[0, 10, 0]) == float(_f32(0))
    from adyolo_amd import _lib
    with pytest.raises(_lib.AdyoloHipError):
        ops.corpus_gather_windows(pcm, torch.tensor([edge], dtype=torch.int64, device=DEV), torch.empty((2, n, 4), device=DEV), status)


# ------------------------------------------------------------------------------------------------------------ the stitch
@pytest.mark.parametrize("trailing", [(8, 4, 5, 16), (8, 4, 5, 15), (13, 15), (13, 4), (1, 1, 1, 15)],
                         ids=["adyolo13-2560", "adyolo12-2400", "adpit13-195", "accdoa13-52", "adyolo12-onecell-15"])
def test_stitch_equals_numpy_slicing(ops, trailing):
    rec = int(np.prod(trailing))
    base = 1000
    # a first window, a middle one, a tail-aligned one (window_plan(50, 20, 4)[0, 1, 3]) and an empty one, in a pass of their own
    plan = [(0, 16), (4, 12), (10, 10), (0, 0)]
    rows, dst = [], base
    for src_lo, cnt in plan:
        rows.append((0, 0, src_lo, dst, cnt, 0, 0, 0))
        dst += cnt
    total = dst - base
    torch.manual_seed(3)
    dec = torch.randn((len(plan) * WF,) + trailing, dtype=torch.float32, device=DEV)
    out = torch.full((len(plan) * WF,) + trailing, -7.0, dtype=torch.float32, device=DEV)
    status = _status()
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    assert ops.decode_stitch(dec, table, WF, base, out, status) is out
    assert int(status.item()) == 0
    host = dec.cpu().numpy().reshape(len(plan), WF, rec)
    want = np.concatenate([host[w, lo:lo + cnt] for w, (lo, cnt) in enumerate(plan)], 0)
    got = out.cpu().numpy().reshape(-1, rec)
    assert total == 38 and np.array_equal(got[:total].view(np.int32), want.view(np.int32))
    assert (got[total:] == -7.0).all()                                      # nothing is written past the run
    # a window that reaches past its own frames, and one whose place is outside the output: skipped, status bit set
    for bad in ((0, 0, 12, base, 10, 0, 0, 0), (0, 0, 0, base - 1, 4, 0, 0, 0), (0, 0, 0, base + len(plan) * WF - 3, 4, 0, 0, 0),
                (0, 0, -1, base, 4, 0, 0, 0), (0, 0, 0, base, -4, 0, 0, 0)):
        out.fill_(-7.0)
        status = _status()
        ops.decode_stitch(dec, torch.tensor([rows[0], bad, rows[2], rows[3]], dtype=torch.int64, device=DEV), WF, base, out, status)
        assert int(status.item()) == BAD_ITEM, bad
        got = out.cpu().numpy().reshape(-1, rec)
        assert np.array_equal(got[:16], want[:16]) and (got[16:28] == -7.0).all() and np.array_equal(got[28:38], want[28:38])


# ----------------------------------------------------------------------------------------------------- the whole pipeline
def _chain(root, loss="adyolo", nb_classes=12):
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.wrapper import WrapperModel
    prm = infer_params(root, loss=loss, nb_classes=nb_classes, device=DEV)
    torch.manual_seed(8)
    model = WrapperModel((1, 7, 80, 64), (), prm).to(DEV).eval()
    return prm, model, FeatureExtractor(None, DEV), LabelPostProcessor(prm)


def _read(folder, names):
    assert sorted(os.listdir(folder)) == sorted(n + ".csv" for n in names)
    return {n: open(os.path.join(folder, n + ".csv"), "rb").read() for n in names}


def test_one_window_recording_equals_the_whole_clip_path(ops, tmp_path):
    from scipy.io import wavfile
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import InferDeviceCorpus, load_infer_split
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.graph import ForwardGraphs
    wavs = tmp_path / "wavs"
    os.makedirs(str(wavs))
    wavfile.write(str(wavs / "clip.wav"), SR, np.random.RandomState(2).randint(-8000, 8000, size=(N, 4)).astype(np.int16))
    prm, model, fx, post = _chain(wavs)
    ds = FoaDataset(prm, "infer", rank=0, world=1)
    want_dir = str(tmp_path / "whole")
    atest.test_epoch_audio(ds, model, fx, None, post, DEV, want_dir, batch_size=1, device_select=True)
    want = _read(want_dir, ["clip"])
    assert len(want["clip"]) > 0
    corpus = InferDeviceCorpus(load_infer_split(prm, rank=0, world=1, verify="all"), prm, DEV, window_s=2, margin_s=0.4,
                               batch_size=1)
    assert (corpus.n_windows, corpus.n_passes, corpus.window_frames, corpus.margin_frames) == (1, 1, WF, MF)
    assert corpus.get_filelist() == ["clip"] and corpus.nbytes() == corpus.pcm.numel() * 2 + 64
    eager_dir = str(tmp_path / "eager")
    info = atest.infer_epoch_corpus(corpus, model, fx, post, eager_dir)
    assert info == {"recordings": 1, "windows": 1, "passes": 1, "frames": WF}
    assert _read(eager_dir, ["clip"]) == want
    fg = ForwardGraphs(model, fx, post, warm_calls=0)
    for k in range(2):                                                      # recorded, then replayed into the graph's own input
        graph_dir = str(tmp_path / ("graph%d" % k))
        atest.infer_epoch_corpus(corpus, model, fx, post, graph_dir, forward=fg)
        assert _read(graph_dir, ["clip"]) == want
    assert fg.captures == 1 and fg.replays == 2 and fg.static_input((1, N, 4)) is not None
    # against the whole-clip path through its own recorded graph as well
    fg_whole = ForwardGraphs(model, fx, post, warm_calls=0)
    whole_graph_dir = str(tmp_path / "whole_graph")
    atest.test_epoch_audio(ds, model, fx, None, post, DEV, whole_graph_dir, batch_size=1, forward=fg_whole, device_select=True)
    assert _read(whole_graph_dir, ["clip"]) == want


def test_mic_audio_runs_through_the_mic_features(ops, tmp_path):
    """The gather does not look at the audio format: a MIC model with ``MicFeatureExtractor`` on a two-window recording and a
    one-window one, the latter against the whole-clip path byte for byte."""
    from scipy.io import wavfile
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import InferDeviceCorpus, load_infer_split
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.features import MicFeatureExtractor
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.wrapper import WrapperModel
    wavs = tmp_path / "wavs"
    os.makedirs(str(wavs))
    rs = np.random.RandomState(4)
    wavfile.write(str(wavs / "one.wav"), SR, rs.randint(-8000, 8000, size=(N, 4)).astype(np.int16))
    prm = infer_params(wavs, loss="accdoa", nb_classes=13, device=DEV)
    prm["data_config"]["audio_format"] = "mic"
    torch.manual_seed(8)
    model = WrapperModel((1, 10, 80, 64), (), prm).to(DEV).eval()
    fx, post = MicFeatureExtractor(None, DEV), LabelPostProcessor(prm)
    want_dir = str(tmp_path / "whole")
    atest.test_epoch_audio(FoaDataset(prm, "infer", rank=0, world=1), model, fx, None, post, DEV, want_dir, batch_size=1,
                           device_select=True)
    want = _read(want_dir, ["one"])
    assert len(want["one"]) > 0
    wavfile.write(str(wavs / "two.wav"), SR, rs.randint(-8000, 8000, size=(72000, 4)).astype(np.int16))
    corpus = InferDeviceCorpus(load_infer_split(prm, rank=0, world=1, files=["one"]), prm, DEV, window_s=2, margin_s=0.4,
                               batch_size=1)
    got_dir = str(tmp_path / "windowed")
    atest.infer_epoch_corpus(corpus, model, fx, post, got_dir)
    assert _read(got_dir, ["one"]) == want
    both = InferDeviceCorpus(load_infer_split(prm, rank=0, world=1), prm, DEV, window_s=2, margin_s=0.4, batch_size=2)
    both_dir = str(tmp_path / "both")
    info = atest.infer_epoch_corpus(both, model, fx, post, both_dir)
    assert info["windows"] == 3 and info["passes"] == 2 and info["frames"] == 50
    got = _read(both_dir, ["one", "two"])
    assert len(got["two"]) > 0 and max(int(line.split(b",")[0]) for line in got["two"].splitlines()) < 30


def _restated(ops, arrays, names, model, fx, post, out_dir, batch=4):
    """The folder's CSV files restated: the same passes formed from ``window_plan``, every window materialised on the host with
    int16 zero fill, the eager forward + ``decode_device`` on the batch, the stitch as NumPy slices, ``select_device_rows`` on
    the run, the rows numbered per recording here."""
    from adyolo_amd.corpus import window_plan
    from adyolo_amd.postprocess import group_rows, write_seld_output_file
    windows = []
    for r, a in enumerate(arrays):
        frames = a.shape[0] // HOP
        if frames:
            windows += [(r,) + w for w in window_plan(frames, WF, MF)]
    outs = [{} for _ in names]
    n_passes = 0
    with torch.no_grad():
        for p0 in range(0, len(windows), batch):
            chunk = windows[p0:p0 + batch]
            pcm = np.zeros((batch, N, 4), dtype=np.int16)                   # int16 zero: the fill, and the empty windows
            for k, (r, start, _, _, _) in enumerate(chunk):
                piece = arrays[r][start * HOP:start * HOP + N]
                pcm[k, :piece.shape[0]] = piece
            audio = ops.pcm16_to_f32(torch.from_numpy(pcm).to(DEV).contiguous()).view(batch, N, 4)
            dec = post.decode_device(model(fx(audio, channels_last8=True), channels_last8=True))
            host = dec.cpu().numpy()
            host = host.reshape((batch, WF) + host.shape[1:])
            run = np.concatenate([host[k, lo:lo + cnt] for k, (_, _, lo, _, cnt) in enumerate(chunk)], 0)
            owner = [(r, dst + i) for r, _, _, dst, cnt in chunk for i in range(cnt)]
            rows, counts = post.select_device_rows(torch.from_numpy(run).to(DEV).contiguous(), 1)
            found = group_rows(rows.cpu().numpy(), counts.cpu().numpy(), 1)[0]
            for f, vals in found.items():
                outs[owner[f][0]][owner[f][1]] = vals
            n_passes += 1
    os.makedirs(out_dir)
    for name, rows in zip(names, outs):
        write_seld_output_file(os.path.join(out_dir, name + ".csv"), rows)
    return len(windows), n_passes


@pytest.mark.parametrize("loss,nb_classes", [("adyolo", 12), ("adpit", 13)])
def test_mixed_folder_equals_the_restatement(ops, tmp_path, loss, nb_classes):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import InferDeviceCorpus, infer_split_from_arrays
    from adyolo_amd.graph import ForwardGraphs
    rs = np.random.RandomState(17)
    names = [n for n, _ in FOLDER]
    arrays = [rs.randint(-8000, 8000, size=(n, 4)).astype(np.int16) for _, n in FOLDER]
    prm, model, fx, post = _chain(tmp_path, loss=loss, nb_classes=nb_classes)
    want_dir = str(tmp_path / "restated")
    n_windows, n_passes = _restated(ops, arrays, names, model, fx, post, want_dir)
    assert (n_windows, n_passes) == (11, 3)                                 # 1 + 1 + 2 + 1 + 6 + 0 windows: one empty window
    want = _read(want_dir, names)
    assert want["r5_none"] == b"" and sum(len(v) for v in want.values()) > 0
    assert all(len(want[n]) > 0 for n in names[:5]), {n: len(v) for n, v in want.items()}

    corpus = InferDeviceCorpus(infer_split_from_arrays(names, arrays, prm), prm, DEV, window_s=2, margin_s=0.4, batch_size=4)
    assert (corpus.n_windows, corpus.n_passes) == (11, 3) and corpus.label_frames == [10, 20, 30, 20, 70, 0]
    assert corpus.pass_frames == [10 + 20 + 16 + 14, 20 + 16 + 12 + 12, 12 + 12 + 6 + 0] and corpus.pass_base == [0, 60, 120]
    assert corpus.table_host[-1].tolist() == [0, 0, 0, 150, 0, -1, 0, 0] and corpus.table_host[0, 1] == 24077
    assert corpus.table_host[3, 1] == N and corpus.table_host[4, 1] == N   # the 401 samples past the last frame are not fed
    eager_dir = str(tmp_path / "eager")
    info = atest.infer_epoch_corpus(corpus, model, fx, post, eager_dir)
    assert info == {"recordings": 6, "windows": 11, "passes": 3, "frames": 150}
    assert _read(eager_dir, names) == want
    corpus.check()

    fg = ForwardGraphs(model, fx, post, warm_calls=0)
    graph_dir = str(tmp_path / "graph")
    atest.infer_epoch_corpus(corpus, model, fx, post, graph_dir, forward=fg)
    assert _read(graph_dir, names) == want
    assert fg.captures == 1 and len(fg.entries) == 1 and fg.replays == 3 and fg.evictions == 0     # one graph for the folder
    assert int(corpus.status.item()) == 0
    # the last frame of every recording is its own (no row numbered past a recording's frames)
    for name, frames in zip(names, corpus.label_frames):
        got = [int(line.split(b",")[0]) for line in want[name].splitlines()]
        assert got == sorted(got) and (not got or (got[0] >= 0 and got[-1] < frames))


def test_windows_must_be_whole_label_hops(ops):
    from adyolo_amd.corpus import InferDeviceCorpus, infer_split_from_arrays
    prm = infer_params("unused")
    hc = infer_split_from_arrays(["a"], [np.zeros((N, 4), dtype=np.int16)], prm)
    for window_s, margin_s in ((2.05, 0.4), (2, 0.45), (2, 1.0), (0.0, 0.0), (2, -0.1)):
        with pytest.raises(ValueError):
            InferDeviceCorpus(hc, prm, DEV, window_s=window_s, margin_s=margin_s)
    default = InferDeviceCorpus(hc, dict(prm, data_config=dict(prm["data_config"], chunk_window_s=20)), DEV)
    assert (default.window_frames, default.margin_frames, default.batch_size, default.n_samples) == (200, 20, 8, 480000)
    assert (default.n_windows, default.n_passes) == (1, 1) and default.table_host[0].tolist() == [0, N, 0, 0, 20, 0, 0, 0]
