"""GPU: tracks carried across runs (``ops.track_run`` / csrc/track.hip ``adyolo_track_run``) and tracking through the windowed
paths (``test.test_epoch_windows`` / ``sweep_conf_thresh_windows`` / ``infer_epoch_corpus`` with ``tracking=``).

The kernels against the host definition, bit for bit: recordings of 1 to 257 frames fed in runs cut at every position and at
random partitions, and a stream of recordings cut into passes that hold several of them, must give the rows, counts, ids and
status of ``postprocess.track_rows`` on each whole recording (which the CPU test holds ``postprocess.track_run`` to).

The pipeline, with the small model of test_gpu_eval_windows.py: the tracked windowed pass against the plain pass's rows tracked
on the host per whole recording (CSV bytes, the loss float, the scorer's accumulators); recordings of exactly one window against
``test_epoch_corpus(track=...)``; inference; the sweep against one fresh pass per threshold (atol 1e-9, the bound
test_gpu_eval_windows.py holds the untracked sweep to); ``tracking=None`` against the untracked calls of the same test."""
import ctypes
import os
import shutil
import warnings

import numpy as np
import pytest
import torch

from test_eval_corpus_cpu import eval_params, write_eval_split
from test_track_windows_cpu import (by_recording, cut_sets, feed, pass_bound_sets, run_plan, same, stream_case,
                                    stream_of_recordings, whole)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 20.0
HOP = 2400
C = 3
LENGTHS = (1, 9, 63, 64, 65, 130, 257)
CORNERS = ((0, 1, 1.0), (2, 3, 0.5), (3, 5, 0.5))               # D = 0; the defaults, H = 7; H = 17


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _opts(corner):
    return {"gate_deg": GATE, "max_gap": corner[0], "min_len": corner[1], "smooth": corner[2]}


def device_step(ops, n_classes, opts, hold):
    """``feed``'s / ``run_plan``'s step on the device: one carry for the stream, buffers per run length pre-filled with junk."""
    carry = ops.track_carry(DEV, n_classes, hold)
    bufs = {}

    def step(rows, counts, seg):
        buf = bufs.get(len(counts))
        if buf is None:
            buf = bufs[len(counts)] = ops.track_run_buffers(DEV, len(counts), n_classes, hold)
            buf["ws"].fill_(float("nan"))
            buf["rows"].fill_(float("nan"))
            buf["counts"].fill_(-7)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        padded = np.concatenate([rows.reshape(-1, 5), np.full((3, 5), 9.0, dtype=np.float32)])
        got = ops.track_run(torch.from_numpy(padded).to(DEV), torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(DEV),
                            torch.from_numpy(np.ascontiguousarray(seg, dtype=np.int32)).to(DEV), n_classes, opts, hold, carry,
                            buf=buf, status=status)
        return (got[0].cpu().numpy(), got[1].cpu().numpy()), got[2].cpu().numpy(), int(status.cpu()[0])
    return step


@pytest.fixture(scope="module")
def recordings():
    """Each length's rows and, per corner, the host definition on the whole recording; computed once."""
    out = {}
    for n in LENGTHS:
        rows, counts = stream_case(500 + n, n, C)
        out[n] = (rows, counts, {corner: whole(rows, counts, C, *corner) for corner in CORNERS})
    return out


@pytest.mark.parametrize("corner", CORNERS, ids=["identity", "defaults", "reach17"])
def test_a_recording_cut_anywhere_gives_the_host_definitions_bits(ops, recordings, corner):
    from adyolo_amd.postprocess import track_hold
    hold = track_hold(corner[0], corner[1])
    n_rows = 0
    for n in LENGTHS:
        rows, counts, want = recordings[n]
        n_rows += len(want[corner][0][0])
        for cuts in [[]] + cut_sets(n, 40 + n):
            same(feed(device_step(ops, C, _opts(corner), hold), rows, counts, cuts), want[corner])
    assert n_rows > 0
    # a hold rounded up to the scorer's block, and a recording that stays open: what it holds back is its last D frames
    rows, counts, want = recordings[130]
    same(feed(device_step(ops, C, _opts(corner), hold + 3), rows, counts, [9, 64, 65, 128]), want[corner])
    # a recording that stays open emits all but its last D frames, and they are final: the whole recording's
    got = feed(device_step(ops, C, _opts(corner), hold), rows, counts, [64], open_end=True)
    (w_rows, w_counts), w_ids, _ = want[corner]
    keep = w_rows[:, 0] < 130 - hold
    assert np.array_equal(got[1], w_counts[:130 - hold]) and got[0].tobytes() == w_rows[keep].tobytes()
    assert np.array_equal(got[2], w_ids[keep])


@pytest.mark.parametrize("corner,block", [(CORNERS[0], 1), (CORNERS[1], 1), (CORNERS[1], 10), (CORNERS[2], 1)],
                         ids=["identity", "defaults", "defaults-block10", "reach17"])
def test_runs_of_several_recordings_give_every_recordings_bits(ops, corner, block):
    from adyolo_amd.corpus import plan_track
    from adyolo_amd.postprocess import track_hold
    lengths = (9, 1, 63, 0, 64, 1, 1, 65, 130, 2, 257, 0)
    rows, counts, start, parts = stream_of_recordings(700, lengths, C)
    hold = -(-track_hold(corner[0], corner[1]) // block) * block
    want, want_status = [], 0
    for r_rows, r_counts in parts:
        if not len(r_counts):
            want.append(None)
            continue
        (w_rows, w_counts), w_ids, st = whole(r_rows, r_counts, C, *corner)
        want.append((w_rows, w_counts, w_ids))
        want_status |= st
    several = 0
    for bounds in pass_bound_sets(int(start[-1]), 23):
        plan = plan_track(start, bounds, hold)
        several += sum(len(s) > 2 and s[0, 2] == 1 and s[-1, 3] == 1 for s in plan["segments_host"])
        got, status = by_recording(run_plan(device_step(ops, C, _opts(corner), hold), rows, counts, plan, bounds), plan, start)
        assert status == want_status
        for r, w in enumerate(want):
            if w is None:
                assert len(got[r][1]) == 0
                continue
            assert got[r][0].tobytes() == w[0].tobytes() and np.array_equal(got[r][1], w[1]) and np.array_equal(got[r][2], w[2])
    assert several > 0                       # closed segments beside a continuing and an open one, in one launch


def test_refusals(ops):
    from adyolo_amd import _lib
    from adyolo_amd.postprocess import TRACK_BAD_ROWS
    lib = _lib.load()
    frames, hold = 6, 7
    opts = _opts(CORNERS[1])
    buf = ops.track_run_buffers(DEV, frames, C, hold)
    for t in (buf["rows"], buf["ws"]):
        t.fill_(float("nan"))
    buf["counts"].fill_(-7)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    carry = ops.track_carry(DEV, C, hold)
    r, c = torch.zeros(8, 5, device=DEV), torch.zeros(frames, dtype=torch.int32, device=DEV)
    seg = torch.tensor([[0, frames, 0, 0]], dtype=torch.int32, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                                    # noqa: E731
    good = dict(rows=P(r), n_rows=8, counts=P(c), frames=frames, seg=P(seg), n_seg=1, C=C, cos=0.9, max_gap=2, min_len=3, a=0.5,
                b=0.5, hold=hold, carry=P(carry), ws=P(buf["ws"]), out=P(buf["rows"]), ids=P(buf["ids"]),
                cap=buf["rows"].shape[0], oc=P(buf["counts"]), status=P(status))
    order = ("rows", "n_rows", "counts", "frames", "seg", "n_seg", "C", "cos", "max_gap", "min_len", "a", "b", "hold", "carry", "ws",
             "out", "ids", "cap", "oc", "status")

    def rc(**kw):
        a = dict(good)
        a.update(kw)
        return lib.adyolo_track_run(*[a[k] for k in order], None)

    bad = [dict(rows=None), dict(counts=None), dict(seg=None), dict(carry=None), dict(ws=None), dict(out=None), dict(ids=None),
           dict(oc=None), dict(status=None), dict(ws=ctypes.c_void_p(buf["ws"].data_ptr() + 4)),
           dict(carry=ctypes.c_void_p(carry.data_ptr() + 4)), dict(seg=ctypes.c_void_p(seg.data_ptr() + 2)),
           dict(out=ctypes.c_void_p(buf["rows"].data_ptr() + 2)), dict(frames=0), dict(n_seg=0), dict(n_seg=frames + 1), dict(C=0),
           dict(max_gap=-1), dict(min_len=0), dict(cos=0.0), dict(cos=1.0), dict(cos=float("nan")), dict(a=0.0), dict(a=1.5),
           dict(hold=6), dict(hold=-1), dict(max_gap=3, min_len=5), dict(cap=(frames + hold) * C * 8 - 1), dict(n_rows=-1)]
    for kw in bad:
        assert rc(**kw) == -1, kw                                                  # ADYOLO_EINVAL, before any launch
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == -7 and bool((buf["counts"] == -7).all()) and bool(torch.isnan(buf["rows"]).all())
    assert bool((carry == 0).all())
    status.zero_()
    assert rc(max_gap=0, min_len=1, hold=0) == 0 and rc() == 0 and rc(a=1.0, b=0.0) == 0
    torch.cuda.synchronize()
    assert buf["counts"].cpu().tolist() == [0] * (frames + hold + 1) + [frames] and int(status.cpu()[0]) == 0
    # tables the host cannot see into: refused on the device, nothing emitted, the carry as it was
    d = [0.6, 0.0, 0.8]
    rows = torch.tensor([[f, 0] + d for f in range(frames)], dtype=torch.float32, device=DEV)
    ones = torch.ones(frames, dtype=torch.int32, device=DEV)
    ops.track_run(rows, ones, torch.tensor([[0, frames, 0, 1]], dtype=torch.int32, device=DEV), C, opts, hold, carry, buf=buf)
    kept = carry.clone()
    assert int(kept.view(torch.int32)[1]) == frames                                 # class 0's head: six frames walked
    for table in ([[0, frames - 1, 0, 0]], [[1, frames - 1, 0, 0]], [[0, 2, 0, 0], [3, frames - 3, 0, 0]],
                  [[0, 4, 0, 0], [2, frames - 2, 0, 0]], [[0, 2, 0, 1], [2, frames - 2, 0, 0]], [[0, 2, 0, 0], [2, frames - 2, 1, 0]],
                  [[0, 0, 0, 0], [0, frames, 0, 0]], [[0, frames, 2, 0]], [[0, frames, 0, -1]], [[0, 2 ** 31 - 1, 0, 0]],
                  [[-4, frames + 4, 0, 0]], [[0, frames + 1, 0, 0]]):
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = ops.track_run(rows, ones, torch.tensor(table, dtype=torch.int32, device=DEV), C, opts, hold, carry, buf=buf, status=st)
        assert int(st.cpu()[0]) == TRACK_BAD_ROWS and got[0].shape[0] == 0 and got[1].numel() == 0, table
        assert torch.equal(carry.view(torch.int32), kept.view(torch.int32)), table    # (bits: an empty cell's id is a NaN)
    # a carry no call leaves behind (the held frames do not match the frames walked): refused when row 0 continues
    broken = kept.clone()
    broken.view(torch.int32)[2] = 2
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    cont = torch.tensor([[0, frames, 1, 0]], dtype=torch.int32, device=DEV)
    got = ops.track_run(rows, ones, cont, C, opts, hold, broken, buf=buf, status=st)
    assert int(st.cpu()[0]) == TRACK_BAD_ROWS and got[1].numel() == 0
    got = ops.track_run(rows, ones, cont, C, opts, hold, carry, buf=buf)           # the good one goes on: twelve hits, one track
    assert got[0].shape[0] == 2 * frames and set(got[2].cpu().tolist()) == {0} and got[1].cpu().tolist() == [1] * (2 * frames)
    assert bool((carry.view(torch.int32)[:C * 4] == 0).all())                      # ... and the closed run empties the carry
    # the Python surface refuses what it can see
    with pytest.raises(_lib.AdyoloHipError, match="segments"):
        ops.track_run(rows, ones, cont.long(), C, opts, hold, carry)
    with pytest.raises(_lib.AdyoloHipError, match="track_run_buffers"):
        ops.track_run(rows, ones, cont, C, opts, hold, carry, buf=ops.track_run_buffers(DEV, frames - 1, C, hold))
    with pytest.raises(_lib.AdyoloHipError, match="track_carry"):
        ops.track_run(rows, ones, cont, C, opts, hold, ops.track_carry(DEV, C, hold)[:-4])
    with pytest.raises(_lib.AdyoloHipError, match="hold"):
        ops.track_run(rows, ones, cont, C, opts, hold - 1, ops.track_carry(DEV, C, hold - 1))
    # trim=False with given buffers and the emitted frames known: the given tensors come back, nothing is allocated
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.track_run(rows, ones, seg, C, opts, hold, carry, buf=buf, status=st, trim=False, emitted=frames)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    out_rows, out_counts, out_ids = ops.track_run(rows, ones, seg, C, opts, hold, carry, buf=buf, status=st, trim=False,
                                                  emitted=frames)
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before
    assert out_rows.data_ptr() == buf["rows"].data_ptr() and out_ids.data_ptr() == buf["ids"].data_ptr()
    assert out_counts.data_ptr() == buf["counts"].data_ptr() and out_counts.shape == (frames,)


# ------------------------------------------------------------------------------------------------------------- the pipeline
WF, MF, BATCH = 30, 10, 3                          # 3 s windows with a 1 s margin, three windows per pass
# label frames 0, 12 (shorter than a window), 30, 45 and 110 (nine windows: it spans four passes)
MIXED = (("m0_past", 1000), ("m1_short", 12 * HOP + 77), ("m2_one", 30 * HOP), ("m3_three", 45 * HOP + 401),
         ("m4_long", 110 * HOP))
FRAMES = (0, 12, 30, 45, 110)
OPTS = {"gate_deg": 20.0, "max_gap": 2, "min_len": 3, "smooth": 0.5}


def _reference_dir(root):
    ref = os.path.join(root, "reference")
    shutil.copytree(os.path.join(root, "metadata_dev", "dev-test"), ref)
    return ref


def _chain(root, loss, nb_classes):
    from adyolo_amd.corpus import load_eval_split
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    prm = eval_params(root, loss=loss, nb_classes=nb_classes, device=DEV)
    torch.manual_seed(8)
    model = WrapperModel((1, 7, 80, 64), (), prm).to(DEV).eval()
    hc = load_eval_split(prm, "test", rank=0, world=1, verify="all")
    return prm, model, FeatureExtractor(None, DEV), WrapperCriterion(prm), LabelPostProcessor(prm), hc


def _read(folder, names):
    assert sorted(os.listdir(folder)) == sorted(n + ".csv" for n in names)
    return {n: open(os.path.join(folder, n + ".csv"), "rb").read() for n in names}


def _acc_bits(scorer):
    acc, names = scorer.accumulators()
    return acc.view(np.int64), names


def _rows_of(data, frames):
    """A plain pass's CSV bytes -> (rows (N, 5) float32 in file order, counts (max(1, frames),))."""
    rows = [[float(v) for i, v in enumerate(line.split(b",")) if i != 2] for line in data.splitlines()]
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 5)
    return rows, np.bincount(rows[:, 0].astype(np.int64), minlength=max(1, frames)).astype(np.int32)


def _tracked_whole(ops, plain, names, frames, nb_classes, opts, prm, ref, out_dir):
    """The baseline: every recording's plain rows through the host ``track_rows`` as ONE clip, written with the ids; a scorer
    fed ``add_rows`` with ``ops.track_rows`` of each whole recording.  -> (scorer, rows in, rows out)"""
    from adyolo_amd.postprocess import group_rows, track_groups, track_rows, write_seld_output_file
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    os.makedirs(out_dir)
    sc = DeviceSELDScorer(prm, ref, DEV)
    n_in = n_out = 0
    for name, n in zip(names, frames):
        rows, counts = _rows_of(plain[name], n)
        (out, oc), ids, _ = track_rows(rows, counts, 1, nb_classes, opts["gate_deg"], opts["max_gap"], opts["min_len"], opts["smooth"])
        n_in, n_out = n_in + len(rows), n_out + len(out)
        write_seld_output_file(os.path.join(out_dir, name + ".csv"), group_rows(out, oc)[0], track_groups(ids, oc)[0])
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        d_rows, d_counts, d_ids = ops.track_rows(torch.from_numpy(rows).to(DEV), torch.from_numpy(counts).to(DEV), 1, nb_classes,
                                                 opts, status=st)
        assert d_rows.cpu().numpy().tobytes() == out.tobytes() and np.array_equal(d_ids.cpu().numpy(), ids)
        sc.add_rows(d_rows, d_counts, [name])
    return sc, n_in, n_out


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("gpu_track_windows"))
    return root, write_eval_split(root, clips=MIXED, seed=9), _reference_dir(root)


@pytest.mark.parametrize("loss,nb_classes", [("adyolo", 12), ("adpit", 13)])
def test_the_tracked_windowed_pass_equals_whole_recordings_tracked_on_the_host(ops, mixed, tmp_path, loss, nb_classes):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import EvalWindowCorpus
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root, _, ref = mixed
    prm, model, fx, crit, post, hc = _chain(root, loss, nb_classes)
    corpus = EvalWindowCorpus(hc, prm, DEV, window_s=3, margin_s=1.0, batch_size=BATCH)
    names = corpus.get_filelist()
    frames = [dict(zip([n for n, _ in MIXED], FRAMES))[n] for n in names]
    assert corpus.label_frames == frames and (corpus.n_windows, corpus.n_passes) == (14, 5)
    plan = corpus.track_plan(OPTS)
    assert plan["hold"] == 10 and sum(plan["pass_frames"]) == sum(frames)
    assert sum(s[0, 2] == 1 for s in plan["segments_host"]) >= 2                    # the long recording spans three passes or more
    sc_plain = DeviceSELDScorer(prm, ref, DEV)
    loss_plain = atest.test_epoch_windows(corpus, model, fx, crit, post, str(tmp_path / "plain"), device_scorer=sc_plain)
    plain = _read(str(tmp_path / "plain"), names)
    sc_want, n_in, n_out = _tracked_whole(ops, plain, names, frames, nb_classes, OPTS, prm, ref, str(tmp_path / "want"))
    want = _read(str(tmp_path / "want"), names)
    print("%s: %d rows, %d tracked, loss %r" % (loss, n_in, n_out, loss_plain))
    assert n_in > 0 and n_out > 0 and want != plain and loss_plain > 0
    bits_want, order_want = _acc_bits(sc_want)
    fg = ForwardGraphs(model, fx, post, warm_calls=0)
    for key, forward, out in (("eager", None, "eager"), ("graph", fg, "graph"), ("graph, no files", fg, None)):
        sc = DeviceSELDScorer(prm, ref, DEV)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                        # (the caps of the definition only warn)
            got_loss = atest.test_epoch_windows(corpus, model, fx, crit, post, None if out is None else str(tmp_path / out),
                                                forward=forward, device_scorer=sc, tracking=OPTS)
        assert got_loss == loss_plain, key
        if out is not None:
            assert _read(str(tmp_path / out), names) == want, key
        bits, order = _acc_bits(sc)
        assert order == order_want and np.array_equal(bits, bits_want), key
        assert int(corpus.status.item()) == 0
    assert fg.captures == 1 and fg.evictions == 0
    # tracking=None: the bytes and accumulator bits of the untracked call above
    sc_again = DeviceSELDScorer(prm, ref, DEV)
    assert atest.test_epoch_windows(corpus, model, fx, crit, post, str(tmp_path / "again"), device_scorer=sc_again,
                                    tracking=None) == loss_plain
    assert _read(str(tmp_path / "again"), names) == plain and np.array_equal(_acc_bits(sc_again)[0], _acc_bits(sc_plain)[0])
    assert all(line.split(b",")[2] == b"0" for data in plain.values() for line in data.splitlines())


ONE_WINDOW = (("fold4_a", 48000), ("fold4_b", 48000), ("fold4_c", 48000), ("fold4_d", 48000))


@pytest.mark.parametrize("loss,nb_classes", [("adyolo", 12), ("adpit", 13)])
def test_one_window_recordings_equal_the_tracked_whole_clip_corpus(ops, tmp_path, loss, nb_classes):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import EvalDeviceCorpus, EvalWindowCorpus
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root = str(tmp_path)
    write_eval_split(root, clips=ONE_WINDOW)
    ref = _reference_dir(root)
    prm, model, fx, crit, post, hc = _chain(root, loss, nb_classes)
    clips = EvalDeviceCorpus(hc, prm, DEV)
    names = clips.get_filelist()
    sc_a, sc_b = DeviceSELDScorer(prm, ref, DEV), DeviceSELDScorer(prm, ref, DEV)
    corpus = EvalWindowCorpus(hc, prm, DEV, window_s=2, margin_s=0.0, batch_size=2)
    assert corpus.track_plan(OPTS)["bounds"].tolist() == corpus.pass_bounds == [0, 40, 80]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss_a = atest.test_epoch_corpus(clips, model, fx, crit, post, str(tmp_path / "clips"), batch_size=2, device_scorer=sc_a,
                                         track=OPTS)
        loss_b = atest.test_epoch_windows(corpus, model, fx, crit, post, str(tmp_path / "windows"), device_scorer=sc_b,
                                          tracking=OPTS)
    want = _read(str(tmp_path / "clips"), names)
    assert loss_a == loss_b and loss_a > 0 and sum(len(v) for v in want.values()) > 0
    assert _read(str(tmp_path / "windows"), names) == want
    (bits_a, names_a), (bits_b, names_b) = _acc_bits(sc_a), _acc_bits(sc_b)
    assert names_a == names_b and len(names_a) == 4 and np.array_equal(bits_a, bits_b)


@pytest.mark.parametrize("loss,nb_classes", [("adyolo", 12), ("adpit", 13)])
def test_tracked_inference_equals_whole_recordings_tracked_on_the_host(ops, mixed, tmp_path, loss, nb_classes):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import InferDeviceCorpus, infer_split_from_arrays
    root, written, ref = mixed
    prm, model, fx, crit, post, hc = _chain(root, loss, nb_classes)
    names = [n for n, _ in MIXED]
    corpus = InferDeviceCorpus(infer_split_from_arrays(names, [written[n][0] for n in names], prm), prm, DEV, window_s=3,
                               margin_s=1.0, batch_size=BATCH)
    assert corpus.label_frames == list(FRAMES) and corpus.track_plan(OPTS)["hold"] == 7
    info = atest.infer_epoch_corpus(corpus, model, fx, post, str(tmp_path / "plain"))
    plain = _read(str(tmp_path / "plain"), names)
    _, n_in, n_out = _tracked_whole(ops, plain, names, FRAMES, nb_classes, OPTS, prm, ref, str(tmp_path / "want"))
    assert n_in > 0 and n_out > 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert atest.infer_epoch_corpus(corpus, model, fx, post, str(tmp_path / "got"), tracking=OPTS) == info
    assert _read(str(tmp_path / "got"), names) == _read(str(tmp_path / "want"), names)
    assert atest.infer_epoch_corpus(corpus, model, fx, post, str(tmp_path / "again"), tracking=None) == info
    assert _read(str(tmp_path / "again"), names) == plain


def test_the_tracked_sweep_equals_one_fresh_tracked_pass_per_threshold(ops, mixed, tmp_path):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import EvalWindowCorpus
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root, _, ref = mixed
    prm, model, fx, crit, post, hc = _chain(root, "adyolo", 12)
    corpus = EvalWindowCorpus(hc, prm, DEV, window_s=3, margin_s=1.0, batch_size=BATCH)
    names = corpus.get_filelist()
    thresholds = (0.3, 0.6, 0.4)
    want, plain_want = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k, th in enumerate(thresholds):
            post_t = LabelPostProcessor(prm)
            post_t.set_conf_thresh(th)
            sc_t = DeviceSELDScorer(prm, ref, DEV)
            loss = atest.test_epoch_windows(corpus, model, fx, crit, post_t, str(tmp_path / ("want%d" % k)), device_scorer=sc_t,
                                            tracking=OPTS)
            want.append([float(v) for v in sc_t.scores()[:5]])
        post_s = LabelPostProcessor(prm)
        new_thresh, table, got_loss = atest.sweep_conf_thresh_windows(corpus, model, fx, crit, post_s, DeviceSELDScorer(prm, ref, DEV),
                                                                      thresholds=thresholds, output_pth=str(tmp_path / "sweep"),
                                                                      tracking=OPTS)
    print("sweep:", new_thresh, table, got_loss)
    np.testing.assert_allclose(np.asarray(table, dtype=np.float64), np.asarray(want), rtol=0, atol=1e-9)
    assert got_loss == loss and new_thresh == thresholds[int(np.argmin([row[4] for row in want]))] == post_s.get_conf_thresh()
    assert _read(str(tmp_path / "sweep"), names) == _read(str(tmp_path / ("want%d" % (len(thresholds) - 1))), names)
    # tracking=None: the sweep as it is without the keyword
    plain = [atest.sweep_conf_thresh_windows(corpus, model, fx, crit, LabelPostProcessor(prm), DeviceSELDScorer(prm, ref, DEV),
                                             thresholds=thresholds, output_pth=str(tmp_path / ("plain%d" % k)), **kw)
             for k, kw in enumerate(({}, {"tracking": None}))]
    assert plain[0] == plain[1] and _read(str(tmp_path / "plain0"), names) == _read(str(tmp_path / "plain1"), names)
    assert plain[0][1] != table
