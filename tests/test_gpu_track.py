"""GPU: tracks across frames.  The kernels (csrc/track.hip ``adyolo_track_rows``) against the host definition
``postprocess.track_rows`` bit for bit -- rows as int32, counts, ids and status -- on the random cases of test_track_cpu.py
(one frame; past the 64-frame prefetch block; several clips and classes; two blocks plus a frame) at three parameter corners;
the status bits and the refusals; then ``test_epoch_corpus(track=...)`` / ``sweep_conf_thresh_corpus(track=...)`` on the split
of test_eval_corpus_cpu.py against the untracked pass's rows tracked on the host."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

from test_eval_corpus_cpu import eval_params, write_eval_split
from test_track_cpu import TRACK_CONFIGS, TRACK_CORNERS, random_tracks, track_features

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 20.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def cases():
    """Every configuration's random rows, and per parameter corner the host definition's result and what the case exercises;
    computed once."""
    from adyolo_amd.postprocess import track_rows
    out = {}
    for n_clips, T, C in TRACK_CONFIGS:
        case = random_tracks(100 + T, n_clips, T, C)
        for corner in TRACK_CORNERS:
            want = track_rows(case["rows"], case["counts"], n_clips, C, GATE, *corner)
            out[(n_clips, T, C), corner] = (case, want, track_features(case, n_clips, T, C, *corner))
    return out


def _opts(corner):
    return {"gate_deg": GATE, "max_gap": corner[0], "min_len": corner[1], "smooth": corner[2]}


def _device_track(ops, rows, counts, n_clips, C, opts, junk=7):
    """``ops.track_rows`` with the rows in a capacity buffer (junk rows behind the counted ones), the workspace and the outputs
    pre-filled -> (rows, counts, ids, status) on the host."""
    frames = len(counts)
    buf = ops.track_buffers(DEV, frames, C)
    buf["ws"].fill_(float("nan"))
    buf["rows"].fill_(float("nan"))
    buf["ids"].fill_(-7)
    buf["counts"].fill_(-7)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    padded = np.concatenate([rows.reshape(-1, 5), np.full((junk, 5), 9.0, dtype=np.float32)])
    got = ops.track_rows(torch.from_numpy(padded).to(DEV), torch.from_numpy(counts).to(DEV), n_clips, C, opts, buf=buf,
                         status=status)
    assert got[1].data_ptr() == buf["counts"].data_ptr() and int(buf["counts"][frames]) == got[0].shape[0] == got[2].shape[0]
    return got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy(), int(status.cpu()[0])


@pytest.mark.parametrize("config", range(len(TRACK_CONFIGS)))
def test_kernels_equal_the_host_definition(ops, cases, config):
    # the inputs are not empty of what the kernels must get right: every rule is reached in some configuration and corner
    # (one frame cannot hold them all), and each configuration reaches what its size allows
    seen = {}
    for (_, _, feat) in cases.values():
        for k, v in feat.items():
            seen[k] = seen.get(k, False) or v
    assert all(seen[k] for k in ("silent_block", "empty_frames", "rows_64", "rows_65", "ninth_track", "pruned_with_fills",
                                 "slot_reuse", "clip_boundary", "bad_vector", "filled", "rows_out")), seen
    n_clips, T, C = TRACK_CONFIGS[config]
    for corner in TRACK_CORNERS:
        case, ((want_rows, want_counts), want_ids, want_status), feat = cases[TRACK_CONFIGS[config], corner]
        assert feat["rows_65"] and feat["ninth_track"]
        if T >= 30:
            assert feat["rows_64"] and feat["bad_vector"] and feat["pruned_with_fills"] == (corner[1] > 2)
            assert feat["slot_reuse"] or (T < 48 and corner[0] == 5)
        assert feat["clip_boundary"] == (n_clips > 1) and (feat["empty_frames"] or T < 60) and (feat["silent_block"] or T < 129)
        rows, counts, ids, status = _device_track(ops, case["rows"], case["counts"], n_clips, C, _opts(corner))
        print("clips %d, T' %d, C %d, corner %s: %d rows in, %d out, status %d" % (n_clips, T, C, corner, len(case["rows"]),
                                                                                   len(want_rows), want_status))
        assert status == want_status
        assert np.array_equal(counts, want_counts)
        assert rows.shape == want_rows.shape and np.array_equal(rows.view(np.int32), want_rows.view(np.int32))
        assert np.array_equal(ids, want_ids)


def test_status_bits_and_refusals(ops):
    from adyolo_amd import _lib
    from adyolo_amd.postprocess import TRACK_BAD_ROWS, track_rows
    d = [0.6, 0.0, 0.8]
    rows = np.asarray([[0, 0] + d, [0, 1] + d, [1, 1] + d, [2, 0] + d], dtype=np.float32)
    opts = {"gate_deg": GATE, "max_gap": 0, "min_len": 1, "smooth": 1.0}

    def both(rows, counts, C, junk):
        (want_rows, want_counts), want_ids, want_status = track_rows(rows, counts, 1, C, GATE, 0, 1, 1.0)
        got = _device_track(ops, rows, np.asarray(counts, dtype=np.int32), 1, C, opts, junk=junk)
        assert got[3] == want_status and np.array_equal(got[1], want_counts) and np.array_equal(got[2], want_ids)
        assert np.array_equal(got[0].view(np.int32), want_rows.view(np.int32))
        return want_status, want_counts.tolist()

    assert both(rows, [2, 1, 1], 2, 3) == (0, [2, 1, 1])
    # counts that run past the rows given (no junk behind them: nothing may be read there), a negative count, a class >= C:
    # reported, and the frames and rows that are in order still come out, as the definition has them
    assert both(rows, [2, 1, 2], 2, 0) == (TRACK_BAD_ROWS, [2, 1, 0])
    assert both(rows, [2, 1, 1000000], 2, 0) == (TRACK_BAD_ROWS, [2, 1, 0])
    assert both(rows, [2, -1, 1], 2, 3) == (TRACK_BAD_ROWS, [2, 0, 1])
    assert both(rows, [2, 1, 1], 1, 3) == (TRACK_BAD_ROWS, [1, 0, 1])
    # every EINVAL of the C entry point, before a launch: the status word and the outputs keep their fill
    lib = _lib.load()
    frames, C = 4, 3
    buf = ops.track_buffers(DEV, frames, C)
    for t in (buf["rows"], buf["ws"]):
        t.fill_(float("nan"))
    buf["counts"].fill_(-7)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    r, c = torch.zeros(8, 5, device=DEV), torch.zeros(frames, dtype=torch.int32, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                                    # noqa: E731
    good = dict(rows=P(r), n_rows=8, counts=P(c), n_clips=2, t_clip=2, C=C, cos=0.9, max_gap=2, min_len=3, a=0.5, b=0.5,
                ws=P(buf["ws"]), out=P(buf["rows"]), ids=P(buf["ids"]), cap=buf["rows"].shape[0], oc=P(buf["counts"]),
                status=P(status))

    def rc(**kw):
        a = dict(good)
        a.update(kw)
        return lib.adyolo_track_rows(*[a[k] for k in ("rows", "n_rows", "counts", "n_clips", "t_clip", "C", "cos", "max_gap",
                                                      "min_len", "a", "b", "ws", "out", "ids", "cap", "oc", "status")], None)

    bad = [dict(rows=None), dict(counts=None), dict(ws=None), dict(out=None), dict(ids=None), dict(oc=None), dict(status=None),
           dict(ws=ctypes.c_void_p(buf["ws"].data_ptr() + 4)), dict(out=ctypes.c_void_p(buf["rows"].data_ptr() + 2)),
           dict(n_clips=0), dict(t_clip=0), dict(n_clips=-1, t_clip=-4), dict(C=0), dict(max_gap=-1), dict(min_len=0),
           dict(cos=0.0), dict(cos=1.0), dict(cos=-0.5), dict(cos=float("nan")), dict(a=0.0), dict(a=1.5), dict(a=float("nan")),
           dict(cap=frames * C * 8 - 1), dict(n_rows=-1)]
    for kw in bad:
        assert rc(**kw) == -1, kw                                                  # ADYOLO_EINVAL
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == -7 and bool((buf["counts"] == -7).all()) and bool(torch.isnan(buf["rows"]).all())
    assert rc() == 0 and rc(a=1.0, b=0.0) == 0
    torch.cuda.synchronize()
    assert buf["counts"].cpu().tolist() == [0] * (frames + 1)
    # the Python surface refuses what it can see
    with pytest.raises(_lib.AdyoloHipError, match="clips"):
        ops.track_rows(r, c, 3, C, opts)
    with pytest.raises(_lib.AdyoloHipError, match="counts"):
        ops.track_rows(r, c.long(), 2, C, opts)
    with pytest.raises(_lib.AdyoloHipError, match="track_buffers"):
        ops.track_rows(r, c, 2, C, opts, buf=ops.track_buffers(DEV, frames - 1, C))
    with pytest.raises(_lib.AdyoloHipError, match="no CPU path"):
        ops.track_rows(r.cpu(), c, 2, C, opts)
    with pytest.raises(_lib.AdyoloHipError, match="cos_gate"):
        ops.track_rows(r, c, 2, C, dict(opts, gate_deg=0.0))
    # trim=False with given buffers: the given tensors come back, nothing is allocated
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.track_rows(r, c, 2, C, opts, buf=buf, status=st, trim=False)              # (the first call may load kernels)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    out_rows, out_counts, out_ids = ops.track_rows(r, c, 2, C, opts, buf=buf, status=st, trim=False)
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before
    assert out_rows.data_ptr() == buf["rows"].data_ptr() and out_rows.shape == buf["rows"].shape
    assert out_ids.data_ptr() == buf["ids"].data_ptr() and out_counts.data_ptr() == buf["counts"].data_ptr()
    assert out_counts.shape == (frames,)


# ------------------------------------------------------------------------------------------------------------ the epochs
def _reference_dir(root):
    ref = os.path.join(root, "reference")
    shutil.copytree(os.path.join(root, "metadata_dev", "dev-test"), ref)
    for name in os.listdir(ref):
        if os.path.getsize(os.path.join(ref, name)) == 0:
            with open(os.path.join(ref, name), "w") as fid:
                fid.write("3,1,0,10.0,5.0\n")
    return ref


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("gpu_track_split"))
    write_eval_split(root)
    return root, _reference_dir(root)


def _chain(root, loss, nb_classes):
    from adyolo_amd.corpus import EvalDeviceCorpus, load_eval_split
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    prm = eval_params(root, loss=loss, nb_classes=nb_classes, device=DEV)
    torch.manual_seed(8)
    model = WrapperModel((1, 7, 80, 64), (), prm).to(DEV).eval()
    corpus = EvalDeviceCorpus(load_eval_split(prm, "test", rank=0, world=1, verify="all"), prm, DEV)
    return prm, model, FeatureExtractor(None, DEV), WrapperCriterion(prm), corpus


class _Recorder:
    """Stands where a device scorer stands in a pass and keeps every batch's rows on the host."""

    def __init__(self, scorer):
        self.scorer, self.batches = scorer, []

    def add_rows(self, rows, counts, clips):
        self.scorer.add_rows(rows, counts, clips)
        counts_h = counts.cpu().numpy()
        self.batches.append((rows[:int(counts_h.sum())].cpu().numpy().copy(), counts_h.copy(), list(clips)))


def _tracked_on_the_host(batches, nb_classes, opts, scorer, out_dir):
    """The baseline: every recorded batch through ``postprocess.track_rows``; the tracked rows uploaded as float32 to the
    scorer and written with their ids.  -> (rows in, rows out, status bits)"""
    from adyolo_amd.postprocess import group_rows, track_groups, track_rows, write_seld_output_file
    if out_dir is not None:
        os.makedirs(out_dir)
    n_in = n_out = bits = 0
    for rows, counts, clips in batches:
        (out, oc), ids, status = track_rows(rows, counts, len(clips), nb_classes, opts["gate_deg"], opts["max_gap"],
                                            opts["min_len"], opts["smooth"])
        n_in, n_out, bits = n_in + len(rows), n_out + len(out), bits | status
        scorer.add_rows(torch.from_numpy(out).to(DEV), torch.from_numpy(oc).to(DEV), clips)
        if out_dir is not None:
            for name, clip_rows, clip_ids in zip(clips, group_rows(out, oc, len(clips)), track_groups(ids, oc, len(clips))):
                write_seld_output_file(os.path.join(out_dir, name + ".csv"), clip_rows, clip_ids)
    return n_in, n_out, bits


def _files(d, names):
    assert sorted(os.listdir(d)) == sorted(n + ".csv" for n in names)
    return [open(os.path.join(d, n + ".csv"), "rb").read() for n in names]


def _same_accumulators(scorer_a, scorer_b):
    (acc_a, names_a), (acc_b, names_b) = scorer_a.accumulators(), scorer_b.accumulators()
    assert names_a == names_b and len(names_a) > 0
    assert np.array_equal(acc_a.view(np.int64), acc_b.view(np.int64))


def _first_threshold_with_rows(atest, corpus, model, fx, crit, post):
    """The first of 0.5, 0.3, 0.1, 0.05 at which the plain pass of the untrained model selects any row."""
    from adyolo_amd.seld_metrics import DeviceSELDScorer

    class _Count:
        n = 0

        def add_rows(self, rows, counts, clips):
            self.n += int(counts.sum())
    for th in (0.5, 0.3, 0.1, 0.05):
        post.set_conf_thresh(th)
        count = _Count()
        atest.test_epoch_corpus(corpus, model, fx, crit, post, None, batch_size=4, device_scorer=count)
        if count.n:
            return th
    raise AssertionError("the untrained model selects no row at any threshold")


@pytest.mark.parametrize("loss,nb_classes", [("adyolo", 12), ("adpit", 13)])
@pytest.mark.parametrize("tta", [None, [0, 5]], ids=["plain", "tta"])
def test_epoch_equals_the_rows_tracked_on_the_host(ops, split, tmp_path, loss, nb_classes, tta):
    import warnings
    from adyolo_amd import test as atest
    from adyolo_amd.augmentations import track_options
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root, ref = split
    prm, model, fx, crit, corpus = _chain(root, loss, nb_classes)
    post = LabelPostProcessor(prm)
    names = corpus.get_filelist()
    prm["test_config"] = {"track": True}
    opts = track_options(prm)
    assert opts == {"gate_deg": 20.0, "max_gap": 2, "min_len": 3, "smooth": 0.5}
    th = _first_threshold_with_rows(atest, corpus, model, fx, crit, post)
    if tta is not None:            # (the untrained AD-YOLO head fills more than the default pool: the largest two views allow)
        tta = {"views": tta, "min_views": 1, "unify_thresh": 15.0, "max_rows_per_frame": 512}
    sc_plain, sc_again, sc_want, sc_got = (DeviceSELDScorer(prm, ref, DEV) for _ in range(4))
    out_plain, out_again, out_want, out_got = (str(tmp_path / k) for k in ("plain", "again", "want", "got"))
    rec = _Recorder(sc_plain)
    loss_plain = atest.test_epoch_corpus(corpus, model, fx, crit, post, out_plain, batch_size=4, device_scorer=rec, tta=tta)
    n_in, n_out, bits = _tracked_on_the_host(rec.batches, nb_classes, opts, sc_want, out_want)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                            # (the caps of the definition only warn)
        loss_got = atest.test_epoch_corpus(corpus, model, fx, crit, post, out_got, batch_size=4, device_scorer=sc_got, tta=tta,
                                           track=opts)
    print("%s at %.2f: %d rows, %d tracked, status %d, mean loss %r" % (loss, th, n_in, n_out, bits, loss_got))
    assert n_in > 0 and loss_got == loss_plain and loss_plain > 0
    assert _files(out_want, names) == _files(out_got, names)
    _same_accumulators(sc_want, sc_got)
    assert _files(out_plain, names) != _files(out_got, names)                      # tracking does change the result
    # without files the pass gives the scorer the same rows (and synchronises once, at its end)
    sc_quiet = DeviceSELDScorer(prm, ref, DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert atest.test_epoch_corpus(corpus, model, fx, crit, post, None, batch_size=4, device_scorer=sc_quiet, tta=tta,
                                       track=opts) == loss_plain
    _same_accumulators(sc_want, sc_quiet)
    # track=None: a second plain call gives the first one's bytes and accumulator bits
    assert atest.test_epoch_corpus(corpus, model, fx, crit, post, out_again, batch_size=4, device_scorer=sc_again, tta=tta,
                                   track=None) == loss_plain
    assert _files(out_plain, names) == _files(out_again, names)
    _same_accumulators(sc_plain, sc_again)
    assert all(line.split(b",")[2] == b"0" for data in _files(out_plain, names) for line in data.splitlines())


def test_sweep_equals_the_rows_tracked_on_the_host_per_threshold(ops, split, tmp_path):
    import warnings
    from adyolo_amd import test as atest
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root, ref = split
    prm, model, fx, crit, corpus = _chain(root, "adyolo", 12)
    names = corpus.get_filelist()
    opts = {"gate_deg": 20.0, "max_gap": 2, "min_len": 3, "smooth": 0.5}
    thresholds = (0.3, 0.6, 0.4)       # (the untrained head selects nothing at 0.6; the last one's files are the ones compared)
    post = LabelPostProcessor(prm)
    table, best, best_th = [], 9999.0, None
    for k, th in enumerate(thresholds):
        post.set_conf_thresh(th)
        rec, sc = _Recorder(DeviceSELDScorer(prm, ref, DEV)), DeviceSELDScorer(prm, ref, DEV)
        loss = atest.test_epoch_corpus(corpus, model, fx, crit, post, None, batch_size=4, device_scorer=rec)
        _tracked_on_the_host(rec.batches, 12, opts, sc, str(tmp_path / ("want%d" % k)))
        table.append(list(sc.scores()[:5]))
        if table[-1][4] < best:
            best_th, best = th, table[-1][4]
    post_b = LabelPostProcessor(prm)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = atest.sweep_conf_thresh_corpus(corpus, model, fx, crit, post_b, DeviceSELDScorer(prm, ref, DEV),
                                             thresholds=thresholds, output_pth=str(tmp_path / "sweep"), batch_size=4, track=opts)
    print("sweep:", got)
    assert got[0] == best_th and post_b.get_conf_thresh() == best_th and got[2] == loss
    assert np.array_equal(np.asarray(got[1], dtype=np.float64).view(np.int64), np.asarray(table, dtype=np.float64).view(np.int64))
    assert _files(str(tmp_path / ("want%d" % (len(thresholds) - 1))), names) == _files(str(tmp_path / "sweep"), names)
    # track=None: the sweep as it was, twice the same table and files
    plain = [atest.sweep_conf_thresh_corpus(corpus, model, fx, crit, LabelPostProcessor(prm), DeviceSELDScorer(prm, ref, DEV),
                                            thresholds=thresholds, output_pth=str(tmp_path / ("plain%d" % k)), batch_size=4,
                                            track=None) for k in range(2)]
    assert plain[0][0] == plain[1][0] and plain[0][2] == plain[1][2] == loss
    assert np.array_equal(np.asarray(plain[0][1]).view(np.int64), np.asarray(plain[1][1]).view(np.int64))
    assert _files(str(tmp_path / "plain0"), names) == _files(str(tmp_path / "plain1"), names)
    assert _files(str(tmp_path / "plain0"), names) != _files(str(tmp_path / "sweep"), names)
