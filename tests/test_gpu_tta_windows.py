"""GPU: rotation test-time augmentation through windows (csrc/corpus.hip ``adyolo_corpus_gather_windows_view``,
``corpus._WindowCorpus.launch_view``, ``test.test_epoch_windows`` / ``sweep_conf_thresh_windows`` / ``infer_epoch_corpus`` with
``tta=``).

The gather against its composition, int32 bit equality: ``ops.corpus_gather_windows`` then ``rotate_audio`` / ``swap_audio``
under all 16 FOA and all 8 MIC combinations, on a table whose ``valid`` is 0, 1, n, n - 1 and a mid value, at an even and an odd
window length (the padding past ``valid`` is turned too); bad rows, combination 16 and a MIC non-symmetry.

The pipeline, with the small model of test_gpu_tta.py on the MIXED recordings of test_gpu_eval_windows.py: the windowed pass with
views against every view run on its own -- the plain window gather, ``rotate_audio`` / ``swap_audio``, the eager forward,
decode, stitch and selection -- merged on the host by ``merge_view_rows`` (CSV bytes, accumulator bits, the loss float of the
plain pass); recordings of exactly one window against ``test_epoch_corpus(tta=...)``; with tracking against the merged whole
recordings tracked by ``track_rows``; inference; the sweep against one fresh pass per threshold (atol 1e-9, the bound
test_gpu_eval_windows.py and test_gpu_track_windows.py hold the windowed sweeps to); one host copy per pass over the split."""
import os
import shutil
import warnings

import numpy as np
import pytest
import torch

from test_eval_corpus_cpu import eval_params, write_eval_split
from test_gpu_eval_windows import BATCH, MIXED, ONE_WINDOW, _acc_bits, _read, _reference_dir
from test_gpu_track_windows import OPTS, _tracked_whole

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = (0, 12, 30, 45, 110)
VIEWS = [0, 5, 10]
# (loss, classes, min_views, pool rows per frame): the cases of test_gpu_tta.py -- the untrained AD-YOLO head selects more than
# 64 rows in a frame, so its pool is the largest three views allow
CASES = [("adyolo", 12, 1, 340), ("adpit", 13, 2, 64), ("accdoa", 13, 1, 64)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


# ---------------------------------------------------------------------------------------------------------------- the gather
def _table(n, n_total):
    """W = 5 windows: valid 0, 1, n, n - 1 and a mid value, at even offsets inside a stream of n_total frames."""
    rows = [(6, 0), (2, 1), (10, n), (4, n - 1), (100, n // 2 + 1)]
    assert all(off % 2 == 0 and off + valid <= n_total for off, valid in rows)
    return torch.tensor([[off, valid, 0, 0, 0, 0, 0, 0] for off, valid in rows], dtype=torch.int64, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n", [4800, 4801], ids=["even", "odd"])
def test_the_view_gather_is_the_plain_gather_then_the_turn(ops, n):
    from adyolo_amd import _lib
    from adyolo_amd.augmentations import COMBINATIONS, MIC_SWAP_COMBS, mic_swap_source, rotate_audio, swap_audio
    n_total = 2 * n + 200
    pcm = torch.randint(-32768, 32768, (n_total, 4), generator=torch.Generator().manual_seed(n), dtype=torch.int32)
    pcm = pcm.to(torch.int16).to(DEV)
    table = _table(n, n_total)
    w = table.shape[0]
    rot = ops.corpus_rot_table(COMBINATIONS)
    mic = ops.corpus_mic_table({k: mic_swap_source(k) for k in MIC_SWAP_COMBS})
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    plain = ops.corpus_gather_windows(pcm, table, torch.empty((w, n, 4), device=DEV), status)
    assert bool((plain[0] == plain[0, 0, 0]).all()) and float(plain[0, 0, 0]) == float(np.float32(1e-8))      # valid = 0: padding
    out = torch.full((w, n, 4), float("nan"), device=DEV)
    for comb in range(16):                                                     # FOA: signs and the swap, the padding included
        out.fill_(float("nan"))
        assert ops.corpus_gather_windows_view(pcm, table, comb, rot, out, status).data_ptr() == out.data_ptr()
        want = rotate_audio(plain, [comb] * w)
        assert torch.equal(_bits(out), _bits(want)), comb
        if comb:
            assert not torch.equal(_bits(out), _bits(plain)), comb
            assert not torch.equal(_bits(out[0]), _bits(plain[0])) or COMBINATIONS[comb][0] == (1, 1, 1)   # the turned padding
    for comb in (0, -1):                                                       # no view: the plain gather's bits, either form
        for kw in ({}, {"mic_src": mic}):
            out.fill_(float("nan"))
            ops.corpus_gather_windows_view(pcm, table, comb, rot, out, status, **kw)
            assert torch.equal(_bits(out), _bits(plain)), comb
    for comb in MIC_SWAP_COMBS:                                                # MIC: the capsules permuted
        out.fill_(float("nan"))
        ops.corpus_gather_windows_view(pcm, table, comb, None, out, status, mic_src=mic)
        assert torch.equal(_bits(out), _bits(swap_audio(plain, [comb] * w))), comb
    assert int(status.item()) == 0
    # refusals.  Bad rows: zeros for that window and the status bit, the neighbours intact
    bad = table.clone()
    bad[1, 0] = 3                                                              # an odd offset
    bad[2, 1] = n + 1                                                          # valid > n
    bad[3, 0] = (n_total - n + 4) // 2 * 2                                     # (even) the window runs past the stream
    for kw, comb, turn in (({}, 6, rotate_audio), ({"mic_src": mic}, 9, swap_audio)):
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        out.fill_(float("nan"))
        ops.corpus_gather_windows_view(pcm, bad, comb, rot, out, st, **kw)
        want = turn(plain, [comb] * w)
        assert int(st.item()) == 2 and bool((out[1:4] == 0).all())
        assert torch.equal(_bits(out[0]), _bits(want[0])) and torch.equal(_bits(out[4]), _bits(want[4]))
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    out.fill_(float("nan"))
    ops.corpus_gather_windows_view(pcm, table, 1, None, out, st, mic_src=mic)  # no symmetry of the array: what corpus_gather does
    assert int(st.item()) == 2 and bool((out == 0).all())
    with pytest.raises(_lib.AdyoloHipError):
        ops.corpus_gather_windows_view(pcm, table, 16, rot, out, st)
    with pytest.raises(_lib.AdyoloHipError, match="rotation table"):
        ops.corpus_gather_windows_view(pcm, table, 3, None, out, st)
    with pytest.raises(_lib.AdyoloHipError):
        ops.corpus_gather_windows_view(pcm, table, 3, rot, out[:4], st)


# -------------------------------------------------------------------------------------------------------------- the pipeline
def _chain(root, loss, nb_classes, mic=False):
    from adyolo_amd.corpus import load_eval_split
    from adyolo_amd.features import FeatureExtractor, MicFeatureExtractor
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    prm = eval_params(root, loss=loss, nb_classes=nb_classes, device=DEV)
    if mic:
        prm["data_config"]["audio_format"] = "mic"
    torch.manual_seed(8)
    model = WrapperModel((1, 10 if mic else 7, 80, 64), (), prm).to(DEV).eval()
    hc = load_eval_split(prm, "test", rank=0, world=1, verify="all")
    fx = MicFeatureExtractor(None, DEV) if mic else FeatureExtractor(None, DEV)
    return prm, model, fx, WrapperCriterion(prm), LabelPostProcessor(prm), hc


def _options(prm, post, views, min_views, pool_rows):
    from adyolo_amd.augmentations import tta_options
    prm["test_config"] = {"tta_views": list(views[1:]), "tta_min_views": min_views, "tta_max_rows_per_frame": pool_rows}
    opt = tta_options(prm, postprocessor=post)
    assert opt["views"] == list(views) and opt["unify_thresh"] == 15.0 and opt["max_rows_per_frame"] == pool_rows
    return opt


def _view_runs(ops, corpus, model, fx, post, views, turn):
    """The reference route, view by view: per pass the plain window gather, the audio turned by ``turn``, the eager forward,
    decode, stitch and device selection of the run -> per pass, per view (rows, counts) on the host."""
    b, wf = corpus.batch_size, corpus.window_frames
    runs = []
    with torch.no_grad():
        for p in range(corpus.n_passes):
            audio = ops.corpus_gather_windows(corpus.pcm, corpus.pass_table(p), torch.empty((b, corpus.n_samples, 4), device=DEV),
                                              corpus.status)
            per_view = []
            for v in views:
                audio_v = audio if v == 0 else turn(audio, [v] * b)
                dec = post.decode_device(model(fx(audio_v, channels_last8=True), channels_last8=True))
                stitched = torch.zeros_like(dec)
                ops.decode_stitch(dec, corpus.pass_table(p), wf, corpus.pass_base[p], stitched, corpus.status)
                rows, counts = post.select_device_rows(stitched[:corpus.pass_frames[p]], 1)
                per_view.append((rows.cpu().numpy(), counts.cpu().numpy()))
            runs.append(per_view)
    corpus.check()
    return runs


def _write(out_dir, names, outs, ids=None):
    from adyolo_amd.postprocess import write_seld_output_file
    os.makedirs(out_dir)
    for k, name in enumerate(names):
        write_seld_output_file(os.path.join(out_dir, name + ".csv"), outs[k], None if ids is None else ids[k])


def _merged_per_run(corpus, runs, opt, scorer, out_dir):
    """``merge_view_rows`` per run; the merged rows to ``scorer`` through ``add_run`` and to files.  -> merged rows in all."""
    from adyolo_amd.corpus import split_pass_rows
    from adyolo_amd.postprocess import merge_view_rows
    names = corpus.get_filelist()
    outs, total = [{} for _ in names], 0
    segments = corpus.segments(scorer) if scorer is not None else None
    for p, per_view in enumerate(runs):
        (rows, counts), status = merge_view_rows(per_view, opt["views"], opt["unify_thresh"], opt["min_views"],
                                                 max_rows_per_frame=opt["max_rows_per_frame"])
        assert status == 0 and len(counts) == corpus.pass_frames[p]
        total += len(rows)
        if scorer is not None:
            scorer.add_run(torch.from_numpy(rows).to(DEV), torch.from_numpy(counts).to(DEV), segments[p])
        for r, found in split_pass_rows(rows, counts, corpus.pass_base[p], corpus.frame_start).items():
            outs[r].update(found)
    _write(out_dir, names, outs)
    return total


def _merged_whole_recordings(corpus, runs, opt, out_dir):
    """Every view's rows laid on the axis of all recordings, cut per recording and merged there whole -> one CSV each."""
    from adyolo_amd.postprocess import group_rows, merge_view_rows
    names = corpus.get_filelist()
    axis = []
    for k in range(len(opt["views"])):
        rows = []
        for p, per_view in enumerate(runs):
            r = per_view[k][0].copy()
            r[:, 0] += corpus.pass_base[p]
            rows.append(r)
        axis.append((np.concatenate(rows), np.concatenate([per_view[k][1] for per_view in runs])))
    start = [int(v) for v in corpus.frame_start]
    outs = []
    for r in range(len(names)):
        lo, hi = start[r], start[r + 1]
        if hi == lo:
            outs.append({})
            continue
        per_view = []
        for rows, counts in axis:
            offs = np.concatenate([[0], np.cumsum(counts)])
            part = rows[offs[lo]:offs[hi]].copy()
            part[:, 0] -= lo
            per_view.append((part, counts[lo:hi]))
        (rows, counts), status = merge_view_rows(per_view, opt["views"], opt["unify_thresh"], opt["min_views"],
                                                 max_rows_per_frame=opt["max_rows_per_frame"])
        assert status == 0
        outs.append(group_rows(rows, counts, 1)[0])
    _write(out_dir, names, outs)


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("gpu_tta_windows"))
    return root, write_eval_split(root, clips=MIXED, seed=9), _reference_dir(root)


@pytest.fixture(scope="module")
def cases(ops, mixed, tmp_path_factory):
    """Per loss, made once and shared: the chain, the windowed corpus, the options, the plain pass (loss, files) and the
    reference route's files and scorer."""
    from adyolo_amd import test as atest
    from adyolo_amd.augmentations import rotate_audio
    from adyolo_amd.corpus import EvalWindowCorpus
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root, written, ref = mixed
    made = {}

    def get(loss):
        if loss in made:
            return made[loss]
        _, nb_classes, min_views, pool_rows = [c for c in CASES if c[0] == loss][0]
        prm, model, fx, crit, post, hc = _chain(root, loss, nb_classes)
        corpus = EvalWindowCorpus(hc, prm, DEV, window_s=3, margin_s=1.0, batch_size=BATCH)
        names = corpus.get_filelist()
        assert corpus.label_frames == [dict(zip([n for n, _ in MIXED], FRAMES))[n] for n in names]
        assert (corpus.n_windows, corpus.n_passes) == (14, 5)
        opt = _options(prm, post, VIEWS, min_views, pool_rows)
        out = str(tmp_path_factory.mktemp("case_" + loss))
        sc_plain, sc_want = DeviceSELDScorer(prm, ref, DEV), DeviceSELDScorer(prm, ref, DEV)
        loss_plain = atest.test_epoch_windows(corpus, model, fx, crit, post, os.path.join(out, "plain"), device_scorer=sc_plain)
        runs = _view_runs(ops, corpus, model, fx, post, VIEWS, rotate_audio)
        n_rows = _merged_per_run(corpus, runs, opt, sc_want, os.path.join(out, "want"))
        made[loss] = dict(prm=prm, model=model, fx=fx, crit=crit, post=post, hc=hc, corpus=corpus, names=names, opt=opt, ref=ref,
                          nb_classes=nb_classes, written=written, out=out, loss_plain=loss_plain, runs=runs, n_rows=n_rows,
                          plain=_read(os.path.join(out, "plain"), names), want=_read(os.path.join(out, "want"), names),
                          sc_want=sc_want)
        return made[loss]
    return get


def test_launch_view_turns_the_pass_with_its_padding(ops, cases):
    from adyolo_amd.augmentations import rotate_audio
    c = cases("adyolo")
    corpus = c["corpus"]
    assert min(int(v) for v in corpus.table_host[:, 1]) < corpus.n_samples                     # short windows: padded
    for p in (0, corpus.n_passes - 1):                                                         # (the last pass: an empty window)
        audio = corpus.launch(p)[0]
        assert torch.equal(_bits(corpus.launch_view(p, 0)), _bits(audio))
        for v in (6, 13):
            out = torch.empty_like(audio)
            assert corpus.launch_view(p, v, out).data_ptr() == out.data_ptr()
            assert torch.equal(_bits(out), _bits(rotate_audio(audio, [v] * corpus.batch_size)))
    with pytest.raises(ValueError):
        corpus.launch_view(0, 16)
    with pytest.raises(ValueError):
        corpus.launch_view(corpus.n_passes, 3)
    corpus.check()


@pytest.mark.parametrize("loss", [c[0] for c in CASES])
def test_mixed_lengths_equal_the_views_merged_on_the_host(ops, cases, tmp_path, loss):
    from adyolo_amd import test as atest
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    c = cases(loss)
    corpus, names, opt = c["corpus"], c["names"], c["opt"]
    bits_want, order_want = _acc_bits(c["sc_want"])
    assert c["n_rows"] > 0 and c["loss_plain"] > 0                                             # merged rows exist
    assert any(c["plain"][n] != c["want"][n] for n in names)                                   # the views do change the result
    fg = ForwardGraphs(c["model"], c["fx"], c["post"], warm_calls=0)
    for key, forward in (("eager", None), ("graph", fg)):
        sc = DeviceSELDScorer(c["prm"], c["ref"], DEV)
        got_loss = atest.test_epoch_windows(corpus, c["model"], c["fx"], c["crit"], c["post"], str(tmp_path / key), forward=forward,
                                            device_scorer=sc, tta=opt)
        print("%s %s: %d merged rows, loss %r, plain %r" % (loss, key, c["n_rows"], got_loss, c["loss_plain"]))
        assert got_loss == c["loss_plain"]                                                     # view 0's: the same float
        assert _read(str(tmp_path / key), names) == c["want"]
        bits, order = _acc_bits(sc)
        assert order == order_want and np.array_equal(bits, bits_want)
        assert int(corpus.status.item()) == 0
    assert fg.captures == 1 and fg.evictions == 0 and fg.replays >= len(VIEWS) * corpus.n_passes - 1     # one graph, every view
    # tta=None: the plain pass's bytes
    assert atest.test_epoch_windows(corpus, c["model"], c["fx"], c["crit"], c["post"], str(tmp_path / "none"),
                                    tta=None) == c["loss_plain"]
    assert _read(str(tmp_path / "none"), names) == c["plain"]


@pytest.mark.parametrize("loss,nb_classes,min_views,pool_rows", CASES[:2])
def test_one_window_recordings_equal_the_whole_clip_pass_with_views(ops, tmp_path, loss, nb_classes, min_views, pool_rows):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import EvalDeviceCorpus, EvalWindowCorpus
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root = str(tmp_path)
    write_eval_split(root, clips=ONE_WINDOW)
    ref = _reference_dir(root)
    prm, model, fx, crit, post, hc = _chain(root, loss, nb_classes)
    opt = _options(prm, post, VIEWS, min_views, pool_rows)
    whole = EvalDeviceCorpus(hc, prm, DEV)
    names = whole.get_filelist()
    corpus = EvalWindowCorpus(hc, prm, DEV, window_s=2, margin_s=0.0, batch_size=2)
    assert (corpus.n_windows, corpus.n_passes) == (4, 2) and corpus.get_filelist() == names
    sc_a, sc_b = DeviceSELDScorer(prm, ref, DEV), DeviceSELDScorer(prm, ref, DEV)
    loss_a = atest.test_epoch_corpus(whole, model, fx, crit, post, str(tmp_path / "whole"), batch_size=2, device_scorer=sc_a, tta=opt)
    loss_b = atest.test_epoch_windows(corpus, model, fx, crit, post, str(tmp_path / "windows"), device_scorer=sc_b, tta=opt)
    want = _read(str(tmp_path / "whole"), names)
    assert loss_a == loss_b and loss_a > 0 and sum(len(v) for v in want.values()) > 0
    assert _read(str(tmp_path / "windows"), names) == want
    (bits_a, names_a), (bits_b, names_b) = _acc_bits(sc_a), _acc_bits(sc_b)
    assert names_a == names_b and len(names_a) == 4 and np.array_equal(bits_a, bits_b)


@pytest.mark.parametrize("loss", ["adyolo", "adpit"])
def test_views_then_tracks_equal_merged_whole_recordings_tracked_on_the_host(ops, cases, tmp_path, loss):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import InferDeviceCorpus, infer_split_from_arrays
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    c = cases(loss)
    corpus, names, opt = c["corpus"], c["names"], c["opt"]
    frames = corpus.label_frames
    # the host route: per-view rows, merge_view_rows on whole recordings (the bytes of the merge run by run), then track_rows
    _merged_whole_recordings(corpus, c["runs"], opt, str(tmp_path / "merged"))
    merged = _read(str(tmp_path / "merged"), names)
    assert merged == c["want"]
    sc_want, n_in, n_out = _tracked_whole(ops, merged, names, frames, c["nb_classes"], OPTS, c["prm"], c["ref"], str(tmp_path / "want"))
    want = _read(str(tmp_path / "want"), names)
    assert n_in > 0 and n_out > 0 and want != merged
    bits_want, order_want = _acc_bits(sc_want)
    sc = DeviceSELDScorer(c["prm"], c["ref"], DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                        # (the caps of the definition only warn)
        got_loss = atest.test_epoch_windows(corpus, c["model"], c["fx"], c["crit"], c["post"], str(tmp_path / "got"),
                                            device_scorer=sc, tta=opt, tracking=OPTS)
    assert got_loss == c["loss_plain"]
    assert _read(str(tmp_path / "got"), names) == want
    bits, order = _acc_bits(sc)
    assert order == order_want and np.array_equal(bits, bits_want)
    # inference: the same recordings without labels, its own hold (7 frames against the scorer's block of 10)
    rec = [n for n, _ in MIXED]
    infer = InferDeviceCorpus(infer_split_from_arrays(rec, [c["written"][n][0] for n in rec], c["prm"]), c["prm"], DEV, window_s=3,
                              margin_s=1.0, batch_size=BATCH)
    assert infer.label_frames == list(FRAMES) and infer.track_plan(OPTS)["hold"] == 7
    info = atest.infer_epoch_corpus(infer, c["model"], c["fx"], c["post"], str(tmp_path / "infer"), tta=opt)
    assert info["passes"] == 5 and _read(str(tmp_path / "infer"), rec) == {n: c["want"][n] for n in rec}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert atest.infer_epoch_corpus(infer, c["model"], c["fx"], c["post"], str(tmp_path / "infer_tracked"), tta=opt,
                                        tracking=OPTS) == info
    assert _read(str(tmp_path / "infer_tracked"), rec) == {n: want[n] for n in rec}
    assert atest.infer_epoch_corpus(infer, c["model"], c["fx"], c["post"], str(tmp_path / "infer_plain"), tta=None) == info
    assert _read(str(tmp_path / "infer_plain"), rec) == {n: c["plain"][n] for n in rec}


def test_mic_recordings_under_two_swap_views(ops, tmp_path):
    from adyolo_amd import test as atest
    from adyolo_amd.augmentations import swap_audio
    from adyolo_amd.corpus import EvalWindowCorpus
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root = str(tmp_path / "split")
    write_eval_split(root, clips=MIXED, seed=9)
    shutil.move(os.path.join(root, "foa_dev"), os.path.join(root, "mic_dev"))
    ref = _reference_dir(root)
    prm, model, fx, crit, post, hc = _chain(root, "adpit", 13, mic=True)
    views = [0, 3, 9]
    opt = _options(prm, post, views, 2, 64)
    corpus = EvalWindowCorpus(hc, prm, DEV, window_s=3, margin_s=1.0, batch_size=BATCH)
    names = corpus.get_filelist()
    audio = corpus.launch(1)[0]
    for v in views[1:]:
        assert torch.equal(_bits(corpus.launch_view(1, v)), _bits(swap_audio(audio, [v] * BATCH)))
    with pytest.raises(ValueError, match="symmetry"):
        corpus.launch_view(1, 1)
    sc_want, sc_got = DeviceSELDScorer(prm, ref, DEV), DeviceSELDScorer(prm, ref, DEV)
    runs = _view_runs(ops, corpus, model, fx, post, views, swap_audio)
    n_rows = _merged_per_run(corpus, runs, opt, sc_want, str(tmp_path / "want"))
    loss_got = atest.test_epoch_windows(corpus, model, fx, crit, post, str(tmp_path / "got"), device_scorer=sc_got, tta=opt)
    loss_plain = atest.test_epoch_windows(corpus, model, fx, crit, post, str(tmp_path / "plain"))
    assert n_rows > 0 and loss_got == loss_plain and loss_plain > 0
    want = _read(str(tmp_path / "want"), names)
    assert _read(str(tmp_path / "got"), names) == want and _read(str(tmp_path / "plain"), names) != want
    (bits_a, names_a), (bits_b, names_b) = _acc_bits(sc_want), _acc_bits(sc_got)
    assert names_a == names_b and np.array_equal(bits_a, bits_b)
    assert int(corpus.status.item()) == 0


def test_the_sweep_equals_one_fresh_pass_per_threshold_and_a_pass_copies_once(ops, cases, tmp_path, monkeypatch):
    from adyolo_amd import test as atest
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    c = cases("adyolo")
    corpus, names, prm, ref = c["corpus"], c["names"], c["prm"], c["ref"]
    model, fx, crit = c["model"], c["fx"], c["crit"]
    thresholds = (0.3, 0.4, 0.6)        # (below 0.3 the untrained head fills more than the largest pool of three views)
    tta = {"views": [0, 5, 10], "min_views": 1, "unify_thresh": 15.0, "max_rows_per_frame": 340}
    want = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k, th in enumerate(thresholds):
            post_t = LabelPostProcessor(prm)
            post_t.set_conf_thresh(th)
            sc_t = DeviceSELDScorer(prm, ref, DEV)
            loss = atest.test_epoch_windows(corpus, model, fx, crit, post_t, str(tmp_path / ("want%d" % k)), device_scorer=sc_t,
                                            tta=tta, tracking=OPTS)
            want.append([float(v) for v in sc_t.scores()[:5]])
        fg = ForwardGraphs(model, fx, LabelPostProcessor(prm), warm_calls=0)
        for key, forward in (("eager", None), ("graph", fg)):
            post_s = LabelPostProcessor(prm)
            new_thresh, table, got_loss = atest.sweep_conf_thresh_windows(
                corpus, model, fx, crit, post_s, DeviceSELDScorer(prm, ref, DEV), thresholds=thresholds,
                output_pth=str(tmp_path / key), forward=forward, tta=tta, tracking=OPTS)
            print(key, "sweep:", new_thresh, table, got_loss)
            np.testing.assert_allclose(np.asarray(table, dtype=np.float64), np.asarray(want), rtol=0, atol=1e-9)
            assert got_loss == loss == c["loss_plain"]
            assert new_thresh == thresholds[int(np.argmin([row[4] for row in want]))] == post_s.get_conf_thresh()
            assert _read(str(tmp_path / key), names) == _read(str(tmp_path / ("want%d" % (len(thresholds) - 1))), names)
        assert fg.captures == 1 and fg.evictions == 0
        # without tracking, against the case's files at the configured threshold
        post_u = LabelPostProcessor(prm)
        th0 = post_u.get_conf_thresh()
        atest.sweep_conf_thresh_windows(corpus, model, fx, crit, post_u, DeviceSELDScorer(prm, ref, DEV), thresholds=(th0,),
                                        output_pth=str(tmp_path / "untracked"), tta=tta)
        assert _read(str(tmp_path / "untracked"), names) == c["want"]

        # one host copy per pass over the split: the loss, the corpus word, the merge's and the tracker's in one to_host_many
        post = c["post"]
        first = atest.test_epoch_windows(corpus, model, fx, crit, post, None, forward=fg, tta=tta, tracking=OPTS)
        calls = {"many": 0, "one": 0}
        many, one = ops.to_host_many, ops.to_host

        def count_many(*ts):
            calls["many"] += 1
            return many(*ts)

        def count_one(t):
            calls["one"] += 1
            return one(t)
        monkeypatch.setattr(ops, "to_host_many", count_many)
        monkeypatch.setattr(ops, "to_host", count_one)
        monkeypatch.setattr(atest, "write_seld_output_file", lambda *a, **k: pytest.fail("a file was written"))
        for kw in ({}, {"tracking": OPTS}):
            calls.update(many=0, one=0)
            sc_n = DeviceSELDScorer(prm, ref, DEV)
            again = atest.test_epoch_windows(corpus, model, fx, crit, post, None, forward=fg, device_scorer=sc_n, tta=tta, **kw)
            assert calls == {"many": 1, "one": 0}, kw
            assert again == first
        monkeypatch.undo()


def test_too_small_a_pool_raises_and_names_the_key(ops, cases, tmp_path):
    """A list of views takes the defaults: 64 rows per frame, too few for the untrained AD-YOLO head."""
    from adyolo_amd import _lib
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import InferDeviceCorpus, infer_split_from_arrays
    c = cases("adyolo")
    with pytest.raises(_lib.AdyoloHipError, match="tta_max_rows_per_frame"):
        atest.test_epoch_windows(c["corpus"], c["model"], c["fx"], c["crit"], c["post"], None, tta=[0, 5, 10])
    rec = [n for n, _ in MIXED]
    infer = InferDeviceCorpus(infer_split_from_arrays(rec, [c["written"][n][0] for n in rec], c["prm"]), c["prm"], DEV, window_s=3,
                              margin_s=1.0, batch_size=BATCH)
    with pytest.raises(_lib.AdyoloHipError, match="tta_max_rows_per_frame"):
        atest.infer_epoch_corpus(infer, c["model"], c["fx"], c["post"], str(tmp_path / "infer"), tta=[0, 5, 10])
