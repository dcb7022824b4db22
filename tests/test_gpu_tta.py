"""GPU: rotation test-time augmentation.  The kernels (csrc/select.hip ``adyolo_tta_collect`` / ``adyolo_tta_merge``) against the
host definition ``postprocess.merge_view_rows`` bit for bit on the random views of test_tta_cpu.py (frames that are no multiple
of a wave or of the scan's block, empty frames, more than 64 candidates in one frame and class, a frame with exactly P and one
with P + 1 rows, min_views from 1 to V); then ``test_epoch_corpus(tta=...)`` / ``sweep_conf_thresh_corpus(tta=...)`` on the split
of test_eval_corpus_cpu.py against every view run on its own (``rotate_audio``, the eager forward, ``select_device_rows``) and
merged on the host."""
import os
import shutil

import numpy as np
import pytest
import torch

from test_eval_corpus_cpu import eval_params, write_eval_split
from test_tta_cpu import CONFIGS, boundary_margin, most_candidates, random_views

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNIFY = 15.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------------------ the kernels
def _device_merge(ops, per_view, views, nb_classes, cap, min_views, pad_rows=5):
    """``tta_collect`` of every view (its rows in a capacity buffer with rows of another frame behind them) and ``tta_merge``
    -> (rows, counts, status) on the host."""
    from adyolo_amd.augmentations import view_matrix
    from adyolo_amd.postprocess import tta_cos
    frames = len(per_view[0][1])
    buf = ops.tta_buffers(DEV, len(views), frames, nb_classes, cap, min_views)
    buf["pool"].fill_(float("nan"))
    buf["pool_counts"].fill_(-7)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k, (rows, counts) in enumerate(per_view):
        padded = np.concatenate([rows, np.full((pad_rows, 5), 9.0, dtype=np.float32)])
        ops.tta_collect(torch.from_numpy(padded).to(DEV), torch.from_numpy(counts).to(DEV), k, view_matrix(views[k]), nb_classes,
                        buf["pool"], buf["pool_counts"], status, buf["ws"])
    rows, counts = ops.tta_merge(buf["pool"], buf["pool_counts"], nb_classes, tta_cos(UNIFY), min_views, status, buf["ws"],
                                 buf["rows"], buf["counts"])
    assert counts.data_ptr() == buf["counts"].data_ptr() and (rows.shape[0] == 0 or rows.data_ptr() == buf["rows"].data_ptr())
    assert int(buf["counts"][frames]) == rows.shape[0]
    return rows.cpu().numpy(), counts.cpu().numpy(), int(status.cpu()[0])


@pytest.mark.parametrize("config", range(len(CONFIGS)))
def test_kernels_equal_the_host_definition(ops, config):
    from adyolo_amd.postprocess import TTA_ROWS_OVERFLOW, merge_view_rows, tta_cos
    frames, nb_classes, views, cap = CONFIGS[config]
    per_view, redrawn = random_views(40 + config, frames, nb_classes, views, UNIFY, rows_cap=cap)
    assert redrawn <= frames // 100                                            # the boundary condition: at most 1 % redrawn ...
    at = [0] * len(views)
    for f in range(frames):                                                    # ... and no pair within 1e-6 of the threshold
        frame_rows = []
        for k, (rows, counts) in enumerate(per_view):
            frame_rows.append(rows[at[k]:at[k] + counts[f], 1:])
            at[k] += int(counts[f])
        assert boundary_margin(frame_rows, views, tta_cos(UNIFY)) > 1e-6
    if frames >= 3:
        assert most_candidates(per_view, cap) > 64
        assert per_view[1][1][0] == cap and per_view[1][1][-1] == cap + 1
        assert min(int(c.min()) for _, c in per_view) == 0                     # empty frames
    n = len(views)
    for min_views in sorted({1, (n + 1) // 2, n}):
        (want_rows, want_counts), want_status = merge_view_rows(per_view, views, UNIFY, min_views, max_rows_per_frame=cap)
        rows, counts, status = _device_merge(ops, per_view, views, nb_classes, cap, min_views)
        print("frames %d, C %d, V %d, P %d, min_views %d: %d rows, status %d" % (frames, nb_classes, n, cap, min_views,
                                                                                 len(want_rows), want_status))
        assert status == want_status == (TTA_ROWS_OVERFLOW if frames >= 3 else 0)
        assert np.array_equal(counts, want_counts)
        assert rows.shape == want_rows.shape and np.array_equal(rows.view(np.int32), want_rows.view(np.int32))
        assert len(want_rows) > 0 or min_views == n


def test_status_bits_and_refusals(ops):
    from adyolo_amd import _lib
    from adyolo_amd.augmentations import view_matrix
    from adyolo_amd.postprocess import TTA_BAD_ROWS, TTA_BAD_VECTOR, TTA_CAND_OVERFLOW, merge_view_rows, tta_cos
    # a zero and a NaN vector are dropped and reported; a class outside the model's is reported
    d = [0.6, 0.0, 0.8]
    rows = np.asarray([[0, 1, 0, 0, 0], [0, 1] + d, [0, 2, float("nan"), 0, 1], [1, 2] + d], dtype=np.float32)
    counts = np.asarray([3, 1], dtype=np.int32)
    per_view = [(rows, counts), (rows, counts)]
    (want_rows, want_counts), want_status = merge_view_rows(per_view, [0, 0], UNIFY, 2)
    got_rows, got_counts, status = _device_merge(ops, per_view, [0, 0], 3, 4, 2)
    assert status == want_status == TTA_BAD_VECTOR and np.array_equal(got_counts, want_counts) and want_counts.tolist() == [1, 1]
    assert np.array_equal(got_rows.view(np.int32), want_rows.view(np.int32))
    assert _device_merge(ops, per_view, [0, 0], 2, 4, 2)[2] == TTA_BAD_VECTOR | TTA_BAD_ROWS
    # counts that run past the rows given: nothing is read there
    short = (rows[:2], counts)
    assert _device_merge(ops, [short, short], [0, 0], 3, 4, 1, pad_rows=0)[2] & TTA_BAD_ROWS
    # more than 1024 candidates in one (frame, class): the slot stays empty, the others are written
    crowd = np.asarray([[0, 0] + d] * 600 + [[1, 1] + d], dtype=np.float32)
    ccounts = np.asarray([600, 1], dtype=np.int32)
    per_view = [(crowd, ccounts), (crowd, ccounts)]
    (want_rows, want_counts), want_status = merge_view_rows(per_view, [0, 5], UNIFY, 1)
    got_rows, got_counts, status = _device_merge(ops, per_view, [0, 5], 2, 600, 1)
    assert status == want_status == TTA_CAND_OVERFLOW and got_counts.tolist() == want_counts.tolist() == [0, 2]
    assert np.array_equal(got_rows.view(np.int32), want_rows.view(np.int32))
    # refusals, before any launch
    buf = ops.tta_buffers(DEV, 2, 4, 3, 8)
    status_w = torch.zeros(1, dtype=torch.int32, device=DEV)
    r, c = torch.zeros(8, 5, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    args = (3, buf["pool"], buf["pool_counts"], status_w, buf["ws"])
    with pytest.raises(_lib.AdyoloHipError, match="view"):
        ops.tta_collect(r, c, 2, view_matrix(0), *args)
    with pytest.raises(ValueError, match="signed permutation"):
        ops.tta_collect(r, c, 0, np.ones((3, 3)), *args)
    with pytest.raises(_lib.AdyoloHipError, match="counts"):
        ops.tta_collect(r, c[:3], 0, view_matrix(0), *args)
    with pytest.raises(_lib.AdyoloHipError, match="workspace"):
        ops.tta_collect(r, c, 0, view_matrix(0), 3, buf["pool"], buf["pool_counts"], status_w, buf["ws"][:4])
    with pytest.raises(_lib.AdyoloHipError, match="min_views"):
        ops.tta_merge(buf["pool"], buf["pool_counts"], 3, tta_cos(UNIFY), 3, status_w, buf["ws"])
    with pytest.raises(_lib.AdyoloHipError, match="rows"):
        ops.tta_merge(buf["pool"], buf["pool_counts"], 3, tta_cos(UNIFY), 1, status_w, buf["ws"], rows=buf["rows"][:8])
    with pytest.raises(_lib.AdyoloHipError, match="no CPU path"):
        ops.tta_merge(buf["pool"].cpu(), buf["pool_counts"], 3, tta_cos(UNIFY), 1, status_w, buf["ws"])
    with pytest.raises(_lib.AdyoloHipError, match="enlarge tta_max_rows_per_frame"):
        ops.tta_status_check(1)
    with pytest.warns(UserWarning, match="dropped"):
        ops.tta_status_check(TTA_BAD_VECTOR)
    ops.tta_status_check(0)


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
    root = str(tmp_path_factory.mktemp("gpu_tta_split"))
    write_eval_split(root)
    return root, _reference_dir(root)


@pytest.fixture(scope="module")
def mic_split(tmp_path_factory):
    """One clip of the split, as MIC-format audio."""
    root = str(tmp_path_factory.mktemp("gpu_tta_mic"))
    write_eval_split(root, clips=(("fold4_a", 48000),))
    shutil.move(os.path.join(root, "foa_dev"), os.path.join(root, "mic_dev"))
    return root, _reference_dir(root)


def _chain(root, loss, nb_classes, mic=False):
    from adyolo_amd.corpus import EvalDeviceCorpus, load_eval_split
    from adyolo_amd.features import FeatureExtractor, MicFeatureExtractor
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    prm = eval_params(root, loss=loss, nb_classes=nb_classes, device=DEV)
    if mic:
        prm["data_config"]["audio_format"] = "mic"
    torch.manual_seed(8)
    model = WrapperModel((1, 10 if mic else 7, 80, 64), (), prm).to(DEV).eval()
    corpus = EvalDeviceCorpus(load_eval_split(prm, "test", rank=0, world=1, verify="all"), prm, DEV)
    fx = MicFeatureExtractor(None, DEV) if mic else FeatureExtractor(None, DEV)
    return prm, model, fx, WrapperCriterion(prm), corpus


def _view_by_view(ops, corpus, model, fx, post, scorer, out_dir, opt, batch_size, turn):
    """The pass another way: every view of every batch on its own -- the plain audio turned by ``turn`` (``rotate_audio`` /
    ``swap_audio``), the eager forward, decode and device selection -- its rows copied to the host, merged there by
    ``merge_view_rows``; the merged rows go to the scorer and the files."""
    from adyolo_amd.postprocess import group_rows, merge_view_rows, write_seld_output_file
    names = corpus.get_filelist()
    os.makedirs(out_dir)
    total = 0
    with torch.no_grad():
        for idx in corpus.batches(batch_size):
            clips = [names[i] for i in idx]
            audio = corpus.launch(idx)[0]
            per_view = []
            for v in opt["views"]:
                audio_v = audio if v == 0 else turn(audio, [v] * len(idx))
                dec = post.decode_device(model(fx(audio_v, channels_last8=True), channels_last8=True))
                rows, counts = post.select_device_rows(dec, len(idx))
                per_view.append((rows.cpu().numpy(), counts.cpu().numpy()))
            (rows, counts), status = merge_view_rows(per_view, opt["views"], opt["unify_thresh"], opt["min_views"],
                                                     max_rows_per_frame=opt["max_rows_per_frame"])
            assert status == 0
            total += len(rows)
            scorer.add_rows(torch.from_numpy(rows).to(DEV), torch.from_numpy(counts).to(DEV), clips)
            for name, clip_rows in zip(clips, group_rows(rows, counts, len(clips))):
                write_seld_output_file(os.path.join(out_dir, name + ".csv"), clip_rows)
    corpus.check()
    return total


def _same_files(dir_a, dir_b, names):
    assert sorted(os.listdir(dir_a)) == sorted(os.listdir(dir_b)) == sorted(n + ".csv" for n in names)
    for n in names:
        assert open(os.path.join(dir_a, n + ".csv"), "rb").read() == open(os.path.join(dir_b, n + ".csv"), "rb").read(), n


def _same_accumulators(scorer_a, scorer_b):
    (acc_a, names_a), (acc_b, names_b) = scorer_a.accumulators(), scorer_b.accumulators()
    assert names_a == names_b and len(names_a) > 0
    assert np.array_equal(acc_a.view(np.int64), acc_b.view(np.int64))


@pytest.mark.parametrize("loss,nb_classes,min_views,pool_rows", [("adyolo", 12, 1, 340), ("adpit", 13, 2, 64), ("accdoa", 13, 1, 64)])
def test_epoch_equals_the_views_merged_on_the_host(ops, split, tmp_path, loss, nb_classes, min_views, pool_rows):
    """pool_rows: the untrained AD-YOLO head selects more than 64 rows in a frame, so its pool is the largest three views allow."""
    from adyolo_amd import test as atest
    from adyolo_amd.augmentations import rotate_audio, tta_options
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root, ref = split
    prm, model, fx, crit, corpus = _chain(root, loss, nb_classes)
    post = LabelPostProcessor(prm)
    names = corpus.get_filelist()
    prm["test_config"] = {"tta_views": [5, 10], "tta_min_views": min_views}
    assert tta_options(prm, postprocessor=post)["max_rows_per_frame"] == 64
    prm["test_config"]["tta_max_rows_per_frame"] = pool_rows
    opt = tta_options(prm, postprocessor=post)
    assert opt["views"] == [0, 5, 10] and opt["unify_thresh"] == 15.0 and opt["max_rows_per_frame"] == pool_rows
    sc_plain, sc_want, sc_got, sc_graph = (DeviceSELDScorer(prm, ref, DEV) for _ in range(4))
    out_plain, out_want, out_got, out_graph = (str(tmp_path / k) for k in ("plain", "want", "got", "graph"))
    loss_plain = atest.test_epoch_corpus(corpus, model, fx, crit, post, out_plain, batch_size=4, device_scorer=sc_plain)
    n_rows = _view_by_view(ops, corpus, model, fx, post, sc_want, out_want, opt, 4, rotate_audio)
    loss_got = atest.test_epoch_corpus(corpus, model, fx, crit, post, out_got, batch_size=4, device_scorer=sc_got, tta=opt)
    print("%s: %d merged rows, mean loss plain %r, with views %r" % (loss, n_rows, loss_plain, loss_got))
    assert n_rows > 0 and loss_got == loss_plain and loss_plain > 0
    _same_files(out_want, out_got, names)
    _same_accumulators(sc_want, sc_got)
    assert any(open(os.path.join(out_plain, n + ".csv"), "rb").read() != open(os.path.join(out_got, n + ".csv"), "rb").read()
               for n in names)                                                 # the views do change the result
    # replayed: ONE graph per batch shape serves every view, and the rows are the eager rows
    fg = ForwardGraphs(model, fx, post, warm_calls=0)
    shapes = {(len(r), corpus.n_hops[r[0]]) for r in corpus.batches(4)}
    loss_graph = atest.test_epoch_corpus(corpus, model, fx, crit, post, out_graph, batch_size=4, forward=fg,
                                         device_scorer=sc_graph, tta=opt)
    assert fg.captures == len(shapes) and fg.replays + fg.captures >= 3 * len(corpus.batches(4))
    assert loss_graph == loss_plain
    _same_files(out_want, out_graph, names)
    _same_accumulators(sc_want, sc_graph)
    if loss == "adpit":                # a list of views takes the defaults, which are this case's: a majority, the head's 15 degrees
        sc_list = DeviceSELDScorer(prm, ref, DEV)
        atest.test_epoch_corpus(corpus, model, fx, crit, post, None, batch_size=4, device_scorer=sc_list, tta=[0, 5, 10])
        _same_accumulators(sc_want, sc_list)
    if loss != "adyolo":
        return
    # a list of views takes the defaults: a majority, the head's unify_thresh, 64 rows (too few for this head: the pass says so)
    from adyolo_amd import _lib
    with pytest.raises(_lib.AdyoloHipError, match="tta_max_rows_per_frame"):
        atest.test_epoch_corpus(corpus, model, fx, crit, post, None, batch_size=4, tta=[0, 5, 10])
    # tta=None: the parent's behaviour, i.e. the host-fed epoch's files and accumulators
    from adyolo_amd.datasets import FoaDataset
    ds = FoaDataset(prm, "test", is_valid=True, rank=0, world=1)
    sc_host, out_host = DeviceSELDScorer(prm, ref, DEV), str(tmp_path / "host")
    loss_host = atest.test_epoch_audio(ds, model, fx, crit, post, DEV, out_host, batch_size=4, device_select=True,
                                       device_scorer=sc_host)
    assert loss_host == loss_plain
    _same_files(out_host, out_plain, names)
    _same_accumulators(sc_host, sc_plain)


def test_mic_clip_under_two_swap_views(ops, mic_split, tmp_path):
    from adyolo_amd import test as atest
    from adyolo_amd.augmentations import swap_audio, tta_options, tta_views
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root, ref = mic_split
    prm, model, fx, crit, corpus = _chain(root, "adpit", 13, mic=True)
    post = LabelPostProcessor(prm)
    prm["test_config"] = {"tta_views": [3, 9], "tta_min_views": 1}
    assert tta_views(prm) == [0, 3, 9]
    opt = tta_options(prm, postprocessor=post)
    audio = corpus.launch([0])[0]
    for v in (3, 9):
        assert torch.equal(corpus.launch_view([0], v).view(torch.int32), swap_audio(audio, [v]).view(torch.int32))
    with pytest.raises(ValueError, match="symmetry"):
        corpus.launch_view([0], 1)
    sc_want, sc_got = DeviceSELDScorer(prm, ref, DEV), DeviceSELDScorer(prm, ref, DEV)
    out_want, out_got = str(tmp_path / "want"), str(tmp_path / "got")
    n_rows = _view_by_view(ops, corpus, model, fx, post, sc_want, out_want, opt, 4, swap_audio)
    loss_got = atest.test_epoch_corpus(corpus, model, fx, crit, post, out_got, batch_size=4, device_scorer=sc_got, tta=opt)
    assert n_rows > 0 and loss_got == atest.test_epoch_corpus(corpus, model, fx, crit, post, None, batch_size=4)
    _same_files(out_want, out_got, corpus.get_filelist())
    _same_accumulators(sc_want, sc_got)


def test_launch_view_rotates_the_plain_audio(ops, split):
    from adyolo_amd.augmentations import rotate_audio
    root, _ = split
    prm, model, fx, crit, corpus = _chain(root, "adyolo", 12)
    for idx in corpus.batches(4)[:2]:
        audio = corpus.launch(idx)[0]
        assert torch.equal(corpus.launch_view(idx, 0).view(torch.int32), audio.view(torch.int32))
        for v in (6, 13):
            out = torch.empty_like(audio)
            assert corpus.launch_view(idx, v, out).data_ptr() == out.data_ptr()
            assert torch.equal(out.view(torch.int32), rotate_audio(audio, [v] * len(idx)).view(torch.int32))
    with pytest.raises(ValueError):
        corpus.launch_view([0], 16)
    corpus.check()


def test_sweep_equals_one_epoch_per_threshold(ops, split, tmp_path):
    from adyolo_amd import test as atest
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root, ref = split
    prm, model, fx, crit, corpus = _chain(root, "adyolo", 12)
    names = corpus.get_filelist()
    thresholds = (0.3, 0.4, 0.6)        # (below 0.3 the untrained head fills more than the largest pool of three views)
    tta = {"views": [0, 5, 10], "min_views": 1, "unify_thresh": 15.0, "max_rows_per_frame": 340}
    post = LabelPostProcessor(prm)
    table, best, best_th, losses = [], 9999.0, None, []
    for k, th in enumerate(thresholds):
        post.set_conf_thresh(th)
        sc = DeviceSELDScorer(prm, ref, DEV)
        losses.append(atest.test_epoch_corpus(corpus, model, fx, crit, post, str(tmp_path / ("epoch%d" % k)), batch_size=4,
                                              device_scorer=sc, tta=tta))
        table.append(list(sc.scores()[:5]))
        if table[-1][4] < best:
            best_th, best = th, table[-1][4]
    for key, forward in (("eager", None), ("graphs", ForwardGraphs(model, fx, LabelPostProcessor(prm), warm_calls=0))):
        post_b = LabelPostProcessor(prm)
        got = atest.sweep_conf_thresh_corpus(corpus, model, fx, crit, post_b, DeviceSELDScorer(prm, ref, DEV),
                                             thresholds=thresholds, output_pth=str(tmp_path / key), batch_size=4, forward=forward,
                                             tta=tta)
        print(key, "sweep:", got)
        assert got[0] == best_th and post_b.get_conf_thresh() == best_th and got[2] == losses[0]
        assert np.array_equal(np.asarray(got[1], dtype=np.float64).view(np.int64), np.asarray(table, dtype=np.float64).view(np.int64))
        _same_files(str(tmp_path / ("epoch%d" % (len(thresholds) - 1))), str(tmp_path / key), names)
