"""GPU: evaluation from an HBM-resident split (``corpus.EvalDeviceCorpus``, ``test.test_epoch_corpus``,
``test.sweep_conf_thresh_corpus``) against the host-fed loops on the same files (``FoaDataset`` -> ``test_epoch_audio`` /
``sweep_conf_thresh`` with the device selection and the device scorer): the audio, the targets, the losses and the scorer's
accumulators bit for bit, the CSV files byte for byte.  The split is the one of test_eval_corpus_cpu.py: clips of 48000,
48000 + 77, 72000 and 48000 + 401 samples, one clip with an empty CSV and one whose CSV has frames past its label frames."""
import os
import shutil

import numpy as np
import pytest
import torch

from test_eval_corpus_cpu import CLIPS, eval_params, write_eval_split

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _reference_dir(root):
    """The split's CSVs as the scorer's reference folder; the empty CSV gets one row (the scorer takes no empty reference)."""
    ref = os.path.join(root, "reference")
    shutil.copytree(os.path.join(root, "metadata_dev", "dev-test"), ref)
    for name in os.listdir(ref):
        if os.path.getsize(os.path.join(ref, name)) == 0:
            with open(os.path.join(ref, name), "w") as fid:
                fid.write("3,1,0,10.0,5.0\n")
    return ref


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("gpu_eval_split"))
    write_eval_split(root)
    return root, _reference_dir(root)


@pytest.fixture(scope="module")
def split_no_empty(tmp_path_factory):
    """The host sweep fails on a clip without rows (an empty AD-YOLO target): the same clips without that one."""
    root = str(tmp_path_factory.mktemp("gpu_eval_sweep"))
    write_eval_split(root, clips=tuple(c for c in CLIPS if not c[0].endswith("empty")))
    return root, _reference_dir(root)


def _chain(root, loss="adyolo", nb_classes=12):
    from adyolo_amd.corpus import EvalDeviceCorpus, load_eval_split
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    prm = eval_params(root, loss=loss, nb_classes=nb_classes, device="cuda:0")
    torch.manual_seed(8)
    model = WrapperModel((1, 7, 80, 64), (), prm).to("cuda:0").eval()
    ds = FoaDataset(prm, "test", is_valid=True, rank=0, world=1)
    corpus = EvalDeviceCorpus(load_eval_split(prm, "test", rank=0, world=1, verify="all"), prm, "cuda:0")
    return prm, model, FeatureExtractor(None, "cuda:0"), WrapperCriterion(prm), ds, corpus


def _host_audio(ops, items):
    t = (items[0][0].shape[0] // 600) * 600
    pcm = torch.from_numpy(np.stack([it[0][:t] for it in items])).to("cuda:0").contiguous()
    return ops.pcm16_to_f32(pcm).view(len(items), t, 4)


def _same_files(dir_a, dir_b, names, some=True):
    assert sorted(os.listdir(dir_a)) == sorted(os.listdir(dir_b)) == sorted(n + ".csv" for n in names)
    total = 0
    for n in names:
        a, b = open(os.path.join(dir_a, n + ".csv"), "rb").read(), open(os.path.join(dir_b, n + ".csv"), "rb").read()
        assert a == b, n
        total += len(a)
    assert total > 0 or not some


def _same_accumulators(scorer_a, scorer_b):
    (acc_a, names_a), (acc_b, names_b) = scorer_a.accumulators(), scorer_b.accumulators()
    assert names_a == names_b and len(names_a) > 0
    assert np.array_equal(acc_a.view(np.int64), acc_b.view(np.int64))


def test_adyolo_batches_equal_the_host_items(ops, split):
    from adyolo_amd.datasets import audio_collate_fn
    root, _ = split
    prm, model, fx, crit, ds, corpus = _chain(root)
    assert corpus.get_filelist() == ds.get_filelist() and len(corpus) == len(CLIPS)
    seen_empty = seen_past = False
    for idx in corpus.batches(4):
        items = [ds[i] for i in idx]
        audio, target, row_start = corpus.launch(idx)
        assert torch.equal(audio.view(torch.int32), _host_audio(ops, items).view(torch.int32))
        counts = [len(it[2]) for it in items]
        starts = row_start.cpu().tolist()
        assert starts == np.concatenate([[0], np.cumsum(counts)]).tolist()
        m = starts[-1]
        assert target.shape == (corpus.cap(len(idx)), 7) and m <= target.shape[0]
        if m:
            want = audio_collate_fn([(it[0][:48000],) + tuple(it[1:]) for it in items])[2]   # rows [b, t, gi, gj, cls, U, V]
            assert torch.equal(target[:m].cpu().view(torch.int32), want.view(torch.int32))
        assert bool((target[m:, 0] == -1).all())
        names = [ds.get_filelist()[i] for i in idx]
        seen_empty |= any(n.endswith("empty") and c == 0 for n, c in zip(names, counts))
        seen_past |= any(n.endswith("past") for n in names)
    corpus.check()
    assert seen_empty and seen_past


def test_adyolo_epoch_equals_the_host_fed_epoch(ops, split, tmp_path, monkeypatch):
    from adyolo_amd import test as atest
    from adyolo_amd.datasets import audio_collate_fn
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root, ref = split
    prm, model, fx, crit, ds, corpus = _chain(root)
    post = LabelPostProcessor(prm)
    names = ds.get_filelist()
    out_a = str(tmp_path / "host")
    sc_a = DeviceSELDScorer(prm, ref, "cuda:0")
    loss_a = atest.test_epoch_audio(ds, model, fx, crit, post, "cuda:0", out_a, batch_size=4, device_select=True,
                                    device_scorer=sc_a)
    # the mean the reference's loop forms: per-clip losses added in float32 in file order, the clip without rows left out
    total, n = np.float32(0.0), 0
    with torch.no_grad():
        for i in range(len(ds)):
            item = ds[i]
            if not item[2]:
                assert names[i].endswith("empty")
                continue
            out = model(fx(_host_audio(ops, [item]), channels_last8=True), channels_last8=True)
            total = np.float32(total + np.float32(crit(out, audio_collate_fn([item])[2]).item()))
            n += 1
    # (one clip per pass here against four there: the forward passes agree to rounding, test_gpu_graph.py)
    assert n == len(CLIPS) - 1 and abs(loss_a - float(total) / n) <= 1e-5 * abs(loss_a) < abs(loss_a - float(total) / (n + 1))

    out_b = str(tmp_path / "corpus_eager")
    sc_b = DeviceSELDScorer(prm, ref, "cuda:0")
    loss_b = atest.test_epoch_corpus(corpus, model, fx, crit, post, out_b, batch_size=4, device_scorer=sc_b)
    print("mean loss: host-fed %r, corpus eager %r" % (loss_a, loss_b))
    assert loss_b == loss_a
    _same_files(out_a, out_b, names)
    _same_accumulators(sc_a, sc_b)

    fg = ForwardGraphs(model, fx, post, warm_calls=0)
    shapes = {(len(r), corpus.n_hops[r[0]]) for r in corpus.batches(4)}
    for k in range(2):                                                         # recorded, then replayed into the graphs' own inputs
        out_g = str(tmp_path / ("corpus_graphs%d" % k))
        sc_g = DeviceSELDScorer(prm, ref, "cuda:0")
        before = (fg.captures, fg.replays)
        loss_g = atest.test_epoch_corpus(corpus, model, fx, crit, post, out_g, batch_size=4, forward=fg, device_scorer=sc_g)
        print("mean loss: corpus graphs pass %d %r" % (k, loss_g))
        assert loss_g == loss_a
        _same_files(out_a, out_g, names)
        _same_accumulators(sc_a, sc_g)
        if k == 0:
            assert fg.captures == len(shapes)
        else:
            assert fg.captures == before[0] and fg.replays == before[1] + len(corpus.batches(4))
            assert all(fg.static_input((b, t, 4)) is not None for b, t in shapes)
    assert fg.static_input((3, 1200, 4)) is None

    # output_pth=None: nothing is written, and the pass reads the device once (the loss accumulator and the status word)
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
    monkeypatch.chdir(tmp_path)
    listing = sorted(os.listdir(tmp_path))
    sc_n = DeviceSELDScorer(prm, ref, "cuda:0")
    loss_n = atest.test_epoch_corpus(corpus, model, fx, crit, post, None, batch_size=4, forward=fg, device_scorer=sc_n)
    assert calls == {"many": 1, "one": 0} and sorted(os.listdir(tmp_path)) == listing
    monkeypatch.undo()
    assert loss_n == loss_a
    _same_accumulators(sc_a, sc_n)


@pytest.mark.parametrize("loss", ["adpit", "accdoa"])
def test_classwise_epoch_equals_the_host_fed_epoch(ops, split, tmp_path, loss):
    from adyolo_amd import test as atest
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root, ref = split
    prm, model, fx, crit, ds, corpus = _chain(root, loss=loss, nb_classes=13)
    post = LabelPostProcessor(prm)
    names = ds.get_filelist()
    for idx in corpus.batches(4):
        items = [ds[i] for i in idx]
        audio, target, row_start = corpus.launch(idx)
        assert row_start is None
        assert torch.equal(audio.view(torch.int32), _host_audio(ops, items).view(torch.int32))
        want = torch.stack([it[2] for it in items], 0)
        assert target.shape == want.shape and torch.equal(target.cpu().view(torch.int32), want.view(torch.int32))
    corpus.check()
    out_a, out_b, out_g = str(tmp_path / "host"), str(tmp_path / "corpus"), str(tmp_path / "graphs")
    sc_a, sc_b, sc_g = (DeviceSELDScorer(prm, ref, "cuda:0") for _ in range(3))
    loss_a = atest.test_epoch_audio(ds, model, fx, crit, post, "cuda:0", out_a, batch_size=4, device_select=True,
                                    device_scorer=sc_a)
    loss_b = atest.test_epoch_corpus(corpus, model, fx, crit, post, out_b, batch_size=4, device_scorer=sc_b)
    fg = ForwardGraphs(model, fx, post, warm_calls=0)
    atest.test_epoch_corpus(corpus, model, fx, crit, post, None, batch_size=4, forward=fg)
    loss_g = atest.test_epoch_corpus(corpus, model, fx, crit, post, out_g, batch_size=4, forward=fg, device_scorer=sc_g)
    print("%s mean loss: host-fed %r, corpus %r, graphs %r" % (loss, loss_a, loss_b, loss_g))
    assert loss_b == loss_a and loss_g == loss_a and loss_a > 0
    for out, sc in ((out_b, sc_b), (out_g, sc_g)):
        _same_files(out_a, out, names)
        _same_accumulators(sc_a, sc)


def test_sweep_equals_the_host_fed_sweep(ops, split_no_empty, tmp_path):
    from adyolo_amd import test as atest
    from adyolo_amd.datasets import audio_collate_fn
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    root, ref = split_no_empty
    prm, model, fx, crit, ds, corpus = _chain(root)
    names = ds.get_filelist()
    thresholds = (0.2, 0.5, 0.8)

    class AudioModel:                          # sweep_conf_thresh feeds ``model(feat)``: here feat is the clip's audio
        def eval(self):
            model.eval()

        def __call__(self, audio):
            return model(fx(audio, channels_last8=True), channels_last8=True)
    loader = []
    for i in range(len(ds)):
        item = ds[i]
        loader.append((_host_audio(ops, [item]), audio_collate_fn([item])[2]))
    post_a = LabelPostProcessor(prm)
    out_a = str(tmp_path / "host")
    want = atest.sweep_conf_thresh(loader, names, AudioModel(), crit, post_a, DeviceSELDScorer(prm, ref, "cuda:0"), "cuda:0",
                                   out_a, thresholds=thresholds, device_select=True, device_score=True)
    for key, forward in (("eager", None), ("graphs", ForwardGraphs(model, fx, LabelPostProcessor(prm), warm_calls=0))):
        post_b = LabelPostProcessor(prm)
        out_b = str(tmp_path / key)
        got = atest.sweep_conf_thresh_corpus(corpus, model, fx, crit, post_b, DeviceSELDScorer(prm, ref, "cuda:0"),
                                             thresholds=thresholds, output_pth=out_b, batch_size=4, forward=forward)
        print(key, "sweep:", got, "host-fed:", want)
        assert got[0] == want[0] and post_b.get_conf_thresh() == post_a.get_conf_thresh() == want[0]
        assert np.array_equal(np.asarray(got[1], dtype=np.float64).view(np.int64),
                              np.asarray(want[1], dtype=np.float64).view(np.int64))
        assert np.asarray(got[1]).shape == (3, 5)
        assert got[2] == want[2] and got[2] > 0
        _same_files(out_a, out_b, names, some=False)      # (the last threshold, 0.8, selects nothing from this model)
    with pytest.raises(ValueError):
        atest.sweep_conf_thresh_corpus(corpus, model, fx, crit, post_b, object())


def test_a_forced_small_capacity_sets_the_status_word(ops, split):
    from adyolo_amd import _lib, test as atest
    from adyolo_amd.corpus import EvalDeviceCorpus
    from adyolo_amd.postprocess import LabelPostProcessor
    root, _ = split
    prm, model, fx, crit, ds, corpus = _chain(root)
    small = EvalDeviceCorpus(corpus.host, prm, "cuda:0", cap_per_clip=1)
    assert small.cap(4) == 4096 and corpus.cap(4) >= 4 * corpus.max_events * corpus.cells
    small.cap = lambda batch: 8                                                # fewer rows than one labelled clip has
    for idx in small.batches(4):
        audio, target, row_start = small.launch(idx)
        assert target.shape == (8, 7) and row_start.shape == (len(idx) + 1,)
    with pytest.raises(_lib.AdyoloHipError, match="capacity"):
        small.check()
    small.reset_status()
    small.check()
    with pytest.raises(_lib.AdyoloHipError, match="capacity"):               # the loop reads the word with the loss
        atest.test_epoch_corpus(small, model, fx, crit, LabelPostProcessor(prm), None, batch_size=4)
