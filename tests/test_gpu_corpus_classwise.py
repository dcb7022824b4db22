"""GPU: class-wise batches from the HBM-resident corpus (csrc/corpus.hip ``adyolo_corpus_classwise_labels``, ad-yolo_amd/corpus.py
``ClasswiseDeviceCorpus``) against the host path iterated in the main process (``FoaDataset`` -> ``audio_collate_fn`` ->
``pcm16_to_f32`` -> ``rotate_audio``): the audio bit for bit, the dense SEDDOA / ACCDOA / ADPIT targets bit for bit (compared as
int32, so signed zeros count), the SpecAug tables; direct kernel calls (a guard band after the target, a bad item, a class outside
the model's, comb -1); ``train_one_epoch_corpus`` against ``train_one_epoch_audio`` step for step, eagerly and replayed from a
hipGraph; and BASELINE config 5 at test size (MIC audio, ADPIT, SpecAug, ``MicFeatureExtractor`` straight into ``TrainStep``)."""
import random

import numpy as np
import pytest
import torch

from test_corpus_classwise_cpu import C, LOSSES, classwise_params, write_classwise_split
from test_gpu_corpus import _force_combinations

pytestmark = pytest.mark.gpu

SR = 24000
RECS = (("fold1_room1_mix001", 6.0), ("fold1_room2_mix002", 3.7), ("fold2_room1_mix003", 2.0), ("take_chunk3_mix", 4.0))
#        5 + 3 + 1 + 3 = 12 chunks of 2 s (1 s stride): 48000 samples, 20 label frames, the test model's shape
T_LABEL = 20
C_TRAIN = 12     # the corpus-against-host training tests; any class count trains (test_train_step_at_13_classes_... below)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    root = tmp_path_factory.mktemp("gpu_corpus_classwise")
    write_classwise_split(root, recordings=RECS, sr=SR, window_s=2, stride_s=1, seed=11)
    return root


@pytest.fixture(scope="module")
def split12(tmp_path_factory):
    root = tmp_path_factory.mktemp("gpu_corpus_classwise_c12")
    write_classwise_split(root, recordings=RECS, sr=SR, window_s=2, stride_s=1, seed=13, nb_classes=C_TRAIN)
    return root


@pytest.fixture(scope="module")
def mic_split(tmp_path_factory):
    root = tmp_path_factory.mktemp("gpu_corpus_classwise_mic")
    write_classwise_split(root, recordings=RECS, sr=SR, window_s=2, stride_s=1, seed=12, nb_classes=C_TRAIN, audio_dir="mic_dev")
    return root


def _prm(root, loss, spec=True, rotation=True, mic=False, nb_classes=C):
    prm = classwise_params(root, loss, batch_size=4, nb_iters=3, spec=spec, rotation=rotation, window_s=2, stride_s=1, sr=SR,
                           nb_classes=nb_classes)
    prm["args"]["device"] = "cuda:0"
    if mic:
        prm["data_config"]["audio_format"] = "mic"
    prm["train_config"].update({"optim": "Adam", "lr": 1e-3, "weight_decay": 0.0})
    prm["aug_config"].update({"spec_augment_thresh": 0.8, "spec_augment_time_mask_param": 30,
                              "spec_augment_freq_mask_param": 40})
    return prm


def _host_batches(prm, seed, epochs):
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    random.seed(seed)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    out = []
    for ep in range(epochs):
        if ep:
            ds.sample_filelist_for_train_iter()
        loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, collate_fn=audio_collate_fn, num_workers=0)
        out += list(loader)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("rotation", [True, False], ids=["all_combinations", "no_rotation"])
@pytest.mark.parametrize("loss", LOSSES)
def test_batches_equal_the_host_path(ops, split, monkeypatch, loss, rotation):
    from adyolo_amd.augmentations import rotate_audio
    from adyolo_amd.corpus import ClasswiseDeviceCorpus, load_chunked_split
    prm = _prm(split, loss, rotation=rotation)
    seed = 17
    reset = _force_combinations(monkeypatch)
    host = _host_batches(prm, seed, 2)
    hc = load_chunked_split(prm, verify="all")
    reset()
    random.seed(seed)
    corpus = ClasswiseDeviceCorpus(hc, prm, "cuda:0", rank=0, world=1)
    got = []
    for ep in range(2):
        if ep:
            corpus.sample_filelist_for_train_iter()
        for b0 in range(0, len(corpus), 4):
            audio, target, spec = corpus.batch(range(b0, b0 + 4))
            got.append((audio.clone(), target.clone(), spec.clone()))
    torch.cuda.synchronize()
    assert len(got) == len(host) == 6
    combs = set()
    for (pcm, cmb, tgt, sp), (audio, target, spec) in zip(host, got):
        combs |= set(int(c) for c in cmb)
        ref = rotate_audio(ops.pcm16_to_f32(pcm.to("cuda:0").contiguous()), cmb)
        assert torch.equal(audio, ref)
        assert tuple(target.shape) == tuple(tgt.shape) == corpus.target_shape(4)
        assert torch.equal(_bits(target.cpu()), _bits(tgt)), (loss, int((_bits(target.cpu()) != _bits(tgt)).sum()))
        assert torch.equal(spec.cpu(), sp)
    assert combs == (set(range(16)) if rotation else {0}), sorted(combs)
    if loss == "adpit":                                       # one, two and three-or-more tracks of a class all occur
        t = torch.stack([g[1] for g in got]).cpu()
        assert all(bool(t[:, :, :, s, 0].any()) for s in range(6))
    corpus.check()


def _table_label(hc, name, drop=()):
    """The chunk's label dict rebuilt from the event table (what load_csv2dict reads; load_chunked_split checked it)."""
    lo, n = hc.chunk_events[name]
    f_off = hc.chunks[name][2]
    label = {}
    for e in range(lo, lo + n):
        if e in drop:
            continue
        fr, cls, src, az, el = hc.events[e].tolist()
        label.setdefault(int(fr) - f_off, []).append([int(cls), int(src), az, el])
    return label


def _host_target(enc, loss, label, comb):
    from adyolo_amd.augmentations import rotate_labels
    from adyolo_amd.datasets import CLASSWISE_LABELS
    if comb >= 0:
        label = rotate_labels(label, comb)
    return getattr(enc, CLASSWISE_LABELS[loss])(label, T_LABEL)


@pytest.mark.parametrize("loss", ["seddoa", "accdoa", "adpit"])
def test_direct_calls_guard_band_bad_items_and_classes(ops, split, loss):
    from adyolo_amd.corpus import ClasswiseDeviceCorpus, load_chunked_split
    from adyolo_amd.datasets import ClasswiseLabelEncoder
    prm = _prm(split, loss)
    hc = load_chunked_split(prm)
    random.seed(2)
    corpus = ClasswiseDeviceCorpus(hc, prm, "cuda:0", rank=0, world=1)
    enc = ClasswiseLabelEncoder(C)
    names = sorted(hc.chunks, key=lambda k: -hc.chunk_events[k][1])[:3] + [hc.total_filelist[0]]
    combs = [5, -1, 15, 0]
    items = torch.zeros(4, 8, dtype=torch.int64)
    for j, (name, comb) in enumerate(zip(names, combs)):
        rec, off, f_off = hc.chunks[name]
        items[j] = torch.tensor([off, f_off, hc.chunk_events[name][0], hc.chunk_events[name][1], comb, rec, 0, 0])
    shape = corpus.target_shape(4)
    n = int(np.prod(shape))
    guard = 97
    buf = torch.full((n + guard,), 7.0, device="cuda:0")      # 7.0 is no label value: every element must be written
    target = buf[:n].view(shape)
    status = torch.zeros(1, dtype=torch.int32, device="cuda:0")

    def run(it, events=None):
        buf.fill_(7.0)
        status.zero_()
        ops.corpus_classwise_labels(corpus.events if events is None else events, it.to("cuda:0"), corpus.xyz,
                                    corpus.max_events, T_LABEL, C, loss, target, status)
        torch.cuda.synchronize()
        assert bool((buf[n:] == 7.0).all())
        return int(status.item())

    want = [_host_target(enc, loss, _table_label(hc, name), comb) for name, comb in zip(names, combs)]
    assert run(items) == 0
    for j in range(4):
        assert torch.equal(_bits(target[j].cpu()), _bits(want[j])), j
    assert bool(want[1].ne(0).any()) and not torch.equal(want[0], _host_target(enc, loss, _table_label(hc, names[0]), -1))
    # an event range longer than max_events, then one outside the corpus: that item all zeros, the others unchanged
    for word, value in ((3, corpus.max_events + 1), (2, corpus.n_events + 5)):
        bad = items.clone()
        bad[1, word] = value
        assert run(bad) == ops.CORPUS_STATUS[1][0]
        assert not bool(target[1].any())
        for j in (0, 2, 3):
            assert torch.equal(_bits(target[j].cpu()), _bits(want[j])), j
    # a combination past the last: the same
    bad = items.clone()
    bad[2, 4] = 16
    assert run(bad) == 2 and not bool(target[2].any()) and torch.equal(_bits(target[0].cpu()), _bits(want[0]))
    # an event of a class outside [0, C): the event is dropped, the status word says so
    lo0, n0 = hc.chunk_events[names[0]]
    e_bad = next(e for e in range(lo0, lo0 + n0)             # an event whose loss changes the item's target
                 if not torch.equal(_host_target(enc, loss, _table_label(hc, names[0], drop={e}), combs[0]), want[0]))
    dropped = [_host_target(enc, loss, _table_label(hc, name, drop={e_bad}), comb) for name, comb in zip(names, combs)]
    assert not torch.equal(dropped[0], want[0])
    for cls in (C, -1):
        ev = corpus.events.clone()
        ev[e_bad, 1] = cls
        assert run(items, ev) == 4
        for j in range(4):                                    # (an overlapping window holds the same event)
            assert torch.equal(_bits(target[j].cpu()), _bits(dropped[j])), (cls, j)


def _trainer(graph, prm, mic=False):
    from adyolo_amd.features import FeatureExtractor, MicFeatureExtractor
    from adyolo_amd.train import TrainStep
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    torch.manual_seed(100)
    mp = {"args": dict(prm["args"]), "data_config": {"nb_classes": prm["data_config"]["nb_classes"]},
          "train_config": dict(prm["train_config"])}
    model = WrapperModel((1, 10 if mic else 7, 80, 64), (), mp).to("cuda:0")
    fx = MicFeatureExtractor(None, "cuda:0") if mic else FeatureExtractor(None, "cuda:0")
    tr = TrainStep(model, WrapperCriterion(mp), fx, mp, graph=graph)
    tr.recorded = []
    inner = tr.step

    def step(audio, target, spec=None):
        loss = inner(audio, target, spec)
        tr.recorded.append((loss.detach().clone(), audio.data_ptr(), target.data_ptr()))
        return loss
    tr.step = step
    return tr


def _epochs_agree(prm, seed, graph, mic=False):
    from adyolo_amd.corpus import ClasswiseDeviceCorpus, load_chunked_split
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    from adyolo_amd.train import train_one_epoch_audio, train_one_epoch_corpus
    random.seed(seed)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, collate_fn=audio_collate_fn, num_workers=0)
    th = _trainer(graph, prm, mic)
    mean_h = train_one_epoch_audio(prm, loader, th)
    state_h = random.getstate()
    hc = load_chunked_split(prm)
    random.seed(seed)
    corpus = ClasswiseDeviceCorpus(hc, prm, "cuda:0", rank=0, world=1)
    assert corpus.get_filelist() == ds.get_filelist()
    tc = _trainer(graph, prm, mic)
    mean_c = train_one_epoch_corpus(prm, corpus, tc)
    torch.cuda.synchronize()
    assert random.getstate() == state_h
    assert len(th.recorded) == len(tc.recorded) == 3
    for i, ((lh, _, _), (lc, _, _)) in enumerate(zip(th.recorded, tc.recorded)):
        assert torch.equal(lh, lc), (i, float(lh), float(lc))
    assert mean_h == mean_c
    assert torch.equal(th.flat.flat, tc.flat.flat)
    assert torch.equal(th.optimizer.exp_avg, tc.optimizer.exp_avg)
    assert torch.equal(th.optimizer.exp_avg_sq, tc.optimizer.exp_avg_sq)
    for (k, a), (_, b) in zip(th.model.named_buffers(), tc.model.named_buffers()):
        assert torch.equal(a, b), k
    if graph:
        g = tc.graphs
        assert g.captures == 1 and g.replays == 2 and g.eager_steps == 1
        (key, ent), = g.entries.items()
        assert tuple(ent.target.shape) == corpus.target_shape(4)
        assert (tc.recorded[2][1], tc.recorded[2][2]) == (ent.audio.data_ptr(), ent.target.data_ptr())   # written in place
        assert th.graphs.captures == 1
    return corpus


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("loss", ["accdoa", "adpit"])
def test_corpus_epoch_equals_the_host_epoch(ops, split12, loss, graph):
    _epochs_agree(_prm(split12, loss, nb_classes=C_TRAIN), 23, graph)


def test_config5_mic_adpit_specaug_epoch_equals_the_host_epoch(ops, mic_split):
    """BASELINE config 5 at test size: a mic_dev split, ADPIT, SpecAug on, ``MicFeatureExtractor`` handed to ``TrainStep`` as is
    (``channels_last8`` is its alias of ``channels_last``), the step replayed from a hipGraph."""
    from adyolo_amd.features import MicFeatureExtractor
    from adyolo_amd.datasets import synthetic_audio
    fx = MicFeatureExtractor(None, "cuda:0")
    audio = synthetic_audio(2, 48000, seed=5).to("cuda:0")
    assert torch.equal(fx(audio, channels_last8=True), fx(audio))
    assert torch.equal(fx(audio, channels_last8=False), fx(audio, channels_last=False))
    prm = _prm(mic_split, "adpit", mic=True, nb_classes=C_TRAIN)
    corpus = _epochs_agree(prm, 31, True, mic=True)
    assert corpus.host.wav_pth.split("/")[-2] == "mic_dev" and corpus.specaug.apply_augment


@pytest.mark.parametrize("loss", ["accdoa", "adpit"])
def test_train_step_at_13_classes_eager_equals_replayed(ops, split, loss):
    """C = 13, the class count of the DCASE2022 data: head widths 39 and 117, no multiples of 4 (``ops.linear_bwd`` pads them).
    Three ``TrainStep`` steps from the corpus, eagerly and with the step replayed from a captured graph: the same bits."""
    from adyolo_amd.corpus import ClasswiseDeviceCorpus, load_chunked_split
    from adyolo_amd.train import train_one_epoch_corpus
    assert C == 13
    prm = _prm(split, loss)
    hc = load_chunked_split(prm)
    runs = []
    for graph in (False, True):
        random.seed(29)
        corpus = ClasswiseDeviceCorpus(hc, prm, "cuda:0", rank=0, world=1)
        tr = _trainer(graph, prm)
        train_one_epoch_corpus(prm, corpus, tr)
        torch.cuda.synchronize()
        runs.append(tr)
    eager, replayed = runs
    assert len(eager.recorded) == len(replayed.recorded) == 3
    assert replayed.graphs.captures == 1 and replayed.graphs.replays == 2
    for i, ((le, _, _), (lr, _, _)) in enumerate(zip(eager.recorded, replayed.recorded)):
        assert bool(torch.isfinite(le)) and torch.equal(le, lr), (i, float(le), float(lr))
    assert torch.equal(eager.flat.flat, replayed.flat.flat)
    assert torch.equal(eager.optimizer.exp_avg, replayed.optimizer.exp_avg)
    assert bool(torch.isfinite(eager.flat.flat).all())
