"""GPU: batches from the HBM-resident corpus (csrc/corpus.hip, ad-yolo_amd/corpus.py) against the host path iterated in the main
process (``FoaDataset`` -> ``audio_collate_fn`` -> ``pcm16_to_f32`` -> ``rotate_audio``): the audio bit for bit, the AD-YOLO rows
exactly and in order (padding b = -1, the row count on the device), the SpecAug tables; ``train_one_epoch_corpus`` against
``train_one_epoch_audio`` step for step, eagerly and replayed from a hipGraph; a capacity forced too small raises."""
import random

import numpy as np
import pytest
import torch

from test_corpus_cpu import params_for, write_split

pytestmark = pytest.mark.gpu

SR = 24000
RECS = (("fold1_room1_mix001", 6.0), ("fold1_room2_mix002", 3.7), ("fold2_room1_mix003", 2.0), ("take_chunk3_mix", 4.0))
#        5 + 3 + 1 + 3 = 12 chunks of 2 s (1 s stride): 48000 samples, 20 label frames, the test model's shape


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    root = tmp_path_factory.mktemp("gpu_corpus")
    write_split(root, recordings=RECS, sr=SR, window_s=2, stride_s=1, seed=11)
    return root


def _prm(root, batch_size=4, nb_iters=3, spec=True):
    prm = params_for(root, batch_size=batch_size, nb_iters=nb_iters, spec=spec, window_s=2, stride_s=1, sr=SR)
    prm["args"]["device"] = "cuda:0"
    prm["data_config"]["nb_classes"] = 12
    prm["train_config"].update({"loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
                                "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0})
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


def _force_combinations(monkeypatch):
    """``random.uniform`` -> every FOA combination in turn (both paths draw through it, item by item); -> the reset."""
    order = [7, 0, 15, 3, 12, 9, 1, 14, 5, 10, 2, 13, 6, 11, 4, 8]
    calls = [0]

    def uniform(a, b):
        k = calls[0]
        calls[0] += 1
        return float(order[k % 16]) + 0.25
    monkeypatch.setattr(random, "uniform", uniform)
    return lambda: calls.__setitem__(0, 0)


def test_batches_equal_the_host_path(ops, split, monkeypatch):
    from adyolo_amd.augmentations import rotate_audio
    from adyolo_amd.corpus import DeviceCorpus, load_chunked_split
    prm = _prm(split)
    seed = 17
    reset = _force_combinations(monkeypatch)
    host = _host_batches(prm, seed, 2)
    hc = load_chunked_split(prm, verify="all")
    reset()
    random.seed(seed)
    corpus = DeviceCorpus(hc, prm, "cuda:0", rank=0, world=1)
    assert corpus.cap % 4096 == 0 and corpus.cap >= 4 * hc.max_events * corpus.cells
    got = []
    for ep in range(2):
        if ep:
            corpus.sample_filelist_for_train_iter()
        for b0 in range(0, len(corpus), 4):
            audio, target, spec = corpus.batch(range(b0, b0 + 4))
            got.append((audio.clone(), target.clone(), spec.clone(), corpus.rows.clone()))
    torch.cuda.synchronize()
    assert len(got) == len(host) == 6
    combs = set()
    for (pcm, cmb, tgt, sp), (audio, target, spec, rows) in zip(host, got):
        combs |= set(int(c) for c in cmb)
        ref = rotate_audio(ops.pcm16_to_f32(pcm.to("cuda:0").contiguous()), cmb)
        assert torch.equal(audio, ref)
        m = tgt.shape[0]
        assert int(rows.item()) == m and m > 0
        assert torch.equal(target[:m].cpu(), tgt)
        assert bool((target[m:, 0] == -1).all())
        assert torch.equal(spec.cpu(), sp)
    assert combs == set(range(16)), sorted(combs)                 # every FOA combination was exercised
    corpus.check()


def test_gather_edges_odd_offsets_no_rotation_and_bad_items(ops):
    """Direct calls: windows starting on odd frames (8-byte path), odd lengths, one and two frames (the tail alone, one
    iteration of the two-frame loop), comb -1 (identity), an item past the end (zeros + status bit 2) -- nothing is read or
    written outside the buffers: for every n the last item ends exactly at the end of ``pcm``."""
    from adyolo_amd.augmentations import COMBINATIONS, rotate_audio
    g = torch.Generator().manual_seed(3)
    pcm = torch.randint(-32768, 32768, (1001, 4), generator=g, dtype=torch.int32).to(torch.int16).to("cuda:0")
    rot = ops.corpus_rot_table(COMBINATIONS)
    for n in (1, 2, 257, 256):
        offs, combs = [0, 1, 3, 744, 1001 - n], [5, -1, 15, 8, 2]
        items = torch.zeros(5, 8, dtype=torch.int64)
        items[:, 0] = torch.tensor(offs)
        items[:, 4] = torch.tensor(combs)
        guard = 64
        buf = torch.full((5 * n * 4 + guard,), 7.0, device="cuda:0")
        out = buf[:5 * n * 4].view(5, n, 4)
        status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        ops.corpus_gather(pcm, items.to("cuda:0"), rot, out, status)
        ref = rotate_audio(ops.pcm16_to_f32(torch.stack([pcm[o:o + n] for o in offs]).contiguous()), [max(c, 0) for c in combs])
        torch.cuda.synchronize()
        assert torch.equal(out, ref) and int(status.item()) == 0
        assert bool((buf[5 * n * 4:] == 7.0).all())
        items[2, 0] = 1001 - n + 1                                   # one frame past the end
        ops.corpus_gather(pcm, items.to("cuda:0"), rot, out, status)
        torch.cuda.synchronize()
        assert int(status.item()) == 2 and not bool(out[2].any()) and torch.equal(out[3], ref[3])


def _trainer(graph):
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.train import TrainStep
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    torch.manual_seed(100)
    prm = {"args": {"device": "cuda:0", "encoder": "se-resnet34", "loss": "adyolo"}, "data_config": {"nb_classes": 12},
           "train_config": {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
                            "loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
                            "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0}}
    model = WrapperModel((1, 7, 80, 64), (), prm).to("cuda:0")
    tr = TrainStep(model, WrapperCriterion(prm), FeatureExtractor(None, "cuda:0"), prm, graph=graph)
    tr.recorded = []
    inner = tr.step

    def step(audio, target, spec=None):
        loss = inner(audio, target, spec)
        tr.recorded.append((loss.detach().clone(), audio.data_ptr(), target.data_ptr()))
        return loss
    tr.step = step
    return tr


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_corpus_epoch_equals_the_host_epoch(ops, split, graph):
    from adyolo_amd.corpus import DeviceCorpus, load_chunked_split
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    from adyolo_amd.train import train_one_epoch_audio, train_one_epoch_corpus
    prm = _prm(split)                                              # 12 files, 3 steps of 4
    seed = 23
    random.seed(seed)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, collate_fn=audio_collate_fn, num_workers=0)
    th = _trainer(graph)
    mean_h = train_one_epoch_audio(prm, loader, th)
    state_h = random.getstate()
    hc = load_chunked_split(prm)
    random.seed(seed)
    corpus = DeviceCorpus(hc, prm, "cuda:0", rank=0, world=1)
    assert corpus.get_filelist() == ds.get_filelist()
    tc = _trainer(graph)
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
        assert (tc.recorded[2][1], tc.recorded[2][2]) == (ent.audio.data_ptr(), ent.target.data_ptr())   # written in place
        assert th.graphs.captures == 1


def test_forced_small_capacity_raises(ops, split):
    from adyolo_amd import _lib
    from adyolo_amd.corpus import DeviceCorpus, load_chunked_split
    from adyolo_amd.train import train_one_epoch_corpus
    prm = _prm(split)
    random.seed(5)
    corpus = DeviceCorpus(load_chunked_split(prm), prm, "cuda:0", rank=0, world=1, cap=8)
    with pytest.raises(_lib.AdyoloHipError, match="capacity"):
        train_one_epoch_corpus(prm, corpus, _trainer(False))
    assert int(corpus.status.item()) & 1
    corpus.reset_status()
    audio, target, _ = corpus.batch(range(4))
    torch.cuda.synchronize()
    assert int(corpus.rows.item()) > 8 and target.shape == (8, 7) and int(corpus.status.item()) == 1
    assert np.isfinite(target.cpu().numpy()).all()
