"""GPU: SpecAug inside the raw-audio train step.  ``FeatureExtractor`` / ``MicFeatureExtractor(.., spec_ranges=)`` mask their
output per feature group with ``adyolo_mask_groups`` (csrc/aug.hip); the result must equal the unmasked features with the
masks applied by torch indexing, bit for bit, for every edge of the range table (out-of-range values clamped, nothing written
outside the tensor).  ``TrainStep.step(.., spec_ranges=)`` (eager and hipGraph-replayed, tables changing every step) and the
WAV/CSV -> ``FoaDataset`` -> ``train_one_epoch_audio`` epoch must equal the same steps driven by hand."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FOA_GROUPS = ((0, 1), (1, 2))
MIC_GROUPS = ((0, 1), (1, 3))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _params(loss="adyolo"):
    return {"args": {"device": "cuda:0", "encoder": "se-resnet34", "loss": loss},
            "data_config": {"nb_classes": 12},
            "train_config": {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
                             "loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
                             "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0}}


def torch_mask(feat, ranges, groups):
    """The reference semantics by torch indexing: per sample and group zero frames [t0,t1) and bins [f0,f1) of the group's
    channels, ranges clamped to the tensor."""
    out = feat.clone()
    _, t, f, _ = out.shape
    for b, row in enumerate(ranges.tolist()):
        for (q0, q1), (t0, t1, f0, f1) in zip(groups, row):
            t0 = min(max(t0, 0), t)
            t1 = min(max(t1, t0), t)
            f0 = min(max(f0, 0), f)
            f1 = min(max(f1, f0), f)
            out[b, t0:t1, :, 4 * q0:4 * q1] = 0.0
            out[b, :, f0:f1, 4 * q0:4 * q1] = 0.0
    return out


I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
TABLES = {      # T = 40 frames, 64 bins
    "edges_b5": [[[0, 0, 0, 0], [0, 0, 0, 0]],                 # empty
                 [[3, 40, 0, 0], [0, 0, 60, 64]],               # t1 = T | f1 = 64
                 [[0, 40, 0, 0], [0, 0, 63, 64]],               # [0, T) | the last bin
                 [[5, 9, 10, 20], [0, 0, 0, 0]],                # one group only
                 [[0, 0, 0, 0], [39, 40, 0, 64]]],              # the other group only, all bins
    "one_b1": [[[2, 7, 30, 50], [11, 12, 1, 2]]],
    "clamped_b3": [[[-5, 3, -10, 4], [35, 1000, 60, 999]],
                   [[I32_MAX, I32_MIN, 70, 100], [-100, -50, 64, 64]],
                   [[I32_MIN, I32_MAX, 9, 3], [20, 10, I32_MIN, I32_MAX]]],
}


@pytest.mark.parametrize("mic", [False, True], ids=["foa", "mic"])
@pytest.mark.parametrize("name", sorted(TABLES))
def test_features_with_spec_ranges_equal_torch_masking(ops, mic, name):
    from adyolo_amd.datasets import synthetic_audio
    from adyolo_amd.features import FeatureExtractor, MicFeatureExtractor
    r = torch.tensor(TABLES[name], dtype=torch.int32)
    audio = synthetic_audio(r.shape[0], 24000, seed=31).to("cuda:0")
    fx = MicFeatureExtractor(None, "cuda:0") if mic else FeatureExtractor(None, "cuda:0")
    groups = MIC_GROUPS if mic else FOA_GROUPS
    plain = fx(audio)
    got_host = fx(audio, spec_ranges=r)                          # table on the host
    got_dev = fx(audio, spec_ranges=r.to("cuda:0"))              # table on the device
    torch.cuda.synchronize()
    ref = torch_mask(plain.cpu(), r, groups)
    assert torch.equal(got_host.cpu(), ref) and torch.equal(got_dev.cpu(), ref)
    assert not torch.equal(ref, plain.cpu())                      # every table masks something


def test_mask_groups_writes_nothing_outside_the_tensor(ops):
    """Out-of-range tables on a tensor inside a larger buffer: the guard regions before and after keep their values."""
    b, t, f, c, guard = 3, 40, 64, 32, 4096
    n = b * t * f * c
    g = torch.Generator().manual_seed(4)
    buf = torch.randn(guard + n + guard, generator=g).add_(7.0).to("cuda:0")
    x0 = buf[guard:guard + n].view(b, t, f, c).cpu()
    r = torch.tensor(TABLES["clamped_b3"], dtype=torch.int32)
    r = torch.cat([r, r.flip(1)[:, :1]], 1)                       # 3 groups: (0,1) (1,3) (3,8)
    feat = buf[guard:guard + n].view(b, t, f, c)
    ops.mask_groups_(feat, r.to("cuda:0"), ((0, 1), (1, 3), (3, 8)))
    torch.cuda.synchronize()
    host = buf.cpu()
    ref = torch_mask(x0, r, ((0, 1), (1, 3), (3, 8)))
    assert torch.equal(host[guard:guard + n].view(b, t, f, c), ref)
    ref_buf = torch.randn(guard + n + guard, generator=torch.Generator().manual_seed(4)).add_(7.0)
    assert torch.equal(host[:guard], ref_buf[:guard]) and torch.equal(host[guard + n:], ref_buf[guard + n:])
    # a full-cover table zeroes exactly the tensor
    ops.mask_groups_(feat, torch.tensor([[[0, t, 0, f]]] * b, dtype=torch.int32, device="cuda:0"), ((0, 8),))
    torch.cuda.synchronize()
    host = buf.cpu()
    assert float(host[guard:guard + n].abs().max()) == 0.0
    assert torch.equal(host[:guard], ref_buf[:guard]) and torch.equal(host[guard + n:], ref_buf[guard + n:])


def test_empty_tables_change_nothing(ops):
    from adyolo_amd.datasets import synthetic_audio, synthetic_targets
    audio = synthetic_audio(2, 48000, seed=5).to("cuda:0")
    target = synthetic_targets(2, 20, 12, seed=6)
    empty = torch.zeros(2, 2, 4, dtype=torch.int32)
    ta, tb = _trainer(False), _trainer(False)
    assert torch.equal(ta.features(audio), ta.features(audio, spec_ranges=empty))
    la = ta.step(audio, target)
    lb = tb.step(audio, target, spec_ranges=empty)
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    _assert_same_state(ta, tb)


# ------------------------------------------------------------------------------------------------ train step
def _trainer(graph, loss="adyolo", features=None):
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.train import TrainStep
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    torch.manual_seed(100)
    prm = _params(loss)
    model = WrapperModel((1, 7, 80, 64), (), prm).to("cuda:0")
    fx = features if features is not None else FeatureExtractor(None, "cuda:0")
    return TrainStep(model, WrapperCriterion(prm), fx, prm, graph=graph)


def _assert_same_state(ta, tb):
    for (k, p), (_, q) in zip(ta.model.named_parameters(), tb.model.named_parameters()):
        assert torch.equal(p, q), "parameter %s differs by %.2e" % (k, float((p - q).abs().max()))
    assert torch.equal(ta.optimizer.exp_avg, tb.optimizer.exp_avg)
    assert torch.equal(ta.optimizer.exp_avg_sq, tb.optimizer.exp_avg_sq)
    assert ta.optimizer.step_count == tb.optimizer.step_count


def _targets(loss, n, seed):
    from adyolo_amd.datasets import ClasswiseLabelEncoder, synthetic_targets
    if loss == "adyolo":
        return [synthetic_targets(2, 20, 12, seed=seed + i) for i in range(n)]
    enc = ClasswiseLabelEncoder(12)
    ev = [{0: [[3, 0, 10.0, 5.0]], 4: [[3, 0, 10.0, 5.0], [3, 1, -170.0, 40.0]], 9: [[1, 0, 0.0, 0.0]]},
          {2: [[5, 0, 90.0, 10.0]], 15: [[7, 0, -30.0, -20.0], [2, 1, 60.0, 0.0]]}]
    return [torch.stack([enc.get_adpit_label(ev[(i + k) % 2], 20) for k in range(2)]) for i in range(n)]


def _tables(n, seed):
    from adyolo_amd.augmentations import SpecAug
    sa = SpecAug({"aug_config": {"spec_augment": True, "spec_augment_thresh": 0.8, "spec_augment_time_mask_param": 30,
                                 "spec_augment_freq_mask_param": 40}}, is_valid=False)
    random.seed(seed)
    return [sa.draw_groups(2, 80, 64, 2) for _ in range(n)]


@pytest.mark.parametrize("loss", ["adyolo", "adpit"])
def test_eager_step_with_tables_equals_torch_masked_features(ops, loss):
    from adyolo_amd.datasets import synthetic_audio
    from adyolo_amd.features import FeatureExtractor
    audio = [synthetic_audio(2, 48000, seed=40 + i).to("cuda:0") for i in range(2)]
    targets, tables = _targets(loss, 2, 50), _tables(2, 7)
    assert any(bool((r[..., 1] > r[..., 0]).any() or (r[..., 3] > r[..., 2]).any()) for r in tables)
    fx = FeatureExtractor(None, "cuda:0")
    cur = {}

    def masked_by_torch(a, channels_last8=True):                 # a feature callable without the keyword
        return torch_mask(fx(a, channels_last8=channels_last8).cpu(), cur["r"], FOA_GROUPS).to("cuda:0")

    ta, tb = _trainer(False, loss), _trainer(False, loss, features=masked_by_torch)
    for i in range(2):
        cur["r"] = tables[i]
        la = ta.step(audio[i], targets[i], spec_ranges=tables[i])
        lb = tb.step(audio[i], targets[i])
        torch.cuda.synchronize()
        assert torch.equal(la, lb), (float(la), float(lb))
    _assert_same_state(ta, tb)


def test_graphed_step_refreshes_the_tables_every_replay(ops):
    from adyolo_amd.datasets import synthetic_audio
    audio = [synthetic_audio(2, 48000, seed=60 + i).to("cuda:0") for i in range(2)]
    targets, tables = _targets("adyolo", 4, 70), _tables(4, 8)
    assert len({tuple(r.flatten().tolist()) for r in tables}) == 4
    te, tg = _trainer(False), _trainer(True)
    le, lg = [], []
    for i in range(4):
        le.append(te.step(audio[i % 2], targets[i], spec_ranges=tables[i]).clone())
        lg.append(tg.step(audio[i % 2], targets[i], spec_ranges=tables[i]).clone())
    torch.cuda.synchronize()
    assert tg.graphs.captures == 1 and tg.graphs.replays == 3 and tg.graphs.eager_steps == 1
    for i, (a, b) in enumerate(zip(le, lg)):
        assert torch.equal(a, b), (i, float(a), float(b))
    _assert_same_state(te, tg)
    # a step without tables at the same shape is a graph of its own; the masked one is not re-recorded
    tg.step(audio[0], targets[0])
    tg.step(audio[0], targets[0])
    tg.step(audio[1], targets[1], spec_ranges=tables[0])
    torch.cuda.synchronize()
    assert tg.graphs.captures == 2 and tg.graphs.replays == 5


# ------------------------------------------------------------------------------------------------ epoch
def _write_files(tmp_path):
    from scipy.io import wavfile
    rs = np.random.RandomState(1)
    sub = "dev-train-chunked_2s_1s"
    wdir, cdir = os.path.join(tmp_path, "foa_dev", sub), os.path.join(tmp_path, "metadata_dev", sub)
    os.makedirs(wdir), os.makedirs(cdir)
    for i in range(4):
        wavfile.write(os.path.join(wdir, "c%d.wav" % i), 24000, rs.randint(-8000, 8000, size=(48000, 4)).astype(np.int16))
        with open(os.path.join(cdir, "c%d.csv" % i), "w") as f:
            for fr in range(0, 20, 2):
                f.write("%d,%d,0,%d,%d\n" % (fr, (fr + i) % 12, (fr * 41 + i * 90) % 360 - 180, (fr * 7) % 120 - 60))


def test_raw_audio_epoch_with_specaug_end_to_end(ops, tmp_path):
    """WAV/CSV -> FoaDataset (rotation + SpecAug) -> DataLoader(audio_collate_fn) -> train_one_epoch_audio equals the same
    steps driven by hand from the same random stream; the masks reach the model (the loss moves without them)."""
    from adyolo_amd.augmentations import rotate_audio
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    from adyolo_amd.train import train_one_epoch_audio
    _write_files(tmp_path)

    def prm_for(spec_on):
        prm = _params()
        prm["aug_config"] = {"rotation_augment": True, "spec_augment": spec_on, "spec_augment_thresh": 1.0,
                             "spec_augment_time_mask_param": 40, "spec_augment_freq_mask_param": 40}
        prm["data_config"].update({"data_pth": str(tmp_path), "chunk_window_s": 2, "chunk_stride_s": 1})
        prm["train_config"].update({"batch_size": 2, "nb_iters": 2})
        return prm

    def epoch(spec_on):
        prm = prm_for(spec_on)
        random.seed(3)
        ds = FoaDataset(prm, "train")
        random.seed(21)
        loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=audio_collate_fn, num_workers=0)
        tr = _trainer(False)
        loss = train_one_epoch_audio(prm, loader, tr)
        torch.cuda.synchronize()
        return ds, tr, loss

    ds, tr, mean_loss = epoch(True)

    def by_hand(with_tables):
        random.seed(21)
        tr2 = _trainer(False)
        losses = []
        for b0 in (0, 2):
            pcm, combs, target, spec = audio_collate_fn([ds[b0], ds[b0 + 1]])
            assert tuple(spec.shape) == (2, 2, 4) and bool((spec[..., 1] > spec[..., 0]).any())
            audio = rotate_audio((pcm.double() / 32768.0 + 1e-8).float().to("cuda:0").contiguous(), combs)
            losses.append(float(tr2.step(audio, target, spec if with_tables else None)))
        torch.cuda.synchronize()
        return tr2, sum(losses) / 2

    tr2, hand = by_hand(True)
    assert mean_loss == hand or abs(mean_loss - hand) <= 1e-7 * abs(mean_loss), (mean_loss, hand)
    for (k, p), (_, q) in zip(tr.model.named_parameters(), tr2.model.named_parameters()):
        assert torch.equal(p, q), "parameter %s differs by %.2e" % (k, float((p - q).abs().max()))
    _, unmasked = by_hand(False)
    assert unmasked != mean_loss
    _, _, off_loss = epoch(False)
    assert off_loss != mean_loss
