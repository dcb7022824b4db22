"""CPU: the host half of SpecAug in the raw-audio train step -- ``SpecAug.draw_groups`` (one independent draw per sample and
feature group, as the reference masks MEL and IV each with its own draw, src/datasets.py:158-159), the place of that draw in
``FoaDataset.__getitem__`` (right after the rotation draw, from the same ``random`` stream) and the 4th element it adds to
the items and to ``audio_collate_fn``."""
import os
import random

import numpy as np
import pytest
import torch

import adyolo_amd  # noqa: F401
from adyolo_amd.augmentations import SpecAug
from adyolo_amd.datasets import FoaDataset, audio_collate_fn


def _aug(on=True, thresh=0.5, t_param=40, f_param=40):
    return {"spec_augment": on, "spec_augment_thresh": thresh, "spec_augment_time_mask_param": t_param,
            "spec_augment_freq_mask_param": f_param}


def _sa(is_valid=False, **kw):
    return SpecAug({"aug_config": _aug(**kw)}, is_valid=is_valid)


def test_draw_groups_shape_bounds_and_independent_groups():
    sa = _sa(thresh=0.5, t_param=40, f_param=40)
    random.seed(0)
    r = sa.draw_groups(200, 100, 64, 2)
    assert r.dtype == torch.int32 and tuple(r.shape) == (200, 2, 4)
    t0, t1, f0, f1 = (r[..., k] for k in range(4))
    assert bool(((0 <= t0) & (t0 <= t1) & (t1 <= 100)).all()) and bool(((0 <= f0) & (f0 <= f1) & (f1 <= 64)).all())
    assert bool((t1 - t0 <= 40).all()) and bool((f1 - f0 <= 40).all())
    masked = (t1 > t0) | (f1 > f0)                                  # (200, 2): does the group get any mask
    assert bool((masked[:, 0] != masked[:, 1]).any())               # thresh in (0, 1): some sample has exactly one group masked
    assert not torch.equal(r[:, 0], r[:, 1])                         # the two groups' ranges are separate draws
    # frames and bins are drawn separately too: some group has a frame mask and no bin mask, and the reverse
    assert bool(((t1 > t0) & (f1 == f0)).any()) and bool(((t1 == t0) & (f1 > f0)).any())


def test_draw_groups_of_one_group_equals_draw():
    sa = _sa(thresh=0.7, t_param=12, f_param=9)
    random.seed(5)
    a = sa.draw(17, 40, 64)
    after_a = random.random()
    random.seed(5)
    b = sa.draw_groups(17, 40, 64, 1)
    after_b = random.random()
    assert tuple(b.shape) == (17, 1, 4) and torch.equal(b[:, 0], a) and after_a == after_b


def test_draw_is_unchanged():
    """``draw``'s output for a seed: the reference's ``_mask`` order restated (mel-bin range, then frame range, each gated)."""
    sa = _sa(thresh=0.5, t_param=8, f_param=6)
    random.seed(11)
    got = sa.draw(6, 30, 64)
    random.seed(11)
    ref = torch.zeros((6, 4), dtype=torch.int32)
    for b in range(6):
        if random.random() <= 0.5:
            v = random.random() * 8
            s = random.random() * (64 - v)
            ref[b, 2], ref[b, 3] = int(s), int(s + v)
        if random.random() <= 0.5:
            v = random.random() * 6
            s = random.random() * (30 - v)
            ref[b, 0], ref[b, 1] = int(s), int(s + v)
    assert got.dtype == torch.int32 and torch.equal(got, ref)


def test_specaug_is_identity_on_validation_and_when_off():
    assert not _sa(is_valid=True).apply_augment
    assert not _sa(on=False).apply_augment
    assert _sa().apply_augment
    feat = torch.ones(2, 4, 64, 8)
    assert _sa(is_valid=True).augment(feat) is feat and _sa(on=False).augment(feat) is feat


# ------------------------------------------------------------------------------------------------ FoaDataset / collate
def _params(tmp_path, aug, loss="adyolo"):
    return {"args": {"device": "cpu", "encoder": "se-resnet34", "loss": loss},
            "data_config": {"nb_classes": 12, "data_pth": str(tmp_path), "chunk_window_s": 1, "chunk_stride_s": 1},
            "train_config": {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
                             "batch_size": 2, "nb_iters": 2},
            "aug_config": aug}


def _files(tmp_path, n=4, n_samples=24000):
    from scipy.io import wavfile
    rs = np.random.RandomState(2)
    sub = "dev-train-chunked_1s_1s"
    for split in (sub, "dev-valid"):
        wdir, cdir = os.path.join(tmp_path, "foa_dev", split), os.path.join(tmp_path, "metadata_dev", split)
        os.makedirs(wdir), os.makedirs(cdir)
        for i in range(n):
            wavfile.write(os.path.join(wdir, "c%d.wav" % i), 24000, rs.randint(-8000, 8000, size=(n_samples, 4)).astype(np.int16))
            with open(os.path.join(cdir, "c%d.csv" % i), "w") as f:
                for fr in range(0, 10, 3):
                    f.write("%d,%d,0,%d,%d\n" % (fr, (fr + i) % 12, (fr * 41 + i * 90) % 360 - 180, (fr * 7) % 120 - 60))


def _dataset(prm, set_type="train", is_valid=False):
    random.seed(3)
    return FoaDataset(prm, set_type, is_valid=is_valid, rank=0, world=1)


def test_dataset_item_draws_rotation_then_mel_then_iv(tmp_path):
    """A seeded ``random``: the item's comb_no and table equal a hand replay of the reference's order -- the rotation's
    ``uniform(0, 16)`` (augmentations.py:76), then SpecAug on MEL, then on IV (datasets.py:158-159)."""
    _files(tmp_path)
    aug = dict(_aug(thresh=0.6, t_param=7, f_param=20), rotation_augment=True)
    ds = _dataset(_params(tmp_path, aug))
    sa = SpecAug({"aug_config": aug}, is_valid=False)
    for seed in range(6):
        random.seed(seed)
        pcm, comb_no, target, spec = ds[seed % len(ds)]
        random.seed(seed)
        comb = int(random.uniform(0, 16))
        mel = sa._draw_one(pcm.shape[0] // 600, 64)
        iv = sa._draw_one(pcm.shape[0] // 600, 64)
        assert comb_no == comb
        assert spec.dtype == torch.int32 and tuple(spec.shape) == (2, 4)
        assert spec.tolist() == [mel, iv]


def test_dataset_and_collate_without_specaug_are_unchanged(tmp_path):
    _files(tmp_path)
    for aug in ({"rotation_augment": True}, dict(_aug(on=False), rotation_augment=True)):
        ds = _dataset(_params(tmp_path, aug))
        random.seed(9)
        items = [ds[0], ds[1]]
        assert all(len(it) == 3 for it in items)
        batch = audio_collate_fn(items)
        assert len(batch) == 3
        pcm, combs, target = batch
        assert pcm.dtype == torch.int16 and tuple(pcm.shape) == (2, 24000, 4)
        assert isinstance(combs, list) and target.shape[1] == 7
    # validation split with SpecAug on: no table either
    ds = _dataset(_params(tmp_path, dict(_aug(on=True), rotation_augment=True)), "valid", is_valid=True)
    assert len(ds[0]) == 3


def test_dataset_and_collate_with_specaug_stack_the_tables(tmp_path):
    _files(tmp_path)
    for loss in ("adyolo", "adpit"):
        prm = _params(tmp_path, dict(_aug(thresh=1.0, t_param=10, f_param=10), rotation_augment=True), loss=loss)
        ds = _dataset(prm)
        random.seed(4)
        items = [ds[i] for i in range(len(ds))]
        assert all(len(it) == 4 for it in items)
        pcm, combs, target, spec = audio_collate_fn(items)
        assert pcm.dtype == torch.int16 and tuple(pcm.shape) == (len(items), 24000, 4) and len(combs) == len(items)
        assert spec.dtype == torch.int32 and tuple(spec.shape) == (len(items), 2, 4)
        assert torch.equal(spec, torch.stack([it[3] for it in items]))
        assert bool((spec[..., 1] <= 40).all()) and bool((spec[..., 3] <= 64).all())
        # the same items without their tables collate exactly as before
        pcm3, combs3, target3 = audio_collate_fn([it[:3] for it in items])
        assert torch.equal(pcm3, pcm) and combs3 == combs and torch.equal(target3, target)


def test_mask_groups_refuses_host_tensors_and_bad_tables():
    from adyolo_amd import _lib, ops
    with pytest.raises(_lib.AdyoloHipError):
        ops.mask_groups_(torch.zeros(1, 4, 64, 8), torch.zeros(1, 2, 4, dtype=torch.int32), ((0, 1), (1, 2)))
