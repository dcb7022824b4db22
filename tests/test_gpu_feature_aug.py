"""GPU: the frequency-shift and cutout augmentation of the features (``adyolo_feat_augment``, csrc/aug.hip), every comparison
exact.  ``ops.feat_augment_`` against the NumPy definition ``augmentations.apply_feature_aug_host`` (shift only, clamped shifts,
cutout only, all three operations overlapping; every-sample-shifted tables are the ones that catch an in-place race), nothing
written outside the tensor; both feature extractors with a (B, 4, 4) table on the host and on the device; ``TrainStep`` eagerly
against the step driven by hand and replayed from ONE hipGraph with the tables changing; and an epoch of
``train_one_epoch_audio`` against ``train_one_epoch_corpus`` under the same seed and keys.  Every case also asserts that its
table did change the features."""
import random

import numpy as np
import pytest
import torch

from test_corpus_classwise_cpu import classwise_params, write_classwise_split
from test_gpu_corpus_classwise import _trainer as _corpus_trainer
from test_gpu_specaug_train import _assert_same_state, _targets, _trainer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FOA_GROUPS, MIC_GROUPS = ((0, 1), (1, 2)), ((0, 1), (1, 3))
FOA_SHIFT, MIC_SHIFT = (True, True), (True, False)
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
B, T = 5, 37                     # T odd: no rows-per-wave or rows-per-workgroup count divides it


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _table(shifts=(0,) * B, cutout=None, spec=None):
    tab = np.zeros((len(shifts), 4, 4), dtype=np.int64)
    tab[:, 3, 0] = shifts
    if cutout is not None:
        tab[:, 2] = cutout
    if spec is not None:
        tab[:, :2] = spec
    return torch.from_numpy(tab.astype(np.int32))


TABLES = {      # B = 5 samples, T = 37 frames, 64 bins
    "shift_small": _table((1, -1, 5, -5, 0)),                                     # one unshifted sample
    "shift_large": _table((63, -63, 0, 5, -1)),
    "shift_every_sample": _table((1, -1, 5, -63, 63)),
    "shift_clamped": _table((64, -64, I32_MAX, I32_MIN, -I32_MAX)),
    "cutout_only": _table(cutout=[[7, 8, 0, 0],                                    # empty in one direction
                                  [0, T, 0, 64],                                   # the whole tensor
                                  [-5, 3, -10, 4],                                 # clamped at the front
                                  [I32_MIN, I32_MAX, 60, I32_MAX],                 # clamped extremes: all frames, the last bins
                                  [I32_MAX, I32_MIN, 70, 100]]),                   # empty after clamping
    "cutout_one_element": _table(cutout=[[36, 37, 63, 64], [0, 1, 0, 1], [0, 0, 0, 0], [18, 19, 5, 6], [0, 0, 0, 0]]),
    "all_three": _table((3, -7, 63, 0, -64),
                        cutout=[[5, 30, 10, 50], [0, T, 20, 22], [30, 100, -3, 40], [2, 9, 0, 64], [I32_MIN, 1, 62, I32_MAX]],
                        spec=[[[2, 7, 30, 50], [11, 12, 1, 2]], [[0, 0, 0, 0], [0, T, 0, 0]], [[-5, 3, -10, 4], [35, 1000, 60, 999]],
                              [[3, 9, 12, 20], [0, 0, 63, 64]], [[I32_MIN, I32_MAX, 9, 3], [20, 10, I32_MIN, I32_MAX]]]),
}
LAYOUTS = {"foa": (8, FOA_GROUPS, FOA_SHIFT), "mic": (32, MIC_GROUPS, MIC_SHIFT)}


@pytest.fixture(scope="module")
def feats():
    """One random tensor per layout (no zeros of its own), shared and never written."""
    return {name: torch.randn(B, T, 64, c, generator=torch.Generator().manual_seed(c)).add_(3.0) for name, (c, _, _) in LAYOUTS.items()}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", sorted(TABLES))
def test_feat_augment_equals_the_host_definition(ops, feats, layout, name):
    from adyolo_amd.augmentations import apply_feature_aug_host
    c, groups, shift = LAYOUTS[layout]
    x, tab = feats[layout], TABLES[name]
    want = apply_feature_aug_host(x, tab, groups, shift)
    feat = x.to(DEV)
    got = ops.feat_augment_(feat, tab.to(DEV), groups, shift)
    torch.cuda.synchronize()
    assert got.data_ptr() == feat.data_ptr()
    got = feat.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), \
        [b for b in range(B) if not np.array_equal(got[b].view(np.int32), want[b].view(np.int32))]
    assert not np.array_equal(want, x.numpy())                     # the table does something
    if layout == "mic" and name.startswith("shift"):               # the GCC-PHAT quads: the input's bits
        assert np.array_equal(got[..., 4:].view(np.int32), x.numpy()[..., 4:].view(np.int32))
        assert not np.array_equal(got[..., :4], x.numpy()[..., :4])


def test_feat_augment_writes_nothing_outside_the_tensor(ops):
    """Out-of-range tables on a tensor inside a larger buffer: the guard regions before and after keep their values."""
    from adyolo_amd.augmentations import apply_feature_aug_host
    b, t, f, c, guard = 5, T, 64, 32, 4096
    n = b * t * f * c
    groups, shift = ((0, 1), (1, 3), (3, 8)), (True, False, True)
    ref_buf = torch.randn(guard + n + guard, generator=torch.Generator().manual_seed(4)).add_(7.0)
    buf = ref_buf.to(DEV)
    x0 = ref_buf[guard:guard + n].view(b, t, f, c)
    base = TABLES["all_three"]
    tab = torch.cat([base[:, :2], base[:, :1].flip(0), base[:, 2:]], 1)           # 3 groups -> (B, 5, 4)
    tab[:, 4, 0] = torch.tensor([I32_MAX, I32_MIN, 63, -63, 64], dtype=torch.int32)
    feat = buf[guard:guard + n].view(b, t, f, c)
    ops.feat_augment_(feat, tab.to(DEV), groups, shift)
    torch.cuda.synchronize()
    host = buf.cpu()
    want = apply_feature_aug_host(x0, tab, groups, shift)
    assert np.array_equal(host[guard:guard + n].view(b, t, f, c).numpy().view(np.int32), want.view(np.int32))
    assert not np.array_equal(want, x0.numpy())
    assert torch.equal(host[:guard], ref_buf[:guard]) and torch.equal(host[guard + n:], ref_buf[guard + n:])
    # a full-cover rectangle zeroes exactly the tensor
    full = torch.zeros(b, 5, 4, dtype=torch.int32)
    full[:, 3] = torch.tensor([I32_MIN, I32_MAX, I32_MIN, I32_MAX], dtype=torch.int32)
    full[:, 4, 0] = 63
    ops.feat_augment_(feat, full.to(DEV), groups, shift)
    torch.cuda.synchronize()
    host = buf.cpu()
    assert float(host[guard:guard + n].abs().max()) == 0.0
    assert torch.equal(host[:guard], ref_buf[:guard]) and torch.equal(host[guard + n:], ref_buf[guard + n:])


def test_feat_augment_refusals(ops):
    from adyolo_amd._lib import AdyoloHipError
    feat = torch.zeros(2, 4, 64, 8, device=DEV)
    tab = torch.zeros(2, 4, 4, dtype=torch.int32, device=DEV)
    for bad in (tab[:, :2].contiguous(), tab[:1], tab.to(torch.int64), tab.cpu(), tab.transpose(1, 2)):
        with pytest.raises(AdyoloHipError):
            ops.feat_augment_(feat, bad, FOA_GROUPS, FOA_SHIFT)
    with pytest.raises(AdyoloHipError):
        ops.feat_augment_(feat, tab, FOA_GROUPS, (True,))
    with pytest.raises(AdyoloHipError):
        ops.feat_augment_(feat, tab, ((0, 1), (1, 3)), FOA_SHIFT)
    with pytest.raises(AdyoloHipError, match="F = 32"):            # a row of 64 bins is one wave: no other width
        ops.feat_augment_(torch.zeros(2, 4, 32, 8, device=DEV), tab, FOA_GROUPS, FOA_SHIFT)


# ------------------------------------------------------------------------------------------------------------ extractors
FX_TABLE = _table((4, -63, 0), cutout=[[3, 40, 10, 30], [0, 0, 0, 0], [-7, 12, 60, 999]],
                  spec=[[[2, 7, 30, 50], [11, 12, 1, 2]], [[0, 0, 0, 0], [35, 1000, 60, 999]], [[5, 9, 10, 20], [0, 0, 0, 0]]])


@pytest.mark.parametrize("mic", [False, True], ids=["foa", "mic"])
def test_extractors_take_the_table(ops, mic):
    from adyolo_amd._lib import AdyoloHipError
    from adyolo_amd.augmentations import apply_feature_aug_host
    from adyolo_amd.datasets import synthetic_audio
    from adyolo_amd.features import FeatureExtractor, MicFeatureExtractor
    audio = synthetic_audio(3, 24000, seed=31).to(DEV)              # 1 s: T = 40
    fx = MicFeatureExtractor(None, DEV) if mic else FeatureExtractor(None, DEV)
    plain = fx(audio)
    got_host = fx(audio, spec_ranges=FX_TABLE)                      # table on the host
    got_dev = fx(audio, spec_ranges=FX_TABLE.to(DEV))               # table on the device
    only_spec = FX_TABLE.clone()
    only_spec[:, 2:] = 0
    got_spec4 = fx(audio, spec_ranges=only_spec)
    got_spec2 = fx(audio, spec_ranges=FX_TABLE[:, :2].contiguous())
    got_zero = fx(audio, spec_ranges=torch.zeros(3, 4, 4, dtype=torch.int32))
    torch.cuda.synchronize()
    want = apply_feature_aug_host(plain, FX_TABLE, fx.SPEC_GROUPS, fx.SHIFT_GROUPS)
    assert tuple(plain.shape) == (3, 40, 64, 32 if mic else 8)
    assert np.array_equal(got_host.cpu().numpy(), want) and np.array_equal(got_dev.cpu().numpy(), want)
    assert not np.array_equal(want, plain.cpu().numpy())
    assert not np.array_equal(want, got_spec2.cpu().numpy())        # the rows 2-3 do something beyond SpecAug
    assert torch.equal(got_spec4, got_spec2) and not torch.equal(got_spec2, plain)
    assert torch.equal(got_zero, plain)
    if mic:                                                         # only the log-mel quad moves
        shift_only = _table((4, -63, 9))
        moved = fx(audio, spec_ranges=shift_only).cpu()
        assert torch.equal(moved[..., 4:], plain.cpu()[..., 4:]) and not torch.equal(moved[..., :4], plain.cpu()[..., :4])
    for bad in (torch.zeros(3, 3, 4, dtype=torch.int32), torch.zeros(2, 4, 4, dtype=torch.int32),
                torch.zeros(3, 4, 4, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int32)):
        with pytest.raises(AdyoloHipError):
            fx(audio, spec_ranges=bad)


# ------------------------------------------------------------------------------------------------------------- train step
def _step_tables(n, seed):
    """n tables (2, 4, 4) for T = 80: SpecAug rows, a cutout and a shift for each sample, every table different."""
    from adyolo_amd.augmentations import draw_feature_aug, feature_aug_config, feature_aug_table
    from test_gpu_specaug_train import _tables
    cfg = feature_aug_config({"aug_config": {"freq_shift_augment": True, "freq_shift_prob": 1.0, "freq_shift_max_bins": 8,
                                             "cutout_augment": True, "cutout_prob": 1.0, "cutout_time_param": 40,
                                             "cutout_freq_param": 20}})
    spec = _tables(n, seed)
    rnd = random.Random(seed)
    return [torch.stack([feature_aug_table(spec[i][b], *draw_feature_aug(rnd, cfg, 80, 64)) for b in range(2)]) for i in range(n)]


@pytest.mark.parametrize("loss", ["adyolo", "adpit"])
def test_eager_step_with_a_table_equals_the_step_driven_by_hand(ops, loss):
    from adyolo_amd.augmentations import apply_feature_aug_host
    from adyolo_amd.datasets import synthetic_audio
    from adyolo_amd.features import FeatureExtractor
    audio = [synthetic_audio(2, 48000, seed=40 + i).to(DEV) for i in range(2)]
    targets, tables = _targets(loss, 2, 50), _step_tables(2, 7)
    assert all(bool((r[:, 3, 0] != 0).all()) and bool((r[:, 2, 1] > r[:, 2, 0]).any()) for r in tables)
    fx = FeatureExtractor(None, DEV)
    cur, changed = {}, []

    def by_hand(a, channels_last8=True):                          # features, then the host definition, then the rest of the step
        plain = fx(a, channels_last8=channels_last8)
        want = apply_feature_aug_host(plain, cur["r"], FOA_GROUPS, FOA_SHIFT)
        changed.append(not np.array_equal(want, plain.cpu().numpy()))
        return torch.from_numpy(want).to(DEV)

    ta, tb = _trainer(False, loss), _trainer(False, loss, features=by_hand)
    for i in range(2):
        cur["r"] = tables[i]
        la = ta.step(audio[i], targets[i], spec_ranges=tables[i])
        lb = tb.step(audio[i], targets[i])
        torch.cuda.synchronize()
        assert torch.equal(la, lb), (float(la), float(lb))
    assert changed == [True, True]
    _assert_same_state(ta, tb)


def test_graphed_step_replays_one_graph_with_changing_tables(ops):
    from adyolo_amd.datasets import synthetic_audio
    audio = [synthetic_audio(2, 48000, seed=60 + i).to(DEV) for i in range(2)]
    targets, tables = _targets("adyolo", 4, 70), _step_tables(4, 8)
    assert len({tuple(r.flatten().tolist()) for r in tables}) == 4
    te, tg = _trainer(False), _trainer(True)
    plain = te.features(audio[0])
    assert all(not torch.equal(te.features(audio[0], spec_ranges=r), plain) for r in tables)
    le, lg = [], []
    for i in range(4):                                            # eager warm-up, the recording, then three replays in all
        le.append(te.step(audio[i % 2], targets[i], spec_ranges=tables[i]).clone())
        lg.append(tg.step(audio[i % 2], targets[i], spec_ranges=tables[i]).clone())
    torch.cuda.synchronize()
    assert tg.graphs.captures == 1 and tg.graphs.replays == 3 and tg.graphs.eager_steps == 1
    for i, (a, b) in enumerate(zip(le, lg)):
        assert torch.equal(a, b), (i, float(a), float(b))
    _assert_same_state(te, tg)
    # the (B, 2, 4) tables at the same shape are a graph of their own; this one is not recorded again
    for _ in range(2):
        tg.step(audio[0], targets[0], spec_ranges=tables[0][:, :2].contiguous())
    tg.step(audio[1], targets[1], spec_ranges=tables[1])
    torch.cuda.synchronize()
    assert tg.graphs.captures == 2 and tg.graphs.replays == 5


# ------------------------------------------------------------------------------------------------------------------ epoch
SR = 24000
RECS = (("fold1_room1_mix001", 4.0), ("fold2_room1_mix003", 3.0))      # 3 + 2 chunks of 2 s


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    root = tmp_path_factory.mktemp("gpu_feature_aug")
    write_classwise_split(root, recordings=RECS, sr=SR, window_s=2, stride_s=1, seed=21, nb_classes=12)
    return root


def _epoch_prm(root, loss, on=True):
    prm = classwise_params(root, loss, batch_size=2, nb_iters=2, spec=True, rotation=True, window_s=2, stride_s=1, sr=SR,
                           nb_classes=12)
    prm["args"]["device"] = DEV
    prm["train_config"].update({"loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
                                "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0})
    prm["aug_config"].update({"spec_augment_thresh": 0.8, "spec_augment_time_mask_param": 30, "spec_augment_freq_mask_param": 40})
    if on:
        prm["aug_config"].update({"freq_shift_augment": True, "freq_shift_prob": 0.8, "freq_shift_max_bins": 6,
                                  "cutout_augment": True, "cutout_prob": 0.8})
    return prm


@pytest.mark.parametrize("loss", ["adyolo", "adpit"])
def test_corpus_epoch_equals_the_host_epoch_with_the_keys_on(ops, split, loss):
    from adyolo_amd.corpus import ClasswiseDeviceCorpus, DeviceCorpus, load_chunked_split
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    from adyolo_amd.train import train_one_epoch_audio, train_one_epoch_corpus
    prm = _epoch_prm(split, loss)
    seed = 29
    random.seed(seed)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=audio_collate_fn, num_workers=0)
    th = _corpus_trainer(False, prm)
    seen = []
    inner = th.step

    def watching(audio, target, spec=None):
        seen.append(spec.clone())
        return inner(audio, target, spec)
    th.step = watching
    mean_h = train_one_epoch_audio(prm, loader, th)
    state_h = random.getstate()
    hc = load_chunked_split(prm)
    random.seed(seed)
    corpus = (DeviceCorpus if loss == "adyolo" else ClasswiseDeviceCorpus)(hc, prm, DEV, rank=0, world=1)
    assert corpus.get_filelist() == ds.get_filelist()
    tc = _corpus_trainer(False, prm)
    mean_c = train_one_epoch_corpus(prm, corpus, tc)
    torch.cuda.synchronize()
    assert random.getstate() == state_h
    assert len(th.recorded) == len(tc.recorded) == 2
    for i, ((lh, _, _), (lc, _, _)) in enumerate(zip(th.recorded, tc.recorded)):
        assert bool(torch.isfinite(lh)) and torch.equal(lh, lc), (i, float(lh), float(lc))
    assert mean_h == mean_c
    assert torch.equal(th.flat.flat, tc.flat.flat)
    assert torch.equal(th.optimizer.exp_avg, tc.optimizer.exp_avg) and torch.equal(th.optimizer.exp_avg_sq, tc.optimizer.exp_avg_sq)
    # the tables reached the steps, and they do change the features
    assert all(tuple(s.shape) == (2, 4, 4) for s in seen)
    tabs = torch.cat([s.cpu() for s in seen])
    assert bool((tabs[:, 3, 0] != 0).any()) and bool((tabs[:, 2, 1] > tabs[:, 2, 0]).any())
    from adyolo_amd.datasets import synthetic_audio
    audio = synthetic_audio(2, 48000, seed=1).to(DEV)
    fx = th.features
    assert not torch.equal(fx(audio, spec_ranges=seen[0]), fx(audio, spec_ranges=seen[0][:, :2].contiguous()))
