"""CPU: the host half of the frequency-shift and cutout augmentation (``aug_config.freq_shift_augment`` / ``cutout_augment``).
The NumPy oracle ``apply_feature_aug_host`` against ``np.pad(mode="reflect")`` and plain slicing; ``feature_aug_config`` (defaults,
every refusal); the draws of ``draw_feature_aug`` (ranges, sign, the exact number of draws); ``FoaDataset`` items and
``audio_collate_fn`` with the keys off (today's items and ``random`` state) and on (a (4, 4) table, everything drawn before it
unchanged); and ``_CorpusBase.draw`` of both device corpora against the dataset under the same seed."""
import os
import random
import re

import numpy as np
import pytest
import torch

import adyolo_amd  # noqa: F401
from adyolo_amd import _lib
from adyolo_amd.augmentations import (FEATURE_AUG_DEFAULTS, apply_feature_aug_host, draw_feature_aug, feature_aug_config,
                                      feature_aug_table)
from adyolo_amd.corpus import ClasswiseDeviceCorpus, DeviceCorpus, load_chunked_split
from adyolo_amd.datasets import FoaDataset, audio_collate_fn
from adyolo_amd.features import FeatureExtractor, MicFeatureExtractor
from test_corpus_classwise_cpu import classwise_params, write_classwise_split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOA_GROUPS, MIC_GROUPS = ((0, 1), (1, 2)), ((0, 1), (1, 3))
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
SR = 2400
RECS = (("fold1_room1_mix001", 6.0), ("fold1_room2_mix002", 3.7), ("fold2_room1_mix003", 2.0), ("take_chunk3_mix", 4.0))
ON = {"freq_shift_augment": True, "freq_shift_prob": 0.7, "freq_shift_max_bins": 9, "cutout_augment": True, "cutout_prob": 0.7,
      "cutout_time_param": 5, "cutout_freq_param": 30}


def _feat(b, t, c, seed=0):
    return np.random.RandomState(seed).randn(b, t, 64, c).astype(np.float32) + 3.0        # no zeros of its own


def _table(b, g=2):
    return np.zeros((b, g + 2, 4), dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------ oracle
def test_the_groups_of_the_extractors():
    assert FeatureExtractor.SPEC_GROUPS == FOA_GROUPS and FeatureExtractor.SHIFT_GROUPS == (True, True)
    assert MicFeatureExtractor.SPEC_GROUPS == MIC_GROUPS and MicFeatureExtractor.SHIFT_GROUPS == (True, False)


@pytest.mark.parametrize("s,eff", [(0, 0), (1, 1), (-1, -1), (5, 5), (-5, -5), (63, 63), (-63, -63), (64, 63), (-64, -63),
                                   (I32_MAX, 63), (-I32_MAX, -63), (I32_MIN, -63)])
def test_shift_is_reflect_padding_and_a_crop(s, eff):
    x = _feat(2, 3, 8, seed=abs(eff))
    tab = _table(2)
    tab[0, 3, 0] = s                                              # sample 1 stays
    got = apply_feature_aug_host(x, tab, FOA_GROUPS, (True, True))
    assert got.dtype == np.float32 and got is not x
    if eff > 0:
        want = np.pad(x[0], ((0, 0), (eff, 0), (0, 0)), mode="reflect")[:, :64]
    elif eff < 0:
        want = np.pad(x[0], ((0, 0), (0, -eff), (0, 0)), mode="reflect")[:, -64:]
    else:
        want = x[0]
    assert np.array_equal(got[0], want) and np.array_equal(got[1], x[1])
    assert (eff == 0) == np.array_equal(got[0], x[0])
    if eff:                                                      # spelled out: bin f reads bin f - eff, mirrored at 0 and 63
        f = np.arange(64)
        u = f - eff
        src = np.where(u < 0, -u, np.where(u > 63, 126 - u, u))
        assert src.min() >= 0 and src.max() <= 63 and np.array_equal(got[0], x[0][:, src])


def test_shift_moves_the_shifting_groups_only():
    x = _feat(2, 4, 32, seed=3)
    tab = _table(2)
    tab[:, 3, 0] = (7, -2)
    got = apply_feature_aug_host(x, tab, MIC_GROUPS, (True, False))
    assert np.array_equal(got[..., 4:], x[..., 4:])              # the GCC-PHAT quads and the padding quads: the input's bits
    for b, s in enumerate((7, -2)):
        one = _table(1)
        one[0, 3, 0] = s
        assert np.array_equal(got[b, ..., :4], apply_feature_aug_host(x[b:b + 1, ..., :8], one, FOA_GROUPS, (True, True))[0, ..., :4])
        assert not np.array_equal(got[b, ..., :4], x[b, ..., :4])
    none = apply_feature_aug_host(x, tab, MIC_GROUPS, (False, False))
    assert np.array_equal(none, x)
    both = apply_feature_aug_host(x, tab, MIC_GROUPS, (True, True))
    assert np.array_equal(both[..., :4], got[..., :4]) and not np.array_equal(both[..., 4:12], x[..., 4:12])
    assert np.array_equal(both[..., 12:], x[..., 12:])            # quads outside every group never move


def _torch_mask(x, ranges, groups):
    """``test_gpu_specaug_train.torch_mask`` in NumPy: the semantics of ``adyolo_mask_groups``."""
    out = x.copy()
    _, t, f, _ = out.shape
    for b, rows in enumerate(ranges.tolist()):
        for (q0, q1), (t0, t1, f0, f1) in zip(groups, rows):
            t0 = min(max(t0, 0), t)
            t1 = min(max(t1, t0), t)
            f0 = min(max(f0, 0), f)
            f1 = min(max(f1, f0), f)
            out[b, t0:t1, :, 4 * q0:4 * q1] = 0.0
            out[b, :, f0:f1, 4 * q0:4 * q1] = 0.0
    return out


CLAMPED = [[[-5, 3, -10, 4], [35, 1000, 60, 999]],               # the int32 extremes of test_gpu_specaug_train.py
           [[I32_MAX, I32_MIN, 70, 100], [-100, -50, 64, 64]],
           [[I32_MIN, I32_MAX, 9, 3], [20, 10, I32_MIN, I32_MAX]]]


def test_rows_below_the_cutout_are_the_specaug_stripes():
    x = _feat(3, 40, 8, seed=5)
    tab = _table(3)
    tab[:, :2] = np.asarray(CLAMPED, dtype=np.int64).astype(np.int32)
    got = apply_feature_aug_host(x, tab, FOA_GROUPS, (True, True))
    assert np.array_equal(got, _torch_mask(x, tab[:, :2], FOA_GROUPS)) and not np.array_equal(got, x)


@pytest.mark.parametrize("row,box", [((-5, 3, -10, 4), (0, 3, 0, 4)), ((35, 1000, 60, 999), (35, 40, 60, 64)),
                                     ((I32_MAX, I32_MIN, 70, 100), None), ((-100, -50, 64, 64), None),
                                     ((I32_MIN, I32_MAX, 9, 3), None), ((20, 10, I32_MIN, I32_MAX), None),
                                     ((I32_MIN, I32_MAX, I32_MIN, I32_MAX), (0, 40, 0, 64)), ((7, 8, 0, 0), None),
                                     ((0, 0, 5, 9), None), ((39, 40, 63, 64), (39, 40, 63, 64))])
def test_cutout_is_one_clamped_rectangle_over_all_channels(row, box):
    x = _feat(2, 40, 32, seed=6)
    tab = _table(2)
    tab[1, 2] = row
    got = apply_feature_aug_host(x, tab, MIC_GROUPS, (True, False))
    want = x.copy()
    if box is not None:
        want[1, box[0]:box[1], box[2]:box[3], :] = 0.0
    assert np.array_equal(got, want) and np.array_equal(got[0], x[0])
    assert (box is None) == np.array_equal(got, x)


def test_the_order_is_shift_then_stripes_then_cutout():
    x = _feat(1, 12, 8, seed=7)
    tab = _table(1)
    tab[0] = [[2, 4, 10, 12], [0, 0, 60, 64], [3, 9, 11, 30], [6, 0, 0, 0]]
    got = apply_feature_aug_host(x, tab, FOA_GROUPS, (True, True))
    only_shift = _table(1)
    only_shift[0, 3, 0] = 6
    want = apply_feature_aug_host(x, only_shift, FOA_GROUPS, (True, True))
    want[0, 2:4, :, :4] = 0.0
    want[0, :, 10:12, :4] = 0.0
    want[0, :, 60:64, 4:] = 0.0
    want[0, 3:9, 11:30, :] = 0.0
    assert np.array_equal(got, want)
    assert float(got[0, 5, 12, 0]) == 0.0 and float(got[0, 0, 16, 0]) == float(x[0, 0, 10, 0])     # masks do not move with the shift
    t = torch.from_numpy(x)
    assert np.array_equal(apply_feature_aug_host(t, torch.from_numpy(tab), FOA_GROUPS, (True, True)), got)     # tensors too
    with pytest.raises(ValueError):
        apply_feature_aug_host(x, tab[:, :3], FOA_GROUPS, (True, True))


# ------------------------------------------------------------------------------------------------------------------ config
def test_config_defaults_and_off():
    assert feature_aug_config({}) is None and feature_aug_config({"aug_config": {"spec_augment": True}}) is None
    assert FEATURE_AUG_DEFAULTS == {"freq_shift_prob": 0.5, "freq_shift_max_bins": 5, "cutout_prob": 0.5, "cutout_time_param": 40,
                                    "cutout_freq_param": 20}
    assert feature_aug_config({"aug_config": {"freq_shift_augment": True}}) == (0.5, 5, None, 0.0, 0.0)
    assert feature_aug_config({"aug_config": {"cutout_augment": True}}) == (None, 5, 0.5, 40.0, 20.0)
    assert feature_aug_config({"aug_config": {"freq_shift_augment": True, "cutout_augment": True}}) == (0.5, 5, 0.5, 40.0, 20.0)
    assert feature_aug_config({"aug_config": ON}) == (0.7, 9, 0.7, 5.0, 30.0)
    assert feature_aug_config({"aug_config": dict(ON, freq_shift_prob=1, freq_shift_max_bins=63, cutout_prob=0)})[:3] == (1.0, 63, 0.0)
    # the keys of an augmentation that is off are not read
    assert feature_aug_config({"aug_config": {"freq_shift_augment": False, "freq_shift_prob": 7, "cutout_augment": False,
                                              "cutout_time_param": -1}}) is None
    assert feature_aug_config({"aug_config": {"cutout_augment": True, "freq_shift_max_bins": 0}}) == (None, 5, 0.5, 40.0, 20.0)
    assert feature_aug_config({"aug_config": {"freq_shift_augment": True, "cutout_prob": 9}}) == (0.5, 5, None, 0.0, 0.0)


@pytest.mark.parametrize("key,value", [("freq_shift_prob", -0.1), ("freq_shift_prob", 1.5), ("freq_shift_prob", "0.5"),
                                       ("freq_shift_prob", True), ("freq_shift_prob", float("nan")),
                                       ("freq_shift_max_bins", 0), ("freq_shift_max_bins", 64), ("freq_shift_max_bins", 2.0),
                                       ("freq_shift_max_bins", True), ("freq_shift_max_bins", -3),
                                       ("cutout_prob", -1e-9), ("cutout_prob", 2), ("cutout_prob", None),
                                       ("cutout_time_param", -1), ("cutout_time_param", float("inf")), ("cutout_time_param", "40"),
                                       ("cutout_freq_param", -0.5), ("cutout_freq_param", float("nan")),
                                       ("cutout_freq_param", False)])
def test_bad_keys_are_refused_by_name(splits, key, value):
    aug = dict(ON)
    aug[key] = value
    with pytest.raises(ValueError, match=key):
        feature_aug_config({"aug_config": aug})
    prm = _prm(splits)
    prm["aug_config"][key] = value
    with pytest.raises(ValueError, match=key):
        FoaDataset(prm, "train", rank=0, world=1)
    with pytest.raises(ValueError, match=key):
        DeviceCorpus(load_chunked_split(_prm(splits, on=False)), prm, "cpu", rank=0, world=1)


# ------------------------------------------------------------------------------------------------------------------- draws
class _Counting:
    """``random``'s surface as ``draw_feature_aug`` uses it, counting the draws."""

    def __init__(self, seed):
        self.r, self.n = random.Random(seed), 0

    def random(self):
        self.n += 1
        return self.r.random()


def test_draws_stay_in_range_and_take_the_stated_number_of_draws():
    t, f = 80, 64
    for shift_on in (False, True):
        for cut_on in (False, True):
            if not shift_on and not cut_on:
                continue
            aug = {"freq_shift_augment": shift_on, "cutout_augment": cut_on, "freq_shift_max_bins": 7, "freq_shift_prob": 0.6,
                   "cutout_prob": 0.6, "cutout_time_param": 40, "cutout_freq_param": 20}
            cfg = feature_aug_config({"aug_config": aug})
            rnd = _Counting(12)
            replay = random.Random(12)
            shifts, boxes = set(), 0
            for _ in range(400):
                n0 = rnd.n
                row, s = draw_feature_aug(rnd, cfg, t, f)
                want = 0
                if shift_on:
                    want += 1
                    drawn = replay.random() < 0.6
                    assert drawn == (s != 0)                      # never 0 when the shift was drawn
                    if drawn:
                        want += 2
                        size = 1 + min(int(replay.random() * 7), 6)
                        assert s == (-size if replay.random() < 0.5 else size)
                else:
                    assert s == 0
                if cut_on:
                    want += 1
                    if replay.random() < 0.6:
                        want += 4
                        ref = []
                        for param, size in ((40, t), (20, f)):
                            value = replay.random() * param
                            start = replay.random() * (size - value)
                            ref += [int(start), int(start + value)]
                        assert row == ref
                        boxes += 1
                    else:
                        assert row == [0, 0, 0, 0]
                else:
                    assert row == [0, 0, 0, 0]
                assert rnd.n - n0 == want
                assert -7 <= s <= 7 and 0 <= row[0] <= row[1] <= t and 0 <= row[2] <= row[3] <= f
                assert row[1] - row[0] <= 40 and row[3] - row[2] <= 20
                shifts.add(s)
            if shift_on:
                assert shifts == set(range(-7, 8))
            if cut_on:
                assert 180 <= boxes <= 300
    # the special probabilities and the largest size
    cfg = feature_aug_config({"aug_config": {"freq_shift_augment": True, "freq_shift_prob": 1.0, "freq_shift_max_bins": 1,
                                             "cutout_augment": True, "cutout_prob": 0.0}})
    rnd = _Counting(1)
    assert {draw_feature_aug(rnd, cfg, t, f)[1] for _ in range(40)} == {-1, 1} and rnd.n == 40 * 4

    class _One:                                                   # random() just below 1: the min() of the size formula
        @staticmethod
        def random():
            return 1.0 - 2.0 ** -53
    cfg = feature_aug_config({"aug_config": {"freq_shift_augment": True, "freq_shift_prob": 1.0, "freq_shift_max_bins": 63}})
    assert draw_feature_aug(_One, cfg, t, f) == ([0, 0, 0, 0], 63)


def test_the_item_table():
    tab = feature_aug_table(torch.tensor([[1, 2, 3, 4], [5, 6, 7, 8]], dtype=torch.int32), [9, 10, 11, 12], -4)
    assert tab.dtype == torch.int32 and tab.tolist() == [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [-4, 0, 0, 0]]


# ----------------------------------------------------------------------------------------------- FoaDataset and the corpora
@pytest.fixture(scope="module")
def splits(tmp_path_factory):
    out = {}
    for fmt in ("foa", "mic"):
        root = tmp_path_factory.mktemp("feature_aug_" + fmt)
        write_classwise_split(root, recordings=RECS, sr=SR, window_s=2, stride_s=1, seed=9, audio_dir=fmt + "_dev")
        out[fmt] = root
    return out


def _prm(splits, loss="adyolo", on=True, spec=True, mix=False, swap=False, keys=None):
    prm = classwise_params(splits["mic" if swap else "foa"], loss, batch_size=4, nb_iters=2, spec=spec, rotation=not swap,
                           window_s=2, stride_s=1, sr=SR)
    if swap:
        prm["data_config"]["audio_format"] = "mic"
        prm["aug_config"]["channel_swap_augment"] = True
    if mix:
        prm["aug_config"].update({"time_mix_augment": True, "time_mix_prob": 0.6, "time_mix_gain_db": [-6.0, 3.0]})
    if on:
        prm["aug_config"].update(ON if keys is None else keys)
    return prm


def _same_item(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert sorted(x) == sorted(y)
            for k in x:
                assert (x[k] is None and y[k] is None) or np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k
        elif isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and torch.equal(x, y)
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        else:
            assert x == y


@pytest.mark.parametrize("spec,mix", [(False, False), (True, False), (True, True)])
def test_keys_off_leave_items_and_random_stream_alone(splits, spec, mix):
    """Absent keys, keys set to false (with their other keys present) and a validation split: the items of today, the state of
    ``random`` after them included -- replayed here from the stated draw order, without the new code in the loop."""
    from adyolo_amd.augmentations import SpecAug, draw_time_mix, time_mix_config
    absent = _prm(splits, on=False, spec=spec, mix=mix)
    false = _prm(splits, on=True, spec=spec, mix=mix, keys=dict(ON, freq_shift_augment=False, cutout_augment=False))
    runs = []
    for prm in (absent, false):
        random.seed(31)
        ds = FoaDataset(prm, "train", rank=0, world=1)
        assert ds.feat_aug is None
        runs.append(([ds[i] for i in range(len(ds))], random.getstate(), ds))
    for a, b in zip(runs[0][0], runs[1][0]):
        _same_item(a, b)
    assert runs[0][1] == runs[1][1]
    items, state, ds = runs[0]
    assert all(len(it) == 3 + spec + mix for it in items)
    if spec:
        assert all(tuple(it[3].shape) == (2, 4) for it in items)
    # today's stream: rotation, SpecAug (MEL, IV), then the mixing draws -- and nothing after them
    random.seed(31)
    FoaDataset(absent, "train", rank=0, world=1)
    sa = SpecAug(absent, False)
    for i, it in enumerate(items):
        assert it[1] == int(random.uniform(0, 16))
        if spec:
            assert it[3].tolist() == [sa._draw_one(2 * SR // 600, 64) for _ in range(2)]
        if mix:
            draw_time_mix(random, time_mix_config(absent), ds.total_filelist, ds.filelist[i], "rotate")
    assert random.getstate() == state
    assert FoaDataset(_prm(splits, spec=spec, mix=mix), "train", is_valid=True, rank=0, world=1).feat_aug is None


@pytest.mark.parametrize("spec,mix,swap", [(True, False, False), (False, False, False), (True, True, False), (False, True, True)])
def test_keys_on_append_the_last_draws_of_an_item(splits, spec, mix, swap):
    """Per item under one seed: the first three elements, rows 0-1 of the table and the mixing dict equal the keys-off item; rows
    2-3 are ``draw_feature_aug`` on the stream right after the keys-off item's draws."""
    loss = "adpit" if swap else "adyolo"
    on, off = _prm(splits, loss, spec=spec, mix=mix, swap=swap), _prm(splits, loss, on=False, spec=spec, mix=mix, swap=swap)
    random.seed(5)
    ds_on = FoaDataset(on, "train", rank=0, world=1)
    random.seed(5)
    ds_off = FoaDataset(off, "train", rank=0, world=1)
    assert ds_on.filelist == ds_off.filelist and ds_on.feat_aug == (0.7, 9, 0.7, 5.0, 30.0)
    t = 2 * SR // 600
    seen_shift, seen_cut, items = set(), 0, []
    for i in range(len(ds_on)):
        random.seed(100 + i)
        a = ds_on[i]
        state_on = random.getstate()
        random.seed(100 + i)
        b = ds_off[i]
        cut, shift = draw_feature_aug(random, ds_on.feat_aug, t, 64)
        assert random.getstate() == state_on
        _same_item(a[:3], b[:3])
        tab = a[3]
        assert isinstance(tab, torch.Tensor) and tab.dtype == torch.int32 and tuple(tab.shape) == (4, 4)
        assert tab[:2].tolist() == (b[3].tolist() if spec else [[0] * 4] * 2)
        assert tab[2].tolist() == cut and tab[3].tolist() == [shift, 0, 0, 0]
        assert len(a) == 4 + mix and len(b) == 3 + spec + mix
        if mix:
            _same_item(a[4:], b[-1:])
        seen_shift.add(shift)
        seen_cut += cut != [0, 0, 0, 0]
        items.append(a)
    assert len(seen_shift) > 2 and 0 in seen_shift and seen_cut >= 2
    batch = audio_collate_fn(items[:4])
    assert len(batch) == 4 + mix
    assert batch[3].dtype == torch.int32 and tuple(batch[3].shape) == (4, 4, 4)
    assert torch.equal(batch[3], torch.stack([it[3] for it in items[:4]]))
    if mix:
        assert isinstance(batch[4], dict)
    # one key alone
    for key in ("freq_shift_augment", "cutout_augment"):
        one = _prm(splits, loss, spec=spec, mix=mix, swap=swap, keys={key: True})
        random.seed(5)
        ds = FoaDataset(one, "train", rank=0, world=1)
        random.seed(77)
        tab = ds[0][3]
        assert tuple(tab.shape) == (4, 4)
        assert (tab[3].tolist() == [0, 0, 0, 0]) if key == "cutout_augment" else (tab[2].tolist() == [0, 0, 0, 0])


@pytest.mark.parametrize("config", ["yolo", "yolo_mix", "yolo_nospec", "adpit_swap", "adpit_swap_mix", "seddoa_mix"])
def test_both_corpora_draw_the_tables_of_the_dataset(splits, config):
    """Three epochs under one seed: ``_CorpusBase.draw`` gives the combination, the (4, 4) table and the mate of every
    ``FoaDataset`` item, and leaves ``random`` in the same state."""
    mix, swap = config.endswith("_mix"), "swap" in config
    loss = config.split("_")[0].replace("yolo", "adyolo")
    prm = _prm(splits, loss, spec=config != "yolo_nospec", mix=mix, swap=swap)
    hc = load_chunked_split(prm)
    make_corpus = DeviceCorpus if loss == "adyolo" else ClasswiseDeviceCorpus

    def host_epoch(ds):
        out = []
        for i in range(len(ds)):
            item = ds[i]
            assert tuple(item[3].shape) == (4, 4)
            mate = None
            if mix and item[-1]["mate_pcm"] is not None:
                mate = (item[-1]["mate_pcm"].tobytes(), item[-1]["mate_comb"], np.float32(item[-1]["gain"]).tobytes())
            out.append((ds.filelist[i], item[1], item[3].tolist(), mate))
        return out

    def corpus_epoch(corpus):
        out = []
        files = corpus.get_filelist()
        for b0 in range(0, len(files), 4):
            idx = range(b0, min(len(files), b0 + 4))
            drawn = corpus.draw(idx)
            assert len(drawn) == 2 + mix
            items, spec = drawn[:2]
            assert spec.dtype == np.int32 and spec.shape == (len(idx), 4, 4)
            for j, i in enumerate(idx):
                mate = None
                if mix and drawn[2][j, 0] != -1:
                    off, _, _, _, m_comb, _, gain, _ = (int(v) for v in drawn[2][j])
                    mate = (hc.audio[off:off + hc.window].tobytes(), max(m_comb, 0),
                            np.array([gain], dtype=np.uint32).view(np.float32).tobytes())
                out.append((files[i], max(int(items[j, 4]), 0), spec[j].tolist(), mate))
        return out

    def run(make, epoch):
        random.seed(97)
        ds = make()
        seq = [epoch(ds)]
        for _ in range(2):
            ds.sample_filelist_for_train_iter()
            seq.append(epoch(ds))
        return seq, random.getstate()

    host, hstate = run(lambda: FoaDataset(prm, "train", rank=0, world=1), host_epoch)
    dev, dstate = run(lambda: make_corpus(hc, prm, "cpu", rank=0, world=1), corpus_epoch)
    assert host == dev and hstate == dstate
    flat = [it for ep in dev for it in ep]
    assert len(flat) == 24
    assert len({it[2][3][0] for it in flat}) > 4 and sum(it[2][2] != [0, 0, 0, 0] for it in flat) >= 8
    assert all(it[2][3][1:] == [0, 0, 0] for it in flat)
    if config == "yolo_nospec":
        assert all(it[2][:2] == [[0] * 4] * 2 for it in flat)
    else:
        assert any(it[2][:2] != [[0] * 4] * 2 for it in flat)
    if mix:
        assert 6 <= sum(it[3] is not None for it in flat) <= 22
    # keys off: the corpus draws today's shapes
    off = make_corpus(hc, _prm(splits, loss, on=False, spec=config != "yolo_nospec", mix=mix, swap=swap), "cpu", rank=0, world=1)
    spec = off.draw(range(4))[1]
    assert off.feat_aug is None and (spec is None if config == "yolo_nospec" else spec.shape == (4, 2, 4))


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_the_new_symbol_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "adyolo_hip.h")).read()
    assert "adyolo_feat_augment" in _lib.SIGNATURES and re.search(r"\badyolo_feat_augment\s*\(", hdr)
    assert getattr(_lib.load(), "adyolo_feat_augment") is not None


def test_feat_augment_refuses_host_tensors_and_bad_tables():
    from adyolo_amd import ops
    with pytest.raises(_lib.AdyoloHipError):
        ops.feat_augment_(torch.zeros(1, 4, 64, 8), torch.zeros(1, 4, 4, dtype=torch.int32), FOA_GROUPS, (True, True))
