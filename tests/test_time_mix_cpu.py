"""CPU: the host half of the time-domain mixing augmentation (``aug_config.time_mix_augment``).  ``merge_labels`` and what the
unchanged encoders make of a merged dict; the refusals of the config keys; the draws of ``_CorpusBase.draw`` against
``FoaDataset`` iterated in the main process (items, mates, combinations, gains and the state of ``random`` after three epochs, in
four configurations); the special probabilities; and the key-off surface, which must be today's."""
import copy
import os
import random
import re

import numpy as np
import pytest
import torch

import adyolo_amd  # noqa: F401
from adyolo_amd import _lib
from adyolo_amd.augmentations import merge_labels, time_mix_enabled
from adyolo_amd.corpus import ClasswiseDeviceCorpus, DeviceCorpus, load_chunked_split
from adyolo_amd.datasets import ClasswiseLabelEncoder, FoaDataset, YoloLabelEncoder, audio_collate_fn
from test_corpus_classwise_cpu import classwise_params, write_classwise_split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 2400
RECS = (("fold1_room1_mix001", 6.0), ("fold1_room2_mix002", 3.7), ("fold2_room1_mix003", 2.0), ("take_chunk3_mix", 4.0))
#        5 + 3 + 1 + 3 = 12 chunks of 2 s (1 s stride)


@pytest.fixture(scope="module")
def splits(tmp_path_factory):
    out = {}
    for fmt in ("foa", "mic"):
        root = tmp_path_factory.mktemp("time_mix_" + fmt)
        write_classwise_split(root, recordings=RECS, sr=SR, window_s=2, stride_s=1, seed=5, audio_dir=fmt + "_dev")
        out[fmt] = root
    return out


def _prm(splits, loss="adyolo", rotation=True, swap=False, spec=False, mix=True, prob=0.6, gain=(-6.0, 3.0)):
    prm = classwise_params(splits["mic" if swap else "foa"], loss, batch_size=4, nb_iters=2, spec=spec, rotation=rotation,
                           window_s=2, stride_s=1, sr=SR)
    if swap:
        prm["data_config"]["audio_format"] = "mic"
        prm["aug_config"]["channel_swap_augment"] = True
    if mix:
        prm["aug_config"].update({"time_mix_augment": True, "time_mix_prob": prob, "time_mix_gain_db": list(gain)})
    return prm


# ------------------------------------------------------------------------------------------------------------ merge_labels
def test_merge_labels_orders_frames_and_sources_and_copies():
    a = {7: [[1, 0, 10.0, 5.0]], 2: [[3, 0, -20.0, 0.0], [4, 1, 30.0, 1.0]]}
    b = {5: [[2, 0, 0.0, 0.0]], 2: [[9, 0, 90.0, -5.0]], 11: [[0, 0, 1.0, 2.0]]}
    a0, b0 = copy.deepcopy(a), copy.deepcopy(b)
    m = merge_labels(a, b)
    assert list(m) == [2, 5, 7, 11]
    assert m[2] == [[3, 0, -20.0, 0.0], [4, 1, 30.0, 1.0], [9, 0, 90.0, -5.0]]          # a before b within a frame
    assert m[5] == b[5] and m[7] == a[7] and m[11] == b[11]
    m[2][0][2] = 123.0
    m[5].append("x")
    assert a == a0 and b == b0                                                           # new dict, new lists, new events
    assert merge_labels({}, {}) == {}
    assert merge_labels(a, {}) == {2: a[2], 7: a[7]} and list(merge_labels(a, {})) == [2, 7]
    assert merge_labels({}, b) == {2: b[2], 5: b[5], 11: b[11]}


def test_merged_labels_through_the_encoders():
    """AD-YOLO rows in frame order, a before b; SEDDOA / ACCDOA: the mate wins a same-class collision; ADPIT: 1+1, 2+1 and 2+2
    events of one class in one frame land in the B, C and C (first three) slots."""
    def ev(cls, az, el=0.0):
        return [cls, 0, az, el]
    enc = ClasswiseLabelEncoder(3)
    one = lambda label: enc.get_adpit_label(label, 4)             # noqa: E731
    a = {0: [ev(1, 10.0)], 1: [ev(1, 10.0), ev(1, 20.0)], 2: [ev(1, 10.0), ev(1, 20.0)], 3: [ev(2, 50.0)]}
    b = {0: [ev(1, 30.0)], 1: [ev(1, 30.0)], 2: [ev(1, 30.0), ev(1, 40.0)]}
    got = one(merge_labels(a, b))
    active = got[:, :, 0, 1]                                      # (frame, slot) activity of class 1
    assert active[0].tolist() == [0, 1, 1, 0, 0, 0]               # 1 + 1 -> B0 B1
    assert active[1].tolist() == [0, 0, 0, 1, 1, 1]               # 2 + 1 -> C0 C1 C2
    assert active[2].tolist() == [0, 0, 0, 1, 1, 1]               # 2 + 2 -> the first three
    assert got[3, 0, 0, 2] == 1 and got[3, :, 0, 1].sum() == 0

    def xyz_of(az):
        return one({0: [ev(1, az)]})[0, 0, 1:, 1]
    assert torch.equal(got[0, 1, 1:, 1], xyz_of(10.0)) and torch.equal(got[0, 2, 1:, 1], xyz_of(30.0))
    assert [torch.equal(got[2, 3 + k, 1:, 1], xyz_of(az)) for k, az in enumerate((10.0, 20.0, 30.0))] == [True] * 3
    sed = enc.get_seddoa_label(merge_labels(a, b), 4)
    assert torch.equal(sed[0], enc.get_seddoa_label({0: [ev(1, 30.0)]}, 1)[0])          # later events overwrite: the mate's
    acc = enc.get_accdoa_label(merge_labels(a, b), 4)
    assert torch.equal(acc[0], enc.get_accdoa_label({0: [ev(1, 30.0)]}, 1)[0])
    yolo = YoloLabelEncoder()
    rows = yolo.get_yolo_label(merge_labels({3: [ev(0, 10.0)], 1: [ev(1, 10.0)]}, {1: [ev(2, 10.0)], 0: [ev(3, 10.0)]}), 4)
    order = []
    for r in rows:
        if (r[0], r[3]) not in order:
            order.append((r[0], r[3]))
    assert order == [(0, 3.0), (1, 1.0), (1, 2.0), (3, 0.0)]


# ------------------------------------------------------------------------------------------------------------------ config
@pytest.mark.parametrize("key,value", [("time_mix_prob", -0.1), ("time_mix_prob", 1.5), ("time_mix_gain_db", [1.0, 0.0]),
                                       ("time_mix_gain_db", [0.0, float("inf")]), ("time_mix_gain_db", [float("nan"), 0.0])])
def test_bad_keys_are_refused_by_name(splits, key, value):
    prm = _prm(splits)
    prm["aug_config"][key] = value
    with pytest.raises(ValueError, match=key):
        time_mix_enabled(prm)
    with pytest.raises(ValueError, match=key):
        FoaDataset(prm, "train", rank=0, world=1)
    with pytest.raises(ValueError, match=key):
        DeviceCorpus(load_chunked_split(_prm(splits, mix=False)), prm, "cpu", rank=0, world=1)
    prm["aug_config"]["time_mix_augment"] = False                 # the keys are read only with the augmentation on
    assert time_mix_enabled(prm) is False


def test_defaults_and_the_enabled_helper(splits):
    from adyolo_amd.augmentations import time_mix_config
    assert time_mix_enabled(_prm(splits, mix=False)) is False and time_mix_enabled({}) is False
    prm = _prm(splits, mix=False)
    prm["aug_config"]["time_mix_augment"] = True
    assert time_mix_enabled(prm) is True and time_mix_config(prm) == (0.5, 0.0, 0.0)
    prm["aug_config"]["time_mix_prob"] = 1
    assert time_mix_config(prm) == (1.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------------------------- draws
def _host_epoch(ds, hc):
    """FoaDataset iterated in the main process: per item (file, comb, spec table, mate) with mate = None or (the mate's chunk
    name found by its audio and label window, combination, float32 gain bits)."""
    out = []
    for i in range(len(ds)):
        item = ds[i]
        mix = item[-1]
        assert isinstance(mix, dict) and sorted(mix) == ["gain", "mate_comb", "mate_pcm"]
        spec = item[3].tolist() if len(item) == 5 else None
        mate = None
        if mix["mate_pcm"] is not None:
            assert mix["mate_pcm"].dtype == np.int16 and mix["mate_pcm"].shape == (hc.window, 4)
            mate = (mix["mate_pcm"].tobytes(), mix["mate_comb"], np.float32(mix["gain"]).tobytes())
        out.append((ds.filelist[i], item[1], spec, mate))
    return out


def _corpus_epoch(corpus, bs, no_comb):
    out = []
    files = corpus.get_filelist()
    hc = corpus.host
    for b0 in range(0, len(files), bs):
        idx = range(b0, min(len(files), b0 + bs))
        items, spec, mates = corpus.draw(idx)
        assert mates.dtype == np.int64 and mates.shape == items.shape
        for j, i in enumerate(idx):
            comb = int(items[j, 4])
            mate = None
            if mates[j, 0] != -1:
                off, f_off, lo, n, m_comb, rec, gain, zero = (int(v) for v in mates[j])
                name = next(k for k, v in hc.chunks.items() if v == (rec, off, f_off))
                assert hc.chunk_events[name] == (lo, n) and zero == 0 and name != files[i] and 0 <= gain < 2 ** 32
                mate = (hc.audio[off:off + hc.window].tobytes(), no_comb if m_comb < 0 else m_comb,
                        np.array([gain], dtype=np.uint32).view(np.float32).tobytes())
            else:
                assert mates[j].tolist() == [-1, 0, 0, 0, -1, 0, 0, 0]
            out.append((files[i], no_comb if comb < 0 else comb, spec[j].tolist() if spec is not None else None, mate))
    return out


@pytest.mark.parametrize("config", ["rotation", "no_rotation", "mic_swap", "specaug"])
def test_three_epochs_draw_what_foadataset_draws(splits, config):
    from adyolo_amd.augmentations import MIC_SWAP_COMBS
    prm = _prm(splits, loss="adpit" if config == "mic_swap" else "adyolo", rotation=config in ("rotation", "specaug"),
               swap=config == "mic_swap", spec=config == "specaug")
    hc = load_chunked_split(prm)
    make_corpus = ClasswiseDeviceCorpus if config == "mic_swap" else DeviceCorpus

    def run(make, epoch):
        random.seed(97)
        ds = make()
        seq = [epoch(ds)]
        for _ in range(2):
            ds.sample_filelist_for_train_iter()
            seq.append(epoch(ds))
        return seq, random.getstate()

    host, hstate = run(lambda: FoaDataset(prm, "train", rank=0, world=1), lambda ds: _host_epoch(ds, hc))
    dev, dstate = run(lambda: make_corpus(hc, prm, "cpu", rank=0, world=1), lambda c: _corpus_epoch(c, 4, 0))
    assert host == dev and hstate == dstate
    flat = [it for ep in dev for it in ep]
    assert len(flat) == 24
    mixed = [it for it in flat if it[3] is not None]
    assert 6 <= len(mixed) <= 22                                   # prob 0.6
    gains = {np.frombuffer(m[3][2], dtype=np.float32)[0] for m in mixed}
    lo, hi = np.float32(10.0 ** (-6.0 / 20.0)), np.float32(10.0 ** (3.0 / 20.0))
    assert len(gains) > 4 and all(lo <= g <= hi for g in gains)
    mate_combs = {m[3][1] for m in mixed}
    if config == "no_rotation":
        assert mate_combs == {0} and {it[1] for it in flat} == {0}
    elif config == "mic_swap":
        assert mate_combs <= set(MIC_SWAP_COMBS) and len(mate_combs) > 2
    else:
        assert len(mate_combs) > 4 and any(it[1] != it[3][1] for it in mixed)
    if config == "specaug":
        assert any(it[2] != [[0, 0, 0, 0], [0, 0, 0, 0]] for it in flat)


def test_the_host_target_is_the_encoding_of_the_merged_labels(splits):
    """One epoch of items: the target of a mixed item is the encoder's output on ``merge_labels`` of both chunks' rotated labels."""
    from adyolo_amd.augmentations import rotate_labels
    prm = _prm(splits, prob=1.0)
    random.seed(3)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    hc = load_chunked_split(prm)
    by_audio = {hc.audio[off:off + hc.window].tobytes(): name for name, (_, off, _) in hc.chunks.items()}
    seen = 0
    for i in range(len(ds)):
        pcm, comb, target, mix = ds[i]
        if mix["mate_pcm"] is None:
            continue
        seen += 1
        mate = by_audio[mix["mate_pcm"].tobytes()]
        la = rotate_labels(ds.load_csv2dict(os.path.join(ds.csv_pth, ds.filelist[i] + ".csv")), comb)
        lb = rotate_labels(ds.load_csv2dict(os.path.join(ds.csv_pth, mate + ".csv")), mix["mate_comb"])
        assert target == ds.encoder.get_yolo_label(merge_labels(la, lb), 20)
        assert mix["gain"] == float(np.float32(mix["gain"]))
    assert seen >= 6


def test_special_probabilities(splits):
    hc = load_chunked_split(_prm(splits))
    for prob in (0.0, 1.0):
        prm = _prm(splits, prob=prob, gain=(0.0, 0.0))
        random.seed(11)
        corpus = DeviceCorpus(hc, prm, "cpu", rank=0, world=1)
        files = corpus.get_filelist()
        items, spec, mates = corpus.draw(range(len(files)))
        if prob == 0.0:
            assert (mates[:, 0] == -1).all()
            continue
        unmixed = np.flatnonzero(mates[:, 0] == -1)
        assert len(unmixed) < len(files) - 2
        one = int(np.float32(1.0).view(np.uint32))
        assert all(int(g) == one for g in mates[mates[:, 0] != -1, 6])          # lo = hi = 0 dB: exactly 1.0
        # an unmixed item at prob 1.0 drew itself: replay the stream
        random.seed(11)
        again = DeviceCorpus(hc, prm, "cpu", rank=0, world=1)
        for j, name in enumerate(again.get_filelist()):
            random.uniform(0, 16)                                                # the item's own combination
            assert random.random() < 1.0
            mate = again.total_filelist[int(random.uniform(0, len(again.total_filelist)))]
            random.uniform(0, 16)
            random.uniform(0.0, 0.0)
            assert (mate == name) == (j in unmixed), j


def test_key_off_is_todays_surface(splits, monkeypatch):
    prm = _prm(splits, mix=False, spec=True)
    hc = load_chunked_split(prm)
    random.seed(5)
    corpus = DeviceCorpus(hc, prm, "cpu", rank=0, world=1)
    drawn = corpus.draw(range(4))
    assert isinstance(drawn, tuple) and len(drawn) == 2 and corpus.mix is None
    random.seed(5)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    item = ds[0]
    assert len(item) == 4 and not isinstance(item[-1], dict) and ds.mix is None
    batch = audio_collate_fn([ds[i] for i in range(4)])
    assert len(batch) == 4 and not isinstance(batch[-1], dict)
    prm_off = _prm(splits, mix=False, spec=False)
    assert len(FoaDataset(prm_off, "train", rank=0, world=1)[0]) == 3
    # the capacity doubles its event term with the key on and only then
    from adyolo_amd import graph
    monkeypatch.setattr(graph, "TARGET_QUANTUM", 1)
    off = DeviceCorpus(hc, prm, "cpu", rank=0, world=1)
    on = DeviceCorpus(hc, _prm(splits, spec=True), "cpu", rank=0, world=1)
    assert off.cap == 4 * hc.max_events * off.cells > 0
    assert on.cap == 4 * 2 * hc.max_events * on.cells == 2 * off.cap and on.target_shape(4) == (on.cap, 7)
    # a validation split ignores the key
    assert FoaDataset(_prm(splits), "train", is_valid=True, rank=0, world=1).mix is None


def test_collate_makes_one_trailing_dict(splits):
    prm = _prm(splits, spec=True, prob=0.5)
    random.seed(8)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    items = [ds[i] for i in range(4)]
    pcm, combs, target, spec, mix = audio_collate_fn(items)
    assert spec.dtype == torch.int32 and tuple(spec.shape) == (4, 2, 4)
    assert sorted(mix) == ["gains", "mate_combs", "mate_pcm", "mixed"]
    assert mix["mate_pcm"].dtype == torch.int16 and tuple(mix["mate_pcm"].shape) == tuple(pcm.shape)
    assert mix["gains"].dtype == torch.float32 and mix["mixed"].dtype == torch.bool and len(mix["mate_combs"]) == 4
    for b, item in enumerate(items):
        m = item[-1]
        assert bool(mix["mixed"][b]) == (m["mate_pcm"] is not None)
        if m["mate_pcm"] is None:
            assert not bool(mix["mate_pcm"][b].any())
        else:
            assert np.array_equal(mix["mate_pcm"][b].numpy(), m["mate_pcm"])
            assert mix["gains"][b].item() == np.float32(m["gain"]) and mix["mate_combs"][b] == m["mate_comb"]


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "adyolo_hip.h")).read()
    names = ("adyolo_corpus_gather", "adyolo_corpus_yolo_labels", "adyolo_corpus_yolo_labels_workspace_words",
             "adyolo_corpus_classwise_labels", "adyolo_audio_mix")
    for name in names:
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    lib = _lib.load()
    for name in names:
        assert getattr(lib, name) is not None
    assert lib.adyolo_corpus_yolo_labels_workspace_words(3, 5, 1) == 30
    assert lib.adyolo_corpus_yolo_labels_workspace_words(3, 0, 1) == 6
    assert lib.adyolo_corpus_yolo_labels_workspace_words(0, 5, 1) < 0
    assert lib.adyolo_corpus_yolo_labels_workspace_words(3, 5, 0) == 15
    assert lib.adyolo_corpus_yolo_labels_workspace_words(3, 0, 0) == 3
