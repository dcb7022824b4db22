"""CPU: the MIC channel-swap augmentation's host half (ad-yolo_amd/augmentations.py ``MIC_SWAP_COMBS`` / ``mic_swap_source`` /
``swap_audio``, ``aug_config.channel_swap_augment`` in ``FoaDataset`` and the device corpora).  No published implementation is at
hand, so the geometry is the pin: a combination is in the set exactly when ``rotate_labels`` maps the four capsules of the array
onto capsules, the channel permutation is the inverse of that map, and with it every capsule hears a moved source as the capsule
it took the place of heard the original one (unit vectors by ``datasets._polar_to_xyz``); the other eight combinations admit no
permutation at all.  Then the draws: ``FoaDataset`` draws one of the eight where it draws the rotation, the corpora draw what it
draws, validation splits draw nothing, and the key is refused outside MIC-format audio or next to ``rotation_augment``."""
import itertools
import os
import random

import numpy as np
import pytest
import torch

import adyolo_amd  # noqa: F401
from adyolo_amd import augmentations as aug
from adyolo_amd.corpus import ClasswiseDeviceCorpus, DeviceCorpus, load_chunked_split
from adyolo_amd.datasets import CLASSWISE_LABELS, FoaDataset, _polar_to_xyz
from test_corpus_classwise_cpu import classwise_params, write_classwise_split
from test_corpus_cpu import _branch, _corpus_epoch, _host_epoch

SR = 2400
RECS = (("fold1_room1_mix001", 6.0), ("fold1_room2_mix002", 3.7), ("fold2_room1_mix003", 2.0), ("take_chunk3_mix", 4.0))
#        5 + 3 + 1 + 3 = 12 chunks of 2 s (1 s stride)
TABLE = {0: (0, 1, 2, 3), 3: (1, 0, 3, 2), 4: (3, 2, 1, 0), 7: (2, 3, 0, 1), 9: (1, 3, 0, 2), 10: (0, 2, 1, 3), 13: (2, 0, 3, 1),
         14: (3, 1, 2, 0)}


def _moved(directions, k):
    """``rotate_labels`` with combination k on (az, el) pairs -> the moved pairs."""
    return [tuple(ev[2:]) for ev in aug.rotate_labels({0: [[0, 0, a, e] for a, e in directions]}, k)[0]]


def _unit(directions):
    return np.asarray([_polar_to_xyz(float(a), float(e)) for a, e in directions], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------- geometry
def test_the_set_is_the_combinations_that_map_capsules_onto_capsules():
    assert aug.MIC_DIRECTIONS == ((45, 35), (-45, -35), (135, -35), (-135, 35))
    assert aug.MIC_SWAP_COMBS == (0, 3, 4, 7, 9, 10, 13, 14) == tuple(sorted(TABLE))
    caps = list(aug.MIC_DIRECTIONS)
    for k in range(16):
        images = _moved(caps, k)
        onto = all(d in caps for d in images)
        assert onto == (k in aug.MIC_SWAP_COMBS), (k, images)
        if not onto:
            with pytest.raises(ValueError, match="symmetry"):
                aug.mic_swap_source(k)
            continue
        pi = [caps.index(d) for d in images]                       # capsule i -> capsule pi[i]
        assert sorted(pi) == [0, 1, 2, 3]
        inv = tuple(pi.index(j) for j in range(4))                 # new[pi(i)] = old[i]  <=>  new[j] = old[pi^-1(j)]
        assert aug.mic_swap_source(k) == inv == TABLE[k], k


def test_the_eight_permutations_are_a_group():
    perms = {aug.mic_swap_source(k) for k in aug.MIC_SWAP_COMBS}
    assert len(perms) == 8 and (0, 1, 2, 3) in perms
    for a in perms:
        for b in perms:
            assert tuple(a[b[j]] for j in range(4)) in perms


# -------------------------------------------------------------------------------------------------------------- physics
def test_a_moved_source_is_heard_by_capsule_j_as_the_original_was_by_its_source_capsule():
    """<u(moved label), p_j> == <u(label), p_{s_j}> for every capsule j and 200 directions: what a capsule picks up from a far
    source depends on the angle between the two only, so the permuted channels are what the array records of the moved source.
    For a combination outside the set no permutation of the channels does that."""
    rs = np.random.RandomState(2022)
    directions = [(int(a), int(e)) for a, e in zip(rs.randint(-180, 181, 200), rs.randint(-90, 91, 200))]
    p = _unit(aug.MIC_DIRECTIONS)                                   # (4, 3)
    before = _unit(directions) @ p.T                               # (200, 4): cos of the angle to each capsule
    worst = 0.0
    for k in range(16):
        after = _unit(_moved(directions, k)) @ p.T
        if k in aug.MIC_SWAP_COMBS:
            err = float(np.abs(after - before[:, list(aug.mic_swap_source(k))]).max())
            worst = max(worst, err)
            assert err <= 1e-12, (k, err)
        else:
            for s in itertools.permutations(range(4)):
                assert float(np.abs(after - before[:, list(s)]).max()) > 1e-12, (k, s)
    print("largest deviation over the eight symmetries: %.3g" % worst)


# -------------------------------------------------------------------------------------------------------------- dataset
def _prm(root, loss, swap=True, rotation=False, spec=True, fmt="mic"):
    prm = classwise_params(root, loss, batch_size=4, nb_iters=3, spec=spec, rotation=rotation, window_s=2, stride_s=1, sr=SR)
    if fmt is not None:
        prm["data_config"]["audio_format"] = fmt
    if swap is not None:
        prm["aug_config"]["channel_swap_augment"] = swap
    return prm


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """A mic_dev training split, the same files under foa_dev (for the refusals) and a one-file validation split."""
    from scipy.io import wavfile
    root = tmp_path_factory.mktemp("mic_swap")
    write_classwise_split(root, recordings=RECS, sr=SR, window_s=2, stride_s=1, seed=21, audio_dir="mic_dev")
    sub = "dev-train-chunked_2s_1s"
    os.makedirs(os.path.join(root, "foa_dev"))
    os.symlink(os.path.join(root, "mic_dev", sub), os.path.join(root, "foa_dev", sub))
    for d in ("mic_dev", "metadata_dev"):
        os.makedirs(os.path.join(root, d, "dev-valid"))
    rs = np.random.RandomState(3)
    wavfile.write(os.path.join(root, "mic_dev", "dev-valid", "fold4_room1_mix001.wav"), SR,
                  rs.randint(-32768, 32768, size=(3 * SR, 4)).astype(np.int16))
    with open(os.path.join(root, "metadata_dev", "dev-valid", "fold4_room1_mix001.csv"), "w") as fid:
        fid.write("0,1,0,30.0,10.0\n4,2,0,-100.0,-20.0\n")
    return root


def _encoded(ds, name, comb):
    """What ``__getitem__`` must return as the target of ``name`` under combination ``comb``: the CSV's labels moved by
    ``rotate_labels`` and encoded by the dataset's own encoder."""
    label = aug.rotate_labels(FoaDataset.load_csv2dict(os.path.join(ds.csv_pth, name + ".csv")), comb)
    frames = 2 * SR // ds.hop_label
    if ds.loss_nm == "adyolo":
        return ds.encoder.get_yolo_label(label, frames)
    return getattr(ds.encoder, CLASSWISE_LABELS[ds.loss_nm])(label, frames)


@pytest.mark.parametrize("loss", ["adyolo", "adpit"])
def test_the_dataset_draws_a_symmetry_and_moves_the_labels_with_it(split, loss):
    seed = 5
    random.seed(seed)
    ds = FoaDataset(_prm(split, loss), "train", rank=0, world=1)
    assert ds.swap and not ds.rotate
    items = [ds[i] for i in range(len(ds))]
    state = random.getstate()
    random.seed(seed)
    rot = FoaDataset(_prm(split, loss, swap=False, rotation=True), "train", rank=0, world=1)
    assert rot.get_filelist() == ds.get_filelist() and not rot.swap
    rot_items = [rot[i] for i in range(len(rot))]
    assert random.getstate() == state                                # the same number of draws as the rotation
    combs = [it[1] for it in items]
    assert set(combs) <= set(aug.MIC_SWAP_COMBS) and len(set(combs) - {0}) >= 3, combs
    assert not set(it[1] for it in rot_items) <= set(aug.MIC_SWAP_COMBS)
    for name, it, rit in zip(ds.get_filelist(), items, rot_items):
        want = _encoded(ds, name, it[1])
        assert torch.equal(it[2], want) if isinstance(want, torch.Tensor) else it[2] == want, name
        assert torch.equal(it[3], rit[3]) and np.array_equal(it[0], rit[0])     # SpecAug tables, audio untouched on the host
    assert any(bool(it[3].any()) for it in items)
    moved = [n for n, it in zip(ds.get_filelist(), items) if it[1] != 0
             and not (torch.equal(it[2], _encoded(ds, n, 0)) if isinstance(it[2], torch.Tensor) else it[2] == _encoded(ds, n, 0))]
    assert moved                                                     # the labels did move


def test_key_absent_or_false_draws_nothing_new(split):
    for swap in (None, False):
        prm = _prm(split, "adpit", swap=swap, spec=False)
        random.seed(9)
        ds = FoaDataset(prm, "train", rank=0, world=1)
        state = random.getstate()
        assert not ds.swap and ds[0][1] == 0 and random.getstate() == state
        c = ClasswiseDeviceCorpus(load_chunked_split(prm), prm, "cpu", rank=0, world=1)
        assert not c.swap and c.mic_src is None and (c.draw(range(4))[0][:, 4] == -1).all()


def test_a_validation_split_draws_nothing(split):
    prm = _prm(split, "adpit")
    random.seed(11)
    ds = FoaDataset(prm, "valid", is_valid=True, rank=0, world=1)
    state = random.getstate()
    item = ds[0]
    assert not ds.swap and len(item) == 3 and item[1] == 0 and random.getstate() == state
    plain = FoaDataset(_prm(split, "adpit", swap=False), "valid", is_valid=True, rank=0, world=1)[0]
    assert torch.equal(item[2], plain[2]) and bool(item[2].any())
    assert not aug.ChannelSwapAug(prm, True).apply_augment and aug.ChannelSwapAug(prm, False).apply_augment
    label = {0: [[1, 0, 30.0, 10.0]]}
    assert aug.ChannelSwapAug(prm, True).augment(None, label) == (None, label)


# --------------------------------------------------------------------------------------------------------- corpus draws
@pytest.mark.parametrize("spec", [True, False], ids=["specaug", "swap_only"])
@pytest.mark.parametrize("loss", ["adyolo", "adpit"])
def test_three_epochs_draw_what_foadataset_draws(split, loss, spec):
    prm = _prm(split, loss, spec=spec)                                # 12 files, 12 per epoch
    prm["train_config"]["nb_iters"] = 2                               # 8 of 12 files per epoch: sample, wrap, ...
    hc = load_chunked_split(prm)
    make_corpus = DeviceCorpus if loss == "adyolo" else ClasswiseDeviceCorpus

    def run(make, epoch):
        random.seed(4321)
        ds = make()
        seq, branches = [epoch(ds)], []
        for _ in range(3):
            branches.append(_branch(ds))
            ds.sample_filelist_for_train_iter()
            seq.append(epoch(ds))
        return seq, branches, random.getstate()

    host, hb, hstate = run(lambda: FoaDataset(prm, "train", rank=0, world=1), _host_epoch)
    dev, db, dstate = run(lambda: make_corpus(hc, prm, "cpu", rank=0, world=1), lambda c: _corpus_epoch(c, 4))
    assert hb == db and "wrap" in hb
    assert host == dev and hstate == dstate
    combs = {c for ep in dev for _, c, _ in ep}
    assert combs <= set(aug.MIC_SWAP_COMBS) and len(combs) >= 6, sorted(combs)
    if spec:
        assert any(s != [[0, 0, 0, 0], [0, 0, 0, 0]] for ep in dev for _, _, s in ep)


def test_the_gather_table_of_a_corpus_is_the_symmetry_table(split):
    from adyolo_amd import ops
    prm = _prm(split, "adpit")
    c = ClasswiseDeviceCorpus(load_chunked_split(prm), prm, "cpu", rank=0, world=1)
    words = list(c.mic_src)
    assert len(words) == 16
    for k in range(16):
        if k in TABLE:
            assert tuple((words[k] >> (8 * j)) & 0xFF for j in range(4)) == TABLE[k]
        else:
            assert words[k] == ops.MIC_SWAP_NONE == 0xFFFFFFFF
    with pytest.raises(ValueError, match="permutation"):
        ops.corpus_mic_table({3: (1, 1, 3, 2)})
    with pytest.raises(ValueError, match="permutation"):
        ops.corpus_mic_table({16: (0, 1, 2, 3)})


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(split):
    hc_mic = load_chunked_split(_prm(split, "adpit"))
    for fmt in ("foa", None):                                         # FOA audio, named or by default
        for loss, corpus in (("adyolo", DeviceCorpus), ("adpit", ClasswiseDeviceCorpus)):
            prm = _prm(split, loss, fmt=fmt)
            with pytest.raises(ValueError, match="audio_format"):
                FoaDataset(prm, "train", rank=0, world=1)
            with pytest.raises(ValueError, match="audio_format"):
                FoaDataset(prm, "valid", is_valid=True, rank=0, world=1)
            with pytest.raises(ValueError, match="audio_format"):
                corpus(hc_mic, prm, "cpu", rank=0, world=1)
    for loss, corpus in (("adyolo", DeviceCorpus), ("adpit", ClasswiseDeviceCorpus)):
        prm = _prm(split, loss, rotation=True)
        with pytest.raises(ValueError, match="rotation_augment"):
            FoaDataset(prm, "train", rank=0, world=1)
        with pytest.raises(ValueError, match="rotation_augment"):
            corpus(hc_mic, prm, "cpu", rank=0, world=1)
        with pytest.raises(ValueError, match="rotation_augment"):
            aug.ChannelSwapAug(prm, False)
        # rotation_augment alone: today's behaviour, in MIC format too
        alone = _prm(split, loss, swap=False, rotation=True)
        assert FoaDataset(alone, "train", rank=0, world=1).rotate and corpus(hc_mic, alone, "cpu", rank=0, world=1).rotate
    audio = torch.zeros(1, 8, 4)                                      # never reaches a launch: the combination is checked first
    for comb in (1, 16, -1):
        with pytest.raises(ValueError, match="symmetry"):
            aug.swap_audio(audio, [comb])
    with pytest.raises(ValueError, match="symmetry"):
        aug.swap_audio(torch.zeros(2, 8, 4), [3, 2])
