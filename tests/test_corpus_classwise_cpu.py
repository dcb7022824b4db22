"""CPU: the host half of the class-wise HBM-resident corpus (ad-yolo_amd/corpus.py ``ClasswiseDeviceCorpus``, ``xyz_table``).
A chunked split is written here with ``chunk_instance`` from test_corpus_cpu.py, its events crafted for the class-wise encoders:
frames with 1, 2, 3 and 4 events of one class and with interleaved classes, events on the first and last frame of windows,
every class up to C - 1, azimuths of +-180, elevations of +-90 and angles of -0.0.  ``xyz_table`` must hold, for every event under
no rotation and each of the 16 FOA combinations, the float32 the host encoder writes, bit for bit; the corpus must draw what
``FoaDataset`` draws; ``target_shape`` and the refusals are checked without a GPU."""
import copy
import csv
import os
import random

import numpy as np
import pytest
import torch

import adyolo_amd  # noqa: F401
from adyolo_amd.corpus import ClasswiseDeviceCorpus, DeviceCorpus, load_chunked_split, xyz_table
from adyolo_amd.datasets import ClasswiseLabelEncoder, FoaDataset
from test_corpus_cpu import _branch, _corpus_epoch, _host_epoch, chunk_instance, params_for

C = 13
SR = 2400
RECORDINGS = (("fold1_room1_mix001", 30.0), ("fold2_room2_mix002", 23.3), ("fold3_room1_mix003", 20.0))   # 11 + 4 + 1 chunks
LOSSES = ("seddoa", "masked-seddoa", "accdoa", "adpit")
SPECIAL = ((180.0, 0.0), (-180.0, 12.5), (0.0, 90.0), (45.0, -90.0), (-0.0, 30.0), (120.0, -0.0), (-0.0, -0.0), (0.0, 0.0),
           (-90.0, 90.0), (179.999, -89.9), (-0.25, -45.0), (90.0, 22.5), (-180.0, -90.0), (180.0, 90.0))


def classwise_events(rs, n_frames, nb_classes=C, window_f=200, stride_f=10):
    """{frame: [[cls, src, az, el], ...]}: frame f holds pattern f % 6 -- none, one event, two / three / four events of one class,
    or 2-6 events drawn from three classes (interleaved); single events cycle through every class; the first and last frame of
    the recording and of the first two windows are never empty."""
    forced = {0, n_frames - 1, window_f - 1, stride_f, stride_f + window_f - 1}
    label, cycle = {}, [0]

    def angle():
        if rs.rand() < 0.4:
            return SPECIAL[rs.randint(len(SPECIAL))]
        return float(np.round(rs.uniform(-180, 180), 1)), float(np.round(rs.uniform(-90, 90), 1))

    for f in range(n_frames):
        kind = f % 6
        if kind == 0 and f in forced:
            kind = 1
        if kind == 0:
            continue
        if kind == 1:
            classes = [cycle[0] % nb_classes]
            cycle[0] += 1
        elif kind in (2, 3, 4):
            classes = [int(rs.randint(nb_classes))] * kind
        else:
            pool = rs.choice(nb_classes, 3, replace=False)
            classes = [int(c) for c in rs.choice(pool, rs.randint(2, 7))]
        label[f] = [[int(c), s] + list(angle()) for s, c in enumerate(classes)]
    return label


def write_classwise_split(root, recordings=RECORDINGS, sr=SR, window_s=20, stride_s=1, hop_s=0.1, seed=0, nb_classes=C,
                          audio_dir="foa_dev"):
    """The chunked training split of ``recordings`` under root (``audio_dir`` / metadata_dev, dev-train-chunked_<w>s_<s>s), cut by
    ``chunk_instance`` with ``classwise_events`` labels."""
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    sub = "dev-train-chunked_{}s_{}s".format(window_s, stride_s)
    wdir, cdir = os.path.join(root, audio_dir, sub), os.path.join(root, "metadata_dev", sub)
    os.makedirs(wdir, exist_ok=True)
    os.makedirs(cdir, exist_ok=True)
    for rec, secs in recordings:
        n = int(round(secs * sr))
        audio = rs.randint(-32768, 32768, size=(n, 4)).astype(np.int16)
        label = classwise_events(rs, int(n / int(sr * hop_s)), nb_classes, int(window_s / hop_s), int(stride_s / hop_s))
        chunks, _ = chunk_instance(audio, label, sr, window_s, stride_s, hop_s)
        for i, (a, sl) in enumerate(chunks):
            name = "%s_chunk%03d" % (rec, i + 1)
            wavfile.write(os.path.join(wdir, name + ".wav"), sr, a)
            with open(os.path.join(cdir, name + ".csv"), "w", newline="") as fid:
                w = csv.writer(fid, delimiter=",", quoting=csv.QUOTE_NONE)
                for frame, events in sl.items():
                    for ev in events:
                        w.writerow([int(frame), int(ev[0]), int(ev[1]), ev[2], ev[3]])


def classwise_params(root, loss, batch_size=4, nb_iters=3, spec=True, rotation=True, window_s=20, stride_s=1, sr=SR,
                     nb_classes=C):
    prm = params_for(root, batch_size=batch_size, nb_iters=nb_iters, rotation=rotation, spec=spec, window_s=window_s,
                     stride_s=stride_s, sr=sr)
    prm["args"]["loss"] = loss
    prm["data_config"]["nb_classes"] = nb_classes
    return prm


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    root = tmp_path_factory.mktemp("corpus_classwise")
    write_classwise_split(root)
    return root


def test_the_split_has_what_the_encoders_need(split):
    hc = load_chunked_split(classwise_params(split, "adpit"), verify="all")
    ev = hc.events
    assert set(ev[:, 1].astype(int)) == set(range(C))
    az, el = ev[:, 3], ev[:, 4]
    assert (az == 180).any() and (az == -180).any() and (el == 90).any() and (el == -90).any()
    assert ((az == 0) & np.signbit(az)).any() and ((el == 0) & np.signbit(el)).any()
    same = set()
    for r in range(len(hc.rec_names)):
        part = ev[hc.ev_start[r]:hc.ev_start[r + 1]]
        for f in np.unique(part[:, 0]):
            cls = part[part[:, 0] == f, 1].astype(int).tolist()
            same |= {cls.count(c) for c in cls}
    assert {1, 2, 3, 4} <= same


def test_xyz_table_is_the_host_encoders_float32(split):
    """Every event under the 17 transforms: the x, y, z ``get_seddoa_label`` and ``get_adpit_label`` write for it alone, compared
    as int32 bit patterns (signed zeros count)."""
    from adyolo_amd.augmentations import rotate_labels
    hc = load_chunked_split(classwise_params(split, "seddoa"))
    tab = xyz_table(hc.events[:, 3], hc.events[:, 4])
    assert tab.shape == (hc.events.shape[0], 17, 3) and tab.dtype == np.float32
    enc = ClasswiseLabelEncoder(C)
    bits = torch.from_numpy(tab).view(torch.int32)
    for e, (_, cls, src, az, el) in enumerate(hc.events.tolist()):
        cls = int(cls)
        for slot in range(17):
            label = {0: [[cls, int(src), az, el]]}
            if slot:
                label = rotate_labels(label, slot - 1)
            sed = enc.get_seddoa_label(label, 1)[0].view(torch.int32)
            want = torch.stack([sed[C + cls], sed[2 * C + cls], sed[3 * C + cls]])
            assert torch.equal(bits[e, slot], want), (e, slot, az, el)
            if slot in (0, 5, 16):
                adpit = enc.get_adpit_label(label, 1)[0, 0, 1:, cls].view(torch.int32)
                assert torch.equal(bits[e, slot], adpit), (e, slot)
    zero = (hc.events[:, 3] == 0) & np.signbit(hc.events[:, 3])
    assert zero.any() and (tab[zero, 0, 1] == 0).all() and np.signbit(tab[zero, 0, 1]).all()    # sin(-0.0) survives slot 0
    assert not np.signbit(tab[zero, 1, 1]).any()                   # combination 0 turns -0.0 into +0.0 (-0.0 * 1 + 0)


def test_xyz_table_edges():
    assert xyz_table([], []).shape == (0, 17, 3)
    a = xyz_table([-0.0, 0.0, -0.0], [10.0, 10.0, 10.0])
    assert np.signbit(a[0, 0, 1]) and not np.signbit(a[1, 0, 1]) and a[0].tobytes() == a[2].tobytes()


@pytest.mark.parametrize("spec", [True, False], ids=["specaug", "rotation_only"])
def test_three_epochs_draw_what_foadataset_draws(split, spec):
    prm = classwise_params(split, "adpit", batch_size=4, nb_iters=3, spec=spec)       # 12 of 16 files per epoch
    hc = load_chunked_split(prm)

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
    dev, db, dstate = run(lambda: ClasswiseDeviceCorpus(hc, prm, "cpu", rank=0, world=1), lambda c: _corpus_epoch(c, 4))
    assert hb == db and "wrap" in hb
    assert host == dev and hstate == dstate
    assert len({c for ep in dev for _, c, _ in ep}) > 8
    if spec:
        assert any(s != [[0, 0, 0, 0], [0, 0, 0, 0]] for ep in dev for _, _, s in ep)


def test_no_rotation_draws_comb_minus_one(split):
    prm = classwise_params(split, "accdoa", rotation=False, spec=False)
    random.seed(1)
    c = ClasswiseDeviceCorpus(load_chunked_split(prm), prm, "cpu", rank=0, world=1)
    items, spec = c.draw(range(4))
    assert spec is None and (items[:, 4] == -1).all()


def test_target_shapes_and_refusals(split):
    hc = load_chunked_split(classwise_params(split, "adpit"))
    t = hc.window_frames
    want = {"seddoa": (5, t, 4 * C), "masked-seddoa": (5, t, 4 * C), "accdoa": (5, t, 3 * C), "adpit": (5, t, 6, 4, C)}
    for loss in LOSSES:
        c = ClasswiseDeviceCorpus(hc, classwise_params(split, loss), "cpu", rank=0, world=1)
        assert c.target_shape(5) == want[loss]
        assert c.xyz.shape == (hc.events.shape[0], 17, 3) and c.nbytes() == hc.nbytes() - hc.events.nbytes + \
            hc.events.shape[0] * (4 * 8 + 17 * 3 * 4)
    for loss in ("adyolo", "masked-accdoa"):
        with pytest.raises(ValueError, match=loss):
            ClasswiseDeviceCorpus(hc, classwise_params(split, loss), "cpu")
    with pytest.raises(NotImplementedError, match="ClasswiseDeviceCorpus"):
        DeviceCorpus(hc, classwise_params(split, "accdoa"), "cpu")
    # a class the model does not have: the recording that holds the first such event is named
    with pytest.raises(ValueError, match="nb_classes"):
        ClasswiseDeviceCorpus(hc, classwise_params(split, "accdoa", nb_classes=C - 1), "cpu")
    bad = copy.copy(hc)
    bad.events = hc.events.copy()
    r = 1
    bad.events[int(hc.ev_start[r]) + 3, 1] = -1
    with pytest.raises(ValueError, match=hc.rec_names[r]):
        ClasswiseDeviceCorpus(bad, classwise_params(split, "seddoa"), "cpu")
    bad.events[int(hc.ev_start[r]) + 3, 1] = C
    with pytest.raises(ValueError, match=hc.rec_names[r]):
        ClasswiseDeviceCorpus(bad, classwise_params(split, "adpit"), "cpu")
