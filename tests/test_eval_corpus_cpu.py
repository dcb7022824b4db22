"""CPU: the host half of evaluation from an HBM-resident split (ad-yolo_amd/corpus.py ``load_eval_split``, ``EvalDeviceCorpus``).
A synthetic labelled split in the reference's layout (``foa_dev/dev-test`` + ``metadata_dev/dev-test``) with clips of several
lengths, one clip with an empty CSV and one whose CSV has frames past its label frames: the loader must hold every clip's
audio bit for bit and every CSV's rows as ``FoaDataset`` reads them, list the files as ``FoaDataset`` lists them (one rank and
a shard), group them as ``test_epoch_audio`` does, and refuse what the host dataset could not evaluate, naming the file."""
import os
import re
import shutil

import numpy as np
import pytest

import adyolo_amd  # noqa: F401
from adyolo_amd import _lib
from adyolo_amd.corpus import EvalDeviceCorpus, load_chunked_split, load_eval_split
from adyolo_amd.datasets import FoaDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 24000
# name -> samples: 48000 + 77 and 48000 + 401 are cut to the whole hops of 48000, 72000 is a batch (and a graph) of its own
CLIPS = (("fold4_a", 48000), ("fold4_b", 48000 + 77), ("fold4_c", 48000), ("fold4_d", 72000), ("fold4_e", 48000 + 401),
         ("fold4_empty", 48000), ("fold4_past", 48000))
SPECIAL = ((180.0, 0.0), (-180.0, 12.5), (0.0, 90.0), (45.0, -90.0), (179.999, 89.9), (-0.25, -45.0), (90.0, 22.5))


def clip_events(rs, name, n_samples, nb_classes=12):
    """[(frame, class, source, azimuth, elevation)] of one clip, frames ascending: 0-3 events per label frame, the first and
    the last frame always labelled; 'empty' none; 'past' also rows in frames past ``n_samples // 2400``."""
    if name.endswith("empty"):
        return []
    frames = n_samples // 2400
    rows = []
    for f in range(frames):
        k = int(rs.choice(4, p=[0.4, 0.35, 0.15, 0.1]))
        if f in (0, frames - 1):
            k = max(k, 1)
        for s in range(k):
            az, el = SPECIAL[rs.randint(len(SPECIAL))] if rs.rand() < 0.3 else \
                (float(np.round(rs.uniform(-180, 180), 2)), float(np.round(rs.uniform(-90, 90), 2)))
            rows.append((f, int(rs.randint(nb_classes)), s, az, el))
    if name.endswith("past"):
        rows += [(frames, 3, 0, 10.0, 5.0), (frames + 7, 4, 0, -20.0, 15.0), (frames + 7, 5, 1, 120.0, -30.0)]
    return rows


def write_eval_split(root, set_type="test", clips=CLIPS, seed=3):
    """The split under root -> {name: (int16 audio, rows)}."""
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    wdir = os.path.join(root, "foa_dev", "dev-" + set_type)
    cdir = os.path.join(root, "metadata_dev", "dev-" + set_type)
    os.makedirs(wdir, exist_ok=True)
    os.makedirs(cdir, exist_ok=True)
    out = {}
    for name, n in clips:
        audio = rs.randint(-8000, 8000, size=(n, 4)).astype(np.int16)
        rows = clip_events(rs, name, n)
        wavfile.write(os.path.join(wdir, name + ".wav"), SR, audio)
        with open(os.path.join(cdir, name + ".csv"), "w") as fid:
            for r in rows:
                fid.write("%d,%d,%d,%r,%r\n" % r)
        out[name] = (audio, rows)
    return out


def eval_params(root, loss="adyolo", nb_classes=12, device="cpu"):
    return {"args": {"device": device, "encoder": "se-resnet34", "loss": loss},
            "data_config": {"nb_classes": nb_classes, "data_pth": str(root), "chunk_window_s": 2, "chunk_stride_s": 1, "sr": SR,
                            "label_hop_len_s": 0.1},
            "train_config": {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
                             "conf_thresh": 0.3, "clss_thresh": 0.3, "unify_thresh": 15.0, "nms": "conn-merge",
                             "loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
                             "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0, "batch_size": 4, "nb_iters": 1},
            "aug_config": {"rotation_augment": True, "spec_augment": True, "spec_augment_thresh": 0.6,
                           "spec_augment_time_mask_param": 20, "spec_augment_freq_mask_param": 16}}


def audio_batches(dataset, batch_size):
    """The batches ``test_epoch_audio`` forms, restated from its loop: lists of item indices."""
    out, i = [], 0
    while i < len(dataset):
        idx, t0 = [], None
        for j in range(i, min(i + max(1, int(batch_size)), len(dataset))):
            t = (dataset[j][0].shape[0] // 600) * 600
            if idx and t != t0:
                break
            idx.append(j)
            t0 = t
        out.append(idx)
        i += len(idx)
    return out


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    root = tmp_path_factory.mktemp("eval_split")
    return root, write_eval_split(root)


def test_loader_holds_what_the_host_dataset_reads(split):
    root, written = split
    prm = eval_params(root)
    ds = FoaDataset(prm, "test", is_valid=True, rank=0, world=1)
    hc = load_eval_split(prm, "test", rank=0, world=1, verify="all")
    assert hc.filelist == ds.get_filelist() == [n.replace(".wav", "") for n in os.listdir(hc.wav_pth)]
    assert hc.rec_names == hc.filelist and len(hc.filelist) == len(CLIPS)
    assert hc.audio.dtype == np.int16 and hc.hop_label == 2400 and hc.window == 72000
    assert hc.rec_start[-1] <= hc.audio.shape[0]
    most = 0
    for i, name in enumerate(hc.filelist):
        pcm = ds[i][0]
        s0, n = int(hc.rec_start[i]), int(hc.lengths[i])
        assert s0 % 16 == 0 and n == pcm.shape[0] == dict(CLIPS)[name]
        assert np.array_equal(hc.audio[s0:s0 + n], pcm) and np.array_equal(pcm, written[name][0])
        assert s0 + n <= int(hc.rec_start[i + 1])
        assert not hc.audio[s0 + n:int(hc.rec_start[i + 1])].any()              # the padding up to the next boundary is silence
        label = FoaDataset.load_csv2dict(os.path.join(hc.csv_pth, name + ".csv"))
        want = [(float(f), float(e[0]), float(e[1]), float(e[2]), float(e[3])) for f, evs in label.items() for e in evs]
        lo, hi = int(hc.ev_start[i]), int(hc.ev_start[i + 1])
        assert [tuple(r) for r in hc.events[lo:hi].tolist()] == want
        assert len(want) == len(written[name][1])
        most = max(most, hi - lo)
    assert hc.max_events == most and hc.events.shape == (int(hc.ev_start[-1]), 5)
    e, p = hc.filelist.index("fold4_empty"), hc.filelist.index("fold4_past")
    assert hc.ev_start[e] == hc.ev_start[e + 1]
    assert hc.events[hc.ev_start[p]:hc.ev_start[p + 1], 0].max() == 48000 // 2400 + 7       # rows past the label frames are kept


def test_filelist_of_a_rank_is_the_datasets_shard(split):
    root, _ = split
    prm = eval_params(root)
    ds = FoaDataset(prm, "test", is_valid=True, rank=1, world=2)
    hc = load_eval_split(prm, "test", rank=1, world=2)
    assert hc.filelist == ds.get_filelist() == sorted(n for n, _ in CLIPS)[1::2]
    assert len(hc.lengths) == len(hc.filelist) == 3                            # only this rank's recordings are loaded
    for i in range(len(hc.filelist)):
        s0 = int(hc.rec_start[i])
        assert np.array_equal(hc.audio[s0:s0 + int(hc.lengths[i])], ds[i][0])


@pytest.mark.parametrize("loss", ["adyolo", "adpit"])
def test_batches_are_those_of_test_epoch_audio(split, loss):
    root, _ = split
    prm = eval_params(root, loss=loss, nb_classes=13 if loss == "adpit" else 12)
    ds = FoaDataset(prm, "test", is_valid=True, rank=0, world=1)
    corpus = EvalDeviceCorpus(load_eval_split(prm, "test", rank=0, world=1, verify="none"), prm, device="cpu")
    assert corpus.get_filelist() == ds.get_filelist() and len(corpus) == len(ds)
    for bs in (4, 1, 8):
        got = [list(r) for r in corpus.batches(bs)]
        assert got == audio_batches(ds, bs), (bs, got)
    assert sum(len(r) for r in corpus.batches(4)) == len(CLIPS)
    assert corpus.nbytes() >= corpus.host.audio.nbytes
    with pytest.raises(ValueError, match="differ in length"):
        corpus.launch([corpus.get_filelist().index("fold4_a"), corpus.get_filelist().index("fold4_d")])


def test_unrotated_directions_are_slot_0_of_the_table(split):
    from adyolo_amd.corpus import xyz_table, xyz_unrotated
    root, _ = split
    hc = load_eval_split(eval_params(root), "test", rank=0, world=1, verify="none")
    az, el = np.concatenate([hc.events[:, 3], [0.0, -0.0, 180.0]]), np.concatenate([hc.events[:, 4], [-0.0, 0.0, 90.0]])
    got, want = xyz_unrotated(az, el), xyz_table(az, el)[:, 0]
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert xyz_unrotated([], []).shape == (0, 3)
    corpus = EvalDeviceCorpus(hc, eval_params(root, loss="accdoa", nb_classes=13), device="cpu")
    assert np.array_equal(corpus.xyz[:, 0].numpy().view(np.int32), xyz_table(hc.events[:, 3], hc.events[:, 4])[:, 0].view(np.int32))


def _small(root, mutate):
    """A two-clip split under root with one file changed by ``mutate(wav_dir, csv_dir)``."""
    write_eval_split(root, clips=(("good", 4800), ("bad", 4800)), seed=5)
    mutate(os.path.join(root, "foa_dev", "dev-test"), os.path.join(root, "metadata_dev", "dev-test"))
    return eval_params(root)


def test_refusals_name_the_file(tmp_path):
    from scipy.io import wavfile

    def float_wav(w, c):
        wavfile.write(os.path.join(w, "bad.wav"), SR, np.zeros((4800, 4), dtype=np.float32))

    def two_channels(w, c):
        wavfile.write(os.path.join(w, "bad.wav"), SR, np.zeros((4800, 2), dtype=np.int16))

    def no_csv(w, c):
        os.remove(os.path.join(c, "bad.csv"))

    def bad_class(w, c):
        with open(os.path.join(c, "bad.csv"), "a") as fid:
            fid.write("1,12,0,10.0,5.0\n")

    def cartesian_row(w, c):
        with open(os.path.join(c, "bad.csv"), "a") as fid:
            fid.write("1,2,0,0.5,0.5,0.7\n")

    for k, (mutate, what) in enumerate(((float_wav, "bad.wav"), (two_channels, "bad.wav"), (no_csv, "bad.csv"),
                                        (bad_class, "bad.csv"), (cartesian_row, "bad.csv"))):
        prm = _small(str(tmp_path / ("case%d" % k)), mutate)
        with pytest.raises(ValueError, match=re.escape(what)):
            load_eval_split(prm, "test", rank=0, world=1)
    prm = _small(str(tmp_path / "fine"), lambda w, c: None)
    assert len(load_eval_split(prm, "test", rank=0, world=1).filelist) == 2
    with pytest.raises(ValueError, match="train"):
        load_eval_split(prm, "train")
    with pytest.raises(ValueError, match="infer"):
        load_eval_split(prm, "infer")
    with pytest.raises(ValueError, match="dev-valid"):
        load_eval_split(prm, "valid")                                          # no such directory here
    with pytest.raises(ValueError, match="verify"):
        load_eval_split(prm, "test", verify="some")
    with pytest.raises(ValueError):                                            # the training loader still refuses the other splits
        load_chunked_split(prm, "test")
    shutil.rmtree(str(tmp_path / "fine"))


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "adyolo_hip.h")).read()
    for name in ("adyolo_loss_per_clip", "adyolo_loss_per_clip_workspace_words", "adyolo_loss_accumulate"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    lib = _lib.load()
    na = 20 * 32 * 5
    assert lib.adyolo_loss_per_clip_workspace_words(8, 20, 32, 5) >= 8 * 4 * na
    assert lib.adyolo_loss_per_clip_workspace_words(0, 20, 32, 5) < 0
