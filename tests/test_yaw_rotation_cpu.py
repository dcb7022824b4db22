"""CPU: the host half of the FOA yaw-rotation augmentation (``aug_config.yaw_rotation_augment`` / ``yaw_step_deg``).  The refusals
of the keys; the key-off surface, which must be today's (draws, item tables, tuples of ``FoaDataset`` and both device corpora);
the draws of the three training paths from one seed with the key on; ``yaw_labels`` (its wraps, its composition with the 16
combinations); ``yaw_cos_sin`` at its exact angles; the NumPy definition of the audio yaw against the combinations it must
reproduce; and the table arithmetic of the class-wise label kernel, emulated in NumPy, against ``ClasswiseLabelEncoder`` for every
whole-degree direction."""
import csv
import os
import random

import numpy as np
import pytest
import torch

import adyolo_amd  # noqa: F401
from adyolo_amd import ops
from adyolo_amd.augmentations import (COMBINATIONS, draw_yaw, rotate_labels, yaw_audio_host, yaw_config, yaw_cos_sin,
                                      yaw_labels)
from adyolo_amd.corpus import ClasswiseDeviceCorpus, DeviceCorpus, load_chunked_split
from adyolo_amd.datasets import ClasswiseLabelEncoder, FoaDataset
from test_corpus_classwise_cpu import classwise_params, write_classwise_split
from test_corpus_cpu import chunk_instance

SR = 2400
RECS = (("fold1_room1_mix001", 6.0), ("fold1_room2_mix002", 3.7), ("fold2_room1_mix003", 2.0), ("take_chunk3_mix", 4.0))
#        5 + 3 + 1 + 3 = 12 chunks of 2 s (1 s stride)
WHOLE = ((180.0, 0.0), (-180.0, 12.0), (0.0, 90.0), (45.0, -90.0), (-0.0, 30.0), (120.0, -0.0), (0.0, 0.0), (-90.0, 90.0),
         (179.0, -89.0), (-1.0, -45.0), (90.0, 22.0), (-180.0, -90.0), (180.0, 90.0), (-135.0, 1.0), (67.0, -67.0))


def whole_degree_events(rs, n_frames, nb_classes, window_f, stride_f):
    """{frame: [[cls, src, az, el], ...]} with whole-degree angles only: frame f holds f % 5 events (0: none, unless the frame is
    the first or last of the recording or of one of its first two windows), about a third of them from ``WHOLE`` (the wraps,
    the poles, signed zeros), same-class events in one frame included."""
    forced = {0, n_frames - 1, window_f - 1, stride_f, stride_f + window_f - 1}
    label = {}
    for f in range(n_frames):
        k = f % 5 or (1 if f in forced else 0)
        evs = []
        for s in range(k):
            az, el = WHOLE[rs.randint(len(WHOLE))] if rs.rand() < 0.35 else (float(rs.randint(-180, 181)), float(rs.randint(-90, 91)))
            cls = int(rs.randint(nb_classes)) if s != 1 else evs[0][0]
            evs.append([cls, s, az, el])
        if evs:
            label[f] = evs
    return label


def write_whole_degree_split(root, recordings=RECS, sr=SR, window_s=2, stride_s=1, hop_s=0.1, seed=0, nb_classes=12):
    """A chunked FOA training split under root (the layout of ``write_classwise_split``) whose labels are whole degrees."""
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    sub = "dev-train-chunked_{}s_{}s".format(window_s, stride_s)
    wdir, cdir = os.path.join(root, "foa_dev", sub), os.path.join(root, "metadata_dev", sub)
    os.makedirs(wdir, exist_ok=True)
    os.makedirs(cdir, exist_ok=True)
    for rec, secs in recordings:
        n = int(round(secs * sr))
        audio = rs.randint(-32768, 32768, size=(n, 4)).astype(np.int16)
        label = whole_degree_events(rs, int(n / int(sr * hop_s)), nb_classes, int(window_s / hop_s), int(stride_s / hop_s))
        for i, (a, sl) in enumerate(chunk_instance(audio, label, sr, window_s, stride_s, hop_s)[0]):
            name = "%s_chunk%03d" % (rec, i + 1)
            wavfile.write(os.path.join(wdir, name + ".wav"), sr, a)
            with open(os.path.join(cdir, name + ".csv"), "w", newline="") as fid:
                w = csv.writer(fid, delimiter=",", quoting=csv.QUOTE_NONE)
                for frame, events in sl.items():
                    for ev in events:
                        w.writerow([int(frame), int(ev[0]), int(ev[1]), ev[2], ev[3]])


def yaw_params(root, loss="adyolo", yaw=True, step=None, rotation=True, spec=True, mix=True, sr=SR, nb_classes=12, nb_iters=2):
    prm = classwise_params(root, loss, batch_size=4, nb_iters=nb_iters, spec=spec, rotation=rotation, window_s=2, stride_s=1,
                           sr=sr, nb_classes=nb_classes)
    if mix:
        prm["aug_config"].update({"time_mix_augment": True, "time_mix_prob": 0.6, "time_mix_gain_db": [-6.0, 3.0]})
    if yaw is not None:
        prm["aug_config"]["yaw_rotation_augment"] = yaw
    if step is not None:
        prm["aug_config"]["yaw_step_deg"] = step
    return prm


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    root = tmp_path_factory.mktemp("yaw_rotation")
    write_whole_degree_split(root, seed=3)
    return root


@pytest.fixture(scope="module")
def fractional_split(tmp_path_factory):
    root = tmp_path_factory.mktemp("yaw_rotation_fractional")
    write_classwise_split(root, recordings=RECS, sr=SR, window_s=2, stride_s=1, seed=5, nb_classes=12)
    return root


# ------------------------------------------------------------------------------------------------------------------ config
def test_the_key_is_refused_for_mic_audio(split):
    prm = yaw_params(split)
    prm["data_config"]["audio_format"] = "mic"
    for make in (lambda: yaw_config(prm), lambda: FoaDataset(prm, "train", rank=0, world=1)):
        with pytest.raises(ValueError, match="channel_swap_augment") as e:
            make()
        assert "yaw_rotation_augment" in str(e.value)
    prm["aug_config"]["yaw_rotation_augment"] = False
    assert yaw_config(prm) is None


@pytest.mark.parametrize("step", [7, 0, -1, 1.5, 2.0, "1", True, 361, 720])
def test_a_bad_step_is_refused_by_name(split, step):
    prm = yaw_params(split, step=step)
    hc = load_chunked_split(yaw_params(split, yaw=None))
    with pytest.raises(ValueError, match="yaw_step_deg"):
        yaw_config(prm)
    with pytest.raises(ValueError, match="yaw_step_deg"):
        FoaDataset(prm, "train", rank=0, world=1)
    with pytest.raises(ValueError, match="yaw_step_deg"):
        DeviceCorpus(hc, prm, "cpu", rank=0, world=1)
    with pytest.raises(ValueError, match="yaw_step_deg"):
        ClasswiseDeviceCorpus(hc, yaw_params(split, "adpit", step=step), "cpu", rank=0, world=1)
    prm["aug_config"]["yaw_rotation_augment"] = False             # the step is read only with the augmentation on
    assert yaw_config(prm) is None


def test_defaults_steps_and_the_range_of_the_draw(split):
    assert yaw_config({}) is None and yaw_config(yaw_params(split, yaw=None)) is None
    assert yaw_config(yaw_params(split)) == 1
    for step in (1, 2, 3, 45, 90, 120, 180, 360):
        assert yaw_config(yaw_params(split, step=step)) == step
        rnd = random.Random(step)
        seen = {draw_yaw(rnd, step) for _ in range(4000)}
        assert seen <= set(range(-180, 180, step)), step
        if step >= 45:
            assert seen == set(range(-180, 180, step)), step

    class Top:                                                    # the largest value random() can return: still inside
        @staticmethod
        def random():
            return 1.0 - 2.0 ** -53
    assert draw_yaw(Top, 1) == 179 and draw_yaw(Top, 90) == 90 and draw_yaw(Top, 360) == -180


def test_validation_and_test_splits_are_never_yawed(split):
    prm = yaw_params(split)
    assert FoaDataset(prm, "train", rank=0, world=1).yaw == 1
    assert FoaDataset(prm, "train", is_valid=True, rank=0, world=1).yaw is None


def test_a_fractional_split_is_refused_by_the_classwise_corpus_only(fractional_split):
    hc = load_chunked_split(yaw_params(fractional_split, yaw=None))
    ang = hc.events[:, 3:5]
    assert (ang != np.round(ang)).any()
    with pytest.raises(ValueError, match="yaw_rotation_augment") as e:
        ClasswiseDeviceCorpus(hc, yaw_params(fractional_split, "adpit"), "cpu", rank=0, world=1)
    first = int(np.flatnonzero((ang != np.round(ang)).any(1))[0])
    rec = hc.rec_names[int(np.searchsorted(hc.ev_start, first, "right")) - 1]
    assert rec in str(e.value) and "whole-degree" in str(e.value)
    ClasswiseDeviceCorpus(hc, yaw_params(fractional_split, "adpit", yaw=False), "cpu", rank=0, world=1)   # off: any angles
    assert DeviceCorpus(hc, yaw_params(fractional_split), "cpu", rank=0, world=1).yaw == 1               # AD-YOLO: any angles
    assert FoaDataset(yaw_params(fractional_split, "adpit"), "train", rank=0, world=1).yaw == 1


# ----------------------------------------------------------------------------------------------------- the key-off surface
def _host_items(prm, seed, epochs=2):
    random.seed(seed)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    out = []
    for ep in range(epochs):
        if ep:
            ds.sample_filelist_for_train_iter()
        out += [(name, ds[i]) for i, name in enumerate(ds.get_filelist())]
    return out, random.getstate()


def _corpus_draws(cls, hc, prm, seed, epochs=2):
    random.seed(seed)
    corpus = cls(hc, prm, "cpu", rank=0, world=1)
    out = []
    for ep in range(epochs):
        if ep:
            corpus.sample_filelist_for_train_iter()
        files = corpus.get_filelist()
        for b0 in range(0, len(files), 4):
            out.append((files[b0:b0 + 4], corpus.draw(range(b0, min(len(files), b0 + 4)))))
    return corpus, out, random.getstate()


def _same(a, b):
    """Structural equality of items / draws: tuples, lists, dicts, arrays and tensors compared by type, shape and value."""
    if type(a) is not type(b):
        return False
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return a == b


@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mix"])
def test_key_off_is_key_absent(split, mix):
    hc = load_chunked_split(yaw_params(split, yaw=None))
    for loss, cls in (("adyolo", DeviceCorpus), ("adpit", ClasswiseDeviceCorpus)):
        absent, off = yaw_params(split, loss, yaw=None, mix=mix), yaw_params(split, loss, yaw=False, mix=mix)
        off["aug_config"]["yaw_step_deg"] = 7                    # not read with the key off
        ia, sa = _host_items(absent, 91)
        io, so = _host_items(off, 91)
        assert sa == so and _same(ia, io)
        assert all(isinstance(item[1], int) and len(item) == (5 if mix else 4) for _, item in io)
        assert not mix or all(set(item[-1]) == {"mate_pcm", "mate_comb", "gain"} for _, item in io)
        ca, da, sa = _corpus_draws(cls, hc, absent, 91)
        co, do, so = _corpus_draws(cls, hc, off, 91)
        assert sa == so and _same(da, do)
        assert all(len(d) == (3 if mix else 2) and not d[0][:, 6:].any() for _, d in do)      # words 6 and 7 of an item stay 0
        assert not mix or all(not d[2][:, 7].any() for _, d in do)
        assert co.yaw is None and co.yaw_tab is None and ca.yaw is None
        assert co.nbytes() == ca.nbytes()
        if cls is ClasswiseDeviceCorpus:
            assert co.yaw_xyz is None and tuple(co.xyz.shape) == (hc.events.shape[0], 17, 3)
    from adyolo_amd.datasets import audio_collate_fn
    batch = audio_collate_fn([item for _, item in io[:4]])
    assert len(batch) == (5 if mix else 4) and batch[1] == [item[1] for _, item in io[:4]]
    assert not mix or set(batch[-1]) == {"mate_pcm", "mate_combs", "gains", "mixed"}


# ------------------------------------------------------------------------------------------------- the draws with the key on
@pytest.mark.parametrize("rotation,mix,step", [(True, True, 1), (True, False, 1), (False, True, 45), (False, False, 3)],
                         ids=["rot_mix", "rot", "mix_step45", "alone_step3"])
def test_three_paths_draw_the_same_from_one_seed(split, rotation, mix, step):
    hc = load_chunked_split(yaw_params(split, yaw=None))

    def prm(loss):
        return yaw_params(split, loss, step=step, rotation=rotation, mix=mix)
    host, state = _host_items(prm("adyolo"), 57)
    host_cw, state_cw = _host_items(prm("adpit"), 57)
    assert state == state_cw
    flat = {}
    for loss, cls in (("adyolo", DeviceCorpus), ("adpit", ClasswiseDeviceCorpus)):
        corpus, draws, st = _corpus_draws(cls, hc, prm(loss), 57)
        assert st == state and corpus.yaw == step
        rows = []
        for files, drawn in draws:
            assert len(drawn) == (3 if mix else 2)
            for j, name in enumerate(files):
                rows.append((name, drawn[0][j], drawn[1][j], drawn[2][j] if mix else None))
        flat[loss] = rows
    assert _same(flat["adyolo"], flat["adpit"])
    yaws, mate_yaws, n_mixed = set(), set(), 0
    for items in (host, host_cw):
        assert len(items) == len(flat["adyolo"]) == 16
        for (name, item), (cname, it, spec, mate) in zip(items, flat["adyolo"]):
            assert name == cname
            comb, phi = item[1]
            assert isinstance(item[1], tuple) and (comb, phi) == (max(int(it[4]), 0), int(it[7]))
            assert (int(it[4]) == -1) == (not rotation) and phi in range(-180, 180, step)
            assert np.array_equal(item[3].numpy(), spec)
            yaws.add(phi)
            if not mix:
                assert len(item) == 4
                continue
            m = item[4]
            assert set(m) == {"mate_pcm", "mate_comb", "gain", "mate_yaw"}
            if m["mate_pcm"] is None:
                assert int(mate[0]) == -1 and m["mate_yaw"] == 0 and not mate[7]
                continue
            n_mixed += 1
            assert np.array_equal(m["mate_pcm"], hc.audio[int(mate[0]):int(mate[0]) + hc.window])
            assert (m["mate_comb"], m["mate_yaw"]) == (max(int(mate[4]), 0), int(mate[7]))
            assert np.float32(m["gain"]).view(np.uint32) == np.uint32(int(mate[6]))
            mate_yaws.add(m["mate_yaw"])
    assert len(yaws) >= 3 and (not mix or (n_mixed >= 8 and len(mate_yaws) >= 2))         # 16 items over at least 8 yaws
    # the collated batch carries the pairs and the mates' yaws
    from adyolo_amd.datasets import audio_collate_fn
    batch = audio_collate_fn([item for _, item in host[:4]])
    assert batch[1] == [item[1] for _, item in host[:4]] and len(batch) == (5 if mix else 4)
    assert not mix or batch[-1]["mate_yaws"] == [item[4]["mate_yaw"] for _, item in host[:4]]
    # the yaw moved the host labels: the same seed without the key gives other rows for a yawed item
    if not mix:
        plain, _ = _host_items(yaw_params(split, "adyolo", yaw=False, rotation=rotation, mix=False), 57)
        assert any(a[1][2] != b[1][2] for a, b in zip(host, plain))


# -------------------------------------------------------------------------------------------------------------- yaw_labels
def test_yaw_labels_wraps_once_and_leaves_the_rest():
    label = {3: [[1, 0, -1.0, 20.0], [2, 1, 1.0, -30.0]], 9: [[0, 0, 180.0, 90.0], [5, 2, -180.0, -90.0], [4, 0, 0.0, -0.0]]}
    keep = {f: [list(e) for e in evs] for f, evs in label.items()}
    got = yaw_labels(label, -180)
    assert label == keep and list(got) == [3, 9]                                       # a copy, the frames in order
    assert [e[2] for e in got[3]] == [179.0, -179.0]                                   # -181 -> 179, and -179 stays
    assert [e[2] for e in yaw_labels(label, 180)[3]] == [179.0, -179.0]               # 179 stays, 181 -> -179
    assert [e[2] for e in got[9]] == [0.0, 0.0, -180.0]                                # 180 - 180, -360 -> 0, exactly -180
    assert [e[2] for e in yaw_labels(label, 0)[9]] == [180.0, -180.0, 0.0]            # exactly +-180 are kept as they are
    assert [e[2] for e in yaw_labels({0: [[0, 0, 1.0, 0.0]]}, 179)[0]] == [180.0]     # exactly 180 is not wrapped
    assert [e[2] for e in yaw_labels({0: [[0, 0, 0.0, 0.0]]}, -180)[0]] == [-180.0]
    for f in label:                                                                   # class, source and elevation untouched
        assert [e[:2] + e[3:] for e in got[f]] == [e[:2] + e[3:] for e in label[f]]
    assert np.signbit(got[9][2][3])
    assert yaw_labels({}, 10) == {}
    assert [e[2] for e in yaw_labels({0: [[0, 0, 10.25, 0.0]]}, -37)[0]] == [-26.75]  # any angles


def test_yaw_labels_after_each_of_the_16_combinations():
    azs = [-180.0, -179.0, -91.0, -90.0, -1.0, 0.0, 1.0, 37.0, 89.0, 90.0, 135.0, 179.0, 180.0]
    label = {0: [[0, 0, az, 25.0] for az in azs]}
    for k, (_, _, pw, dpi, tw) in enumerate(COMBINATIONS):
        for phi in (-180, -179, -90, -37, -1, 0, 1, 37, 90, 179):
            got = yaw_labels(rotate_labels(label, k), phi)[0]
            for az, ev in zip(azs, got):
                want = pw * az + dpi + phi                                             # the moved azimuth, anywhere on the circle
                assert -180.0 <= ev[2] <= 180.0 and (ev[2] - want) % 360.0 == 0.0, (k, phi, az, ev[2])
                assert ev[3] == 25.0 * tw
            # and, evaluated on the unit circle, it is the combination's direction turned by phi about the vertical axis
            before = rotate_labels(label, k)[0]
            for b, a in zip(before, got):
                turned = np.exp(1j * np.radians(b[2])) * np.exp(1j * np.radians(phi))
                assert abs(np.exp(1j * np.radians(a[2])) - turned) < 1e-12


# ------------------------------------------------------------------------------------------------------- yaw_cos_sin, audio
def test_yaw_cos_sin_is_exact_at_the_quarter_turns():
    want = {0: (1, 0), 90: (0, 1), 180: (-1, 0), -180: (-1, 0), -90: (0, -1), 270: (0, -1), 360: (1, 0), -270: (0, 1)}
    for phi, (c, s) in want.items():
        got = yaw_cos_sin(phi)
        assert all(type(v) is np.float32 for v in got)
        assert (float(got[0]), float(got[1])) == (float(c), float(s)) and not np.signbit(got[0] if c == 0 else got[1]), phi
    import math
    for phi in (1, -1, 37, -179, 45, 89, 91, 0.5):
        c, s = yaw_cos_sin(phi)
        assert type(c) is np.float32 and type(s) is np.float32
        assert c == np.float32(math.cos(math.radians(phi))) and s == np.float32(math.sin(math.radians(phi)))


def test_the_audio_definition_reproduces_four_combinations_bit_for_bit():
    rs = np.random.RandomState(4)
    pcm = rs.randint(-32768, 32768, size=(257, 4)).astype(np.int16)
    pcm[:4] = [[0, 0, 0, 0], [-32768, 32767, -1, 1], [1, -1, 0, 32767], [5, 0, -7, 0]]
    a = (pcm.astype(np.float32) / np.float32(32768.0) + np.float32(1e-8)).astype(np.float32)

    def comb(x, k):
        (sy, sz, sx), swap = COMBINATIONS[k][:2]
        y, z, xx = x[:, 1] * np.float32(sy), x[:, 2] * np.float32(sz), x[:, 3] * np.float32(sx)
        return np.stack([x[:, 0], xx, z, y] if swap else [x[:, 0], y, z, xx], 1).astype(np.float32)
    for phi, k in ((0, 0), (180, 4), (-180, 4), (90, 8), (-90, 12)):
        assert yaw_audio_host(a, phi).tobytes() == comb(a, k).tobytes(), (phi, k)
    for k in range(16):                                           # a yaw of 0 after any combination changes no bit
        assert yaw_audio_host(comb(a, k), 0).tobytes() == comb(a, k).tobytes()
    got = yaw_audio_host(a, 37)                                   # W and Z are never touched; the rotation is a rotation
    assert got[:, 0].tobytes() == a[:, 0].tobytes() and got[:, 2].tobytes() == a[:, 2].tobytes()
    c, s = np.cos(np.radians(37.0)), np.sin(np.radians(37.0))
    y, x = a[:, 1].astype(np.float64), a[:, 3].astype(np.float64)
    assert np.abs(got[:, 1] - (y * c + x * s)).max() < 3e-7 and np.abs(got[:, 3] - (x * c - y * s)).max() < 3e-7
    assert got.dtype == np.float32 and a.tobytes() != got.tobytes()


# -------------------------------------------------------------------------------- the class-wise kernel's table arithmetic
def test_table_arithmetic_is_the_encoders_float32_for_every_whole_degree_direction():
    """x = (float)(cos_az * cos_el), y = (float)(sin_az * cos_el) from ``ops.corpus_yaw_xyz_tables`` against ``ClasswiseLabelEncoder``
    for all 361 x 181 directions, as int32 bit patterns; z (read from the xyz slot on the device) is ``xyz_table``'s."""
    from adyolo_amd.corpus import xyz_table
    az, el = ops.corpus_yaw_xyz_tables("cpu")
    assert az.dtype == torch.float64 and tuple(az.shape) == (361, 2) and el.dtype == torch.float64 and tuple(el.shape) == (181,)
    az, el = az.numpy(), el.numpy()
    x = (az[:, 0][:, None] * el[None, :]).astype(np.float32)      # one float64 product, rounded once
    y = (az[:, 1][:, None] * el[None, :]).astype(np.float32)
    enc = ClasswiseLabelEncoder(1)
    n = 361 * 181
    label = {i * 181 + j: [[0, 0, float(a), float(e)]] for i, a in enumerate(range(-180, 181)) for j, e in enumerate(range(-90, 91))}
    sed = enc.get_seddoa_label(label, n).view(torch.int32).numpy()                    # (n, 4): se, x, y, z
    assert np.array_equal(sed[:, 1].reshape(361, 181), x.view(np.int32))
    assert np.array_equal(sed[:, 2].reshape(361, 181), y.view(np.int32))
    adpit = enc.get_adpit_label(label, n)[:, 0, :, 0].view(torch.int32).numpy()
    assert np.array_equal(adpit[:, 1].reshape(361, 181), x.view(np.int32))
    assert np.array_equal(adpit[:, 2].reshape(361, 181), y.view(np.int32))
    acc = enc.get_accdoa_label(label, n).view(torch.int32).numpy()
    assert np.array_equal(acc[:, 0].reshape(361, 181), x.view(np.int32)) and np.array_equal(acc[:, 1].reshape(361, 181), y.view(np.int32))
    # the edges by name: the poles, az' = +-180, and an elevation of -0.0 (0 under an elevation flip): x, y as at +0.0, z = -0.0
    for a, e in ((0.0, 90.0), (45.0, -90.0), (180.0, 0.0), (-180.0, 0.0), (37.0, -0.0), (-180.0, -0.0)):
        one = enc.get_seddoa_label({0: [[0, 0, a, e]]}, 1)[0].view(torch.int32)
        ia, ie = int(a) + 180, int(e) + 90
        assert int(one[1]) == int(x[ia, ie].view(np.int32)) and int(one[2]) == int(y[ia, ie].view(np.int32)), (a, e)
        z = xyz_table([a], [e])[0, 0, 2]
        assert int(one[3]) == int(z.view(np.int32)) and (np.signbit(z) if np.signbit(e) and e == 0 else True)
    # every azimuth the label arithmetic can produce is a table entry: rotate_labels then yaw_labels never gives -0.0
    for k in range(16):
        for phi in (-180, -90, 0, 90):
            for a0 in (-0.0, 0.0, 180.0, -180.0, 90.0, -90.0):
                a1 = yaw_labels(rotate_labels({0: [[0, 0, a0, 0.0]]}, k), phi)[0][0][2]
                assert a1 == int(a1) and -180 <= a1 <= 180 and not (a1 == 0 and np.signbit(a1)), (k, phi, a0)
    assert not np.signbit(yaw_labels({0: [[0, 0, -0.0, 0.0]]}, 0)[0][0][2])
