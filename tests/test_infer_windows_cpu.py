"""CPU: the host half of windowed inference (ad-yolo_amd/corpus.py ``window_plan``, ``load_infer_split``,
``infer_split_from_arrays``, ``split_pass_rows``): the window plan's invariants over every length 1..200, the split loaders on a
temporary folder of WAV files (lengths, alignment, the file list rule of ``FoaDataset('infer')``, the rank shards, ``files=``,
a float WAV refused by name) and the split of a pass's selected rows at the recording boundaries."""
import math
import os
import re

import numpy as np
import pytest

import adyolo_amd  # noqa: F401
from adyolo_amd import _lib
from adyolo_amd import corpus as C
from adyolo_amd.datasets import FoaDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 24000
PLANS = ((20, 4), (20, 0), (7, 3), (3, 1))


def infer_params(root, loss="adyolo", nb_classes=12, device="cpu"):
    return {"args": {"device": device, "encoder": "se-resnet34", "loss": loss, "infer_pth": str(root)},
            "data_config": {"nb_classes": nb_classes, "data_pth": str(root), "chunk_window_s": 2, "chunk_stride_s": 1, "sr": SR,
                            "label_hop_len_s": 0.1},
            "train_config": {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
                             "conf_thresh": 0.3, "clss_thresh": 0.3, "unify_thresh": 15.0, "nms": "conn-merge",
                             "loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
                             "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0, "batch_size": 4, "nb_iters": 1},
            "aug_config": {}}


# ------------------------------------------------------------------------------------------------------------- window_plan
@pytest.mark.parametrize("wf,mf", PLANS)
def test_window_plan_tiles_every_length_in_order_with_context(wf, mf):
    s = wf - 2 * mf
    for f in range(1, 201):
        plan = C.window_plan(f, wf, mf)
        # K is minimal: window 0 and the last one keep at most Wf - Mf frames, every other one at most S, so K windows cover at
        # most 2 (Wf - Mf) + (K - 2) S = Wf + (K - 1) S frames -- F needs K >= (F - Wf) / S + 1
        want_k = 1 if f <= wf else math.ceil((f - wf) / s) + 1
        assert len(plan) == want_k, (f, plan)
        if f > wf:
            assert wf + (want_k - 2) * s < f <= wf + (want_k - 1) * s
        pos = 0
        for k, (start, src_lo, dst_lo, n) in enumerate(plan):
            assert all(isinstance(v, int) for v in (start, src_lo, dst_lo, n))
            assert dst_lo == pos and n > 0, (f, plan)                       # exact tiling, in order
            assert start + src_lo == dst_lo                                 # window-local against the recording's axis
            assert start >= 0 and start + wf <= max(f, wf)                  # no window below 0 or past the recording
            assert 0 <= src_lo and src_lo + n <= min(wf, f)
            # context: Mf frames of its own window on each side, unless the recording's edge is nearer
            assert src_lo >= min(mf, dst_lo), (f, plan, k)
            assert min(wf, f) - (src_lo + n) >= min(mf, f - (dst_lo + n)), (f, plan, k)
            if f > wf:
                assert start == (k * s if k < len(plan) - 1 else f - wf)
                if 0 < k < len(plan) - 1:
                    assert (src_lo, n) == (mf, s)
            pos += n
        assert pos == f
        if f > wf:
            assert plan[0] == (0, 0, 0, wf - mf) and plan[-1][0] + wf == f   # tail-aligned: no padding in the last window


def test_window_plan_single_window_and_refusals():
    for wf, mf in PLANS:
        for f in range(1, wf + 1):
            assert C.window_plan(f, wf, mf) == [(0, 0, 0, f)]
        assert len(C.window_plan(wf + 1, wf, mf)) == 2
    assert C.window_plan(0, 20, 4) == [(0, 0, 0, 0)]
    assert C.window_plan(50, 20, 4) == [(0, 0, 0, 16), (12, 4, 16, 12), (24, 4, 28, 12), (30, 10, 40, 10)]
    for wf, mf in ((8, 4), (7, 4), (0, 0), (20, -1), (1, 1)):
        with pytest.raises(ValueError):
            C.window_plan(10, wf, mf)


# ----------------------------------------------------------------------------------------------------------- split loaders
LENGTHS = (("rec_c", 24000 + 77), ("rec_a", 48000), ("rec_d", 72000), ("rec_b", 48000 + 401), ("rec_e", 1000), ("rec_f", 168000))


def write_folder(root, lengths=LENGTHS, seed=11):
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    os.makedirs(str(root), exist_ok=True)
    out = {}
    for name, n in lengths:
        out[name] = rs.randint(-8000, 8000, size=(n, 4)).astype(np.int16)
        wavfile.write(os.path.join(str(root), name + ".wav"), SR, out[name])
    return out


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("infer_folder")
    return root, write_folder(root)


def _check_layout(hc, written, names):
    assert hc.rec_names == hc.filelist == hc.total_filelist == names
    assert hc.audio.dtype == np.int16 and hc.audio.shape[1] == 4 and hc.hop_label == 2400 and hc.set_type == "infer"
    assert hc.lengths.tolist() == [written[n].shape[0] for n in names]
    assert hc.events.shape == (0, 5) and hc.ev_start.tolist() == [0] * (len(names) + 1) and hc.max_events == 0
    assert hc.rec_start[0] == 0 and hc.rec_start[-1] <= hc.audio.shape[0]
    for i, name in enumerate(names):
        s0, n = int(hc.rec_start[i]), int(hc.lengths[i])
        assert s0 % 16 == 0 and int(hc.rec_start[i + 1]) == s0 + (n + 15) // 16 * 16
        assert np.array_equal(hc.audio[s0:s0 + n], written[name])
        assert not hc.audio[s0 + n:int(hc.rec_start[i + 1])].any()          # the alignment gap is int16 zero


def test_load_infer_split_lists_and_lays_out_the_folder(folder):
    root, written = folder
    prm = infer_params(root)
    listed = [n.replace(".wav", "") for n in os.listdir(str(root))]
    ds = FoaDataset(prm, "infer", rank=0, world=1)
    hc = C.load_infer_split(prm, rank=0, world=1, verify="all")
    assert hc.filelist == ds.get_filelist() == listed and hc.wav_pth == str(root) and hc.csv_pth is None
    _check_layout(hc, written, listed)
    for rank in range(2):                                                   # the rank shards of FoaDataset
        shard = C.load_infer_split(prm, rank=rank, world=2)
        assert shard.filelist == FoaDataset(prm, "infer", rank=rank, world=2).get_filelist() == sorted(listed)[rank::2]
        assert (shard.rank, shard.world) == (rank, 2)
        _check_layout(shard, written, sorted(listed)[rank::2])
    part = C.load_infer_split(prm, rank=0, world=1, files=["rec_f", "rec_a"])
    _check_layout(part, written, [n for n in listed if n in ("rec_f", "rec_a")])
    with pytest.raises(ValueError, match="rec_zz"):
        C.load_infer_split(prm, rank=0, world=1, files=["rec_a", "rec_zz"])
    with pytest.raises(ValueError, match="verify"):
        C.load_infer_split(prm, rank=0, world=1, verify="some")
    with pytest.raises(ValueError, match="rec_b"):                          # a shard does not hold the other rank's files
        C.load_infer_split(prm, rank=0, world=2, files=[sorted(listed)[1]])


def test_infer_split_from_arrays_is_the_same_structure(folder):
    root, written = folder
    prm = infer_params(root)
    names = [n for n, _ in LENGTHS]
    hc = C.infer_split_from_arrays(names, [written[n] for n in names], prm)
    _check_layout(hc, written, names)
    ref = C.load_infer_split(prm, rank=0, world=1, files=names)
    order = [names.index(n) for n in ref.filelist]
    assert [hc.lengths[i] for i in order] == ref.lengths.tolist()
    with pytest.raises(ValueError, match="bad_one"):
        C.infer_split_from_arrays(["ok", "bad_one"], [written["rec_a"], written["rec_a"].astype(np.float32)], prm)
    with pytest.raises(ValueError, match="three"):
        C.infer_split_from_arrays(["three"], [written["rec_a"][:, :3]], prm)
    with pytest.raises(ValueError):
        C.infer_split_from_arrays(["a", "b"], [written["rec_a"]], prm)
    empty = C.infer_split_from_arrays([], [], prm)
    assert empty.filelist == [] and empty.rec_start.tolist() == [0] and empty.audio.shape == (16, 4)


def test_a_float_wav_is_refused_by_name(tmp_path):
    from scipy.io import wavfile
    write_folder(tmp_path, lengths=(("fine", 4800),))
    wavfile.write(str(tmp_path / "floaty.wav"), SR, np.zeros((4800, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="floaty.wav"):
        C.load_infer_split(infer_params(tmp_path), rank=0, world=1)
    wavfile.write(str(tmp_path / "floaty.wav"), SR, np.zeros((4800, 2), dtype=np.int16))      # int16, but two channels
    with pytest.raises(ValueError, match="floaty.wav"):
        C.load_infer_split(infer_params(tmp_path), rank=0, world=1)
    with pytest.raises(ValueError, match="not a directory"):
        C.load_infer_split(infer_params(tmp_path / "nowhere"), rank=0, world=1)


# ---------------------------------------------------------------------------------------------------------- the row split
def test_split_pass_rows_crosses_recording_boundaries():
    # recordings of 5, 3, 0, 4 and 6 label frames laid end to end: [0, 5) [5, 8) [8, 8) [8, 12) [12, 18); the pass holds the
    # frames [3, 14): the end of recording 0, recording 1 (no rows), the empty recording 2, recording 3 whole, the start of 4
    frame_start = np.asarray([0, 5, 8, 8, 12, 18])
    counts = np.asarray([2, 0, 0, 0, 0, 1, 0, 0, 3, 0, 1], dtype=np.int32)           # run frames 0..10 = axis frames 3..13
    rows = np.asarray([[0, 1, .1, .2, .3], [0, 2, .4, .5, .6], [5, 3, .7, .8, .9],
                       [8, 4, 1., 0., 0.], [8, 4, 0., 1., 0.], [8, 5, 0., 0., 1.], [10, 6, .5, .5, .5]], dtype=np.float32)
    got = C.split_pass_rows(rows, counts, 3, frame_start)
    vals = rows[:, 1:].tolist()
    assert got == {0: {3: vals[0:2]}, 3: {0: vals[2:3], 3: vals[3:6]}, 4: {1: vals[6:7]}}
    assert list(got[3]) == [0, 3] and all(isinstance(k, int) for r in got.values() for k in r)
    assert 1 not in got and 2 not in got                                    # a recording without rows, one without frames
    # the same rows as group_rows gives for one clip, frame numbers apart
    from adyolo_amd.postprocess import group_rows
    whole = group_rows(rows, counts, 1)[0]
    assert [v for r in sorted(got) for v in got[r].values()] == list(whole.values())
    assert C.split_pass_rows(np.zeros((0, 5), dtype=np.float32), np.zeros(4, dtype=np.int32), 14, frame_start) == {}
    with pytest.raises(ValueError):
        C.split_pass_rows(rows, counts[:-1], 3, frame_start)                # counts do not sum to the rows
    with pytest.raises(ValueError):
        C.split_pass_rows(rows, counts, 8, frame_start)                     # the run ends past the last recording


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_new_symbols_are_declared_bound_and_wrapped():
    from adyolo_amd import ops, test as atest
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adyolo_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("adyolo_corpus_gather_windows", "adyolo_decode_stitch"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
        assert getattr(lib, name) is not None
    assert "#define ADYOLO_WINDOW_WORDS 8" in hdr and ops.WINDOW_WORDS == 8
    assert callable(ops.corpus_gather_windows) and callable(ops.decode_stitch) and callable(atest.infer_epoch_corpus)
    assert callable(C.InferDeviceCorpus)
