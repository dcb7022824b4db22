"""GPU: ``ops.csv_format`` (csrc/csv.hip) against ``postprocess.format_rows`` on bytes and segment offsets, at the shapes where
the kernels can break -- one frame, more rows in a frame than a wave, a frame's rows across a wave and a 256-row tile boundary,
frame numbers that gain a digit, the float edges of ``test_csv_format_cpu.structured_bits``, garbage behind the rows, runs that
start and end on recording boundaries, every status bit with guard bytes behind the buffer -- and the five device loops with
``device_csv=True`` against their host writer: the same folders, byte for byte, with no more host copies."""
import os
import shutil
import warnings

import numpy as np
import pytest
import torch

from test_csv_format_cpu import structured_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR, HOP = 24000, 2400


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


# ---------------------------------------------------------------------------------------------- the kernel on synthetic rows
def _rows(rng, counts, nb_classes=13):
    n = int(np.sum(counts))
    rows = np.zeros((n, 5), dtype=np.float32)
    rows[:, 0] = rng.integers(0, 7, n)                             # not what the frame field is made from
    rows[:, 1] = rng.integers(0, nb_classes, n)
    rows[:, 2:] = rng.standard_normal((n, 3)).astype(np.float32)
    return rows


def _device_format(ops, rows, counts, table, ids=None, spare=0, garbage=None, n_bytes=None, guard=64):
    """rows (+ ``spare`` capacity rows of ``garbage`` bits behind them) through ``ops.csv_format`` -> (bytes, seg_bytes, status,
    the whole byte buffer with ``guard`` bytes behind the stated capacity, all 0xAB before the call)."""
    n = len(rows)
    cap_rows = np.zeros((n + spare, 5), dtype=np.float32)
    cap_rows[:n] = rows
    cap_ids = None
    if ids is not None:
        cap_ids = np.zeros(n + spare, dtype=np.int32)
        cap_ids[:n] = ids
    if garbage is not None:
        cap_rows[n:] = np.frombuffer(np.uint32(garbage).tobytes(), dtype=np.float32)[0]
        if cap_ids is not None:
            cap_ids[n:] = -5
    d_rows = torch.from_numpy(cap_rows).to(DEV)
    d_counts = torch.from_numpy(np.asarray(counts, dtype=np.int32)).to(DEV)
    d_table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(DEV)
    d_ids = None if cap_ids is None else torch.from_numpy(cap_ids).to(DEV)
    if n_bytes is None:
        n_bytes = len(cap_rows) * ops.CSV_LINE_MAX
    buf = ops.csv_buffers(DEV, len(counts), len(cap_rows), len(table), n_bytes + guard)
    whole = buf["out"]
    whole.fill_(0xAB)
    buf["out"] = whole[:n_bytes]
    out, seg_bytes, status = ops.csv_format(d_rows, d_counts, d_table, d_ids, buf=buf)
    seg_bytes, status, whole = seg_bytes.cpu().numpy(), int(status.cpu()[0]), whole.cpu().numpy()
    total = int(seg_bytes[-1])
    return whole[:min(total, n_bytes)].tobytes(), seg_bytes, status, whole


def _check(ops, rows, counts, table, ids=None, **kw):
    from adyolo_amd.postprocess import format_rows
    want, want_seg = format_rows(rows, counts, table, ids)
    got, seg, status, whole = _device_format(ops, rows, counts, table, ids, **kw)
    assert status == 0
    assert seg.tolist() == want_seg.tolist()
    assert got == want
    assert (whole[len(want):] == 0xAB).all()                       # nothing behind the total
    return want


def _counts(rng, mode, n):
    if mode == "none":
        return np.zeros(n, dtype=np.int64)
    if mode == "few":
        return rng.integers(0, 4, n)
    c = rng.integers(0, 4, n)
    if mode == "wave":
        c[n // 2] = 65                                             # more rows in one frame than a wave has lanes
        return c
    # rows 0 .. of frame 0 run across lanes 63 | 64 and rows 255 | 256: a wave and a tile (workgroup) boundary inside one
    # frame; with more frames, five rows each put further frames across the later boundaries
    c[:] = 5
    c[0] = 300 if n == 1 else 250
    if n > 1:
        c[1] = 9                                                   # rows 250 .. 258
    return c


@pytest.mark.parametrize("mode", ["none", "few", "wave", "straddle"])
def test_kernel_matches_format_rows_on_clips(ops, mode):
    from adyolo_amd.postprocess import csv_segments_clips
    rng = np.random.default_rng(3)
    for t in (1, 63, 130):
        for clips in (1, 3):
            counts = _counts(rng, mode, t * clips)
            rows = _rows(rng, counts)
            for ids in (None, rng.integers(0, 30, len(rows)).astype(np.int32)):
                want = _check(ops, rows, counts, csv_segments_clips(clips, t), ids)
                assert (len(want) > 0) == (mode != "none")


def test_frame_numbers_gain_digits(ops):
    from adyolo_amd.postprocess import csv_segments_clips
    rng = np.random.default_rng(4)
    counts = rng.integers(0, 3, 1001)
    counts[[9, 10, 99, 100, 999, 1000]] = 1
    want = _check(ops, _rows(rng, counts), counts, csv_segments_clips(1, 1001))
    firsts = {line.split(b",")[0] for line in want.split(b"\n") if line}
    assert {b"9", b"10", b"99", b"100", b"999", b"1000"} <= firsts


def test_classes_and_ids(ops):
    from adyolo_amd.postprocess import csv_segments_clips
    rng = np.random.default_rng(5)
    counts = np.array([4, 0, 4, 4, 4])
    rows = _rows(rng, counts)
    rows[:, 1] = [0, 9, 10, 12] * 4
    rows[12:, 1] = [-1.0, 11.75, 2147483520.0, -2147483520.0]     # int() truncates; the float32s next to +-2^31
    for ids in (None, np.zeros(16, dtype=np.int32), np.full(16, 7, dtype=np.int32),
                np.array([0, 7, 2 ** 31 - 1, 10] * 4, dtype=np.int32)):
        want = _check(ops, rows, counts, csv_segments_clips(1, 5), ids)
    assert b",12,10," in want and b"4,-1,0," in want and b"4,11,7," in want and b"4,2147483520,2147483647," in want
    assert b"4,-2147483520,10," in want


def test_float_edges_in_x_y_and_z(ops):
    from adyolo_amd.postprocess import csv_segments_clips
    bits = structured_bits()
    n = len(bits)
    rows = np.zeros((n + 2, 5), dtype=np.float32)
    xyz = rows[:, 2:].view(np.uint32)
    xyz[:n, 0], xyz[:n, 1], xyz[:n, 2] = bits, np.roll(bits, 1), np.roll(bits, 2)
    rows[:n, 1] = np.arange(n) % 13
    rows[n, 1:] = [-2147483520.0] + [-1.1754943508222875e-38] * 3   # the longest line next to the shortest
    rows[n + 1, 2:].view(np.uint32)[:] = 0x7fc00000
    counts = np.full(1000, (n + 2) // 1000)
    counts[-1] = n + 2 - counts[:-1].sum()
    ids = np.zeros(n + 2, dtype=np.int32)
    ids[n] = 2 ** 31 - 1
    with np.errstate(invalid="ignore"):
        want = _check(ops, rows, counts, np.array([[0, 2 ** 31 - 1000]]), ids)
    tail = want.split(b"\n")[-3:-1]
    assert len(tail[0]) + 1 == 106 and tail[1] == b"2147483647,0,0,nan,nan,nan"


def test_garbage_behind_the_rows_is_not_read(ops):
    from adyolo_amd.postprocess import csv_segments_clips
    rng = np.random.default_rng(6)
    counts = rng.integers(0, 4, 130)
    rows = _rows(rng, counts)
    ids = rng.integers(0, 9, len(rows)).astype(np.int32)
    table = csv_segments_clips(2, 65)
    clean = _check(ops, rows, counts, table, ids, spare=700)
    # NaN classes and negative ids there would raise ADYOLO_CSV_BAD_VALUE (``_check`` asserts status 0) if they were read
    assert _check(ops, rows, counts, table, ids, spare=700, garbage=0xffc12345) == clean
    assert _check(ops, rows, counts, table, None, spare=3, garbage=0x7fffffff) == _check(ops, rows, counts, table, None)


def test_runs_split_at_the_recording_boundaries(ops):
    from adyolo_amd.postprocess import csv_segments_run
    rng = np.random.default_rng(7)
    frame_start = np.array([0, 20, 50, 50, 75, 110, 130])
    for base, n in ((33, 60), (20, 30), (20, 31), (49, 2), (60, 5), (0, 130), (75, 35)):
        r0, table = csv_segments_run(base, n, frame_start)
        counts = rng.integers(0, 4, n)
        counts[0] = counts[-1] = 2
        rows = _rows(rng, counts)
        ids = rng.integers(0, 9, len(rows)).astype(np.int32)
        want = _check(ops, rows, counts, table, ids)
        assert want.startswith(b"%d," % (base - frame_start[r0]))
        counts[0] = counts[-1] = 0                                 # segments that start (and end) without a row
        rows = _rows(rng, counts)
        _check(ops, rows, counts, table)
    assert len(csv_segments_run(60, 5, frame_start)[1]) == 1 and len(csv_segments_run(0, 130, frame_start)[1]) == 6


def test_status_bits_and_the_bytes_behind_the_capacity(ops):
    from adyolo_amd.postprocess import CSV_BAD_COUNTS, CSV_BAD_TABLE, CSV_BAD_VALUE, CSV_OVERFLOW, csv_segments_clips, format_rows
    rng = np.random.default_rng(8)
    counts = rng.integers(1, 4, 130)
    rows = _rows(rng, counts)
    table = csv_segments_clips(2, 65)
    want, want_seg = format_rows(rows, counts, table)
    # the capacity to the byte: everything is written, nothing behind it
    got, seg, status, whole = _device_format(ops, rows, counts, table, n_bytes=len(want))
    assert status == 0 and got == want and (whole[len(want):] == 0xAB).all() and len(whole) >= len(want) + 64
    # one byte short: the true offsets, the bit, and not one byte written
    for short in (1, len(want) - 1, len(want)):
        got, seg, status, whole = _device_format(ops, rows, counts, table, n_bytes=len(want) - short)
        assert status == CSV_OVERFLOW and seg.tolist() == want_seg.tolist() and (whole == 0xAB).all()
    # counts that run past the rows given, a negative count
    for bad in (counts + (np.arange(130) == 129), np.where(np.arange(130) == 5, -1, counts)):
        got, seg, status, whole = _device_format(ops, rows, bad, table)
        assert status == CSV_BAD_COUNTS and not seg.any() and (whole == 0xAB).all()
    # a table that does not start at frame 0, descends, leaves the frames, or numbers a frame below 0
    for bad in ([[1, 0]], [[0, 0], [70, 0], [65, 0]], [[0, 0], [131, 0]], [[0, -1]], [[0, 2 ** 31 - 100]]):
        got, seg, status, whole = _device_format(ops, rows, counts, np.array(bad))
        assert status == CSV_BAD_TABLE and not seg.any() and (whole == 0xAB).all()
    # a class int() refuses, one outside int32, a negative id: the bit, and the field written as 0
    ids = rng.integers(1, 9, len(rows)).astype(np.int32)
    for col, value in ((1, np.nan), (1, np.inf), (1, -np.inf), (1, 2.0 ** 31), (1, -2.0 ** 31), (None, -1), (None, -2 ** 31)):
        r, i = rows.copy(), ids.copy()
        fixed_r, fixed_i = rows.copy(), ids.copy()
        if col is None:
            i[70], fixed_i[70] = value, 0
        else:
            r[70, col], fixed_r[70, col] = value, 0
        with pytest.raises(ValueError):
            format_rows(r, counts, table, i)
        got, seg, status, whole = _device_format(ops, r, counts, table, i)
        fixed, fixed_seg = format_rows(fixed_r, counts, table, fixed_i)
        assert status == CSV_BAD_VALUE and got == fixed and seg.tolist() == fixed_seg.tolist()
        assert (whole[len(fixed):] == 0xAB).all()
    for word in (CSV_OVERFLOW, CSV_BAD_COUNTS, CSV_BAD_VALUE, CSV_BAD_TABLE):
        with pytest.raises(Exception, match="csv_format"):
            ops.csv_status_check(word)
    ops.csv_status_check(0)


# ------------------------------------------------------------------------------------------------------------- the loops
# (the small builders of the device loops' own GPU tests, copied)
SPECIAL = ((180.0, 0.0), (-180.0, 12.5), (0.0, 90.0), (45.0, -90.0), (179.999, 89.9), (-0.25, -45.0), (90.0, 22.5))
CLIPS = (("c0_short", 12 * HOP + 77), ("c1_long", 70 * HOP), ("c2_one", 30 * HOP), ("c3_one", 30 * HOP))
# label frames 0 (its reference still has events: rows past the audio), 12, 30 (one 3 s window), 45 and 110 (cut by passes)
MIXED = (("m0_past", 1000), ("m1_short", 12 * HOP + 77), ("m2_one", 30 * HOP), ("m3_three", 45 * HOP + 401),
         ("m4_long", 110 * HOP))
OPTS = {"gate_deg": 20.0, "max_gap": 2, "min_len": 3, "smooth": 0.5}
VIEWS = [0, 5]


def _clip_events(rs, name, n_samples, nb_classes=12):
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


def _write_split(root, clips, seed):
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    wdir, cdir = os.path.join(root, "foa_dev", "dev-test"), os.path.join(root, "metadata_dev", "dev-test")
    os.makedirs(wdir)
    os.makedirs(cdir)
    out = {}
    for name, n in clips:
        audio = rs.randint(-8000, 8000, size=(n, 4)).astype(np.int16)
        rows = _clip_events(rs, name, n)
        wavfile.write(os.path.join(wdir, name + ".wav"), SR, audio)
        with open(os.path.join(cdir, name + ".csv"), "w") as fid:
            for r in rows:
                fid.write("%d,%d,%d,%r,%r\n" % r)
        out[name] = audio
    shutil.copytree(cdir, os.path.join(root, "reference"))
    return out


def _params(root, loss, nb_classes):
    return {"args": {"device": DEV, "encoder": "se-resnet34", "loss": loss},
            "data_config": {"nb_classes": nb_classes, "data_pth": str(root), "chunk_window_s": 2, "chunk_stride_s": 1, "sr": SR,
                            "label_hop_len_s": 0.1},
            "train_config": {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
                             "conf_thresh": 0.3, "clss_thresh": 0.3, "unify_thresh": 15.0, "nms": "conn-merge",
                             "loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
                             "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0, "batch_size": 4, "nb_iters": 1},
            "aug_config": {"rotation_augment": True, "spec_augment": True, "spec_augment_thresh": 0.6,
                           "spec_augment_time_mask_param": 20, "spec_augment_freq_mask_param": 16},
            # the untrained AD-YOLO head selects hundreds of rows in a frame
            "test_config": {"tta_views": VIEWS[1:], "tta_min_views": 1, "tta_max_rows_per_frame": 340}}


def _world(tmp_path_factory, loss, nb_classes):
    from adyolo_amd.augmentations import tta_options
    from adyolo_amd.corpus import (EvalDeviceCorpus, EvalWindowCorpus, InferDeviceCorpus, infer_split_from_arrays,
                                   load_eval_split)
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    w = {}
    for key, clips in (("clips", CLIPS), ("mixed", MIXED)):
        root = str(tmp_path_factory.mktemp("gpu_csv_%s_%s" % (loss, key)))
        w[key + "_audio"] = _write_split(root, clips, seed=9)
        w[key + "_prm"] = _params(root, loss, nb_classes)
        w[key + "_ref"] = os.path.join(root, "reference")
        w[key + "_hc"] = load_eval_split(w[key + "_prm"], "test", rank=0, world=1, verify="all")
    prm = w["prm"] = w["clips_prm"]
    torch.manual_seed(8)
    w["model"] = WrapperModel((1, 7, 80, 64), (), prm).to(DEV).eval()
    w["fx"], w["crit"], w["post"] = FeatureExtractor(None, DEV), WrapperCriterion(prm), LabelPostProcessor(prm)
    w["tta"] = tta_options(prm, postprocessor=w["post"])
    w["clips"] = EvalDeviceCorpus(w["clips_hc"], prm, DEV)
    w["windows"] = EvalWindowCorpus(w["mixed_hc"], w["mixed_prm"], DEV, window_s=3, margin_s=1.0, batch_size=3)
    names = w["windows"].get_filelist()
    w["infer"] = InferDeviceCorpus(infer_split_from_arrays(names, [w["mixed_audio"][n] for n in names], prm), prm, DEV,
                                   window_s=3, margin_s=1.0, batch_size=3)
    for key in ("windows", "infer"):
        corpus = w[key]
        per_rec = np.diff(np.asarray(corpus.frame_start))
        assert sorted(per_rec.tolist()) == [0, 12, 30, 45, 110] and corpus.n_passes >= 3   # empty, one window, cut by passes
    return w


@pytest.fixture(scope="module")
def yolo(ops, tmp_path_factory):
    return _world(tmp_path_factory, "adyolo", 12)


@pytest.fixture(scope="module")
def adpit(ops, tmp_path_factory):
    return _world(tmp_path_factory, "adpit", 13)


def _folder(path):
    return {name: open(os.path.join(path, name), "rb").read() for name in sorted(os.listdir(path))}


def _same_folders(host, device, names):
    a, b = _folder(host), _folder(device)
    assert sorted(a) == sorted(n + ".csv" for n in names) == sorted(b)
    for name in a:
        assert a[name] == b[name], name
    assert any(len(v) for v in a.values())
    return a


def _both(tmp_path, run):
    """``run(output_pth, device_csv)`` with the host writer, then with the device's -> both results."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                            # (the caps of the tracking definition only warn)
        return run(str(tmp_path / "host"), False), run(str(tmp_path / "device"), True)


@pytest.mark.parametrize("config", ["plain", "track", "tta"])
@pytest.mark.parametrize("loss", ["adyolo", "adpit"])
def test_test_epoch_corpus_writes_the_same_folder(request, tmp_path, loss, config):
    from adyolo_amd import test as atest
    w = request.getfixturevalue("yolo" if loss == "adyolo" else "adpit")

    def run(out, device_csv):
        return atest.test_epoch_corpus(w["clips"], w["model"], w["fx"], w["crit"], w["post"], out, batch_size=2,
                                       tta=w["tta"] if config == "tta" else None, track=OPTS if config == "track" else None,
                                       device_csv=device_csv)
    loss_h, loss_d = _both(tmp_path, run)
    assert loss_h == loss_d
    files = _same_folders(str(tmp_path / "host"), str(tmp_path / "device"), w["clips"].get_filelist())
    if config == "track":                                          # the third column carries ids
        assert any(line.split(b",")[2] != b"0" for v in files.values() for line in v.split(b"\n") if line)


@pytest.mark.parametrize("tracked", [False, True], ids=["plain", "tracking"])
def test_infer_epoch_corpus_writes_the_same_folder(yolo, tmp_path, tracked):
    from adyolo_amd import test as atest
    w = yolo

    def run(out, device_csv):
        return atest.infer_epoch_corpus(w["infer"], w["model"], w["fx"], w["post"], out, tracking=OPTS if tracked else None,
                                        device_csv=device_csv)
    info_h, info_d = _both(tmp_path, run)
    assert info_h == info_d
    files = _same_folders(str(tmp_path / "host"), str(tmp_path / "device"), w["infer"].get_filelist())
    assert files["m0_past.csv"] == b"" and all(len(files[n + ".csv"]) for n in ("m2_one", "m4_long"))


def test_test_epoch_windows_with_a_device_scorer(yolo, tmp_path):
    from adyolo_amd import test as atest
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    w = yolo
    scorers = []

    def run(out, device_csv):
        scorers.append(DeviceSELDScorer(w["mixed_prm"], w["mixed_ref"], DEV))
        return atest.test_epoch_windows(w["windows"], w["model"], w["fx"], w["crit"], w["post"], out, device_scorer=scorers[-1],
                                        device_csv=device_csv)
    loss_h, loss_d = _both(tmp_path, run)
    assert loss_h == loss_d
    _same_folders(str(tmp_path / "host"), str(tmp_path / "device"), w["windows"].get_filelist())
    (acc_h, names_h), (acc_d, names_d) = scorers[0].accumulators(), scorers[1].accumulators()
    assert names_h == names_d and np.array_equal(np.asarray(acc_h).view(np.int64), np.asarray(acc_d).view(np.int64))
    np.testing.assert_equal(scorers[0].scores(), scorers[1].scores())


@pytest.mark.parametrize("windowed", [False, True], ids=["corpus", "windows"])
def test_the_sweeps_leave_the_same_last_threshold_folder(yolo, tmp_path, windowed):
    from adyolo_amd import test as atest
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    w = yolo

    def run(out, device_csv):
        post = LabelPostProcessor(w["prm"])
        if windowed:
            scorer = DeviceSELDScorer(w["mixed_prm"], w["mixed_ref"], DEV)
            return atest.sweep_conf_thresh_windows(w["windows"], w["model"], w["fx"], w["crit"], post, scorer,
                                                   thresholds=(0.6, 0.3), output_pth=out, tracking=OPTS, device_csv=device_csv)
        scorer = DeviceSELDScorer(w["prm"], w["clips_ref"], DEV)
        return atest.sweep_conf_thresh_corpus(w["clips"], w["model"], w["fx"], w["crit"], post, scorer, thresholds=(0.6, 0.3),
                                              output_pth=out, batch_size=2, device_csv=device_csv)
    got_h, got_d = _both(tmp_path, run)
    np.testing.assert_equal(got_h, got_d)                          # (threshold, score table, loss; a nan equals a nan)
    _same_folders(str(tmp_path / "host"), str(tmp_path / "device"), (w["windows"] if windowed else w["clips"]).get_filelist())


LOOPS = ("test_epoch_corpus", "sweep_conf_thresh_corpus", "test_epoch_windows", "sweep_conf_thresh_windows",
         "infer_epoch_corpus")
THRESHOLDS = (0.6, 0.3)


@pytest.mark.parametrize("loop", LOOPS)
def test_device_csv_synchronises_no_more_often_than_the_host_writer(ops, yolo, tmp_path, monkeypatch, loop):
    """What can synchronise in a loop: ``to_host`` / ``to_host_many`` (counted) and a host-to-device upload.  The writer's
    only upload is ``_CsvWriter._upload``: it must come from page-locked memory (so it does not block), and in the windowed
    loops once, before the first pass's rows are selected -- no pass uploads anything.  Per walk, the first included (the
    writer's buffers are made in it): with U batches or passes, at most 2 U + 1 copies (two per unit and the closing status
    read; the sweeps: besides the forward phase's read and two per threshold for the scores), and never more than the host
    writer makes."""
    from adyolo_amd import test as atest
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    w = yolo
    log = []
    many, one, upload, select = ops.to_host_many, ops.to_host, atest._CsvWriter._upload, atest._select_rows

    def count_many(*ts):
        log.append("copy")
        return many(*ts)

    def count_one(t):
        log.append("copy")
        return one(t)

    def count_upload(self, pinned):
        assert pinned.is_pinned() and not pinned.is_cuda
        log.append("upload")
        return upload(self, pinned)

    def count_select(*args, **kw):
        log.append("select")
        return select(*args, **kw)
    monkeypatch.setattr(ops, "to_host_many", count_many)
    monkeypatch.setattr(ops, "to_host", count_one)
    monkeypatch.setattr(atest._CsvWriter, "_upload", count_upload)
    monkeypatch.setattr(atest, "_select_rows", count_select)
    windowed, sweep = "windows" in loop or loop == "infer_epoch_corpus", loop.startswith("sweep")
    units = w["windows"].n_passes if windowed else len(list(w["clips"].batches(2)))

    def run(out, dc, trk):
        post = LabelPostProcessor(w["prm"])
        if loop == "test_epoch_corpus":
            return atest.test_epoch_corpus(w["clips"], w["model"], w["fx"], w["crit"], post, out, batch_size=2, track=trk,
                                           device_csv=dc)
        if loop == "sweep_conf_thresh_corpus":
            return atest.sweep_conf_thresh_corpus(w["clips"], w["model"], w["fx"], w["crit"], post,
                                                  DeviceSELDScorer(w["prm"], w["clips_ref"], DEV), thresholds=THRESHOLDS,
                                                  output_pth=out, batch_size=2, track=trk, device_csv=dc)
        if loop == "test_epoch_windows":
            return atest.test_epoch_windows(w["windows"], w["model"], w["fx"], w["crit"], post, out, tracking=trk, device_csv=dc)
        if loop == "sweep_conf_thresh_windows":
            return atest.sweep_conf_thresh_windows(w["windows"], w["model"], w["fx"], w["crit"], post,
                                                   DeviceSELDScorer(w["mixed_prm"], w["mixed_ref"], DEV), thresholds=THRESHOLDS,
                                                   output_pth=out, tracking=trk, device_csv=dc)
        return atest.infer_epoch_corpus(w["infer"], w["model"], w["fx"], post, out, tracking=trk, device_csv=dc)

    for trk in (None, OPTS):
        seen = {}
        for dc in (False, True):
            del log[:]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                run(str(tmp_path / ("%d_%d" % (trk is not None, dc))), dc, trk)
            seen[dc] = list(log)
        host, dev = seen[False].count("copy"), seen[True].count("copy")
        uploads = [k for k, what in enumerate(seen[True]) if what == "upload"]
        print(loop, "tracking" if trk else "plain", "units %d: host writer %d copies, device_csv %d copies, %d uploads"
              % (units, host, dev, len(uploads)))
        assert "upload" not in seen[False] and seen[True].count("select") >= units
        bound = 2 * units + 1 + ((1 + 2 * len(THRESHOLDS)) if sweep else 0)
        assert dev <= host and dev <= bound and host > units
        if windowed:
            assert len(uploads) == 1 and uploads[0] < seen[True].index("select")
        else:
            assert 1 <= len(uploads) <= units                      # one per batch shape, page-locked
