"""GPU: the device SELD scorer (``ops.seld_score``, csrc/seld.hip; ``seld_metrics.DeviceSELDScorer``;
``test_epoch_audio(device_scorer=...)``; ``sweep_conf_thresh(device_score=True)``) against the reference-made fixtures and
the host ``SELDScorer`` on the CSV files of the same rows.

The device distances use OCML's float64 atan2 / sin / cos / acos, which may differ from the host's libm by an ulp; counts
are therefore compared exactly only on data whose track averages are checked to lie farther than 1e-9 degree from the
20-degree threshold, and float sums within rtol 1e-12.  The synthetic ties are kept to those the tie rules alone decide
(``_robust_ties``)."""
import os
import sys

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = pytest.mark.gpu
PRM = {"data_config": {"nb_classes": 12, "sr": 24000, "label_hop_len_s": 0.1}}
C = 12


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _scores(res):
    return np.asarray([float(v) for v in res[:5]]), np.asarray(res[5], dtype=np.float64)


def _metrics_fixture(tmp_path):
    g = np.load(os.path.join(G, "metrics.npz"))
    ref_dir, pred_dir = tmp_path / "ref", tmp_path / "pred"
    ref_dir.mkdir()
    pred_dir.mkdir()
    preds = {}
    for i, name in enumerate(g["names"]):
        with open(ref_dir / str(name), "w") as f:
            for r in g["ref_%d" % i]:
                f.write("%d,%d,%d,%d,%d\n" % tuple(int(v) for v in r))
        d = {}
        with open(pred_dir / str(name), "w") as f:
            for r in g["pred_%d" % i]:
                f.write("{},{},{},{},{},{}\n".format(int(r[0]), int(r[1]), 0, float(r[3]), float(r[4]), float(r[5])))
                d.setdefault(int(r[0]), []).append([int(r[1]), float(r[3]), float(r[4]), float(r[5])])
        preds[str(name)] = d
    return g, str(ref_dir), str(pred_dir), preds


# ------------------------------------------------------------------------------------------------ reference fixtures
def test_metrics_fixture_through_add_dict(ops, tmp_path):
    """All scores, classwise tables, both overlap variants and the jackknife of metrics.npz (made by the reference)."""
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    g, ref_dir, _, preds = _metrics_fixture(tmp_path)
    order = [str(n) for n in g["jk_order"]]
    dev = DeviceSELDScorer(PRM, ref_dir)
    for name in order:
        dev.add_dict(name, preds[name])
    s, cw = _scores(dev.scores())
    np.testing.assert_allclose(s, g["scores"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(cw, g["classwise"], rtol=1e-9, atol=1e-9)
    jk = dev.scores(is_jackknife=True)
    np.testing.assert_allclose(np.asarray([np.asarray(jk[i][1]) for i in range(5)]), g["jk_conf"], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(jk[5][1], g["jk_classwise_conf"], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose([float(jk[i][0]) for i in range(5)], g["jk_points"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(jk[5][0], g["jk_classwise"], rtol=1e-9, atol=1e-9)
    for tag, ov in (("poly", "polyphony"), ("homog", "homogenous")):
        dev = DeviceSELDScorer(PRM, ref_dir, overlap=ov)
        assert dev.nb_overlap_files == int(g["ov_%s_nfiles" % tag]) and dev.nb_overlap_frames == int(g["ov_%s_nframes" % tag])
        for name in order:
            dev.add_dict(name, preds[name])
        s, cw = _scores(dev.scores())
        np.testing.assert_allclose(s, g["ov_%s_scores" % tag], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(cw, g["ov_%s_classwise" % tag], rtol=1e-9, atol=1e-9)
    dev.reset()
    dev.add_dict(order[0], {})
    assert dev.accumulators()[1] == [order[0]]


def test_seld_chain_fixture_through_add_dict(ops, tmp_path):
    """The reference's prediction rows of seld_chain.npz give its scores (and the host scores of their CSV files)."""
    from adyolo_amd.postprocess import write_seld_output_file
    from adyolo_amd.seld_metrics import ComputeSELDResults, DeviceSELDScorer
    g = np.load(os.path.join(G, "seld_chain.npz"))
    ref_dir, out_dir = tmp_path / "ref", tmp_path / "out"
    ref_dir.mkdir(), out_dir.mkdir()
    rows = {}
    for name in g["names"]:
        name = str(name)
        with open(ref_dir / (name + ".csv"), "w") as f:
            for r in g["ref_" + name]:
                f.write("%d,%d,%d,%d,%d\n" % tuple(int(v) for v in r))
        pred = g["pred_" + name]
        rows[name] = {int(fr): [list(r[[1, 3, 4, 5]]) for r in pred[pred[:, 0] == fr]] for fr in np.unique(pred[:, 0])}
        write_seld_output_file(str(out_dir / (name + ".csv")), rows[name])
    dev = DeviceSELDScorer(PRM, str(ref_dir))
    for name, d in rows.items():
        dev.add_dict(name, d)
    s, cw = _scores(dev.scores())
    np.testing.assert_allclose(s, g["scores"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(cw, g["classwise"], rtol=0, atol=1e-6)
    hs, hcw = _scores(ComputeSELDResults(PRM, str(ref_dir)).get_SELD_Results(str(out_dir)))
    np.testing.assert_allclose(s, hs, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(cw, hcw, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ synthetic splits
def _track_averages(pred, ref, nb_classes):
    """The per-track average distances SELDScorer.update forms for one recording (same loop, same assignment)."""
    from scipy.optimize import linear_sum_assignment
    from adyolo_amd.seld_metrics import _great_circle_deg
    out = []
    for blk in range(len(ref)):
        pb, rb = pred.get(blk, {}), ref[blk]
        for c in range(nb_classes):
            if c not in rb or c not in pb:
                continue
            tracks = {}
            for fr, ref_vals in rb[c].items():
                if fr not in pb[c]:
                    continue
                gg = np.asarray(ref_vals, dtype=float)[:, 1:] * np.pi / 180.0
                p = np.asarray(pb[c][fr], dtype=float)[:, 1:] * np.pi / 180.0
                cost = _great_circle_deg(gg[:, None, 0], gg[:, None, 1], p[None, :, 0], p[None, :, 1])
                for r, cc in zip(*linear_sum_assignment(cost)):
                    tracks.setdefault(int(r), []).append(cost[r, cc])
            out.extend(sum(d) / len(d) for d in tracks.values())
    return out


def _unit(az_deg, el_deg):
    az, el = np.deg2rad(az_deg), np.deg2rad(el_deg)
    return [np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)]


def _robust_ties(rows, frame_refs):
    """Keep the ties whose outcome the tie rules alone decide.  Co-located events (or duplicate predictions) tie every
    assignment, and scipy's choice among them then rests on the rules only while the smaller side has one entry; with two or
    more on both sides it also rests on the rounding of the dual updates (((a + b) - a) against b), so a one-ulp difference
    between OCML's and the host's acos may pick the other of two equal-cost assignments.  Here: one prediction at most for a
    class with co-located events in the frame, and no duplicate prediction of a class with two or more events in it."""
    n_ref, coloc = {}, set()
    for e in frame_refs:
        n_ref[e[1]] = n_ref.get(e[1], 0) + 1
    for i, e in enumerate(frame_refs):
        if any(e[1:] == f[1:] for f in frame_refs[:i]):
            coloc.add(e[1])
    out, seen = [], {}
    for r in rows:
        if (r[0] in coloc and seen.get(r[0])) or (n_ref.get(r[0], 0) >= 2 and r in out):
            continue
        out.append(r)
        seen[r[0]] = 1
    return out


def _synthetic_split(rng, n_files, t_clip, dense):
    """Reference CSV rows and float32 prediction dicts: co-located reference events of one class, duplicate predictions,
    classes on one side only (refs 0-6, predictions 2-9), predictions past the recording length, an empty file, rows out of
    class order within a frame, and both n_ref > n_pred and n_pred > n_ref."""
    refs, preds = [], []
    for k in range(n_files):
        length = int(rng.integers(t_clip // 2, t_clip - 5))
        ref = []
        for fr in range(length + 1):
            if fr != length and rng.random() < 0.25:
                continue
            for _ in range(int(rng.integers(1, 4))):
                ev = [fr, int(rng.integers(0, 7)), 0, int(rng.integers(-180, 180)), int(rng.integers(-90, 91))]
                ref.append(ev)
                if rng.random() < 0.15:
                    ref.append(list(ev))                                # co-located event of the same class
        pred = {}
        if k != 1:                                                      # file 1: no predictions at all
            for fr in range(t_clip):
                rows = []
                near = [e for e in ref if e[0] == fr]
                n = int(rng.poisson(18 if dense else 1.5))
                for _ in range(n):
                    if near and rng.random() < 0.7:
                        e = near[int(rng.integers(len(near)))]
                        cls, az, el = (e[1] if rng.random() < 0.8 else int(rng.integers(2, 10))), e[3], e[4]
                        az, el = az + rng.normal(0, 12), np.clip(el + rng.normal(0, 12), -89, 89)
                    else:
                        cls, az, el = int(rng.integers(2, 10)), rng.uniform(-180, 180), rng.uniform(-89, 89)
                    rows.append([cls] + [float(np.float32(v)) for v in _unit(az, el)])
                    if rng.random() < 0.1:
                        rows.append(list(rows[-1]))                     # duplicate prediction
                rows = _robust_ties(rows, [e for e in ref if e[0] == fr])
                if rows:
                    rng.shuffle(rows)                                   # classes in any order within the frame
                    pred[fr] = rows
        refs.append(ref)
        preds.append(pred)
    return refs, preds


def _score_split(tmp_path, tag, refs, preds, t_clip, ops):
    from adyolo_amd.postprocess import write_seld_output_file
    from adyolo_amd.seld_metrics import ComputeSELDResults, DeviceSELDScorer, SELDScorer
    ref_dir, pred_dir = tmp_path / ("ref_" + tag), tmp_path / ("pred_" + tag)
    ref_dir.mkdir(), pred_dir.mkdir()
    names = ["f%02d" % k for k in range(len(refs))]
    for name, ref, pred in zip(names, refs, preds):
        with open(ref_dir / (name + ".csv"), "w") as f:
            for r in ref:
                f.write("%d,%d,%d,%d,%d\n" % tuple(r))
        write_seld_output_file(str(pred_dir / (name + ".csv")), pred)
    host = ComputeSELDResults(PRM, str(ref_dir))
    want, avgs = [], []
    for name in names:
        labels = host._pred_labels(str(pred_dir), name + ".csv")
        sc = SELDScorer(C, 20.0)
        sc.update(labels, host._ref[name + ".csv"][0])
        want.append(sc.accumulator())
        avgs += _track_averages(labels, host._ref[name + ".csv"][0], C)
    assert len(avgs) > 50
    assert min(abs(a - 20.0) for a in avgs) > 1e-9
    # device: every clip in one call, float32 rows in frame order as yolo_select leaves them
    rows, counts = [], np.zeros((len(names), t_clip), dtype=np.int32)
    for k, pred in enumerate(preds):
        for fr in sorted(pred):
            counts[k, fr] = len(pred[fr])
            rows += [[k * t_clip + fr] + r for r in pred[fr]]
    rows = torch.tensor(rows, dtype=torch.float32).reshape(-1, 5).cuda()
    dev = DeviceSELDScorer(PRM, str(ref_dir))
    dev.add_rows(rows, torch.from_numpy(counts.reshape(-1)).cuda(), names)
    got, got_names = dev.accumulators()
    assert got_names == [n + ".csv" for n in names]
    want = np.asarray(want)
    de = slice(5 * C, 6 * C)                                            # total_DE: a float sum
    exact = np.r_[0:5 * C, 6 * C:9 * C + 3]
    np.testing.assert_array_equal(got[:, exact], want[:, exact])
    np.testing.assert_allclose(got[:, de], want[:, de], rtol=1e-12, atol=0)
    hs, hcw = _scores(host.get_SELD_Results(str(pred_dir)))
    s, cw = _scores(dev.scores())
    np.testing.assert_allclose(s, hs, rtol=1e-12)
    np.testing.assert_allclose(cw, hcw, rtol=1e-12)
    return want


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_synthetic_split_matches_host_per_file(ops, tmp_path, dense):
    rng = np.random.default_rng(7 if dense else 5)
    t_clip = 90
    refs, preds = _synthetic_split(rng, 8, t_clip, dense)
    assert any(fr >= max(e[0] for e in ref) for ref, pred in zip(refs, preds) for fr in pred)   # rows past the length
    want = _score_split(tmp_path, "d" if dense else "s", refs, preds, t_clip, ops)
    fp, fn = want[:, C:2 * C].sum(), want[:, 3 * C:4 * C].sum()
    assert fp > 0 and fn > 0 and want[:, 0:C].sum() > 0 and want[:, 2 * C:3 * C].sum() > 0


# ------------------------------------------------------------------------------------------------ the device chain
def _chain(tmp_path, nms="conn-merge"):
    sys.path.insert(0, G)
    from scipy.io import wavfile
    from oracle.filler import fill_module_
    from seld_chain_inputs import CLIPS, chain_clip, crc
    from adyolo_amd.features import FeatureExtractor, load_scaler_npz
    from adyolo_amd.wrapper import WrapperModel
    g = np.load(os.path.join(G, "seld_chain.npz"))
    wdir, cdir = os.path.join(tmp_path, "foa_dev", "dev-test"), os.path.join(tmp_path, "metadata_dev", "dev-test")
    os.makedirs(wdir), os.makedirs(cdir)
    for i, (name, seed, n) in enumerate(CLIPS):
        pcm = chain_clip(seed, n)
        assert crc(pcm) == int(g["crc32"][i])
        wavfile.write(os.path.join(wdir, name + ".wav"), 24000, pcm)
        with open(os.path.join(cdir, name + ".csv"), "w") as f:
            for r in g["ref_" + name]:
                f.write("%d,%d,%d,%d,%d\n" % tuple(int(v) for v in r))
    prm = {"args": {"device": "cuda:0", "encoder": "se-resnet34", "loss": "adyolo"},
           "data_config": {"nb_classes": 12, "sr": 24000, "label_hop_len_s": 0.1, "data_pth": str(tmp_path)},
           "train_config": {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
                            "conf_thresh": float(g["conf_thresh"]), "clss_thresh": float(g["clss_thresh"]),
                            "unify_thresh": float(g["unify_thresh"]), "nms": nms,
                            "loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0}},
           "aug_config": {"rotation_augment": False, "spec_augment": False}}
    model = WrapperModel((1, 7, 400, 64), (), prm)
    fill_module_(model)
    model = model.to("cuda:0").eval()
    fx = FeatureExtractor(load_scaler_npz(os.path.join(G, "scaler_DCASE2021.npz")), "cuda:0")
    return prm, model, fx, cdir


@pytest.mark.parametrize("mode", ["eager", "graphs-batched"])
def test_device_chain_equals_host_scores_of_the_csv_folder(ops, tmp_path, mode):
    """``test_epoch_audio(device_select=True, device_scorer=...)``: the device rows go to ``add_rows`` without a host copy
    (eager: one clip per call; graphs-batched: the two equal-length clips in one call); the scores equal the host's on the
    CSV folder the same call writes."""
    from adyolo_amd import test as atest
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import ComputeSELDResults, DeviceSELDScorer
    from adyolo_amd.wrapper import WrapperCriterion
    prm, model, fx, cdir = _chain(tmp_path)
    crit, post = WrapperCriterion(prm), LabelPostProcessor(prm)
    ds = FoaDataset(prm, "test", is_valid=True)
    kw = {} if mode == "eager" else {"batch_size": 4, "forward": ForwardGraphs(model, fx, post, warm_calls=0)}
    out = os.path.join(tmp_path, "out")
    dev = DeviceSELDScorer(prm, cdir)
    atest.test_epoch_audio(ds, model, fx, crit, post, "cuda:0", out, device_select=True, device_scorer=dev, **kw)
    assert sorted(dev.accumulators()[1]) == sorted(n + ".csv" for n in ds.get_filelist())
    s, cw = _scores(dev.scores())
    hs, hcw = _scores(ComputeSELDResults(prm, cdir).get_SELD_Results(out))
    np.testing.assert_allclose(s, hs, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(cw, hcw, rtol=1e-9, atol=1e-12)
    # the same rows added by hand from one batched selection of all three clips' decodes (equal length: the first 400 frames)
    decs = []
    with torch.no_grad():
        for i in range(len(ds)):
            pcm = ds[i][0][:400 * 600]
            audio = ops.pcm16_to_f32(torch.from_numpy(np.ascontiguousarray(pcm)).cuda()).view(1, 400 * 600, 4)
            decs.append(post.decode_device(model(fx(audio, channels_last8=True), channels_last8=True)))
    dec3 = torch.cat(decs, 0)
    one, three = DeviceSELDScorer(prm, cdir), DeviceSELDScorer(prm, cdir)
    for i, name in enumerate(ds.get_filelist()):
        one.add_rows(*post.select_device_rows(decs[i], 1, trim=False), [name])
    three.add_rows(*post.select_device_rows(dec3, 3, trim=False), ds.get_filelist())
    np.testing.assert_array_equal(one.accumulators()[0], three.accumulators()[0])


def _sweep_batches(ops, ds):
    from adyolo_amd.datasets import audio_collate_fn
    batches = []
    for i in range(len(ds)):
        pcm, _, rows = ds[i]
        t = (pcm.shape[0] // 600) * 600
        audio = ops.pcm16_to_f32(torch.from_numpy(np.ascontiguousarray(pcm[:t])).cuda()).view(1, t, 4)
        batches.append((audio, audio_collate_fn([(pcm, 0, rows)])[2]))
    return batches


@pytest.mark.parametrize("nms", ["conn-merge", "soft-merge"])
def test_sweep_device_score_equals_device_select_sweep(ops, tmp_path, nms):
    """``sweep_conf_thresh(device_select=True, device_score=True)``: the same new threshold and loss, a score table within
    1e-9 and a byte-identical output folder, against ``device_select=True`` alone."""
    from adyolo_amd import test as atest
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import ComputeSELDResults, DeviceSELDScorer
    from adyolo_amd.wrapper import WrapperCriterion
    prm, model, fx, cdir = _chain(tmp_path, nms=nms)
    crit = WrapperCriterion(prm)
    ds = FoaDataset(prm, "test", is_valid=True)
    names = ds.get_filelist()
    batches = _sweep_batches(ops, ds)

    class AudioModel:                          # sweep_conf_thresh feeds ``model(feat)``: here feat is the clip's audio
        def eval(self):
            model.eval()

        def __call__(self, audio):
            return model(fx(audio, channels_last8=True), channels_last8=True)
    got = {}
    for device_score in (False, True):
        post = LabelPostProcessor(prm)
        scorer = DeviceSELDScorer(prm, cdir) if device_score else ComputeSELDResults(prm, cdir)
        out = os.path.join(tmp_path, "sweep_%d" % device_score)
        got[device_score] = atest.sweep_conf_thresh(batches, names, AudioModel(), crit, post, scorer, "cuda:0", out,
                                                    device_select=True, device_score=device_score)
        assert post.get_conf_thresh() == got[device_score][0]
    (new_h, table_h, loss_h), (new_d, table_d, loss_d) = got[False], got[True]
    assert new_d == new_h and loss_d == loss_h
    np.testing.assert_allclose(np.asarray(table_d, dtype=np.float64), np.asarray(table_h, dtype=np.float64), rtol=0, atol=1e-9)
    assert len({tuple(r) for r in table_h}) > 1
    a, b = os.path.join(tmp_path, "sweep_0"), os.path.join(tmp_path, "sweep_1")
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) == len(names)
    for f in os.listdir(a):
        with open(os.path.join(a, f), "rb") as x, open(os.path.join(b, f), "rb") as y:
            assert x.read() == y.read(), f
    with pytest.raises(ValueError, match="DeviceSELDScorer"):
        atest.sweep_conf_thresh(batches, names, AudioModel(), crit, LabelPostProcessor(prm), ComputeSELDResults(prm, cdir),
                                "cuda:0", out, device_select=True, device_score=True)


# ------------------------------------------------------------------------------------------------ errors
def test_errors_are_returned_codes(ops, tmp_path):
    from adyolo_amd import _lib
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    _, ref_dir, _, _ = _metrics_fixture(tmp_path)
    dev = DeviceSELDScorer(PRM, ref_dir)
    name = dev.names[0]
    t = dev._frames[0]
    lib = _lib.load()
    tb = dev.table
    acc = torch.zeros(tb.n_files, 9 * C + 3, dtype=torch.float64, device="cuda:0")
    status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    ws = torch.empty(1 << 16, dtype=torch.float32, device="cuda:0")
    counts = torch.zeros(t, dtype=torch.int32, device="cuda:0")
    fid = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    p = ops._p

    def call(**over):
        a = dict(rows=None, f64=0, n_rows=0, counts=p(counts), n_clips=1, t_clip=t, fid=p(fid), info=p(tb.file_info),
                 off=p(tb.ref_off), ev=p(tb.ref_ev), keep=None, n_files=tb.n_files, c=C, fpb=10, mb=tb.max_blocks,
                 thr=20.0, ws=p(ws), acc=p(acc), status=p(status))
        a.update(over)
        return lib.adyolo_seld_score(*a.values(), None)
    assert call() == 0
    torch.cuda.synchronize()
    for bad in ({"counts": None}, {"acc": None}, {"status": None}, {"n_clips": 0}, {"t_clip": 0}, {"fpb": 65},
                {"c": 0}, {"mb": 0}, {"f64": 2}, {"n_rows": 5}, {"thr": float("nan")}, {"n_files": 0}):
        assert call(**bad) == -1, bad
    assert int(status.item()) == 0 and float(acc.abs().sum()) > 0
    with pytest.raises(_lib.AdyoloHipError, match="float32 or float64"):
        ops.seld_score(torch.zeros(4, 5, dtype=torch.float16, device="cuda:0"), counts, tb, fid, t, acc)
    with pytest.raises(_lib.AdyoloHipError, match="frame counts"):
        ops.seld_score(torch.zeros(4, 5, device="cuda:0"), counts[:-1], tb, fid, t, acc)
    # a file index outside the table and counts past the rows are caught on the device and leave acc as it was
    before = acc.clone()
    with pytest.raises(_lib.AdyoloHipError, match="file index"):
        ops.seld_score(torch.zeros(4, 5, device="cuda:0"), counts, tb, fid + 99, t, acc)
    with pytest.raises(_lib.AdyoloHipError, match="counts"):
        ops.seld_score(torch.zeros(4, 5, device="cuda:0"), counts + 1, tb, fid, t, acc)
    assert torch.equal(acc, before)
    # more than 8 reference events of one class in one frame: refused when the table is built
    big = tmp_path / "big"
    big.mkdir()
    with open(big / "x.csv", "w") as f:
        for k in range(9):
            f.write("3,2,%d,10,10\n" % k)
        f.write("25,1,0,0,0\n")
    with pytest.raises(ValueError, match="reference events"):
        DeviceSELDScorer(PRM, str(big))
    # 1025 predictions of one class in one frame: only the device knows; the overflow word raises ENOSUP on read
    fr = 0
    dev.add_dict(name, {fr: [[2, 1.0, 0.0, 0.0]] * 1025})
    with pytest.raises(_lib.AdyoloHipError, match="rc=-2.*1024"):
        dev.scores()
    dev.reset()
    dev.add_dict(name, {fr: [[2, 1.0, 0.0, 0.0]] * 1024})
    assert np.isfinite(dev.scores()[0])
    rows = torch.tensor([[fr, 2, 1.0, 0.0, 0.0]] * 1025, dtype=torch.float32, device="cuda:0")
    cnt = torch.zeros(t, dtype=torch.int32)
    cnt[fr] = 1025
    with pytest.raises(_lib.AdyoloHipError, match="rc=-2"):
        ops.seld_score(rows, cnt.cuda(), tb, fid, t, acc)
    assert torch.equal(acc, before)
