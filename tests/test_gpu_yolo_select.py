"""GPU: the opt-in device selection of the AD-YOLO head (``ops.yolo_select``, csrc/select.hip; ``LabelPostProcessor.select_device``,
``postprocess(on_device=True)``, ``test_epoch_audio(device_select=True)``, ``sweep_conf_thresh(device_select=True)``) against the
host path ``postprocess.nms_decoded`` on the same decode: the same rows in the same order for the three ``nms`` modes.

xyz tolerance: 5e-5 for thresholds >= 0.3; 2e-3 below, where the vote's exp(exp(c^2 / t) - max) turns a one-ulp difference of
the inner exp into a relative weight error of up to ulp(e^(1/t)) (about 2e-3 at t = 0.1).  Synthetic clips are redrawn until
no candidate pair of one frame and class lies within 1e-3 degree of unify_thresh (float64), where a one-ulp difference of the
float32 acos could flip a cluster."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = pytest.mark.gpu

NMS = ["conn-merge", "soft-merge", "default"]
UNIFY = 20.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _params(nb_classes=12, thresh=0.5, unify=UNIFY, nms="conn-merge"):
    return {"args": {"device": "cuda:0", "encoder": "se-resnet34", "loss": "adyolo"},
            "data_config": {"nb_classes": nb_classes},
            "train_config": {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
                             "conf_thresh": thresh, "clss_thresh": thresh, "unify_thresh": unify, "nms": nms}}


def _flat(res):
    """{frame: [[class, x, y, z], ...]} -> (N, 5) float64 [frame, class, x, y, z] in dict order."""
    rows = [[fr] + [float(v) for v in d] for fr, dets in res.items() for d in dets]
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), 5)


def _assert_same_rows(got, ref, tol, what):
    assert list(got.keys()) == list(ref.keys()), what
    g, r = _flat(got), _flat(ref)
    assert g.shape == r.shape, "%s: %d rows, host %d" % (what, len(g), len(r))
    np.testing.assert_array_equal(g[:, :2], r[:, :2], err_msg=what)
    if len(g):
        err = float(np.abs(g[:, 2:] - r[:, 2:]).max())
        assert err <= tol, "%s: xyz differ by %.3e" % (what, err)


# ------------------------------------------------------------------------------------------------ reference golden
@pytest.mark.parametrize("nms", NMS)
def test_device_select_matches_reference_golden(ops, nms):
    """``postprocess(logit, on_device=True)`` gives the rows the reference wrote (tests/golden/postprocess.npz)."""
    from adyolo_amd.postprocess import LabelPostProcessor
    g = np.load(os.path.join(G, "postprocess.npz"))
    pp = LabelPostProcessor(_params(thresh=0.5, unify=15.0, nms=nms))
    res = pp.postprocess(torch.from_numpy(g["logit"]).cuda(), on_device=True)
    rows, ref = _flat(res), g["rows_" + nms]
    assert rows.shape == ref.shape
    np.testing.assert_array_equal(rows[:, :2], ref[:, :2])
    np.testing.assert_allclose(rows[:, 2:], ref[:, 2:], rtol=0, atol=5e-5)
    _assert_same_rows(res, pp.postprocess(torch.from_numpy(g["logit"]).cuda()), 5e-5, nms)


# ------------------------------------------------------------------------------------------------ synthetic decodes
def _near_unify_frames(dec, c, thresh, unify):
    """Frames of a host decode [T][G][C+3] with a candidate pair (same class, both passing ``thresh``) whose float64 angular
    distance lies within 1e-3 degree of ``unify``."""
    bad = []
    for f in range(dec.shape[0]):
        fo = dec[f]
        ok = fo[:, 0] > thresh
        for k in range(c):
            sel = fo[ok & (fo[:, 1 + k] > thresh)]
            if len(sel) < 2:
                continue
            r = np.deg2rad(sel[:, -2:].astype(np.float64))
            d = (np.sin(r[:, None, 1]) * np.sin(r[None, :, 1])
                 + np.cos(r[:, None, 1]) * np.cos(r[None, :, 1]) * np.cos(r[:, None, 0] - r[None, :, 0]))
            d = np.rad2deg(np.arccos(np.clip(d, -1.0, 1.0)))
            if (np.abs(d - unify) < 1e-3).any():
                bad.append(f)
                break
    return bad


def _clip(ops, kind, c, t, seed, unify=UNIFY):
    """A decoded synthetic clip on the device, [t][8][4][5][c+3]: 'empty' (no detection at any threshold), 'single' (one
    candidate per class in every frame), 'dense' (random logits, biases -2 / -1 / 0 on the objectness)."""
    rs = np.random.RandomState(seed)
    ch = c + 3
    n = 8 * 4 * 5

    def draw(frames):
        if kind == "empty":
            lg = rs.normal(-12.0, 1.0, size=(frames, n, ch))
        elif kind == "single":
            lg = np.full((frames, n, ch), -12.0)
            lg[..., -2:] = rs.normal(0.0, 1.0, size=(frames, n, 2))
            for f in range(frames):
                a = rs.choice(n, size=c, replace=False)
                lg[f, a, 0] = 6.0
                lg[f, a, 1 + np.arange(c)] = 6.0
        else:
            lg = rs.normal(0.0, 1.5, size=(frames, n, ch))
            lg[..., 0] += np.asarray([-2.0, -1.0, 0.0])[np.arange(frames) % 3][:, None]
        return lg.astype(np.float32)

    lg = draw(t)
    for _ in range(50):
        dev = torch.from_numpy(lg).cuda().view(1, t, -1)
        dec = ops.yolo_decode(dev, c)
        bad = _near_unify_frames(dec.cpu().numpy().reshape(t, n, ch), c, 0.1, unify)
        if not bad:
            return dec
        lg[bad] = draw(len(bad))
    raise AssertionError("could not draw a clip without near-ties at unify_thresh")


THRESHOLDS = [0.1, 0.2, 0.5, 0.9, 0.1 * 3, np.arange(0.1, 1.0, 0.1)[2]]


@pytest.mark.parametrize("c", [12, 13])
@pytest.mark.parametrize("kind", ["empty", "single", "dense"])
def test_device_select_equals_host_select(ops, kind, c):
    """``select_device`` equals ``select`` on the same ``yolo_decode`` output for the three nms modes and thresholds 0.1 .. 0.9,
    a float64 Python threshold (0.1 * 3) and a float64 NumPy one (np.arange, compared in float64 by the host)."""
    from adyolo_amd.postprocess import LabelPostProcessor
    t = 48
    dec = _clip(ops, kind, c, t, seed=100 * c + len(kind))
    host = dec.cpu().numpy()
    total = 0
    for nms in NMS:
        pp = LabelPostProcessor(_params(nb_classes=c, nms=nms))
        for th in THRESHOLDS:
            pp.set_conf_thresh(th)
            ref = pp.select(host)
            got = pp.select_device(dec)
            assert len(got) == 1
            _assert_same_rows(got[0], ref, 5e-5 if th >= 0.3 else 2e-3, "%s C=%d %s thresh %r" % (kind, c, nms, th))
            total += len(_flat(ref))
    if kind == "empty":
        assert total == 0
    elif kind == "single":
        assert total == len(NMS) * len(THRESHOLDS) * t * c                    # sigmoid(6)^2 ~ 0.995 passes every threshold
    else:
        assert total > 1000


def test_device_select_splits_clips(ops):
    """Several clips in one decode: one dict per clip, frames counted from 0 in each; the per-frame counts add up to the rows."""
    from adyolo_amd.postprocess import LabelPostProcessor
    dec = _clip(ops, "dense", 12, 30, seed=7)
    pp = LabelPostProcessor(_params(thresh=0.3))
    rows, counts = ops.yolo_select(dec, 12, 0.3, 0.3, UNIFY, "conn-merge")
    assert rows.is_cuda and counts.is_cuda and counts.dtype == torch.int32 and counts.shape == (30,)
    assert int(counts.sum()) == rows.shape[0] and rows.shape[1] == 5
    fr = rows[:, 0].cpu().numpy()
    assert (np.diff(fr) >= 0).all()
    np.testing.assert_array_equal(np.bincount(fr.astype(np.int64), minlength=30), counts.cpu().numpy())
    host = dec.cpu().numpy()
    got = pp.select_device(dec, n_clips=3)
    for i in range(3):
        _assert_same_rows(got[i], pp.select(host[10 * i:10 * (i + 1)]), 5e-5, "clip %d" % i)


# ------------------------------------------------------------------------------------------------ errors
def test_yolo_select_errors(ops):
    """More candidates per frame and class than ADYOLO_SELECT_MAX_N: ENOSUP, nothing written; bad arguments: EINVAL; a CPU
    tensor is refused."""
    from adyolo_amd import _lib
    lib = _lib.load()
    c, n = 12, 1025
    dec = torch.full((2, n, c + 3), 0.9, device="cuda:0")
    with pytest.raises(_lib.AdyoloHipError, match="rc=-2"):
        ops.yolo_select(dec, c, 0.5, 0.5, UNIFY, "conn-merge")
    ws = torch.full((4096,), 7.0, device="cuda:0")
    rows = torch.full((4096,), 7.0, device="cuda:0")
    counts = torch.full((3,), 7, dtype=torch.int32, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                     # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (p(dec), p(ws), p(rows), p(counts), 2, n, c, 0.5, 0.5, 20.0, 0.5, 1, st)
    assert lib.adyolo_yolo_select(*args) == -2
    assert lib.adyolo_yolo_select(None, *args[1:]) == -1
    assert lib.adyolo_yolo_select(*args[:4], 0, *args[5:]) == -1
    assert lib.adyolo_yolo_select(p(dec), p(ws), p(rows), p(counts), 2, 160, c, 0.5, 0.5, 20.0, 0.5, 3, st) == -1
    torch.cuda.synchronize()
    assert bool((ws == 7.0).all()) and bool((rows == 7.0).all()) and bool((counts == 7).all())
    with pytest.raises(_lib.AdyoloHipError, match="HIP device"):
        ops.yolo_select(torch.zeros(2, 160, c + 3), c, 0.5, 0.5, UNIFY, "conn-merge")


# ------------------------------------------------------------------------------------------------ whole chain
def _rows_csv(path):
    rows = [[float(v) for v in line.strip().split(",")] for line in open(path) if line.strip()]
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), 6)


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
    prm = _params(thresh=float(g["conf_thresh"]), unify=float(g["unify_thresh"]), nms=nms)
    prm["train_config"]["clss_thresh"] = float(g["clss_thresh"])
    prm["data_config"].update(sr=24000, label_hop_len_s=0.1, data_pth=str(tmp_path))
    prm["aug_config"] = {"rotation_augment": False, "spec_augment": False}
    prm["train_config"]["loss_gains"] = {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0}
    model = WrapperModel((1, 7, 400, 64), (), prm)
    fill_module_(model)
    model = model.to("cuda:0").eval()
    fx = FeatureExtractor(load_scaler_npz(os.path.join(G, "scaler_DCASE2021.npz")), "cuda:0")
    return prm, model, fx, cdir, [c[0] for c in CLIPS]


@pytest.mark.parametrize("mode", ["eager", "graphs", "graphs-batched"])
def test_seld_chain_device_select_equals_host_select(ops, tmp_path, mode):
    """``test_epoch_audio(device_select=True)`` writes the CSV lines of the host selection (frame and class equal, in the same
    order; xyz within 5e-5), the same loss and scores within 1e-4: eager, ``ForwardGraphs`` one clip per replay and batched."""
    from adyolo_amd import test as atest
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import ComputeSELDResults
    from adyolo_amd.wrapper import WrapperCriterion
    prm, model, fx, cdir, names = _chain(tmp_path)
    crit, post = WrapperCriterion(prm), LabelPostProcessor(prm)
    ds = FoaDataset(prm, "test", is_valid=True)
    res = {}
    for device_select in (False, True):
        out = os.path.join(tmp_path, "out_%d" % device_select)
        kw = {}
        if mode != "eager":
            kw = {"batch_size": 1 if mode == "graphs" else 4, "forward": ForwardGraphs(model, fx, post, warm_calls=0)}
        loss = atest.test_epoch_audio(ds, model, fx, crit, post, "cuda:0", out, device_select=device_select, **kw)
        scores = np.asarray([float(v) for v in ComputeSELDResults(prm, cdir).get_SELD_Results(out)[:5]])
        res[device_select] = (out, loss, scores)
    (out_h, loss_h, sc_h), (out_d, loss_d, sc_d) = res[False], res[True]
    n = 0
    for name in names:
        h, d = _rows_csv(os.path.join(out_h, name + ".csv")), _rows_csv(os.path.join(out_d, name + ".csv"))
        assert h.shape == d.shape, name
        np.testing.assert_array_equal(d[:, :3], h[:, :3], err_msg=name)
        if len(h):
            assert float(np.abs(d[:, 3:] - h[:, 3:]).max()) <= 5e-5, name
        n += len(h)
    assert n > 0
    assert loss_d == loss_h
    assert np.all(np.abs(sc_d - sc_h) <= 1e-4), (sc_d, sc_h)


@pytest.mark.parametrize("nms", ["conn-merge", "soft-merge"])
def test_sweep_device_select_equals_host_sweep(ops, tmp_path, nms):
    """``sweep_conf_thresh(device_select=True)``: the same new threshold, the same loss and a score table within 1e-4 of the
    host sweep (np.arange thresholds: float64 NumPy scalars)."""
    from adyolo_amd import test as atest
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import ComputeSELDResults
    from adyolo_amd.wrapper import WrapperCriterion
    prm, model, fx, cdir, _ = _chain(tmp_path, nms=nms)
    crit, scorer = WrapperCriterion(prm), ComputeSELDResults(prm, cdir)
    ds = FoaDataset(prm, "test", is_valid=True)
    names = ds.get_filelist()

    class AudioModel:                          # sweep_conf_thresh feeds ``model(feat)``: here feat is the clip's audio
        def eval(self):
            model.eval()

        def __call__(self, audio):
            return model(fx(audio, channels_last8=True), channels_last8=True)
    batches = []
    for i in range(len(ds)):
        pcm, _, rows = ds[i]
        t = (pcm.shape[0] // 600) * 600
        audio = ops.pcm16_to_f32(torch.from_numpy(np.ascontiguousarray(pcm[:t])).cuda()).view(1, t, 4)
        batches.append((audio, audio_collate_fn([(pcm, 0, rows)])[2]))
    got = {}
    for device_select in (False, True):
        post = LabelPostProcessor(prm)
        out = os.path.join(tmp_path, "sweep_%d" % device_select)
        got[device_select] = atest.sweep_conf_thresh(batches, names, AudioModel(), crit, post, scorer, "cuda:0", out,
                                                     device_select=device_select)
        assert post.get_conf_thresh() == got[device_select][0]
    (new_h, table_h, loss_h), (new_d, table_d, loss_d) = got[False], got[True]
    assert new_d == new_h and loss_d == loss_h
    assert np.asarray(table_d).shape == (9, 5)
    assert np.all(np.abs(np.asarray(table_d, dtype=np.float64) - np.asarray(table_h, dtype=np.float64)) <= 1e-4)
    assert len({tuple(r) for r in table_h}) > 1
