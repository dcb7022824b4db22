"""GPU: the class-wise evaluation path (``--loss seddoa | masked-seddoa | accdoa | adpit``) on the MI355X.

* ``ops.classwise_decode`` (csrc/losses.hip) against the NumPy statement of its record: activities and xyz bit-equal,
  pair distances within 0.05 degree; its error codes.
* ``LabelPostProcessor.postprocess`` on the GPU against the rows of the REAL reference (``postprocess_classwise.npz``).
* The whole ADPIT evaluation chain against the reference run in ``seld_chain_adpit.npz`` (make_golden_classwise.py), like
  test_gpu_seld_chain.py: eager, ``ForwardGraphs`` and batched ``ForwardGraphs``, Winograd and direct convolutions.
* ``sweep_conf_thresh`` equals nine ``test_epoch_audio`` runs; ``train_one_epoch_audio`` with ``loss='adpit'`` from a DCASE
  folder equals ``TrainStep.step`` on the same audio and ``ClasswiseLabelEncoder`` targets, bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, G)
from classwise_decode_np import decode as np_decode  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _random_outputs(loss, c, frames, seed):
    rs = np.random.RandomState(seed)
    w = {"adpit": 9, "accdoa": 3}.get(loss, 4)
    out = rs.uniform(-1.0, 1.0, size=(frames, w * c)).astype(np.float32)
    if loss == "adpit":                            # some tracks nearly or exactly on top of each other, some zero
        v = out.reshape(frames, 3, 3, c)
        v[::3, 1] = v[::3, 0] + rs.uniform(-1e-3, 1e-3, size=v[::3, 0].shape).astype(np.float32)
        v[1::5, 2] = v[1::5, 1]
        v[2::7, 0] = 0.0
    return out


@pytest.mark.parametrize("c", [12, 13])
@pytest.mark.parametrize("loss", ["seddoa", "accdoa", "adpit"])
def test_classwise_decode_matches_numpy(ops, loss, c):
    g = np.load(os.path.join(G, "postprocess_classwise.npz"))
    for out in (g["out_%s_C%d" % (loss, c)][0], _random_outputs(loss, c, 1237, 3 + c)):
        dev = torch.from_numpy(out).cuda()
        got = ops.classwise_decode(dev.view(1, out.shape[0], -1), c, loss).cpu().numpy()
        ref = np_decode(out, loss, c)
        assert got.shape == ref.shape == (out.shape[0], c, 16 if loss == "adpit" else 4)
        n = 12 if loss == "adpit" else 4                                        # activities + xyz
        np.testing.assert_array_equal(_bits(got[..., :n]), _bits(ref[..., :n]))
        if loss == "adpit":
            d = np.abs(got[..., 12:15].astype(np.float64) - ref[..., 12:15])
            assert float(d.max()) <= 0.05, float(d.max())
            assert not got[..., 15].any()


def test_classwise_decode_error_codes(ops):
    from adyolo_amd import _lib
    lib = _lib.load()
    out = torch.zeros(4, 9 * 12, device="cuda:0")
    dec = torch.zeros(4 * 12 * 16 + 4, device="cuda:0")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)                         # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.adyolo_classwise_decode(None, p(dec), 4, 12, 2, st) == -1
    assert lib.adyolo_classwise_decode(p(out), None, 4, 12, 2, st) == -1
    assert lib.adyolo_classwise_decode(p(out), p(dec), 0, 12, 2, st) == -1
    assert lib.adyolo_classwise_decode(p(out), p(dec), 4, 0, 2, st) == -1
    assert lib.adyolo_classwise_decode(p(out), p(dec, 4), 4, 12, 2, st) == -1        # record stores need 16-byte alignment
    assert lib.adyolo_classwise_decode(p(out), p(dec), 4, 12, 3, st) == -2
    assert lib.adyolo_classwise_decode(p(out), p(dec), 4, 12, -1, st) == -2
    assert b"mode" in lib.adyolo_last_error()
    assert lib.adyolo_classwise_decode(p(out), p(dec), 4, 12, 2, st) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.AdyoloHipError):
        ops.classwise_decode(torch.zeros(5, 7, device="cuda:0"), 12, "adpit")       # not whole frames of 9 * C


@pytest.mark.parametrize("c", [12, 13])
@pytest.mark.parametrize("loss", ["seddoa", "masked-seddoa", "accdoa", "adpit"])
def test_postprocess_on_the_gpu_matches_the_reference_rows(ops, loss, c):
    from adyolo_amd.postprocess import LabelPostProcessor
    g = np.load(os.path.join(G, "postprocess_classwise.npz"))
    src = "seddoa" if loss == "masked-seddoa" else loss
    out = torch.from_numpy(g["out_%s_C%d" % (src, c)]).cuda()
    pp = LabelPostProcessor({"args": {"loss": loss}, "data_config": {"nb_classes": c},
                             "train_config": {"conf_thresh": 0.5, "unify_thresh": 15.0}})
    ths = list(g["conf_thresholds"]) + ([] if src == "seddoa" else [float(g["high_thresh"])])
    for i, th in enumerate(ths):
        pp.set_conf_thresh(th)
        for u in (g["unify_thresholds"] if src == "adpit" else (None,)):
            key = "rows_%s_C%d_t%d" % (src, c, i) + ("" if u is None else "_u%d" % int(u))
            if u is not None:
                pp.unify_thresh = float(u)
            res = pp.postprocess(out)
            got = np.asarray([[fr] + [float(v) for v in r] for fr, rr in res.items() for r in rr], dtype=np.float64).reshape(-1, 5)
            ref = g[key]
            assert got.shape == ref.shape, key
            np.testing.assert_array_equal(got[:, :2], ref[:, :2], err_msg=key)
            np.testing.assert_array_equal(_bits(got[:, 2:]), _bits(ref[:, 2:]), err_msg=key)


# ---------------------------------------------------------------------------------------------------- ADPIT chain
def _chain_params(data_pth, g):
    return {"args": {"device": "cuda:0", "encoder": "se-resnet34", "loss": "adpit"},
            "data_config": {"nb_classes": 12, "sr": 24000, "label_hop_len_s": 0.1, "data_pth": str(data_pth)},
            "aug_config": {"rotation_augment": False, "spec_augment": False},
            "train_config": {"conf_thresh": float(g["conf_thresh"]), "unify_thresh": float(g["unify_thresh"])}}


def _rows(path):
    rows = [[float(v) for v in line.strip().split(",")] for line in open(path) if line.strip()]
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), 6)


def _chain_setup(tmp_path, g):
    from scipy.io import wavfile
    from oracle.filler import fill_module_
    from seld_chain_inputs import CLIPS, chain_clip, crc
    from adyolo_amd.wrapper import WrapperModel
    wdir, cdir = os.path.join(tmp_path, "foa_dev", "dev-test"), os.path.join(tmp_path, "metadata_dev", "dev-test")
    os.makedirs(wdir), os.makedirs(cdir)
    for i, (name, seed, n) in enumerate(CLIPS):
        pcm = chain_clip(seed, n)
        assert crc(pcm) == int(g["crc32"][i])
        wavfile.write(os.path.join(wdir, name + ".wav"), 24000, pcm)
        with open(os.path.join(cdir, name + ".csv"), "w") as f:
            for r in g["ref_" + name]:
                f.write("%d,%d,%d,%d,%d\n" % tuple(int(v) for v in r))
    prm = _chain_params(tmp_path, g)
    model = WrapperModel((1, 7, 400, 64), (), prm)
    fill_module_(model)
    return prm, model.to("cuda:0").eval(), cdir, CLIPS


@pytest.mark.parametrize("algo", ["winograd4", "direct"])
@pytest.mark.parametrize("mode", ["eager", "graphs", "graphs-batched"])
def test_adpit_chain_matches_the_reference_run(ops, tmp_path, monkeypatch, mode, algo):
    """Rows as the reference wrote them (frame, class and order exact; xyz and their unit vectors within 5e-3), the mean
    ADPIT loss (1e-3 relative) and ER / F / LE / LR / SELD within 0.01."""
    monkeypatch.setenv("ADYOLO_CONV_ALGO", algo)
    from adyolo_amd import test as atest
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.features import FeatureExtractor, load_scaler_npz
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import ComputeSELDResults
    from adyolo_amd.wrapper import WrapperCriterion
    g = np.load(os.path.join(G, "seld_chain_adpit.npz"))
    prm, model, cdir, clips = _chain_setup(tmp_path, g)
    fx = FeatureExtractor(load_scaler_npz(os.path.join(G, "scaler_DCASE2021.npz")), "cuda:0")
    crit, post = WrapperCriterion(prm), LabelPostProcessor(prm)
    ds = FoaDataset(prm, "test", is_valid=True)
    out = os.path.join(tmp_path, "output_test")
    if mode == "eager":
        loss = atest.test_epoch_audio(ds, model, fx, crit, post, "cuda:0", out)
    else:
        fg = ForwardGraphs(model, fx, post, warm_calls=0)
        loss = atest.test_epoch_audio(ds, model, fx, crit, post, "cuda:0", out, batch_size=1 if mode == "graphs" else 4,
                                      forward=fg)
        assert fg.captures >= 2 and fg.replays >= 2
    assert abs(loss - float(g["mean_loss"])) <= 1e-3 * float(g["mean_loss"]), (loss, float(g["mean_loss"]))
    worst = worst_raw = 0.0
    for name, _, _ in clips:
        got, ref = _rows(os.path.join(out, name + ".csv")), g["pred_" + name]
        assert got.shape == ref.shape, "%s: %d rows, the reference wrote %d" % (name, len(got), len(ref))
        np.testing.assert_array_equal(got[:, :3], ref[:, :3], err_msg=name)              # frame, class, track 0, in order
        unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)                     # noqa: E731
        worst = max(worst, float(np.abs(unit(got[:, 3:]) - unit(ref[:, 3:])).max()))
        worst_raw = max(worst_raw, float(np.abs(got[:, 3:] - ref[:, 3:]).max()))
    # the ADPIT rows are the head's tanh outputs themselves (the AD-YOLO rows are angles of a decoded cell), so the network's
    # own difference from the float32 CPU reference shows in them directly: measured 3.1e-3 (unit vectors) / 3.7e-3 (xyz)
    # with the Winograd convolutions, 1.6e-3 / 1.4e-3 with the direct kernel
    assert worst <= 5e-3 and worst_raw <= 5e-3, "unit vectors differ by %.3e, xyz by %.3e" % (worst, worst_raw)
    res = ComputeSELDResults(prm, cdir).get_SELD_Results(out)
    got = np.asarray([float(v) for v in res[:5]])
    assert np.all(np.abs(got - g["scores"]) <= 0.01), (got, g["scores"])
    print("adpit chain %s/%s: worst unit-vector diff %.2e, xyz diff %.2e, loss %.6f (ref %.6f), scores %s (ref %s)"
          % (mode, algo, worst, worst_raw, loss, float(g["mean_loss"]), got, g["scores"]))


def test_sweep_equals_nine_evaluation_runs(ops, tmp_path):
    """``sweep_conf_thresh`` (network once per file, select per threshold) gives the table of nine ``test_epoch_audio`` runs."""
    from adyolo_amd import test as atest
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.features import FeatureExtractor, load_scaler_npz
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import ComputeSELDResults
    from adyolo_amd.wrapper import WrapperCriterion
    g = np.load(os.path.join(G, "seld_chain_adpit.npz"))
    prm, model, cdir, _ = _chain_setup(tmp_path, g)
    fx = FeatureExtractor(load_scaler_npz(os.path.join(G, "scaler_DCASE2021.npz")), "cuda:0")
    crit, post, scorer = WrapperCriterion(prm), LabelPostProcessor(prm), ComputeSELDResults(prm, cdir)
    ds = FoaDataset(prm, "test", is_valid=True)
    names = ds.get_filelist()

    class AudioModel:                          # sweep_conf_thresh feeds ``model(feat)``: here feat is the clip's audio
        def eval(self):
            model.eval()

        def __call__(self, audio):
            return model(fx(audio, channels_last8=True), channels_last8=True)
    batches = []
    for i in range(len(ds)):
        pcm, _, lab = ds[i]
        t = (pcm.shape[0] // 600) * 600
        audio = ops.pcm16_to_f32(torch.from_numpy(np.ascontiguousarray(pcm[:t])).cuda()).view(1, t, 4)
        batches.append((audio, lab.unsqueeze(0)))
    out = os.path.join(tmp_path, "sweep")
    new, table, loss = atest.sweep_conf_thresh(batches, names, AudioModel(), crit, post, scorer, "cuda:0", out)
    assert post.get_conf_thresh() == new                       # the sweep leaves its choice set
    ths = np.arange(0.1, 1.0, 0.1)
    want, losses = [], []
    for th in ths:
        post.set_conf_thresh(th)
        losses.append(atest.test_epoch_audio(ds, model, fx, crit, post, "cuda:0", out))
        want.append(list(scorer.get_SELD_Results(out)[:5]))
    assert np.asarray(table).shape == (9, 5)
    np.testing.assert_array_equal(np.asarray(table, dtype=np.float64), np.asarray(want, dtype=np.float64))
    assert all(v == losses[0] for v in losses) and loss == losses[0], (loss, losses)
    seld = [r[4] for r in want]
    assert new == ths[int(np.argmin(seld))]
    assert len({tuple(r) for r in want}) > 1                   # the threshold does change the rows


# ---------------------------------------------------------------------------------------------------------- training
@pytest.mark.parametrize("graph", [False, True])
def test_adpit_epoch_from_a_dcase_folder_equals_the_train_steps(ops, tmp_path, graph):
    import random
    from scipy.io import wavfile
    from adyolo_amd.augmentations import rotate_audio, rotate_labels
    from adyolo_amd.datasets import ClasswiseLabelEncoder, FoaDataset, audio_collate_fn
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.train import TrainStep, train_one_epoch_audio
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    rs = np.random.RandomState(4)
    sub = "dev-train-chunked_2s_1s"
    wdir, cdir = os.path.join(tmp_path, "foa_dev", sub), os.path.join(tmp_path, "metadata_dev", sub)
    os.makedirs(wdir), os.makedirs(cdir)
    for i in range(4):
        wavfile.write(os.path.join(wdir, "c%d.wav" % i), 24000, rs.randint(-8000, 8000, size=(48000, 4)).astype(np.int16))
        with open(os.path.join(cdir, "c%d.csv" % i), "w") as f:
            for fr in range(0, 20):
                for src in range(fr % 4):
                    f.write("%d,%d,%d,%d,%d\n" % (fr, (fr + i) % 3 if src else (fr * 5 + i) % 12, src,
                                                  (fr * 41 + i * 90 + src * 77) % 360 - 180, (fr * 7 + src * 13) % 120 - 60))
    prm = {"args": {"device": "cuda:0", "encoder": "se-resnet34", "loss": "adpit"},
           "data_config": {"nb_classes": 12, "sr": 24000, "label_hop_len_s": 0.1, "data_pth": str(tmp_path),
                           "chunk_window_s": 2, "chunk_stride_s": 1},
           "aug_config": {"rotation_augment": True},
           "train_config": {"batch_size": 2, "nb_iters": 2, "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0}}

    def make():
        torch.manual_seed(5)
        model = WrapperModel((1, 7, 80, 64), (), prm).to("cuda:0")
        model.encoder.lstm.dropout = 0.0
        return TrainStep(model, WrapperCriterion(prm), FeatureExtractor(None, "cuda:0"), prm, graph=graph)

    random.seed(3)
    ds = FoaDataset(prm, "train")
    random.seed(21)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=audio_collate_fn, num_workers=0)
    tr = make()
    mean_loss = train_one_epoch_audio(prm, loader, tr)
    torch.cuda.synchronize()
    # by hand: the same files and rotation draws, targets from ClasswiseLabelEncoder on the rotated CSV labels
    random.seed(21)
    tr2 = make()
    enc = ClasswiseLabelEncoder(12)
    losses, combs_seen = [], set()
    for b0 in (0, 2):
        pcms, combs, targets = [], [], []
        for j in (b0, b0 + 1):
            pcm, comb, _ = ds[j]
            label = rotate_labels(FoaDataset.load_csv2dict(os.path.join(cdir, ds.get_filelist()[j] + ".csv")), comb)
            pcms.append(torch.from_numpy(pcm)), combs.append(comb), targets.append(enc.get_adpit_label(label, 20))
        combs_seen.update(combs)
        audio = ops.pcm16_to_f32(torch.stack(pcms).cuda()).view(2, 48000, 4)
        if any(combs):
            audio = rotate_audio(audio, combs)
        losses.append(tr2.step(audio, torch.stack(targets)).clone())
    torch.cuda.synchronize()
    assert combs_seen != {0}
    total = losses[0].reshape(-1)[:1] + losses[1].reshape(-1)[:1]           # summed on the device, as the epoch does
    assert mean_loss == float(total) / 2, (mean_loss, [float(v) for v in losses])
    for (k, p), (_, q) in zip(tr.model.named_parameters(), tr2.model.named_parameters()):
        assert torch.equal(p, q), "parameter %s differs by %.2e" % (k, float((p - q).abs().max()))
    if graph:
        assert tr.graphs.captures == 1 and tr2.graphs.captures == 1
