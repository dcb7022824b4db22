"""CPU: the oracle (oracle/*.py) against the golden vectors generated from the real reference."""
import os
import sys

import numpy as np
import pytest
import torch

import adyolo_amd  # noqa: F401
from oracle import adyolo_loss as oloss
from oracle import features as ofeat
from oracle import labels as olab
from oracle import seresnet as onet
from oracle.filler import fill_state_dict

G = os.path.join(os.path.dirname(__file__), "golden")

EVENTS = {
    0: [[3, 0, 10.0, 5.0]],
    1: [[3, 0, 10.0, 5.0], [7, 1, -170.0, 40.0]],
    2: [[0, 0, 180.0, -30.0], [0, 1, 175.0, -35.0]],
    3: [[11, 0, -180.0, 89.0]],
    4: [[5, 0, 44.9, -90.0], [5, 1, 50.0, -80.0], [2, 2, 47.0, -85.0]],
    5: [[1, 0, 0.0, 90.0]],
    6: [[9, 0, -135.0, 0.0]],
    7: [[4, 0, 120.5, 60.25], [4, 1, 121.0, 59.0], [8, 2, -60.0, -45.0]],
    9: [[6, 0, 20.0, 20.0]],
}


def test_label_rows_match_reference():
    g = np.load(os.path.join(G, "labels.npz"))
    grid = olab.YoloGrid()
    np.testing.assert_array_equal(grid.lb, g["grid_lb"])
    np.testing.assert_array_equal(grid.ub, g["grid_ub"])
    rows = np.asarray(olab.yolo_label({k: [list(e) for e in v] for k, v in EVENTS.items()}, 8), dtype=np.float64)
    np.testing.assert_array_equal(rows, g["rows"])


def test_label_boundary_sweep_matches_reference():
    g = np.load(os.path.join(G, "labels.npz"))
    grid = olab.YoloGrid()
    got = []
    for i, (az, el) in enumerate(g["sweep_in"]):
        for r in olab.yolo_label({0: [[1, 0, float(az), float(el)]]}, 1, grid):
            got.append([i] + [float(v) for v in r])
    np.testing.assert_array_equal(np.asarray(got), g["sweep_rows"])
    # elevation == +90 exactly produces no rows (reference quirk, datasets.py:473)
    assert olab.yolo_label({0: [[1, 0, 0.0, 90.0]]}, 1, grid) == []


def test_collate_matches_reference():
    g = np.load(os.path.join(G, "labels.npz"))
    lab0 = olab.yolo_label({k: [list(e) for e in v] for k, v in EVENTS.items() if k < 3}, 8)
    lab2 = olab.yolo_label({k: [list(e) for e in v] for k, v in EVENTS.items() if 3 <= k < 8}, 8)
    feats = [np.zeros((7, 8, 4)), np.ones((7, 8, 4)), np.full((7, 8, 4), 2.0)]
    feat, target = olab.collate(feats, [lab0, [], lab2])
    assert tuple(feat.shape) == tuple(g["collate_feat_shape"])
    np.testing.assert_array_equal(target, g["collate_target"])
    with pytest.raises(RuntimeError):
        olab.collate(feats, [[], [], []])


@pytest.mark.parametrize("tag,nb_classes", [("c12", 12), ("c13", 13), ("sat", 12)])
def test_loss_matches_reference(tag, nb_classes):
    g = np.load(os.path.join(G, "adyolo_loss.npz"))
    logit = torch.from_numpy(g[tag + "_logit"]).requires_grad_(True)
    target = torch.from_numpy(g[tag + "_target"])
    loss = oloss.adyolo_loss(logit, target, nb_classes)
    assert loss.shape == (1,)
    loss.backward()
    np.testing.assert_allclose(loss.detach().numpy(), g[tag + "_loss"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(logit.grad.numpy(), g[tag + "_dlogit"], rtol=1e-5, atol=1e-8)


def _filled_sd():
    sd = fill_state_dict(onet.state_dict_spec())
    return onet.split_state_dict(sd)


def test_state_dict_spec_counts():
    spec = onet.state_dict_spec()
    enc = [k for k, _ in spec if k.startswith("encoder.")]
    head = [k for k, _ in spec if k.startswith("head.")]
    assert len(enc) == 301 and len(head) == 4
    n_param = sum(int(np.prod(s)) for k, s in spec
                  if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    assert n_param == 6682093        # 5 999 501 + 682 592


def _filled_sd_as(dtype):
    enc, head = _filled_sd()
    cast = lambda sd: {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}   # noqa: E731
    return cast(enc), cast(head)


# encoder.npz holds the reference's float32 outputs; encoder_f64.npz the same modules and inputs in float64.  The float32
# outputs carry the round-off of the CPU and the BLAS / oneDNN kernels they were made with (3e-4 on y_eval, up to 7e-3 of
# absmax on the gradients, where a few ReLU masks flip), which no other machine reproduces element for element.  So the
# oracle is pinned to the reference in float64, where the two agree to 1e-14, and its float32 run must stay within
# float32 round-off of that: the bounds smoke() and the GPU tests hold against the oracle (1e-3 of absmax on outputs,
# 1e-2 on gradients).  encoder_f64.npz keeps 2048 evenly strided elements of every flattened tensor
# (make_golden.strided_sample): the same elements are picked here from the oracle's whole tensor.
F64_RTOL = 1e-9
F64_SAMPLE = 2048


def _sampled(got):
    flat = np.asarray(got, dtype=np.float64).reshape(-1)
    return flat[np.arange(0, flat.size, max(1, flat.size // F64_SAMPLE))[:F64_SAMPLE]]


def _assert_f64(got, ref, what):
    np.testing.assert_allclose(_sampled(got), ref, rtol=F64_RTOL, atol=F64_RTOL * max(1.0, float(np.abs(ref).max())),
                               err_msg=what + " (float64)")


def _assert_f32(got, ref, bound, what):
    dev = float(np.abs(_sampled(got) - ref).max())
    assert dev <= bound * max(1.0, float(np.abs(ref).max())), "%s (float32): %.3e from float64" % (what, dev)


def _encoder_eval(dtype, x):
    enc, head = _filled_sd_as(dtype)
    x = x.to(dtype)
    taps = {}
    with torch.no_grad():
        out = {"y_eval": onet.encoder_forward(enc, x, training=False, taps=taps),
               "y_eval_b1": onet.encoder_forward(enc, x[:1], training=False)}
        out["head_eval"] = onet.adyolo_head(head, out["y_eval"])
    for k in ("stem", "layer1", "layer4"):
        out["tap_eval_" + k] = taps[k][:, :4]
    return {k: v.numpy() for k, v in out.items()}


def test_encoder_eval_matches_reference():
    g32 = np.load(os.path.join(G, "encoder.npz"))
    g = np.load(os.path.join(G, "encoder_f64.npz"))
    x = torch.from_numpy(g32["x"])
    for k, v in _encoder_eval(torch.float64, x).items():
        _assert_f64(v, g[k], k)
    for k, v in _encoder_eval(torch.float32, x).items():
        _assert_f32(v, g[k], 1e-3, k)


def _encoder_train(dtype, g32):
    enc, _ = _filled_sd_as(dtype)
    for k, v in enc.items():
        if v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(True)
    x = torch.from_numpy(g32["x"]).to(dtype).requires_grad_(True)
    y = onet.encoder_forward(enc, x, training=True, update_stats=True)
    (y * torch.from_numpy(g32["probe"]).to(dtype)).sum().backward()
    out = {"y_train": y.detach().numpy(), "dx_train": x.grad.numpy()}
    for key in g32.files:
        if key.startswith("grad_"):
            out[key] = enc[key[5:]].grad.numpy()
        if key.startswith("stat_") and not key.endswith("num_batches_tracked"):
            out[key] = enc[key[5:]].detach().numpy()
    return out


def test_encoder_train_and_grads_match_reference():
    g32 = np.load(os.path.join(G, "encoder.npz"))
    g = np.load(os.path.join(G, "encoder_f64.npz"))
    got64 = _encoder_train(torch.float64, g32)
    assert len(got64) == 2 + sum(k.startswith(("grad_", "stat_")) and not k.endswith("num_batches_tracked") for k in g32.files)
    for k, v in got64.items():
        _assert_f64(v, g[k], k)
    for k, v in _encoder_train(torch.float32, g32).items():
        _assert_f32(v, g[k], 1e-2 if k.startswith(("grad_", "dx_")) else 1e-3, k)


def test_head_grads_match_reference():
    g = np.load(os.path.join(G, "head.npz"))
    _, head = _filled_sd()
    for v in head.values():
        v.requires_grad_(True)
    x = torch.from_numpy(g["x"]).requires_grad_(True)
    y = onet.adyolo_head(head, x)
    (y * torch.from_numpy(g["probe"])).sum().backward()
    np.testing.assert_allclose(y.detach().numpy(), g["y"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(x.grad.numpy(), g["dx"], rtol=1e-4, atol=1e-3)
    for key in g.files:
        if key.startswith("grad_"):
            got = head[key[5:]].grad.numpy().reshape(-1)[:g[key].size]
            np.testing.assert_allclose(got, g[key].reshape(-1), rtol=1e-4, atol=1e-3)


def test_explicit_gru_equals_library_gru():
    enc, _ = _filled_sd()
    torch.manual_seed(3)
    x = torch.randn(2, 9, 256)
    lib = onet._bigru_layer(enc, 0, x)
    fwd = onet.gru_cell_steps(x, enc["lstm.weight_ih_l0"], enc["lstm.weight_hh_l0"],
                              enc["lstm.bias_ih_l0"], enc["lstm.bias_hh_l0"])
    bwd = onet.gru_cell_steps(x, enc["lstm.weight_ih_l0_reverse"], enc["lstm.weight_hh_l0_reverse"],
                              enc["lstm.bias_ih_l0_reverse"], enc["lstm.bias_hh_l0_reverse"], reverse=True)
    np.testing.assert_allclose(lib.numpy(), torch.cat([fwd, bwd], -1).numpy(), rtol=1e-5, atol=1e-6)


# ---- feature pipeline: parity unpinned at the librosa boundary; independent cross-checks only ----

def test_stft_matches_torch_stft():
    rng = np.random.default_rng(5)
    audio = rng.normal(0, 0.1, size=(4800, 2))
    spec = ofeat.stft(audio)
    for ch in range(2):
        ref = torch.stft(torch.from_numpy(audio[:, ch]), n_fft=1200, hop_length=600, win_length=1200,
                         window=torch.hann_window(1200, periodic=True, dtype=torch.float64),
                         center=True, pad_mode="reflect", return_complex=True).numpy()
        np.testing.assert_allclose(spec[:, :, ch], ref.T[:spec.shape[0]], rtol=0, atol=1e-11)


def test_mel_matches_transformers_filter_bank():
    au = pytest.importorskip("transformers.audio_utils")
    ref = au.mel_filter_bank(601, 64, 0.0, 12000.0, 24000, norm="slaney", mel_scale="slaney")
    mel = ofeat.mel_filterbank()
    assert mel.shape == (601, 64) and mel.dtype == np.float32
    np.testing.assert_allclose(mel, ref.astype(np.float32), rtol=0, atol=2e-8)
    assert int((mel != 0).sum()) == 1165            # SURVEY.md section 2 probe


def test_feature_shapes_and_topdb():
    rng = np.random.default_rng(6)
    pcm = np.round(np.clip(rng.normal(0, 0.1, size=(24000, 4)), -1, 1) * 32767).astype(np.int16)
    feat, nlab = ofeat.get_feature(ofeat.int16_to_audio(pcm))
    assert feat.shape == (7, 40, 64) and feat.dtype == np.float32 and nlab == 10
    for ch in range(4):
        assert feat[ch].max() - feat[ch].min() <= 80.0 + 1e-4
    g = np.load(os.path.join(G, "scaler_DCASE2021.npz"))
    assert g["mel_mean"].shape == (1, 64, 4) and g["iv_std"].shape == (1, 64, 3)


def test_logmel_end_to_end_matches_transformers_spectrogram():
    """One independent END-TO-END check of STFT -> |.|^2 -> mel -> power_to_db(top_db=80): transformers' librosa-compatible
    ``spectrogram(..., power=2, center=True, pad_mode='reflect', log_mel='dB', db_range=80)`` with its own Slaney filter
    bank (datasets.py:252-267 + librosa 0.8.1 stft / filters.mel / power_to_db).  This does not pin the oracle to
    librosa (it stays "parity unpinned"), it removes the chance of an error private to the restatement."""
    au = pytest.importorskip("transformers.audio_utils")
    rng = np.random.default_rng(8)
    # a loud burst on a quiet floor: the top_db clip is active (dynamic range > 80 dB)
    audio = rng.normal(0, 1e-5, size=(9600, 2))
    audio[2400:3600] += rng.normal(0, 0.3, size=(1200, 2))
    spec = ofeat.stft(audio)
    mel = ofeat.logmel(spec, ofeat.mel_filterbank())                       # (T, 64, C)
    filt = au.mel_filter_bank(601, 64, 0.0, 12000.0, 24000, norm="slaney", mel_scale="slaney").astype(np.float32)
    win = au.window_function(1200, "hann", periodic=True)
    clipped = 0
    for ch in range(2):
        ref = au.spectrogram(audio[:, ch], win, frame_length=1200, hop_length=600, fft_length=1200, power=2.0, center=True,
                             pad_mode="reflect", onesided=True, mel_filters=filt, mel_floor=1e-10, log_mel="dB",
                             reference=1.0, min_value=1e-10, db_range=None, dtype=np.float64)     # (64, T + 1)
        ref = ref[:, :mel.shape[0]].T
        # the clip is relative to the maximum of the frames the reference keeps (datasets.py:257 drops the last one first)
        ref = np.maximum(ref, ref.max() - 80.0)
        np.testing.assert_allclose(mel[:, :, ch], ref, rtol=0, atol=1e-6)
        clipped += int((mel[:, :, ch] == mel[:, :, ch].max() - 80.0).sum())
    assert clipped > 0, "the test signal must exercise the top_db clip"


def test_power_to_db_hand_computed():
    """librosa.power_to_db(S, ref=1.0, amin=1e-10, top_db=80) on three bins worked by hand: 10 log10(1e3) = 30,
    10 log10(1e-3) = -30, amin floor 10 log10(1e-10) = -100 -> clipped to max - 80 = -50."""
    s = np.array([[1e3, 1e-3, 1e-14]])
    np.testing.assert_allclose(ofeat.power_to_db(s), [[30.0, -30.0, -50.0]], rtol=0, atol=1e-12)
    # without a value within 80 dB of the floor nothing is clipped; the floor itself is amin
    np.testing.assert_allclose(ofeat.power_to_db(np.array([1e-9, 0.0, 1e-12])), [-90.0, -100.0, -100.0], rtol=0, atol=1e-12)
    # the clip follows the maximum of the WHOLE array handed in (one (T, 64) channel of one clip, datasets.py:265)
    two = ofeat.power_to_db(np.array([[1.0, 1e-9], [1e2, 1e-9]]))
    np.testing.assert_allclose(two, [[0.0, -60.0], [20.0, -60.0]], rtol=0, atol=1e-12)


def test_intensity_vector_hand_computed():
    """datasets.py:269-279 on one bin by hand: W = 1+1j, Y = 2, Z = -1j, X = 0: I = Re(conj(W) [Y, Z, X]) = [2, -1, 0],
    E = 1e-8 + |W|^2 + (|Y|^2 + |Z|^2 + |X|^2) / 3 = 1e-8 + 2 + 5/3; an identity 'mel' matrix leaves I / E."""
    spec = np.zeros((1, 1, 4), dtype=np.complex128)
    spec[0, 0] = [1 + 1j, 2.0, -1j, 0.0]
    iv = ofeat.foa_intensity(spec, np.ones((1, 1), dtype=np.float32))
    e = 1e-8 + 2.0 + 5.0 / 3.0
    np.testing.assert_allclose(iv[0, 0], [2.0 / e, -1.0 / e, 0.0], rtol=0, atol=1e-15)


# ---- the other --loss plugins (SEDDOA / masked-SEDDOA / ACCDOA / ADPIT) -------------------------------------
OTHER_EVENTS = {0: [[3, 0, 10.0, 5.0]], 1: [[3, 0, 10.0, 5.0], [7, 1, -170.0, 40.0]],
                2: [[0, 0, 180.0, -30.0], [0, 1, 175.0, -35.0]],
                3: [[5, 0, 44.9, -90.0], [5, 1, 50.0, -80.0], [5, 2, 47.0, -85.0]],
                4: [[2, 0, 1.0, 2.0], [2, 1, 3.0, 4.0], [2, 2, 5.0, 6.0], [2, 3, 7.0, 8.0], [9, 4, -60.0, 30.0]],
                6: [[11, 0, -90.0, 0.0], [4, 1, 90.0, 0.0], [11, 2, 0.0, 45.0]], 9: [[6, 0, 20.0, 20.0]]}


def test_feature_chain_after_the_stft_matches_the_real_reference():
    """a5 / a6 (and the mel product of a4) against the reference's OWN NumPy code: ``features_ref.npz`` was made by the real
    ``FeatureLabelProcessor.get_feature`` / ``get_melscale_foa_intensity_vectors`` / ``get_logmel_spectrogram``
    (datasets.py:260-292) on an injected spectrum with the shipped DCASE2021 scaler (tests/golden/make_golden.py
    ``gen_features_ref``); only librosa's stft / power_to_db / filters.mel were shims there."""
    g = np.load(os.path.join(G, "features_ref.npz"))
    z = np.load(os.path.join(G, "scaler_DCASE2021.npz"))
    scaler = {"MEL": {"mean": z["mel_mean"], "std": z["mel_std"]}, "IV": {"mean": z["iv_mean"], "std": z["iv_std"]}}
    t = int(g["spec_t"])
    spec = ofeat.synthetic_spectrum(int(g["spec_seed"]), t)[:t]          # the cut of datasets.py:257
    mel_wts = ofeat.mel_filterbank()
    np.testing.assert_allclose(ofeat.foa_intensity(spec, mel_wts), g["spec_iv_raw"], rtol=1e-12, atol=1e-15)
    melpow = np.stack([np.dot(np.abs(spec[:, :, c]) ** 2, mel_wts) for c in range(4)], -1)
    np.testing.assert_allclose(melpow, g["spec_melpow"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(ofeat.logmel(spec, mel_wts), g["spec_logmel_raw"], rtol=1e-12, atol=1e-12)
    mel_z, iv_z = ofeat.features_from_spectrum(spec, scaler, mel_wts)
    np.testing.assert_allclose(mel_z, g["spec_mel_z"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(iv_z, g["spec_iv_z"], rtol=1e-11, atol=1e-12)
    assert float(np.abs(g["spec_iv_z"]).max()) > 1.0                      # the z-score (std ~ 0.01) is really exercised
    # audio case: int16 -> /32768 + 1e-8 -> [oracle STFT] -> reference code -> (7, T, 64) float32
    audio = ofeat.int16_to_audio(g["audio_pcm16"])
    feat, nb_label = ofeat.get_feature(audio, scaler, mel_wts)
    assert nb_label == int(g["audio_nb_label_frames"]) == 10 and feat.dtype == np.float32
    np.testing.assert_allclose(feat, g["audio_feat"], rtol=0, atol=1e-6)
    assert int(g["spec_nb_label_frames"]) == t * 600 // 2400


def test_gcc_phat_oracle_finds_the_inter_microphone_delay():
    """GCC-PHAT (MIC features of BASELINE config 5) has no counterpart in the reference -- parity unpinned -- so the oracle's
    restatement of the DCASE2022 baseline definition is pinned by its defining PROPERTY: for microphone n = microphone m
    delayed by d samples, cc of pair (m, n) peaks at lag +d, i.e. at bin 32 + d of concat(cc[-32:], cc[:32]); plus shapes,
    the irfft normalisation (a zero-delay pair peaks at 1.0 for identical channels) and the pair order."""
    rng = np.random.default_rng(7)
    n = 24000
    base = rng.normal(0.0, 0.1, size=n + 64)
    delays = [0, 3, 7, 12]
    audio = np.stack([base[32 - d:32 - d + n] for d in delays], axis=1)           # mic c = base delayed by delays[c]
    spec = ofeat.stft(audio)
    g = ofeat.gcc_phat(spec)
    assert g.shape == (40, 64, 6)
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    for p, (m, k) in enumerate(pairs):
        want = 32 + (delays[k] - delays[m])
        assert (np.argmax(g[5:35, :, p], axis=1) == want).all(), (p, want)
        assert g[5:35, want, p].min() > 0.9                                       # PHAT weighting: a pure delay is a unit impulse
    same = ofeat.gcc_phat(ofeat.stft(np.stack([base[:n]] * 4, axis=1)))
    np.testing.assert_allclose(same[:, 32, :], 1.0, atol=1e-12)
    feat, nb = ofeat.get_feature_mic(audio)
    assert feat.shape == (10, 40, 64) and feat.dtype == np.float32 and nb == 10
    np.testing.assert_allclose(feat[:4], ofeat.get_feature(audio)[0][:4], atol=0)    # the log-mel half is the FOA code on MIC audio


def test_other_label_encoders_match_reference():
    from oracle import other_losses as ool
    from adyolo_amd.datasets import ClasswiseLabelEncoder
    g = np.load(os.path.join(G, "other_losses.npz"))
    ev = lambda: {k: [list(e) for e in v] for k, v in OTHER_EVENTS.items()}   # noqa: E731
    np.testing.assert_array_equal(ool.seddoa_label(ev(), 8, 12), g["label_seddoa"])
    np.testing.assert_array_equal(ool.accdoa_label(ev(), 8, 12), g["label_accdoa"])
    np.testing.assert_array_equal(ool.adpit_label(ev(), 8, 12), g["label_adpit"])
    enc = ClasswiseLabelEncoder(12)
    np.testing.assert_array_equal(enc.get_seddoa_label(ev(), 8).numpy(), g["label_seddoa"])
    np.testing.assert_array_equal(enc.get_accdoa_label(ev(), 8).numpy(), g["label_accdoa"])
    np.testing.assert_array_equal(enc.get_adpit_label(ev(), 8).numpy(), g["label_adpit"])


def test_other_losses_match_reference():
    from oracle import other_losses as ool
    g = np.load(os.path.join(G, "other_losses.npz"))
    cases = [("seddoa", lambda o: ool.seddoa_loss(o, torch.from_numpy(g["sed_target"]), 12, False)),
             ("masked", lambda o: ool.seddoa_loss(o, torch.from_numpy(g["sed_target"]), 12, True)),
             ("accdoa", lambda o: ool.accdoa_loss(o, torch.from_numpy(g["accdoa_target"]))),
             ("adpit", lambda o: ool.adpit_loss(o, torch.from_numpy(g["adpit_target"]), 12))]
    for tag, fn in cases:
        o = torch.from_numpy(g[tag + "_out"]).requires_grad_(True)
        loss = fn(o)
        loss.backward()
        np.testing.assert_allclose(loss.detach().numpy(), g[tag + "_loss"], rtol=1e-5, atol=1e-6, err_msg=tag)
        np.testing.assert_allclose(o.grad.numpy(), g[tag + "_dout"], rtol=1e-4, atol=1e-7, err_msg=tag)


# ---- ResNet-Conformer (config 4) -------------------------------------------------------------------------------
def _conformer_sd():
    g = np.load(os.path.join(G, "conformer.npz"))
    import ast
    from oracle.filler import fill_value
    sd = {}
    for k, shp in zip(g["names"], g["shapes"]):
        sd[str(k)] = fill_value("encoder." + str(k), ast.literal_eval(str(shp)))
    return g, sd


def test_conformer_oracle_matches_reference():
    from oracle import conformer as ocf
    g, sd = _conformer_sd()
    x = torch.from_numpy(g["x"])
    with torch.no_grad():
        y = ocf.encoder_forward(sd, x, training=False)
    np.testing.assert_allclose(y.numpy(), g["y_eval"], rtol=1e-4, atol=5e-5)
    for k, v in sd.items():
        if "running" not in k:
            v.requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    yt = ocf.encoder_forward(sd, xg, training=True)
    (yt * torch.from_numpy(g["probe"])).sum().backward()
    np.testing.assert_allclose(yt.detach().numpy(), g["y_train"], rtol=1e-4, atol=5e-5)
    for key in g.files:
        if key.startswith("grad_"):
            got = sd[key[5:]].grad.numpy().reshape(-1)[:g[key].size]
            ref = g[key].reshape(-1)
            np.testing.assert_allclose(got, ref, rtol=5e-3, atol=5e-3 * max(1e-3, float(np.abs(ref).max())), err_msg=key)


# ---- inference post-processing (decode + NMS) ------------------------------------------------------------------
@pytest.mark.parametrize("nms", ["conn-merge", "soft-merge", "default"])
def test_postprocess_decode_and_nms_match_reference(nms):
    from oracle import postprocess as opp
    from adyolo_amd.postprocess import nms_decoded
    g = np.load(os.path.join(G, "postprocess.npz"))
    dec = opp.decode(g["logit"], 12)
    res = nms_decoded(dec, 12, 0.5, 0.5, 15.0, nms)
    rows = np.asarray([[fr] + [float(x) for x in d] for fr, dets in res.items() for d in dets], dtype=np.float64)
    ref = g["rows_" + nms]
    assert rows.shape == ref.shape
    np.testing.assert_array_equal(rows[:, :2], ref[:, :2])          # frame, class: exact
    np.testing.assert_allclose(rows[:, 2:], ref[:, 2:], rtol=0, atol=2e-5)


# ---- whole evaluation chain -------------------------------------------------------------
def _chain_rows(det):
    return np.asarray(sorted([fr, int(d[0]), float(d[1]), float(d[2]), float(d[3])] for fr, dets in det.items() for d in dets),
                      dtype=np.float64).reshape(-1, 5)


def test_seld_chain_oracle_reproduces_the_reference_run(tmp_path):
    """``seld_chain.npz`` = the REAL reference run end to end on three synthetic clips (WAV -> datasets.Dataset('test') ->
    WrapperModel.eval -> loss -> LabelPostProcessor -> CSV rows -> ComputeSELDResults; make_golden.py::gen_seld_chain).
    Here the CPU side: the clips regenerate bit for bit from their seeds; the oracle chain (features -> float64 encoder +
    head -> label encoder -> loss -> decode) plus the host NMS give the same rows (frame / class exact, xyz 1e-3) and loss; the host SELD metrics on the stored rows give the stored scores."""
    sys.path.insert(0, G)
    from seld_chain_inputs import CLIPS, chain_clip, crc
    from oracle import postprocess as opp
    from oracle import labels as olab
    from adyolo_amd.postprocess import nms_decoded, write_seld_output_file
    from adyolo_amd.features import load_scaler_npz
    from adyolo_amd.seld_metrics import ComputeSELDResults
    g = np.load(os.path.join(G, "seld_chain.npz"))
    scaler = load_scaler_npz(os.path.join(G, "scaler_DCASE2021.npz"))
    enc, head = _filled_sd()
    enc = {k: (v.double() if v.is_floating_point() else v) for k, v in enc.items()}
    head = {k: (v.double() if v.is_floating_point() else v) for k, v in head.items()}
    ct, kt, ut = float(g["conf_thresh"]), float(g["clss_thresh"]), float(g["unify_thresh"])
    ref_dir, out_dir = tmp_path / "ref", tmp_path / "out"
    ref_dir.mkdir(), out_dir.mkdir()
    for i, (name, seed, n) in enumerate(CLIPS):
        pcm = chain_clip(seed, n)
        assert crc(pcm) == int(g["crc32"][i]) and str(g["names"][i]) == name
        with open(ref_dir / (name + ".csv"), "w") as f:
            for r in g["ref_" + name]:
                f.write("%d,%d,%d,%d,%d\n" % tuple(int(v) for v in r))
        pred = g["pred_" + name]
        write_seld_output_file(str(out_dir / (name + ".csv")),
                               {int(fr): [list(r[[1, 3, 4, 5]]) for r in pred[pred[:, 0] == fr]] for fr in np.unique(pred[:, 0])})
        feat, nb_label = ofeat.get_feature(ofeat.int16_to_audio(pcm), scaler)
        idx = np.arange(0, feat.size, max(1, feat.size // 4096))[:4096]
        np.testing.assert_allclose(feat.reshape(-1)[idx], g["feat_sample_" + name], rtol=0, atol=2e-4)
        with torch.no_grad():
            logit = onet.adyolo_head(head, onet.encoder_forward(enc, torch.from_numpy(feat)[None].double(), training=False))
        idx = np.arange(0, logit.numel(), max(1, logit.numel() // 4096))[:4096]
        np.testing.assert_allclose(logit.reshape(-1)[idx].numpy(), g["logit_sample_" + name], rtol=0,
                                   atol=1e-3 * float(g["logit_absmax_" + name]))
        events = {}
        for fr, cls, src, az, el in g["ref_" + name]:
            events.setdefault(int(fr), []).append([int(cls), int(src), float(az), float(el)])
        rows = olab.yolo_label(events, int(nb_label))
        _, target = olab.collate([torch.zeros(1)], [rows])
        target = torch.as_tensor(np.asarray(target, dtype=np.float32))
        np.testing.assert_allclose(target.numpy(), g["target_" + name], rtol=0, atol=1e-5)
        loss = oloss.adyolo_loss(logit.float(), target, 12)
        np.testing.assert_allclose(float(loss), float(g["losses"][i]), rtol=1e-4)
        got = _chain_rows(nms_decoded(opp.decode(logit.float().numpy(), 12), 12, ct, kt, ut, "conn-merge"))
        ref = np.asarray(sorted(pred[:, [0, 1, 3, 4, 5]].tolist()))
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        np.testing.assert_array_equal(got[:, :2], ref[:, :2])
        np.testing.assert_allclose(got[:, 2:], ref[:, 2:], rtol=0, atol=1e-3)
    prm = {"data_config": {"nb_classes": 12, "sr": 24000, "label_hop_len_s": 0.1}}
    res = ComputeSELDResults(prm, str(ref_dir)).get_SELD_Results(str(out_dir))
    np.testing.assert_allclose([float(v) for v in res[:5]], g["scores"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(np.asarray(res[5], dtype=np.float64), g["classwise"], rtol=0, atol=1e-6)
