"""GPU tests of the feature front end (run with ``-m gpu`` on an MI355X): K1 of csrc/features.hip (STFT, log-mel, intensity vector,
``feat_finish``), K1m of csrc/features_mic.hip (GCC-PHAT) and the input-pipeline kernels of csrc/aug.hip (PCM conversion, column
statistics, FOA rotation), each against a float64 evaluation of the float32 numbers the kernel sees (cases, inputs and references:
oracle/feature_stage.py, pinned on the CPU by tests/test_feature_stage_cpu.py).

Bars, none taken from what a kernel returns (oracle/checks.py):

* value: err = max |q - q64| / max |q64| <= max(4 err_ref, 16 * 2^-24), err_ref the same error of a float32 PyTorch-CPU evaluation
  of the same formulas (torch.fft); one check per quantity and case, each relative to its own float64 absmax, with scaler=None so
  that the figures are dB and raw ratios (the CPU module holds err_ref <= 8e-6 for every one of them);
* sums: |sum - sum64| <= an a-priori bound computed from the inputs (``oracle.feature_stage.colstats_reference``);
* exact: the two layouts, a clip alone and in a batch, two runs, chunk windows against materialised windows, digital silence,
  and everything in aug.hip except the sums.

Every check prints its figures; the ones of an MI355X run stand next to the asserts and in DESIGN.md (K1 / K1m)."""
import os

import numpy as np
import pytest
import torch

from oracle import feature_stage as fs
from oracle.checks import Collect, sum_check, value_check

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K1_CASES = [(f, t) for f in fs.FAMILIES for t in fs.ALL_T]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def fx(ops):
    from adyolo_amd.features import FeatureExtractor
    return FeatureExtractor(None, "cuda:0")


@pytest.fixture(scope="module")
def fx_scaled(ops):
    from adyolo_amd.features import FeatureExtractor, load_scaler_npz
    scaler = load_scaler_npz(os.path.join(G, "scaler_DCASE2021.npz"))
    return FeatureExtractor(scaler, "cuda:0"), scaler


@pytest.fixture(scope="module")
def fx_mic(ops):
    from adyolo_amd.features import MicFeatureExtractor
    return MicFeatureExtractor(fs.mic_scaler(), "cuda:0")


def dev(t):
    return t.to("cuda:0").contiguous()


def k1(fx, audio, **kw):
    """-> log-mel (B, T, 64, 4) and intensity vector (B, T, 64, 3) on the host, from the (B, 7, T, 64) layout."""
    out = fx(dev(audio), channels_last8=False, **kw)
    torch.cuda.synchronize()
    out = out.cpu()
    return out[:, :4].permute(0, 2, 3, 1), out[:, 4:].permute(0, 2, 3, 1)


# ================================================================================================================= K1
@pytest.mark.parametrize("family,t", K1_CASES)
def test_k1_logmel_and_intensity_vector(fx, family, t):
    # MI355X, worst over the T by err_gpu / bar (err_gpu, err_ref, bar).  log-mel: plane 2.1e-7, 1.7e-7, 9.5e-7; levels 3.8e-7, 4.3e-8,
    # 9.5e-7; silence 0; fullscale 2.1e-7, 2.1e-7, 9.5e-7.  Intensity vector: plane 6.3e-6, 2.1e-6, 8.5e-6 (T = 2: 0.73 of the bar,
    # the module's closest); levels 1.1e-6, 6.4e-7, 2.5e-6; silence 6.9e-8, 7.1e-8, 9.5e-7; fullscale 6.7e-7, 4.7e-7, 1.9e-6.
    # Elsewhere in the module: tones 1.4e-6, 3.1e-6, 1.2e-5; chunks 2.3e-7 / 4.1e-7; mic log-mel 2.5e-7, GCC-PHAT 2.4e-6, 1.0e-6, 4.0e-6
    ref = fs.reference(family, t)
    mel, iv = k1(fx, fs.case_audio(family, t))
    col = Collect()
    col(value_check, "%s T %d log-mel" % (family, t), mel, ref["mel64"], ref["mel32"])
    col(value_check, "%s T %d intensity vector" % (family, t), iv, ref["iv64"], ref["iv32"])
    col.finish()


def test_k1_tones_land_in_their_bands(fx):
    """One tone per clip, bins whose digits k1 + 10 k2 + 100 k3 cover every row of the three in-place passes (``fpos``): the
    log-mel entries within 60 dB of their frame-and-channel maximum by value, and the arg-max band of every frame and channel."""
    ref = fs.reference("tones", fs.TONES_T)
    mel, _ = k1(fx, fs.case_audio("tones", fs.TONES_T))
    col = Collect()
    col(value_check, "tones log-mel within 60 dB of the maximum", mel, ref["mel64"], ref["mel32"], keep=ref["keep"])

    def bands():
        assert torch.equal(mel.argmax(dim=2), ref["mel64"].argmax(dim=2)), "a tone's arg-max band differs from float64's"
    col(bands)
    col.finish()


@pytest.mark.parametrize("family", ["plane", "levels"])
def test_k1_with_the_real_scaler(fx_scaled, family):
    """T = 9 once more with tests/golden/scaler_DCASE2021.npz; MEL and IV judged separately, each against its z-scored absmax."""
    fxs, scaler = fx_scaled
    z = fs.scaled(fs.reference(family, 9), scaler)
    mel, iv = k1(fxs, fs.case_audio(family, 9))
    col = Collect()
    col(value_check, "%s T 9 z-scored log-mel" % family, mel, z["mel64"], z["mel32"])
    col(value_check, "%s T 9 z-scored intensity vector" % family, iv, z["iv64"], z["iv32"])
    col.finish()


@pytest.mark.parametrize("family,t", K1_CASES + [("tones", fs.TONES_T)])
def test_k1_layouts_batching_and_reruns_give_the_same_bits(fx, family, t):
    audio = dev(fs.case_audio(family, t))
    nchw = fx(audio, channels_last8=False)
    cl8 = fx(audio, channels_last8=True)
    again = fx(audio, channels_last8=False)
    last = fx(audio[-1:].contiguous(), channels_last8=False)
    torch.cuda.synchronize()
    b = audio.shape[0]
    assert nchw.shape == (b, 7, t, 64) and cl8.shape == (b, t, 64, 8)
    assert torch.equal(cl8[..., :7].permute(0, 3, 1, 2), nchw), "the two layouts differ"
    assert float(cl8[..., 7].abs().max()) == 0.0
    assert torch.equal(again, nchw), "two runs differ"
    assert torch.equal(last[0], nchw[-1]), "a clip alone differs from the same clip in its batch"


@pytest.mark.parametrize("t", fs.ALL_T)
def test_k1_digital_silence_is_the_floor_exactly(fx, fx_scaled, t):
    """PCM zeros: every log-mel entry is 10 log10(1e-10) = -100 dB (the floor -180 does not reach it), z-scored as the kernel
    does, (-100 - mean) * rstd in float32; channel 3 of ``levels`` the same.  The intensity vector is finite (by value: above)."""
    fxs, _ = fx_scaled
    for name, f in (("no scaler", fx), ("real scaler", fxs)):
        want = ((np.float32(-100.0) - f.sc_mean[:4].cpu().numpy()) * f.sc_rstd[:4].cpu().numpy()).T       # (64, 4) float32
        want = torch.from_numpy(np.ascontiguousarray(want))
        mel, iv = k1(f, fs.case_audio("silence", t))
        assert torch.equal(mel, want.expand_as(mel)), "silence, %s: log-mel is not float32((-100 - mean) * rstd)" % name
        assert bool(torch.isfinite(iv).all())
        mel, iv = k1(f, fs.case_audio("levels", t))
        assert torch.equal(mel[..., 3], want[:, 3].expand_as(mel[..., 3])), "levels channel 3, %s" % name
        assert bool(torch.isfinite(iv).all())


@pytest.mark.parametrize("t", fs.CHUNK_T)
def test_k1_chunk_windows_at_odd_offsets(fx, t):
    """``chunk_offsets`` {0, 1, 601, 2345} into one recording, a stretch 100 times louder directly before each window start: the
    bits of the kernel on the materialised window (own reflect padding, own top_db reference), and float64 by value."""
    rec = dev(fs.case_audio("chunks", 0))
    offs = torch.tensor(fs.CHUNK_OFFSETS, dtype=torch.int64, device="cuda:0")
    got = fx(rec, channels_last8=False, chunk_offsets=offs, chunk_samples=600 * t)
    torch.cuda.synchronize()
    assert got.shape == (len(fs.CHUNK_OFFSETS), 7, t, 64)
    col = Collect()
    for i, off in enumerate(fs.CHUNK_OFFSETS):
        same = fx(dev(fs.chunk_window(off, t)[None]), channels_last8=False)
        assert torch.equal(got[i], same[0]), "window at %d differs from the kernel on the materialised window" % off
        ref = fs.chunk_reference(off, t)
        g = got[i:i + 1].cpu()
        col(value_check, "chunk at %d T %d log-mel" % (off, t), g[:, :4].permute(0, 2, 3, 1), ref["mel64"], ref["mel32"])
        col(value_check, "chunk at %d T %d intensity vector" % (off, t), g[:, 4:].permute(0, 2, 3, 1), ref["iv64"], ref["iv32"])
    col.finish()


# ================================================================================================================ K1m
def k1m(fx_mic, audio):
    """-> log-mel (B, T, 64, 4), z-scored GCC-PHAT (B, T, 64, 6), and the (B, T, 64, 32) pixels."""
    a = dev(audio)
    pix = fx_mic(a)
    planes = fx_mic(a, channels_last=False)
    torch.cuda.synchronize()
    assert torch.equal(pix[..., :10].permute(0, 3, 1, 2), planes), "the two layouts differ"
    assert float(pix[..., 10:].abs().max()) == 0.0
    pix = pix.cpu()
    return pix[..., :4], pix[..., 4:10], pix


@pytest.mark.parametrize("t", fs.ALL_T)
def test_k1m_gcc_phat_with_delays_at_the_ends_of_the_lag_window(fx_mic, t):
    """Delayed copies of one source (pair delays -32, -31, +31 among them: lag bins 0, 1, 63, which read transform positions
    N - 32, N - 31 and 31), and four identical channels (a unit peak at lag bin 32); GCC-PHAT z-scored with a seeded scaler."""
    ref = fs.reference("mic", t)
    mel, gcc, pix = k1m(fx_mic, fs.case_audio("mic", t))
    col = Collect()
    col(value_check, "mic T %d log-mel" % t, mel, ref["mel64"], ref["mel32"])
    col(value_check, "mic T %d GCC-PHAT" % t, gcc, ref["gcc64"], ref["gcc32"])

    again = k1m(fx_mic, fs.case_audio("mic", t))[2]
    alone = k1m(fx_mic, fs.case_audio("mic", t)[-1:])[2]
    assert torch.equal(again, pix), "two runs differ"
    assert torch.equal(alone[0], pix[-1]), "a clip alone differs from the same clip in its batch"
    col.finish()


@pytest.mark.parametrize("t", fs.ALL_T)
def test_k1m_digital_silence_is_finite(fx_mic, t):
    """The phase of a zero cross spectrum's round-off is undefined in the reference as well: finite, and the log-mel exact."""
    mel, gcc, _ = k1m(fx_mic, fs.case_audio("silence", t))
    assert bool(torch.isfinite(gcc).all())
    assert bool((mel == -100.0).all())


# ============================================================================================================ aug.hip
@pytest.mark.parametrize("n", fs.PCM_SIZES)
def test_pcm16_to_f32_is_the_numpy_formula_exactly(ops, n):
    pcm = fs.pcm_input(n)
    got = ops.pcm16_to_f32(dev(pcm))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), fs.pcm_reference(pcm))


def test_rotate_audio_all_combinations_past_the_grid(ops):
    from adyolo_amd.augmentations import COMBINATIONS, rotate_audio
    g = torch.Generator().manual_seed(71)
    audio = torch.randn(16, fs.ROTATE_SAMPLES, 4, generator=g)
    got = rotate_audio(dev(audio), list(range(16)))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), fs.rotate_reference(audio, COMBINATIONS))


@pytest.mark.parametrize("rows", fs.COLSTATS_ROWS)
def test_colstats_block_split_and_column_tails(ops, rows):
    col = Collect()
    for cols in fs.COLSTATS_COLS:
        a = fs.colstats_input(rows, cols)
        ref, bound = fs.colstats_reference(a)
        got = ops.colstats(dev(a))
        torch.cuda.synchronize()
        got = got.cpu()
        assert got.dtype == torch.float64 and got.shape == (4, cols)

        def extremes():
            assert torch.equal(got[2:], ref[2:]), "colstats %d x %d: max / min differ" % (rows, cols)
        col(extremes)
        col(sum_check, "colstats %d x %d sum" % (rows, cols), got[0], ref[0], bound[0])
        col(sum_check, "colstats %d x %d sum of squares" % (rows, cols), got[1], ref[1], bound[1])
    col.finish()
