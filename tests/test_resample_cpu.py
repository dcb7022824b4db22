"""CPU: the host half of sample-rate conversion (ad-yolo_amd/resample.py ``plan``, corpus.py ``load_infer_split(resample=True)`` /
``infer_split_from_arrays(rates=...)``) against a restatement of the definition written here in NumPy int64 (``ref_plan``,
``ref_q23``, ``ref_resample``; tests/test_gpu_resample.py compares the kernel with the same functions for equality): the plan's
numbers and refusals, a constant reproduced exactly, tones against the float64 sine at the output instants, alias rejection,
the loaders on a folder of mixed rates and sample formats, and the ABI of the new entry point.

The tone bounds: an int16 tone of amplitude 20 000 has a rounding floor of 20 log10((1 / sqrt(12)) / (20000 / sqrt(2))) =
-93.8 dB; the source is rounded to int16 once and the output once more, and the filter's own pass-band error lies below both, so
the bound is -86 dB (RMS error over RMS tone), 3 dB above the -89.3 dB a prototype of this design measured at worst.  The alias
bound, -88 dB, stands against a measured -94.3 dB (what is left is the output's rounding)."""
import math
import os
import re
import struct

import numpy as np
import pytest

import adyolo_amd  # noqa: F401
from adyolo_amd import _lib
from adyolo_amd import corpus as C
from adyolo_amd import resample as R

from test_infer_windows_cpu import SR, infer_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_RATES = (48000, 44100, 32000, 16000, 22050, 8000)
ALL_RATES = (8000, 11025, 12000, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 192000)


# ------------------------------------------------------------------------------------------------- the definition, restated
def ref_plan(rate_in, rate_out, zeros=32, beta=9.0, rolloff=0.95):
    g = math.gcd(rate_in, rate_out)
    big_l, big_m = rate_out // g, rate_in // g
    p_max = max(big_l, big_m)
    n, c = 2 * zeros * p_max + 1, zeros * p_max
    fc = rolloff / p_max
    h = np.asarray([big_l * fc * float(np.sinc(fc * (i - c))) for i in range(n)]) * np.kaiser(n, beta)
    k = (n + big_l - 1) // big_l
    taps = np.zeros((big_l, k), dtype=np.int64)
    for p in range(big_l):
        row = np.zeros(k, dtype=np.float64)
        for i, v in enumerate(h[p::big_l]):
            row[i] = v
        row = row / row.sum()
        q = np.rint(row * 2.0 ** 30).astype(np.int64)
        q[int(np.abs(q).argmax())] += 2 ** 30 - int(q.sum())
        taps[p] = q
    return big_l, big_m, k, c, taps


def ref_q23(x):
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.int64) * 256
    if x.dtype == np.int32:
        return x.astype(np.int64) >> 8
    assert x.dtype == np.float32
    v = x.astype(np.float64)
    v = np.where(np.isfinite(v), v, 0.0)
    return np.clip(np.rint(v * 2.0 ** 23), -2.0 ** 23, 2.0 ** 23 - 1).astype(np.int64)


def ref_resample(x, big_l, big_m, k_n, centre, taps):
    """x (n, 4) int16 / int32 / float32 -> int16 (n_out, 4): the definition of adyolo_hip.h, one tap at a time in int64."""
    q = ref_q23(x)
    n = q.shape[0]
    n_out = (n * big_l + big_m - 1) // big_m
    t = np.arange(n_out, dtype=np.int64) * big_m + centre
    p, i0 = t % big_l, t // big_l
    taps = np.asarray(taps, dtype=np.int64)
    acc = np.zeros((n_out, q.shape[1]), dtype=np.int64)
    for k in range(k_n):
        i = i0 - k
        ok = (i >= 0) & (i < n)
        acc[ok] += q[i[ok]] * taps[p[ok], k][:, None]
    y = (acc + (2 ** 37 - 1) + ((acc >> 38) & 1)) >> 38
    return np.clip(y, -32768, 32767).astype(np.int16)


def ref_convert(x, rate_in, rate_out):
    if rate_in == rate_out:
        return ref_resample(x, 1, 1, 1, 0, np.asarray([[2 ** 30]]))
    return ref_resample(x, *ref_plan(rate_in, rate_out))


@pytest.fixture(scope="module")
def plans():
    return {rate: R.plan(rate, SR) for rate in ALL_RATES}


# ------------------------------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("rate", PLAN_RATES)
def test_plan_is_the_definition(plans, rate):
    pl = plans[rate]
    big_l, big_m, k, c, taps = ref_plan(rate, SR)
    g = math.gcd(rate, SR)
    assert (pl["L"], pl["M"]) == (SR // g, rate // g) == (big_l, big_m)
    p_max = max(big_l, big_m)
    assert pl["K"] == k == math.ceil((64 * p_max + 1) / big_l) and pl["centre"] == c == 32 * p_max
    assert pl["taps"].dtype == np.int32 and pl["taps"].shape == (big_l, k) and pl["taps"].flags["C_CONTIGUOUS"]
    assert np.array_equal(pl["taps"].astype(np.int64), taps)
    assert (taps.sum(axis=1) == 2 ** 30).all()                              # DC gain exactly 1 in every phase
    assert taps.max() < 2 ** 31 and taps.min() >= -2 ** 31
    assert np.abs(taps).sum(axis=1).max() <= 3 * 2 ** 30                    # |acc| <= 2^23 * 3 * 2^30 < 2^55: no int64 overflow
    assert R.n_out(1001, big_l, big_m) == (1001 * big_l + big_m - 1) // big_m


def test_plan_numbers_for_the_usual_rates_and_refusals(plans):
    assert [(plans[r]["L"], plans[r]["M"], plans[r]["K"]) for r in (48000, 44100, 32000, 16000, 8000, 11025)] == \
        [(1, 2, 129), (80, 147, 118), (3, 4, 86), (3, 2, 65), (3, 1, 65), (320, 147, 65)]
    assert plans[11025]["taps"].nbytes == 320 * 65 * 4                      # the largest table plan() makes
    for rate in ALL_RATES:                                                  # every standard rate has a plan that cannot overflow
        taps = plans[rate]["taps"].astype(np.int64)
        assert (taps.sum(axis=1) == 2 ** 30).all() and np.abs(taps).sum(axis=1).max() <= 3 * 2 ** 30
    with pytest.raises(ValueError, match="24000.*24000"):
        R.plan(SR, SR)
    with pytest.raises(ValueError, match="44100.*16000"):                   # 441 / 160: P = 441
        R.plan(44100, 16000)
    with pytest.raises(ValueError):
        R.plan(0, SR)
    fmt = R.plan_for(SR, SR)
    assert (fmt["L"], fmt["M"], fmt["K"], fmt["centre"], fmt["taps"].tolist()) == (1, 1, 1, 0, [[2 ** 30]])
    assert R.plan_for(48000, SR)["K"] == 129


# --------------------------------------------------------------------------------------------------------- what it computes
@pytest.mark.parametrize("rate", PLAN_RATES)
def test_a_constant_comes_back_exactly(plans, rate):
    pl = plans[rate]
    n = 13 * pl["K"] * pl["M"] // pl["L"] + 1                               # about 13 K output frames
    y = ref_resample(np.full((n, 4), 12345, dtype=np.int16), pl["L"], pl["M"], pl["K"], pl["centre"], pl["taps"])
    edge = 4 * pl["K"]
    assert y.shape[0] > 3 * edge and (y[edge:-edge] == 12345).all()


def _tone(rate, freq, seconds=0.5, amp=20000.0):
    t = np.arange(int(rate * seconds), dtype=np.float64) / rate
    return np.rint(amp * np.sin(2 * np.pi * freq * t)).astype(np.int16)


def _db(err, ref):
    return 10 * math.log10(float(np.mean(np.square(err))) / float(np.mean(np.square(ref))))


@pytest.mark.parametrize("rate", ALL_RATES)
def test_tones_come_out_as_the_sine_at_the_output_instants(plans, rate):
    pl = plans[rate]
    nyq = min(rate, SR) / 2.0
    for freq in (1000.0, 0.70 * nyq, 0.84 * nyq):
        x = _tone(rate, freq)
        y = ref_resample(x[:, None], pl["L"], pl["M"], pl["K"], pl["centre"], pl["taps"])[:, 0]
        want = 20000.0 * np.sin(2 * np.pi * freq * np.arange(y.shape[0], dtype=np.float64) / SR)
        assert y.shape[0] == R.n_out(x.shape[0], pl["L"], pl["M"]) > 1000
        db = _db(y[200:-200].astype(np.float64) - want[200:-200], want[200:-200])
        print("rate %d tone %.0f Hz: %.1f dB" % (rate, freq, db))
        assert db <= -86.0, (rate, freq, db)


def test_a_tone_above_the_new_nyquist_is_rejected(plans):
    pl = plans[44100]
    x = _tone(44100, 13500.0)
    y = ref_resample(x[:, None], pl["L"], pl["M"], pl["K"], pl["centre"], pl["taps"])[:, 0]
    db = 10 * math.log10(float(np.mean(np.square(y[200:-200].astype(np.float64)))) / (20000.0 ** 2 / 2))
    print("13.5 kHz in 44.1 kHz -> 24 kHz: %.1f dB" % db)
    assert db <= -88.0, db


def test_the_sample_formats_agree_where_they_hold_the_same_value():
    rs = np.random.RandomState(3)
    x16 = rs.randint(-32768, 32768, size=(700, 4)).astype(np.int16)
    x32 = x16.astype(np.int32) << 16                                        # the same values as 24-bit PCM, left-justified
    xf = (x16.astype(np.float64) / 32768.0).astype(np.float32)
    want = ref_convert(x16, 48000, SR)
    assert np.array_equal(ref_convert(x32, 48000, SR), want) and np.array_equal(ref_convert(xf, 48000, SR), want)
    assert np.array_equal(ref_convert(x32, SR, SR), x16) and np.array_equal(ref_convert(xf, SR, SR), x16)
    # the float rule: ties to even, the clamp, non-finite as 0
    f = np.asarray([0.5, 1.5, 2.5, -0.5, -1.5], dtype=np.float64) * 2.0 ** -23
    assert ref_q23(f.astype(np.float32)).tolist() == [0, 2, 2, 0, -2]
    assert ref_q23(np.asarray([1.0, -1.0, 7.0, np.nan, np.inf], dtype=np.float32)).tolist() == [2 ** 23 - 1, -2 ** 23, 2 ** 23 - 1, 0, 0]


# ----------------------------------------------------------------------------------------------------------- the loaders
def write_wav24(path, rate, data):
    """int32 (n, c) holding 24-bit values left-justified -> a 24-bit PCM WAV file (scipy reads it back as those int32)."""
    n, c = data.shape
    raw = (data.astype("<i4") >> 8).astype("<i4").view(np.uint8).reshape(n, c, 4)[:, :, :3].tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, c, rate, rate * c * 3, c * 3, 24))
        f.write(b"data" + struct.pack("<I", len(raw)) + raw)


def write_mixed_folder(root, seed=21):
    """One int16 file at SR, one int16 file at 2 SR, one float32 file at 44 100 Hz, one 24-bit file at SR -> {name: (rate, data)}."""
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    os.makedirs(str(root), exist_ok=True)
    out = {"a_native": (SR, rs.randint(-8000, 8000, size=(4800 + 7, 4)).astype(np.int16)),
           "b_double": (2 * SR, rs.randint(-8000, 8000, size=(9600 + 5, 4)).astype(np.int16)),
           "c_float": (44100, (rs.randint(-8000, 8000, size=(4410 + 3, 4)) / 32768.0).astype(np.float32)),
           "d_24bit": (SR, (rs.randint(-2 ** 21, 2 ** 21, size=(2400 + 1, 4)) << 8).astype(np.int32))}
    for name, (rate, data) in out.items():
        if data.dtype == np.int32:
            write_wav24(os.path.join(str(root), name + ".wav"), rate, data)
        else:
            wavfile.write(os.path.join(str(root), name + ".wav"), rate, data)
    return out


def test_load_infer_split_reads_rates_and_formats(tmp_path):
    from scipy.io import wavfile
    written = write_mixed_folder(tmp_path)
    prm = infer_params(tmp_path)
    hc = C.load_infer_split(prm, rank=0, world=1, verify="all", resample=True)
    names = hc.filelist
    assert sorted(names) == sorted(written) and hc.set_type == "infer" and hc.hop_label == 2400
    want_len = {"a_native": 4807, "b_double": (9605 + 1) // 2, "c_float": (4413 * 80 + 146) // 147, "d_24bit": 2401}
    assert hc.lengths.tolist() == [want_len[n] for n in names]
    assert hc.native_lengths.tolist() == [written[n][1].shape[0] for n in names]
    assert hc.rates.tolist() == [written[n][0] for n in names]
    assert hc.kinds.tolist() == [{"a_native": 0, "b_double": 0, "c_float": 2, "d_24bit": 1}[n] for n in names]
    assert hc.rec_start[0] == 0 and hc.audio.dtype == np.int16 and hc.rec_start[-1] <= hc.audio.shape[0]
    for i, name in enumerate(names):
        s0, n = int(hc.rec_start[i]), int(hc.lengths[i])
        assert s0 % 16 == 0 and int(hc.rec_start[i + 1]) == s0 + (n + 15) // 16 * 16
        if name == "a_native":                                              # today's bytes, and nothing kept beside them
            assert np.array_equal(hc.audio[s0:s0 + n], written[name][1]) and hc.native[i] is None
        else:                                                               # a zeroed place; the samples wait on the host
            assert not hc.audio[s0:int(hc.rec_start[i + 1])].any()
            assert hc.native[i].dtype == written[name][1].dtype and np.array_equal(hc.native[i], written[name][1])
    kept = sum(written[n][1].nbytes for n in names if n != "a_native")
    assert hc.nbytes() == hc.audio.nbytes + hc.events.nbytes + kept         # the host footprint counts the native samples
    same = C.infer_split_from_arrays(names, [written[n][1] for n in names], prm, rates=[written[n][0] for n in names])
    assert same.lengths.tolist() == hc.lengths.tolist() and same.rec_start.tolist() == hc.rec_start.tolist()
    assert np.array_equal(same.audio, hc.audio) and same.kinds.tolist() == hc.kinds.tolist()
    # without the keyword the folder is refused as before: by the first file that is not int16
    with pytest.raises(ValueError):
        C.load_infer_split(prm, rank=0, world=1)
    with pytest.raises(ValueError, match=r"c_float\.wav"):
        C.load_infer_split(prm, rank=0, world=1, files=["a_native", "c_float"])
    plain = C.infer_split_from_arrays(["a"], [written["a_native"][1]], prm)
    assert plain.native is None and plain.rates is None
    # refused by path: two channels, float64, a rate beyond the plan
    wavfile.write(str(tmp_path / "e_stereo.wav"), 48000, np.zeros((480, 2), dtype=np.int16))
    with pytest.raises(ValueError, match=r"e_stereo\.wav"):
        C.load_infer_split(prm, rank=0, world=1, resample=True)
    os.remove(str(tmp_path / "e_stereo.wav"))
    wavfile.write(str(tmp_path / "f_double.wav"), 48000, np.zeros((480, 4), dtype=np.float64))
    with pytest.raises(ValueError, match=r"f_double\.wav"):
        C.load_infer_split(prm, rank=0, world=1, resample=True)
    os.remove(str(tmp_path / "f_double.wav"))
    wavfile.write(str(tmp_path / "g_odd.wav"), 44101, np.zeros((480, 4), dtype=np.int16))
    with pytest.raises(ValueError, match=r"g_odd\.wav.*44101"):
        C.load_infer_split(prm, rank=0, world=1, resample=True)
    os.remove(str(tmp_path / "g_odd.wav"))
    assert C.load_infer_split(prm, rank=0, world=1, resample=True, files=["b_double"]).lengths.tolist() == [4803]
    with pytest.raises(ValueError, match="odd_rate.*44101"):
        C.infer_split_from_arrays(["odd_rate"], [written["a_native"][1]], prm, rates=[44101])
    with pytest.raises(ValueError, match="wide"):
        C.infer_split_from_arrays(["wide"], [written["a_native"][1].astype(np.float64)], prm, rates=[SR])
    with pytest.raises(ValueError):
        C.infer_split_from_arrays(["a", "b"], [written["a_native"][1]] * 2, prm, rates=[SR])


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_the_new_symbol_is_declared_bound_and_wrapped():
    from adyolo_amd import ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adyolo_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    assert "adyolo_resample_pcm" in _lib.SIGNATURES and re.search(r"\badyolo_resample_pcm\s*\(", hdr)
    assert lib.adyolo_resample_pcm is not None and callable(ops.resample_pcm) and callable(R.resample_device)
    assert "#define ADYOLO_RESAMPLE_WORDS 4" in hdr and ops.RESAMPLE_WORDS == 4
    tile = int(re.search(r"#define ADYOLO_RESAMPLE_TILE\s+(\d+)", hdr).group(1))
    assert ops.RESAMPLE_TILE == tile
    for name, kind in (("INT16", 0), ("INT32", 1), ("FLOAT32", 2)):
        assert int(re.search(r"#define ADYOLO_RESAMPLE_%s\s+(\d+)" % name, hdr).group(1)) == kind
    import torch
    assert ops.RESAMPLE_KINDS == {torch.int16: 0, torch.int32: 1, torch.float32: 2}
    assert {np.dtype(k).name: v for k, v in R.KINDS.items()} == {"int16": 0, "int32": 1, "float32": 2}
    bit = int(re.search(r"#define ADYOLO_CORPUS_NONFINITE\s+(\d+)", hdr).group(1))
    assert bit == 8 and any(b == bit for b, _ in ops.CORPUS_STATUS)
    assert "resample.hip" in open(os.path.join(ROOT, "ad-yolo_amd", "build.py")).read()
    with pytest.raises(_lib.AdyoloHipError):                                # a host tensor is refused by the wrapper
        ops.resample_pcm(torch.zeros((8, 4), dtype=torch.int16), torch.zeros((1, 4), dtype=torch.int64),
                         torch.zeros((1, 129), dtype=torch.int32), 2, 64, torch.zeros((4, 4), dtype=torch.int16),
                         torch.zeros(1, dtype=torch.int32))
    x = torch.zeros((8, 4), dtype=torch.int16)
    assert R.resample_device(x, SR, SR) is x                                # equal rates, int16: the input itself
    with pytest.raises(ValueError):
        R.resample_device(torch.zeros((8, 2), dtype=torch.int16), 48000, SR)
