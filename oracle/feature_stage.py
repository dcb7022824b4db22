"""Oracle (test infrastructure): cases, inputs and float64 / float32 references of the feature front end's tests
(tests/test_feature_stage_cpu.py pins them on the CPU, tests/test_gpu_feature_stage.py compares csrc/features.hip (K1),
csrc/features_mic.hip (K1m) and csrc/aug.hip with them).  Everything is seeded.

All audio is built the way the product sees it: a float64 signal, int16 quantisation (round, clip to -32768 .. 32767), then
``/ 32768 + 1e-8`` rounded to float32 (datasets.py:147); "PCM zeros" are therefore samples of exactly float32(1e-8).  A case is
a family and a frame count T: a (B, 600 T, 4) batch whose clips differ (B = 1 at the long T).  ``reference(family, t)``
evaluates, per clip, the parts of oracle/features.py in float64 WITHOUT the cast of ``get_feature`` (log-mel in dB, intensity
vector, GCC-PHAT), and the same formulas in float32 on the CPU (``features32``: float32 window, torch.fft.rfft / irfft, matmul
with the float32 mel matrix), which supplies err_ref of ``oracle.checks.value_check``.  ``features32`` takes one of ``ERRORS``:
deliberate mistakes that the CPU module shows the cases reject.

Frame counts: K1 walks FR = 8 frames per workgroup, K1m GR = 4.  2 is the smallest clip the ABI accepts (below one group), 3 a
ragged GR group, 7 / 8 / 9 = FR - 1 / FR / FR + 1, 13 a ragged second group for both; 1027 frames are 4 * 1027 * 64 = 262 912
log-mel values, past the 1024 x 256 lanes of ``feat_finish``, and ragged for both."""
import functools
import math

import numpy as np
import torch

from . import features as ofeat
from .checks import FLOOR, U

FR, GR = 8, 4                                   # frames per workgroup of K1 / K1m
FRAME_COUNTS = (2, 3, 7, 8, 9, 13)
LONG_T = 1027
ALL_T = FRAME_COUNTS + (LONG_T,)
GAINS = (1.0, 0.6, -0.5, 0.3)
FAMILIES = ("plane", "levels", "silence", "fullscale")      # K1 families used at every T
TONE_BINS = (109, 218, 327, 436, 545, 54, 163, 272, 381, 490)
TONES_T = 3
TONE_KEEP_DB = 60.0
# per clip: the delay of each microphone in samples (None: four identical channels).  Pair (m, n) peaks at lag d_n - d_m, lag
# bin 32 + lag: clip 0 reaches bins 35, 1, 49, 46 (-34 and +48 fall outside), clip 2 the mirror image (29, 63, 15, 18), clip 3
# the two end bins themselves (0 and 63) and 33, 62
MIC_DELAYS = ((0, 3, -31, 17), None, (0, -3, 31, -17), (0, -32, 1, 31))
MIC_PEAK_BINS = ((35, 1, 49, None, 46, None), (32,) * 6, (29, 63, 15, None, 18, None), (0, 33, 63, None, None, 62))
CHUNK_SAMPLES = 7800                            # the smallest multiple of 600 that holds a 9-frame window at offset 2345
CHUNK_OFFSETS = (0, 1, 601, 2345)
CHUNK_T = (2, 9)
WELL_CONDITIONED = 8e-6                         # gate on err_ref of every value-checked quantity (a condition on the inputs)
ERRORS = ("reflect", "clip_max", "no_floor", "no_div3", "no_eps", "lag_shift", "pair_sign")
_FAMILY_ID = {"plane": 1, "levels": 2, "silence": 3, "fullscale": 4, "tones": 5, "mic": 6, "chunks": 7}
# cases drawn again, as the well-conditioned gate asks: one bin with a nearly empty cross spectrum decides the float32 oracle's own
# GCC-PHAT error, which came out at 1.0e-5 (T = 2) and 6.4e-6 to 7.0e-6 depending on the host's FFT (T = 3) with the first draw
RESEED = {("mic", 2): 1, ("mic", 3): 1}


# ---------------------------------------------------------------------------------------------------------- audio
def quantise(x):
    """float64 signal -> (int16 PCM, float32 audio as the product sees it)."""
    pcm = np.clip(np.round(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    return pcm, (pcm.astype(np.float64) / 32768.0 + 1e-8).astype(np.float32)


def batch_size(family, t):
    if family == "tones":
        return len(TONE_BINS)
    if family == "chunks" or t == LONG_T:
        return 1
    return len(MIC_DELAYS) if family == "mic" else 2


def levels_variant(t, b):
    """Channel 2 of ``levels``: 0 = loud noise after a silent start, 1 = PCM zeros up to a loud last frame (the long clip and
    every second clip of a batch)."""
    return (b + (t == LONG_T)) % 2


def levels_silent_frames(t, b=0):
    """Frames 0 .. n - 1 of channel 2 are PCM zeros.  Variant 0: one below 7 frames, else a quarter of the clip rounded up.
    Variant 1: all but the last, so that the channel's maximum (positive) comes from the last workgroup alone, a ragged one at
    T = 9, 13 and 1027, every other workgroup reports -100 dB, and the floor max - 80 lifts every silent frame."""
    if levels_variant(t, b):
        return t - 1
    return 1 if t < 7 else int(math.ceil(t / 4.0))


def _signal(family, t, b):
    rng = np.random.default_rng([_FAMILY_ID[family], int(t), int(b), RESEED.get((family, int(t)), 0)])
    n = 600 * t
    g = np.asarray(GAINS)
    if family == "plane":
        w = rng.normal(0.0, 0.1, size=n)
        return w[:, None] * g[None, :] + rng.normal(0.0, 0.01, size=(n, 4)) * np.abs(g)[None, :]     # 10 % of each channel's level
    if family == "levels":
        x = np.zeros((n, 4))
        x[:, 0] = rng.normal(0.0, 0.01, size=n)
        x[(t - 1) * 600:, 0] = rng.normal(0.0, 0.5, size=600)        # only frame T - 1 sees these samples (frame T - 2 ends before)
        x[:, 1] = rng.normal(0.0, 0.01, size=n)
        x[:, 2] = rng.normal(0.0, 0.5 if levels_variant(t, b) else 0.1, size=n)
        x[:600 * levels_silent_frames(t, b) + 1, 2] = 0.0            # frame 0 reads sample 600 through its reflect padding
        return x
    if family == "silence":
        return np.zeros((n, 4))
    if family == "fullscale":
        w = rng.normal(0.0, 1.5, size=n)
        return w[:, None] * g[None, :] + rng.normal(0.0, 0.15, size=(n, 4))
    if family == "tones":
        k = TONE_BINS[b]
        return 0.5 * np.sin(2.0 * np.pi * k * np.arange(n) / 1200.0 + 0.3)[:, None] * g[None, :]
    if family == "mic":
        base = rng.normal(0.0, 0.1, size=n + 128)
        delays = MIC_DELAYS[b]
        if delays is None:
            return np.repeat(base[64:64 + n, None], 4, axis=1)
        return np.stack([base[64 - d:64 - d + n] for d in delays], axis=1) + rng.normal(0.0, 0.001, size=(n, 4))
    if family == "chunks":
        x = rng.normal(0.0, 0.003, size=(CHUNK_SAMPLES, 4))
        for o in CHUNK_OFFSETS:
            x[max(0, o - 200):o] *= 100.0                            # a loud stretch directly before each window start
        return x
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def _case(family, t):
    pcm, audio = quantise(np.stack([_signal(family, t, b) for b in range(batch_size(family, t))]))
    return torch.from_numpy(pcm), torch.from_numpy(audio)


def case_pcm(family, t):
    return _case(family, t)[0].clone()


def case_audio(family, t):
    """-> float32 (B, 600 T, 4); ``chunks``: the (1, 7800, 4) recording whatever t."""
    return _case(family, 0 if family == "chunks" else t)[1].clone()


def chunk_window(offset, t):
    return case_audio("chunks", 0)[0, offset:offset + 600 * t].contiguous()


# ----------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def mel_weights():
    return ofeat.mel_filterbank()                                    # (601, 64) float32


def logmel_unclipped(spec):
    """(T, 601, C) spectrum -> 10 log10(max(1e-10, mel power)) before the top_db floor, (T, 64, C) float64."""
    mag = np.abs(spec) ** 2
    return 10.0 * np.log10(np.maximum(1e-10, np.einsum("tfc,fm->tmc", mag, mel_weights().astype(np.float64))))


def features64(audio):
    """audio (n, 4) float32 / float64 -> float64 log-mel (T, 64, 4) in dB, intensity vector (T, 64, 3), GCC-PHAT (T, 64, 6)."""
    spec = ofeat.stft(np.asarray(audio, dtype=np.float64))
    mw = mel_weights()
    return ofeat.logmel(spec, mw), ofeat.foa_intensity(spec, mw), ofeat.gcc_phat(spec)


def features32(audio, err=None):
    """The same formulas in float32 on the CPU.  audio (n, 4) float32 tensor -> float32 tensors of the shapes above.
    err: None or one of ``ERRORS``, a deliberate mistake."""
    assert err is None or err in ERRORS
    x = audio.float()
    n = x.shape[0]
    t = n // 600
    win = torch.from_numpy(ofeat.hann_periodic().astype(np.float32))
    left = x[0:600] if err == "reflect" else x[1:601]                # reflect index -s - 1 instead of -s
    y = torch.cat([left.flip(0), x], dim=0)                          # (frames 0 .. T - 1 never reach the right padding)
    idx = (torch.arange(t) * 600)[:, None] + torch.arange(1200)[None, :]
    spec = torch.fft.rfft(y[idx] * win[None, :, None], dim=1)        # (T, 601, 4) complex64
    assert spec.dtype == torch.complex64
    mw = torch.from_numpy(mel_weights())
    power = spec.real ** 2 + spec.imag ** 2
    db = 10.0 * torch.log10(torch.clamp(torch.einsum("tfc,fm->tmc", power, mw), min=1e-10))
    if err != "no_floor":
        top = db.amax() if err == "clip_max" else db.amax(dim=(0, 1), keepdim=True)
        db = torch.maximum(db, top - 80.0)
    w = spec[:, :, :1]
    inten = (torch.conj(w) * spec[:, :, 1:]).real
    rest = power[:, :, 1:].sum(-1)
    energy = (0.0 if err == "no_eps" else 1e-8) + (power[:, :, 0] + (rest if err == "no_div3" else rest / 3.0))
    iv = torch.einsum("tfc,fm->tmc", inten / energy[:, :, None], mw)
    gcc = torch.zeros(t, 64, 6)
    p = 0
    for m in range(4):
        for k in range(m + 1, 4):
            r = torch.conj(spec[:, :, m]) * spec[:, :, k]
            if err == "pair_sign" and p == 2:
                r = torch.conj(r)
            cc = torch.fft.irfft(torch.polar(torch.ones_like(r.real), torch.angle(r)), n=1200, dim=1)
            lo = 33 if err == "lag_shift" else 32
            gcc[:, :, p] = torch.cat([cc[:, 1200 - lo:], cc[:, :64 - lo]], dim=-1)
            p += 1
    assert db.dtype == iv.dtype == gcc.dtype == torch.float32
    return db, iv, gcc


def mic_scaler(seed=3):
    """The seeded GCC scaler of test_mic_gcc_phat_features_match_oracle; log-mel unscaled."""
    rng = np.random.default_rng(seed)
    rng.normal(-40, 5, (1, 64, 4)), rng.uniform(5, 15, (1, 64, 4))   # (the draws that test spends on its MEL scaler)
    return {"MEL": {"mean": np.zeros((1, 64, 4)), "std": np.ones((1, 64, 4))},
            "GCC": {"mean": rng.normal(0, 0.01, (1, 64, 6)), "std": rng.uniform(0.05, 0.2, (1, 64, 6))}}


def zscore(q, mean, std):
    """(q - mean) / std in q's precision; q (..., 64, C), mean / std (1, 64, C)."""
    if q.dtype == torch.float64:
        return (q - torch.from_numpy(np.asarray(mean, dtype=np.float64))) / torch.from_numpy(np.asarray(std, dtype=np.float64))
    return (q - torch.from_numpy(np.asarray(mean, dtype=np.float32))) / torch.from_numpy(np.asarray(std, dtype=np.float32))


def reference_of(audio, err=None):
    """audio (B, n, 4) float32 -> {"mel64", "iv64", "gcc64", "mel32", "iv32", "gcc32"}: (B, T, 64, 4 / 3 / 6); the GCC-PHAT
    z-scored with ``mic_scaler``.  With err only the float32 entries, evaluated with that mistake."""
    sc = mic_scaler()["GCC"]
    out = {}
    f32 = [features32(a, err) for a in audio]
    for i, k in enumerate(("mel32", "iv32", "gcc32")):
        out[k] = torch.stack([f[i] for f in f32])
    out["gcc32"] = zscore(out["gcc32"], sc["mean"], sc["std"])
    if err is None:
        f64 = [features64(a.numpy()) for a in audio]
        for i, k in enumerate(("mel64", "iv64", "gcc64")):
            out[k] = torch.from_numpy(np.stack([f[i] for f in f64]))
        out["gcc64"] = zscore(out["gcc64"], sc["mean"], sc["std"])
    return out


@functools.lru_cache(maxsize=None)
def reference(family, t):
    """``reference_of`` of a case, computed once per process.  ``tones`` adds "keep" (B, T, 64, 4): the log-mel entries within
    60 dB of their frame-and-channel maximum, judged on float64 alone (below, a float32 transform's round-off floor decides)."""
    ref = reference_of(case_audio(family, t))
    if family == "tones":
        ref["keep"] = ref["mel64"] >= ref["mel64"].amax(dim=2, keepdim=True) - TONE_KEEP_DB
    return ref


def scaled(ref, scaler):
    """The MEL / IV z-score of a scaler dictionary applied to a reference: -> {"mel64", "iv64", "mel32", "iv32"}."""
    out = {}
    for q, key in (("mel", "MEL"), ("iv", "IV")):
        for p in ("64", "32"):
            out[q + p] = zscore(ref[q + p], scaler[key]["mean"], scaler[key]["std"])
    return out


@functools.lru_cache(maxsize=None)
def chunk_reference(offset, t):
    return reference_of(chunk_window(offset, t)[None])


def quantities(family):
    """The quantities of a family that go through ``value_check``."""
    return {"tones": ("mel",), "mic": ("mel", "gcc"), "silence": ("mel", "iv")}.get(family, ("mel", "iv"))


def rel_err(q, ref64, keep=None):
    """max |q - ref64| / max |ref64|, as ``value_check`` measures it."""
    if not bool(torch.isfinite(q).all()):
        return float("inf")
    d = (q.double() - ref64).abs()
    if keep is not None:
        d = d[keep]
    scale = float(ref64.abs().max())
    return float(d.max()) / scale if scale > 0 else float(d.max())


def bar(err_ref):
    return max(4 * err_ref, FLOOR)


def value_cases():
    """Every (family, T) whose quantities are value-checked."""
    return [(f, t) for f in FAMILIES + ("mic",) for t in ALL_T] + [("tones", TONES_T)]


# ----------------------------------------------------------------------------------------------------------- aug.hip
PCM_SIZES = (1, 7, 8, 9, 8192 * 256 * 8 + 29)      # one thread converts 8 samples as two float4; 8192 x 256 threads at most
ROTATE_SAMPLES = 2048 * 256 + 37                   # foa_rotate: 2048 x 256 lanes per clip at most
COLSTATS_ROWS = (1, 7, 1023, 1024, 1025, 2049)
COLSTATS_COLS = (1, 7, 300, 512)


def pcm_input(n, seed=51):
    """int16 [n], seeded, with -32768, 0, 32767 at the start, across the seam of a thread's two float4 stores (samples 3 .. 5),
    across two threads (7 .. 9), at the first sample of the grid-stride round and at the start of the scalar tail (the last n % 8
    samples; the last three samples where the tail is shorter), wherever n holds them; later placements overwrite earlier ones."""
    g = torch.Generator().manual_seed(seed + n % 1000)
    pcm = torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int32).to(torch.int16)
    special = torch.tensor([-32768, 0, 32767], dtype=torch.int16)
    tail = n - n % 8 if n % 8 >= 3 else n - 3
    for start in (0, 3, 7, 8192 * 256 * 8 - 1, tail):
        for j in range(3):
            if 0 <= start + j < n:
                pcm[start + j] = special[j]
    return pcm


def pcm_reference(pcm):
    """The NumPy formula of datasets.py:147 in float32, as the kernel evaluates it: float32(x) / 32768 (exact) + float32(1e-8)."""
    return torch.from_numpy(pcm.numpy().astype(np.float32) / np.float32(32768.0) + np.float32(1e-8))


def rotate_reference(audio, combinations):
    """audio (B, n, 4), clip b rotated by combinations[b] = ((sy, sz, sx), swap, ...) by tensor indexing."""
    out = audio.clone()
    for b, comb in enumerate(combinations):
        (sy, sz, sx), swap = comb[0], comb[1]
        y, z, x = audio[b, :, 1] * sy, audio[b, :, 2] * sz, audio[b, :, 3] * sx
        out[b, :, 1], out[b, :, 2], out[b, :, 3] = (x, z, y) if swap else (y, z, x)
    return out


def colstats_split(rows):
    """-> (nblk, per, blocks that hold rows) of adyolo_colstats: nblk = min(rows, 1024) workgroups of per = ceil(rows / nblk)
    consecutive rows each."""
    nblk = min(rows, 1024)
    per = -(-rows // nblk)
    return nblk, per, -(-rows // per)


def colstats_input(rows, cols, seed=61):
    """Values like unscaled log-mel: a large common offset (mean about -60), spread about 5."""
    g = torch.Generator().manual_seed(seed + rows + cols)
    return (torch.randn(rows, cols, generator=g) * 5.0 - 60.0).contiguous()


def colstats_reference(a):
    """-> float64 [4][cols] (sum, sum of squares, max, min) and the a-priori bounds [2][cols] on sum and sum of squares.

    The kernel adds the ``per`` rows of a block one after the other in float32 and the blocks in float64.  A running float32 sum
    of n terms is off by at most (n - 1) u sum |x| (the first addition, to 0, is exact; Higham, Accuracy and Stability, 4.2); a
    running sum of squares rounds every one of its n steps (the product and the addition, or the one rounding of a fused
    multiply-add), each by at most u times a partial sum <= sum x^2 (1 + u)^n: n u sum x^2 to first order, taken as
    1.01 n u sum x^2.  The float64 additions across the blocks and of the reference add rows 2^-52 of the same sums."""
    rows, cols = a.shape
    _, per, _ = colstats_split(rows)
    d = a.double()
    ref = torch.stack([d.sum(0), (d * d).sum(0), d.amax(0), d.amin(0)])
    abs_sum, sq_sum = d.abs().sum(0), (d * d).sum(0)
    f64 = rows * 2.0 ** -52
    bound = torch.stack([((per - 1) * U + f64) * abs_sum, (1.01 * per * U + f64) * sq_sum])
    return ref, bound
