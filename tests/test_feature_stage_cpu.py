"""CPU tests of the cases and references behind tests/test_gpu_feature_stage.py (oracle/feature_stage.py): shapes and seeds, that
every case contains what it is there for (judged on the float64 reference alone), that the float32 CPU evaluation agrees with
float64 well enough to keep the GPU module's bar at float32 level (the well-conditioned gate), that the cases reject seven
deliberate mistakes, and the grid arithmetic the sizes were chosen for.  Every condition prints its figure."""
import os

import numpy as np
import pytest
import torch

import adyolo_amd  # noqa: F401  (import shim at the repo root)
from oracle import feature_stage as fs
from oracle import features as ofeat

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K1_CASES = [(f, t) for f in fs.FAMILIES for t in fs.ALL_T]


def golden_scaler():
    from adyolo_amd.features import load_scaler_npz
    return load_scaler_npz(os.path.join(G, "scaler_DCASE2021.npz"))


# ------------------------------------------------------------------------------------------------- tables and inputs
def test_product_and_oracle_mel_matrices_are_bit_equal():
    from adyolo_amd.features import slaney_mel_matrix
    prod, orc = slaney_mel_matrix(), ofeat.mel_filterbank()
    assert prod.dtype == orc.dtype == np.float32 and prod.shape == (64, 601) and orc.shape == (601, 64)
    assert np.array_equal(prod.T, orc)
    assert bool((orc[0] == 0).all()) and int((orc > 0).sum()) == 1165       # bin 0 belongs to no filter; K1's 1165 weights


@pytest.mark.parametrize("family,t", K1_CASES + [("mic", t) for t in fs.ALL_T] + [("tones", fs.TONES_T), ("chunks", 0)])
def test_inputs_are_seeded_pcm_audio_whose_clips_differ(family, t):
    audio, pcm = fs.case_audio(family, t), fs.case_pcm(family, t)
    b, n = fs.batch_size(family, t), fs.CHUNK_SAMPLES if family == "chunks" else 600 * t
    assert audio.shape == pcm.shape == (b, n, 4) and audio.dtype == torch.float32 and pcm.dtype == torch.int16
    assert torch.equal(audio, fs._case.__wrapped__(family, t)[1])                        # a second build: the same bits
    assert np.array_equal(audio.numpy(), (pcm.numpy().astype(np.float64) / 32768.0 + 1e-8).astype(np.float32))
    if family != "silence":
        assert all(not torch.equal(audio[i], audio[j]) for i in range(b) for j in range(i))
    assert (b == 1) == (t == fs.LONG_T or family == "chunks")


def test_frame_counts_and_grid_arithmetic():
    """What the sizes were chosen for: the frame groups of K1 (FR = 8) and K1m (GR = 4), feat_finish's 1024 x 256 lanes,
    pcm16_to_f32's 8192 x 256 threads of 8 samples, foa_rotate's 2048 x 256 lanes, colstats' block split."""
    assert fs.FRAME_COUNTS == (2, 3, 7, 8, 9, 13) and fs.LONG_T == 1027
    assert 2 < fs.GR and 3 % fs.GR and 7 == fs.FR - 1 and 9 == fs.FR + 1 and 13 > fs.FR and 13 % fs.FR and 13 % fs.GR
    assert 4 * 1027 * 64 > 1024 * 256 >= 4 * 1024 * 64 and 1027 % fs.FR and 1027 % fs.GR
    n = fs.PCM_SIZES[-1]
    assert -(-n // 8) == 8192 * 256 + 4 and n % 8 == 5                  # 4 threads' worth in the second round, the last a tail
    assert fs.ROTATE_SAMPLES == 2048 * 256 + 37
    split = {r: fs.colstats_split(r) for r in fs.COLSTATS_ROWS}
    print("colstats rows -> (workgroups, rows each, workgroups that hold rows):", split)
    assert split == {1: (1, 1, 1), 7: (7, 1, 7), 1023: (1023, 1, 1023), 1024: (1024, 1, 1024), 1025: (1024, 2, 513),
                     2049: (1024, 3, 683)}
    assert any(c % 256 for c in fs.COLSTATS_COLS) and 300 > 256 and 512 in fs.COLSTATS_COLS
    for off in fs.CHUNK_OFFSETS:
        assert off + 600 * max(fs.CHUNK_T) <= fs.CHUNK_SAMPLES
    assert any(off % 600 for off in fs.CHUNK_OFFSETS) and fs.CHUNK_SAMPLES - 600 < 2345 + 600 * 9


# --------------------------------------------------------------------------------------- what each case is there for
@pytest.mark.parametrize("t", fs.ALL_T)
def test_plane_is_coherent(t):
    """The float64 intensity vector's mean per channel has the sign of its gain and exceeds half that channel's absmax."""
    iv = fs.reference("plane", t)["iv64"]
    for c in range(3):
        mean, top = float(iv[..., c].mean()), float(iv[..., c].abs().max())
        print("plane T %d: IV channel %d (gain %+.1f) mean %+.4f, absmax %.4f" % (t, c, fs.GAINS[c + 1], mean, top))
        assert np.sign(mean) == np.sign(fs.GAINS[c + 1]) and abs(mean) > 0.5 * top


@pytest.mark.parametrize("t", fs.ALL_T)
def test_levels_make_the_clip_and_the_maximum_decide(t):
    audio = fs.case_audio("levels", t)
    pcm_zero = float(np.float32(1e-8))
    for b in range(audio.shape[0]):
        spec = ofeat.stft(audio[b].double().numpy())
        raw = fs.logmel_unclipped(spec)                                   # (T, 64, 4) before the floor
        mel = fs.reference("levels", t)["mel64"][b].numpy()
        top = raw.max(axis=(0, 1))
        changed = (raw < top - 80.0).mean(axis=(0, 1)).tolist()
        assert float(np.abs(mel - np.maximum(raw, top - 80.0)).max()) < 1e-10
        silent = [k for k in range(t) if bool((audio[b, max(0, 600 * (k - 1)):600 * (k + 1) + (k == 0), 2] == pcm_zero).all())]
        print("levels T %d clip %d: channel maxima %s dB; channel 0's maximum in frame %d; share of entries the floor changes %s; "
              "channel 2: %d of %d frames PCM zeros" % (t, b, np.round(top, 2).tolist(), int(raw[:, :, 0].max(axis=1).argmax()),
                                                         np.round(changed, 4).tolist(), len(silent), t))
        assert top[0] > 0 and int(raw[:, :, 0].max(axis=1).argmax()) == t - 1 and bool((raw[:t - 1, :, 0] < 0).all())
        assert top[1] < 0
        assert top[2] > -20.0 and changed[0] == 0.0 and changed[1] == 0.0
        assert len(silent) == fs.levels_silent_frames(t, b) and bool((raw[silent, :, 2] == -100.0).all())
        if t != 2:                                                        # T = 2: one silent frame, the share is a printed figure
            assert len(silent) >= 0.25 * t and changed[2] >= 0.10
        if fs.levels_variant(t, b):                                       # the maximum is positive and the last frame's alone
            assert top[2] > 0 and bool((raw[:t - 1, :, 2] == -100.0).all()) and changed[2] == (t - 1.0) / t
        assert bool((audio[b, :, 3] == pcm_zero).all()) and bool((mel[:, :, 3] == -100.0).all())
    if t in (9, 13):                                                      # channel 0's maximum comes from the ragged group
        assert (t - 1) // fs.FR == 1 and t % fs.FR


def test_the_round_one_feature_test_input_and_its_pcm_zero_frames():
    """``test_features_match_oracle`` scaled one channel by 1e-4 "so the top_db clip actually bites": the floor is per clip and
    channel, so it changed nothing.  With a stretch of PCM zeros in a loud channel (what that test uses now) it does."""
    from adyolo_amd.datasets import synthetic_audio
    audio = synthetic_audio(2, 24000 * 2, seed=9)
    audio[1, :, 2] *= 1e-4
    share = {}
    for name in ("as it was", "with PCM zeros"):
        if name == "with PCM zeros":
            audio[1, 6000:12000, 0] = float(np.float32(1e-8))
        for b in range(2):
            spec = ofeat.stft(audio[b].double().numpy())
            raw = fs.logmel_unclipped(spec)
            share[name, b] = (raw < raw.max(axis=(0, 1)) - 80.0).mean(axis=(0, 1)).tolist()
            print("test_features_match_oracle input %s, clip %d: share of entries the top_db floor changes per channel %s" % (
                name, b, np.round(share[name, b], 4).tolist()))
    assert all(s == 0.0 for b in range(2) for s in share["as it was", b])
    assert share["with PCM zeros", 1][0] > 0.10


@pytest.mark.parametrize("t", fs.ALL_T)
def test_silence_is_pcm_zeros_and_minus_100_db(t):
    audio, ref = fs.case_audio("silence", t), fs.reference("silence", t)
    assert bool((audio == float(np.float32(1e-8))).all()) and bool((fs.case_pcm("silence", t) == 0).all())
    assert bool((ref["mel64"] == -100.0).all()) and bool((ref["mel32"] == -100.0).all())
    print("silence T %d: float64 IV absmax %.3e (1e-8 of E decides it)" % (t, float(ref["iv64"].abs().max())))
    assert 0 < float(ref["iv64"].abs().max()) < 1e-4


@pytest.mark.parametrize("t", fs.ALL_T)
def test_fullscale_holds_both_rails(t):
    pcm = fs.case_pcm("fullscale", t)
    rails = float(((pcm == -32768) | (pcm == 32767)).float().mean())
    print("fullscale T %d: %.1f %% of the samples sit on a rail" % (t, 100 * rails))
    assert int(pcm.min()) == -32768 and int(pcm.max()) == 32767 and rails > 0.10
    assert float(fs.case_audio("fullscale", t).max()) == float(np.float32(32767 / 32768.0 + 1e-8))


def test_tones_hit_every_digit_row_and_keep_their_bands():
    ks = fs.TONE_BINS
    assert {k % 10 for k in ks} == set(range(10)) and {k // 10 % 10 for k in ks} == set(range(10))
    assert {k // 100 for k in ks} == set(range(6)) and max(ks) <= 600
    ref, mw = fs.reference("tones", fs.TONES_T), fs.mel_weights()
    kept = ref["keep"].sum(dim=2)                                         # (B, T, 4)
    top = ref["mel64"].argmax(dim=2)
    print("tones: bands kept per frame and channel %d .. %d of 64; %d of %d entries compared" % (
        int(kept.min()), int(kept.max()), int(ref["keep"].sum()), ref["keep"].numel()))
    # (the issue asked for 3: a tone on a bin leaves power in bins k - 1, k, k + 1 alone, every bin lies in two filters, and above
    #  1 kHz the three bins share their two filters; everything else is quantisation noise 90 dB down)
    assert int(kept.min()) >= 2 and int(kept[:, 0].min()) >= 3             # (frame 0's reflected half is no pure tone)
    for b, k in enumerate(ks):
        holds = mw[k, top[b].reshape(-1)]
        print("tone bin %d: arg-max band(s) %s, the filter weight there %.4f" % (k, sorted(set(top[b].reshape(-1).tolist())),
                                                                                 float(holds.min())))
        assert bool((holds > 0).all())
    e = fs.rel_err(ref["mel32"], ref["mel64"], ref["keep"])
    print("tones: err_ref of the kept log-mel entries %.3e" % e)
    assert e <= fs.WELL_CONDITIONED


@pytest.mark.parametrize("t", fs.FRAME_COUNTS)
def test_mic_peaks_reach_both_ends_of_the_lag_window(t):
    audio = fs.case_audio("mic", t)
    found = set()
    for b in range(audio.shape[0]):
        gcc = fs.features64(audio[b].numpy())[2]                          # (T, 64, 6), not z-scored
        for p, m in enumerate(fs.MIC_PEAK_BINS[b]):
            if m is None:
                continue
            peak = float(gcc[1:, m, p].min())                             # (frame 0's reflected half mirrors the delay)
            print("mic T %d clip %d pair %d: lag bin %d holds %.4f in its weakest frame after frame 0, %.4f in frame 0" % (
                t, b, p, m, peak, float(gcc[0, m, p])))
            assert peak > 0.5 and bool((gcc[1:, :, p].argmax(axis=1) == m).all())
            found.add(m)
        if fs.MIC_DELAYS[b] is None:
            unit = np.zeros((t, 64, 6))
            unit[:, 32, :] = 1.0
            print("mic T %d clip %d (identical channels): float64 GCC is a unit peak at lag bin 32 to %.1e" % (
                t, b, float(np.abs(gcc - unit).max())))
            assert float(np.abs(gcc - unit).max()) < 1e-12
    assert {0, 1, 62, 63} <= found


def test_chunk_windows_follow_a_loud_stretch():
    rec = fs.case_audio("chunks", 0)[0]
    assert rec.shape == (fs.CHUNK_SAMPLES, 4)
    for off in fs.CHUNK_OFFSETS:
        for t in fs.CHUNK_T:
            w = fs.chunk_window(off, t)
            assert w.shape == (600 * t, 4) and torch.equal(w, rec[off:off + 600 * t])
        if off:
            before, after = float(rec[max(0, off - 200):off].abs().mean()), float(rec[off:off + 200].abs().mean())
            print("chunk offset %d: mean |x| %.4f before the window start, %.4f after" % (off, before, after))
            assert before > 30 * after


# ----------------------------------------------------------------------------------------------------- the bar's gate
@pytest.mark.parametrize("family,t", fs.value_cases())
def test_float32_reference_keeps_the_bar_at_float32_level(family, t):
    """err_ref <= 8e-6 for every quantity that goes through ``value_check``: a condition on the inputs, so that 4 err_ref stays
    near float32 level.  (Left out on purpose: the intensity vector of ``tones`` and the GCC-PHAT of ``silence``, ratios of
    round-off that float64 does not define either; the GPU module checks them for finiteness / not at all.)"""
    ref = fs.reference(family, t)
    for q in fs.quantities(family):
        e = fs.rel_err(ref[q + "32"], ref[q + "64"], ref.get("keep") if q == "mel" else None)
        print("%-9s T %-4d %-3s err_ref %.3e (float64 absmax %.3e)" % (family, t, q, e, float(ref[q + "64"].abs().max())))
        assert e <= fs.WELL_CONDITIONED
    assert all(v.dtype == (torch.float64 if k.endswith("64") else torch.float32) for k, v in ref.items() if k != "keep")
    if family == "silence":
        print("silence T %d: err_ref of the GCC-PHAT %.3e (not value-checked)" % (t, fs.rel_err(ref["gcc32"], ref["gcc64"])))


def test_float32_reference_of_the_scaled_and_chunked_runs():
    sc = golden_scaler()
    for family in ("plane", "levels"):
        z = fs.scaled(fs.reference(family, 9), sc)
        for q in ("mel", "iv"):
            e = fs.rel_err(z[q + "32"], z[q + "64"])
            print("%-9s T 9 z-scored %-3s err_ref %.3e (float64 absmax %.3e)" % (family, q, e, float(z[q + "64"].abs().max())))
            assert e <= fs.WELL_CONDITIONED
    for off in fs.CHUNK_OFFSETS:
        for t in fs.CHUNK_T:
            ref = fs.chunk_reference(off, t)
            for q in ("mel", "iv"):
                e = fs.rel_err(ref[q + "32"], ref[q + "64"])
                print("chunk offset %-4d T %d %-3s err_ref %.3e" % (off, t, q, e))
                assert e <= fs.WELL_CONDITIONED


# -------------------------------------------------------------------------------------------------------- sensitivity
SENSITIVITY_CASES = [(f, t) for f in fs.FAMILIES + ("mic",) for t in (2, 9)] + [("tones", fs.TONES_T)]


@pytest.mark.parametrize("err", fs.ERRORS)
def test_cases_reject_a_deliberate_mistake(err):
    """The float32 CPU evaluation with one deliberate mistake must miss the bar max(4 err_ref, 16 * 2^-24) in at least one case
    (T = 2 and 9 of every family, and the tones, are enough); the missing 1e-8 of E must be caught by ``silence``."""
    rejected = []
    for family, t in SENSITIVITY_CASES:
        ref, bad = fs.reference(family, t), fs.reference_of(fs.case_audio(family, t), err)
        for q in fs.quantities(family):
            keep = ref.get("keep") if q == "mel" else None
            e_bad, e_ref = fs.rel_err(bad[q + "32"], ref[q + "64"], keep), fs.rel_err(ref[q + "32"], ref[q + "64"], keep)
            if e_bad > fs.bar(e_ref):
                rejected.append((family, t, q, e_bad / fs.bar(e_ref)))
    print("%-9s rejected by %d checks; err / bar of the worst: %s" % (
        err, len(rejected), ["%s T %d %s %.1e" % r for r in sorted(rejected, key=lambda r: -r[3])[:4]]))
    assert rejected
    if err == "no_eps":
        assert any(r[0] == "silence" for r in rejected)
    if err in ("lag_shift", "pair_sign"):
        assert all(r[2] == "gcc" for r in rejected)


# ------------------------------------------------------------------------------------------------------------ aug.hip
@pytest.mark.parametrize("n", fs.PCM_SIZES)
def test_pcm_input_holds_the_extremes_where_the_kernel_changes_path(n):
    pcm = fs.pcm_input(n)
    assert pcm.shape == (n,) and pcm.dtype == torch.int16 and torch.equal(pcm, fs.pcm_input(n))
    want = [-32768, 0, 32767]
    assert int(pcm[0]) in want and (n < 3 or (int(pcm[0]) == -32768 and set(want) <= set(pcm.tolist()[:9] + pcm.tolist()[-8:])))
    if n > 8192 * 256 * 8:                                                  # (the small sizes hold what fits, overlapping)
        assert pcm[:3].tolist() == want and pcm[3:6].tolist() == want       # across a thread's two float4 stores
        assert pcm[7:10].tolist() == want                                   # across two threads' eight samples
        assert pcm[8192 * 256 * 8 - 1:8192 * 256 * 8 + 2].tolist() == want  # into the grid-stride round
        assert pcm[n - n % 8:n - n % 8 + 3].tolist() == want               # the scalar tail
    ref = fs.pcm_reference(pcm)
    assert ref.dtype == torch.float32 and float(ref.min()) >= -1.0 and float(ref.max()) < 1.0


def test_rotate_reference_is_the_sixteen_combinations():
    from adyolo_amd.augmentations import COMBINATIONS
    g = np.load(os.path.join(G, "rotation.npz"))
    audio = torch.from_numpy(g["audio"].astype(np.float32))
    out = fs.rotate_reference(audio[None].repeat(16, 1, 1), COMBINATIONS)
    assert np.array_equal(out.numpy(), g["audio_rot"].astype(np.float32))
    assert len({(c[0], c[1]) for c in COMBINATIONS}) == 16


@pytest.mark.parametrize("rows,cols", [(1, 7), (1025, 300), (2049, 7)])
def test_colstats_bound_covers_a_float32_running_sum(rows, cols):
    """The kernel's arithmetic restated in NumPy (float32 running sums over the rows of a block, float64 over the blocks) stays
    within the a-priori bound, and the bound is no more than 2 per x 2^-24 of the sums."""
    a = fs.colstats_input(rows, cols)
    ref, bound = fs.colstats_reference(a)
    nblk, per, used = fs.colstats_split(rows)
    s, q = np.zeros(cols), np.zeros(cols)
    x = a.numpy()
    for blk in range(used):
        ps, pq = np.zeros(cols, np.float32), np.zeros(cols, np.float32)
        for r in range(blk * per, min(rows, (blk + 1) * per)):
            ps, pq = ps + x[r], pq + x[r] * x[r]
        s, q = s + ps.astype(np.float64), q + pq.astype(np.float64)
    e = np.abs(np.stack([s, q]) - ref[:2].numpy())
    print("colstats %d x %d: restated kernel err / bound %.3f (sum), %.3f (squares); mean %.2f, spread %.2f" % (
        rows, cols, float((e[0] / bound[0].numpy()).max()), float((e[1] / bound[1].numpy()).max()), float(a.mean()), float(a.std()) if rows > 1 else 0.0))
    assert bool((e <= bound.numpy()).all())
    assert bool((bound[0] <= 2 * per * fs.U * a.double().abs().sum(0)).all()) and -70 < float(a.mean()) < -50
