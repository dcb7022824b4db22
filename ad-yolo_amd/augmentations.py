"""FOA rotation and MIC channel-swap augmentation.  Mirror of ``RotationAug`` (/root/reference/src/utils/augmentations.py:36-111): 16
combinations of channel sign flips / X-Y swap with the matching azimuth / elevation remapping of the labels.
``rotate_labels`` is the host half (label dict); ``rotate_audio`` applies the channel transform to a whole batch of raw
audio on the GPU (csrc/aug.hip ``foa_rotate_kernel``).  ``yaw_config`` / ``draw_yaw`` / ``yaw_cos_sin`` / ``yaw_labels`` /
``rotate_audio_yaw`` are the yaw rotation: the FOA sound field turned about the vertical axis by any whole angle after the
combination (no reference; ``aug_config.yaw_rotation_augment``, csrc/aug.hip ``foa_rotate_yaw_kernel``).
``swap_audio`` / ``ChannelSwapAug`` are the MIC-format counterpart (no
reference: a permutation of the four capsules by a symmetry of the array, derived below from ``rotate_labels``).  ``SpecAug``
(augmentations.py:6-33) masks the GPU feature tensor (csrc/aug.hip); its random draw restates torchaudio 0.10, which is absent
here (parity of the stream unpinned).  ``feature_aug_config`` / ``draw_feature_aug`` / ``apply_feature_aug_host`` are the keys,
draws and NumPy definition of the frequency-shift and cutout augmentation of the features (csrc/aug.hip ``feat_augment_kernel``)."""
import random

import torch

from . import _lib
from .ops import _p, _stream

# (yzx sign weights, xy swap, azimuth weight, azimuth offset, elevation weight) -- augmentations.py:45-68
COMBINATIONS = [
    ((1, 1, 1), False, 1, 0, 1), ((1, -1, 1), False, 1, 0, -1),
    ((-1, 1, 1), False, -1, 0, 1), ((-1, -1, 1), False, -1, 0, -1),
    ((-1, 1, -1), False, 1, 180, 1), ((-1, -1, -1), False, 1, 180, -1),
    ((1, 1, -1), False, -1, 180, 1), ((1, -1, -1), False, -1, 180, -1),
    ((-1, 1, 1), True, 1, 90, 1), ((-1, -1, 1), True, 1, 90, -1),
    ((1, 1, 1), True, -1, 90, 1), ((1, -1, 1), True, -1, 90, -1),
    ((1, 1, -1), True, 1, -90, 1), ((1, -1, -1), True, 1, -90, -1),
    ((-1, 1, -1), True, -1, -90, 1), ((-1, -1, -1), True, -1, -90, -1),
]


def rotate_labels(label: dict, comb_no: int):
    """label {frame: [[cls, src, az, el], ...]} -> rotated copy (augmentations.py:98-109)."""
    _, _, pw, dpi, tw = COMBINATIONS[int(comb_no)]
    out = {}
    for frame, events in label.items():
        rows = []
        for ev in events:
            pi = ev[-2] * pw + dpi
            if pi < -180:
                pi += 360
            elif pi > 180:
                pi -= 360
            rows.append(list(ev[:-2]) + [pi, ev[-1] * tw])
        out[frame] = rows
    return out


def rotate_audio(audio, comb_nos):
    """audio (B, n_samples, 4) float32 on the GPU, comb_nos: B combination indices -> rotated audio (new tensor)."""
    if not audio.is_cuda or audio.dtype != torch.float32 or not audio.is_contiguous():
        raise _lib.AdyoloHipError("rotate_audio needs contiguous float32 audio (B, n_samples, 4) on the GPU")
    b, n, _ = audio.shape
    cfg = torch.tensor([[*COMBINATIONS[int(c)][0], float(COMBINATIONS[int(c)][1])] for c in comb_nos],
                       dtype=torch.float32).to(audio.device)
    out = torch.empty_like(audio)
    _lib.call("adyolo_foa_rotate", _p(audio), _p(out), _p(cfg), b, n, _stream())
    return out


# ---- Yaw rotation: the sound field turned about the vertical axis by any whole angle (``aug_config.yaw_rotation_augment``), an
# exact symmetry of the B-format: X' = X cos - Y sin, Y' = Y cos + X sin, W and Z unchanged, every azimuth moved by the angle.
def yaw_config(params):
    """``aug_config.yaw_rotation_augment`` and ``yaw_step_deg`` -> None (off; ``yaw_step_deg`` is not read) or the step in
    degrees (default 1): an integer >= 1 that divides 360 (``ValueError`` naming the key otherwise).  FOA only: with
    ``data_config.audio_format: mic`` the key raises ``ValueError`` (a yaw is no symmetry of the microphone array;
    ``channel_swap_augment`` is the MIC augmentation)."""
    aug = params.get("aug_config", {})
    if not bool(aug.get("yaw_rotation_augment", False)):
        return None
    fmt = str(params.get("data_config", {}).get("audio_format", "foa")).lower()
    if fmt != "foa":
        raise ValueError("aug_config.yaw_rotation_augment turns the B-format sound field: it needs data_config.audio_format "
                         "'foa' (got %r; channel_swap_augment is the MIC augmentation)" % fmt)
    step = aug.get("yaw_step_deg", 1)
    if isinstance(step, bool) or not isinstance(step, int) or step < 1 or 360 % step:
        raise ValueError("aug_config.yaw_step_deg must be an integer >= 1 that divides 360 (got %r)" % (step,))
    return int(step)


def draw_yaw(rnd, config):
    """One yaw draw from ``rnd`` (the dataset's ``random`` module), right after a combination draw (or where it would stand):
    phi = -180 + step * k degrees, k uniform in 0 .. 360 / step - 1 -> int in [-180, 180).  One helper for ``FoaDataset`` and both
    device corpora (the mate's yaw is drawn inside ``draw_time_mix``): the same seed draws the same yaws on every path."""
    n = 360 // config
    return -180 + config * min(int(rnd.random() * n), n - 1)


def yaw_cos_sin(phi):
    """Yaw in degrees -> (cos, sin) as two ``np.float32``: exact at the multiples of 90 degrees, elsewhere the float32 of
    ``math.cos`` / ``math.sin`` of ``math.radians(phi)``."""
    import math
    import numpy as np
    exact = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), 270: (0.0, -1.0)}.get(phi % 360 if phi == int(phi) else None)
    if exact is not None:
        return np.float32(exact[0]), np.float32(exact[1])
    return np.float32(math.cos(math.radians(phi))), np.float32(math.sin(math.radians(phi)))


def yaw_labels(label: dict, phi):
    """label {frame: [[cls, src, az, el], ...]} (already moved by ``rotate_labels``, if at all) -> copy with every azimuth moved
    by ``phi`` degrees and wrapped as ``rotate_labels`` wraps (one wrap suffices for az in [-180, 180], phi in [-180, 180));
    the elevation is untouched."""
    out = {}
    for frame, events in label.items():
        rows = []
        for ev in events:
            az = ev[-2] + phi
            if az < -180:
                az += 360
            elif az > 180:
                az -= 360
            rows.append(list(ev[:-2]) + [az, ev[-1]])
        out[frame] = rows
    return out


def yaw_audio_host(audio, phi):
    """The definition of the yaw on audio, in NumPy float32: audio (..., 4) float32 frames (W, Y, Z, X) -> new array with
    Y' = fl(fl(Y c) + fl(X s)), X' = fl(fl(X c) - fl(Y s)), (c, s) = ``yaw_cos_sin(phi)``; every product and sum rounded."""
    import numpy as np
    a = np.asarray(audio, dtype=np.float32)
    c, s = yaw_cos_sin(phi)
    out = a.copy()
    y, x = a[..., 1], a[..., 3]
    out[..., 1] = (y * c).astype(np.float32) + (x * s).astype(np.float32)
    out[..., 3] = (x * c).astype(np.float32) - (y * s).astype(np.float32)
    return out


def rotate_audio_yaw(audio, comb_nos, phis):
    """audio (B, n_samples, 4) float32 on the GPU, comb_nos: B combination indices (None or negative: no combination), phis: B
    yaws in degrees -> the audio under its combinations, then yawed (new tensor; csrc/aug.hip ``foa_rotate_yaw_kernel``)."""
    if not audio.is_cuda or audio.dtype != torch.float32 or not audio.is_contiguous() or audio.dim() != 3 or audio.shape[2] != 4:
        raise _lib.AdyoloHipError("rotate_audio_yaw needs contiguous float32 audio (B, n_samples, 4) on the GPU")
    b, n, _ = audio.shape
    if len(comb_nos) != b or len(phis) != b:
        raise _lib.AdyoloHipError("rotate_audio_yaw: %d combinations and %d yaws for a batch of %d" % (len(comb_nos), len(phis), b))
    rows = []
    for c, phi in zip(comb_nos, phis):
        signs, swap = ((1, 1, 1), False) if c is None or int(c) < 0 else COMBINATIONS[int(c)][:2]
        cos, sin = yaw_cos_sin(phi)
        rows.append([*signs, float(swap), float(cos), float(sin)])
    cfg = torch.tensor(rows, dtype=torch.float32).to(audio.device)
    out = torch.empty_like(audio)
    _lib.call("adyolo_foa_rotate_yaw", _p(audio), _p(out), _p(cfg), b, n, _stream())
    return out


# ---- MIC channel swap (ACS): the MIC-format counterpart of the FOA rotation.  The four capsules of the DCASE tetrahedral array
# (channel 0..3 = M1..M4, azimuth / elevation in degrees); a label map of COMBINATIONS that sends every capsule onto a capsule
# is a symmetry of the array, and permuting the channels the same way keeps the audio in agreement with the moved labels.
MIC_DIRECTIONS = ((45, 35), (-45, -35), (135, -35), (-135, 35))


def _mic_symmetries():
    """{combination: (s0, s1, s2, s3)}, derived from ``rotate_labels``: combination k maps capsule i onto capsule pi(i) (or is
    no symmetry); a source heard by capsule i is, after the map, heard by capsule pi(i): new[pi(i)] = old[i], s = pi^-1."""
    out = {}
    for k in range(len(COMBINATIONS)):
        images = [tuple(ev[2:]) for ev in rotate_labels({0: [[0, 0, az, el] for az, el in MIC_DIRECTIONS]}, k)[0]]
        if all(d in MIC_DIRECTIONS for d in images):
            pi = [MIC_DIRECTIONS.index(d) for d in images]
            out[k] = tuple(pi.index(j) for j in range(4))
    return out


_MIC_SWAP_SOURCE = _mic_symmetries()
MIC_SWAP_COMBS = tuple(sorted(_MIC_SWAP_SOURCE))
assert MIC_SWAP_COMBS == (0, 3, 4, 7, 9, 10, 13, 14), MIC_SWAP_COMBS
assert [_MIC_SWAP_SOURCE[k] for k in MIC_SWAP_COMBS] == [(0, 1, 2, 3), (1, 0, 3, 2), (3, 2, 1, 0), (2, 3, 0, 1), (1, 3, 0, 2),
                                                        (0, 2, 1, 3), (2, 0, 3, 1), (3, 1, 2, 0)], _MIC_SWAP_SOURCE


def mic_swap_source(comb_no):
    """Combination (one of ``MIC_SWAP_COMBS``) -> (s0, s1, s2, s3): output channel j is input channel s_j."""
    src = _MIC_SWAP_SOURCE.get(int(comb_no))
    if src is None:
        raise ValueError("mic_swap_source: combination %r is not a symmetry of the microphone array (the symmetries are %s)"
                         % (comb_no, list(MIC_SWAP_COMBS)))
    return src


# ---- Rotation test-time augmentation: a clip evaluated under several combinations, the detections turned back and merged
# (``postprocess.merge_view_rows``, csrc/select.hip ``adyolo_tta_collect`` / ``adyolo_tta_merge``).
def _view_matrices():
    """[M_k]: the 3x3 signed permutation that takes a direction vector (x, y, z) to where combination k puts it, derived from
    ``rotate_labels`` on the three axis directions (column j of M_k is the image of axis j)."""
    import math
    axes = ((0, 0), (90, 0), (0, 90))                                            # (azimuth, elevation) of x, y, z
    out = []
    for k in range(len(COMBINATIONS)):
        m = [[0] * 3 for _ in range(3)]
        for j, ev in enumerate(rotate_labels({0: [[0, 0, az, el] for az, el in axes]}, k)[0]):
            az, el = math.radians(ev[2]), math.radians(ev[3])
            image = (math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el))
            for i in range(3):
                m[i][j] = int(round(image[i]))
        out.append(tuple(tuple(row) for row in m))
    return tuple(out)


_VIEW_MATRICES = _view_matrices()
assert all(sorted(abs(v) for row in m for v in row) == [0] * 6 + [1] * 3 and all(sum(abs(v) for v in row) == 1 for row in m)
           and all(sum(abs(m[i][j]) for i in range(3)) == 1 for j in range(3)) for m in _VIEW_MATRICES), _VIEW_MATRICES
assert _VIEW_MATRICES[0] == ((1, 0, 0), (0, 1, 0), (0, 0, 1)), _VIEW_MATRICES[0]


def view_matrix(comb_no):
    """Combination -> M (3x3 ``np.float32``, entries exactly 0 or +-1, inverse = transpose): a source at direction d is, in the
    clip under that combination, at M d; a detection there is turned back by M^T."""
    import numpy as np
    if isinstance(comb_no, bool) or int(comb_no) != comb_no or not 0 <= int(comb_no) < len(COMBINATIONS):
        raise ValueError("view_matrix: combination %r is not one of 0..%d" % (comb_no, len(COMBINATIONS) - 1))
    return np.asarray(_VIEW_MATRICES[int(comb_no)], dtype=np.float32)


TTA_DEFAULT_UNIFY_DEG = 15.0
TTA_DEFAULT_ROWS_PER_FRAME = 64


def _tta_key(params, key, default=None):
    for section in ("test_config", "train_config"):
        if params.get(section, {}).get(key) is not None:
            return params[section][key], "%s.%s" % (section, key)
    return default, "test_config.%s" % key


def tta_views(params):
    """``test_config.tta_views`` (falling back to ``train_config.tta_views``) -> None (absent or None: off) or the list of
    combinations a clip is evaluated under.  "all": every combination that is a symmetry of the format, 0..15 for FOA and
    ``MIC_SWAP_COMBS`` with ``data_config.audio_format: mic``; a list of combination numbers: those.  The unrotated clip is
    always view 0 and is not listed twice.  ``ValueError`` naming the key: anything else, or a combination that is no symmetry
    of the format."""
    value, where = _tta_key(params, "tta_views")
    if value is None:
        return None
    fmt = str(params.get("data_config", {}).get("audio_format", "foa")).lower()
    allowed = tuple(MIC_SWAP_COMBS) if fmt == "mic" else tuple(range(len(COMBINATIONS)))
    if isinstance(value, str):
        if value.lower() != "all":
            raise ValueError("%s must be 'all' or a list of combination numbers (got %r)" % (where, value))
        return list(allowed)
    if not isinstance(value, (list, tuple)):
        raise ValueError("%s must be 'all' or a list of combination numbers (got %r)" % (where, value))
    views = [0]
    for v in value:
        if isinstance(v, bool) or not isinstance(v, int) or v not in allowed:
            raise ValueError("%s: %r is no symmetry of the %s format (the symmetries are %s)" % (where, v, fmt, list(allowed)))
        if v not in views:
            views.append(v)
    return views


def tta_options(params, views=None, postprocessor=None):
    """What ``test.test_epoch_corpus(tta=...)`` takes: None (``tta_views`` is off) or {'views', 'min_views', 'unify_thresh',
    'max_rows_per_frame'}.  views: the list to use instead of ``tta_views(params)``.  The other keys are read like
    ``tta_views`` (``test_config``, then ``train_config``): ``tta_min_views`` (default a majority, (V + 1) // 2; an integer in
    [1, V]), ``tta_unify_thresh`` (degrees in (0, 180]; default the head's ``unify_thresh`` -- ``postprocessor``'s, or
    ``train_config``'s for adyolo and adpit -- else 15) and ``tta_max_rows_per_frame`` (default 64; an integer in [1, 1024]).
    ``ValueError`` naming the key otherwise."""
    import math
    views = tta_views(params) if views is None else list(views)
    if views is None:
        return None
    if not views or views[0] != 0 or len(set(views)) != len(views) or any(not 0 <= int(v) < len(COMBINATIONS) for v in views):
        raise ValueError("tta_options: views %r must start with 0 and hold distinct combinations" % (views,))
    n = len(views)
    min_views, where = _tta_key(params, "tta_min_views", (n + 1) // 2)
    if isinstance(min_views, bool) or not isinstance(min_views, int) or not 1 <= min_views <= n:
        raise ValueError("%s must be an integer in [1, %d] (got %r)" % (where, n, min_views))
    head = getattr(postprocessor, "unify_thresh", None)
    if postprocessor is None and params.get("args", {}).get("loss") in ("adyolo", "adpit"):
        head = params.get("train_config", {}).get("unify_thresh")
    unify, where = _tta_key(params, "tta_unify_thresh", TTA_DEFAULT_UNIFY_DEG if head is None else head)
    if isinstance(unify, bool) or not isinstance(unify, (int, float)) or not math.isfinite(unify) or not 0.0 < unify <= 180.0:
        raise ValueError("%s must be an angle in (0, 180] degrees (got %r)" % (where, unify))
    cap, where = _tta_key(params, "tta_max_rows_per_frame", TTA_DEFAULT_ROWS_PER_FRAME)
    if isinstance(cap, bool) or not isinstance(cap, int) or not 1 <= cap <= 1024:
        raise ValueError("%s must be an integer in [1, 1024] (got %r)" % (where, cap))
    return {"views": [int(v) for v in views], "min_views": int(min_views), "unify_thresh": float(unify),
            "max_rows_per_frame": int(cap)}


TRACK_DEFAULT_GATE_DEG = 20.0                                 # the scorer's DOA threshold
TRACK_DEFAULT_MAX_GAP = 2
TRACK_DEFAULT_MIN_LEN = 3
TRACK_DEFAULT_SMOOTH = 0.5


def track_options(params):
    """What ``test.test_epoch_corpus(track=...)`` takes: None (tracking is off) or {'gate_deg', 'max_gap', 'min_len',
    'smooth'}, the parameters of ``postprocess.track_rows``.  The keys are read from ``test_config``, then ``train_config``.
    Only ``track: true`` switches tracking on (absent or false: None).  ``track_gate_deg``: the association gate, an angle in
    (0, 90) degrees, default 20 (the scorer's DOA threshold); ``track_max_gap``: the longest gap in frames that is bridged and
    filled, an integer >= 0, default 2; ``track_min_len``: the fewest hits a track needs to be kept, an integer >= 1, default
    3; ``track_smooth``: the weight of a new detection in the track's direction, in (0, 1], default 0.5 (1: no smoothing).
    None of the defaults is tuned on data.  ``ValueError`` naming the key otherwise."""
    import math
    import numpy as np
    on, where = _tta_key(params, "track", False)
    if not isinstance(on, bool):
        raise ValueError("%s must be true or false (got %r)" % (where, on))
    if not on:
        return None
    gate, where = _tta_key(params, "track_gate_deg", TRACK_DEFAULT_GATE_DEG)
    if isinstance(gate, bool) or not isinstance(gate, (int, float)) or not math.isfinite(gate) or not 0.0 < gate < 90.0 \
            or not 0.0 < np.float32(math.cos(math.radians(gate))) < 1.0:       # (the float32 cosine is what the gate compares)
        raise ValueError("%s must be an angle in (0, 90) degrees (got %r)" % (where, gate))
    max_gap, where = _tta_key(params, "track_max_gap", TRACK_DEFAULT_MAX_GAP)
    if isinstance(max_gap, bool) or not isinstance(max_gap, int) or max_gap < 0:
        raise ValueError("%s must be an integer >= 0 (got %r)" % (where, max_gap))
    min_len, where = _tta_key(params, "track_min_len", TRACK_DEFAULT_MIN_LEN)
    if isinstance(min_len, bool) or not isinstance(min_len, int) or min_len < 1:
        raise ValueError("%s must be an integer >= 1 (got %r)" % (where, min_len))
    smooth, where = _tta_key(params, "track_smooth", TRACK_DEFAULT_SMOOTH)
    if isinstance(smooth, bool) or not isinstance(smooth, (int, float)) or not math.isfinite(smooth) or not 0.0 < smooth <= 1.0:
        raise ValueError("%s must lie in (0, 1] (got %r)" % (where, smooth))
    return {"gate_deg": float(gate), "max_gap": int(max_gap), "min_len": int(min_len), "smooth": float(smooth)}


def channel_swap_enabled(params):
    """``aug_config.channel_swap_augment``, with its two refusals: MIC-format audio only, and not together with the FOA
    rotation (``ValueError``: both would move the labels)."""
    aug = params.get("aug_config", {})
    if not bool(aug.get("channel_swap_augment", False)):
        return False
    fmt = str(params.get("data_config", {}).get("audio_format", "foa")).lower()
    if fmt != "mic":
        raise ValueError("aug_config.channel_swap_augment permutes microphone capsules: it needs data_config.audio_format "
                         "'mic' (got %r; rotation_augment is the FOA augmentation)" % fmt)
    if bool(aug.get("rotation_augment", False)):
        raise ValueError("aug_config.channel_swap_augment and aug_config.rotation_augment are both on: rotation_augment is "
                         "the FOA augmentation, a MIC run takes channel_swap_augment alone")
    return True


# ---- Time-domain mixing: the audio of two training chunks summed, their labels united (``aug_config.time_mix_augment``).
def time_mix_config(params):
    """``aug_config.time_mix_augment`` and its keys -> None (off) or (prob, gain_lo_db, gain_hi_db).  ``time_mix_prob`` (default
    0.5) must be in [0, 1]; ``time_mix_gain_db`` (default [0.0, 0.0]) must be two finite numbers lo <= hi (``ValueError`` naming
    the key otherwise)."""
    import math
    aug = params.get("aug_config", {})
    if not bool(aug.get("time_mix_augment", False)):
        return None
    prob = aug.get("time_mix_prob", 0.5)
    if isinstance(prob, bool) or not isinstance(prob, (int, float)) or not 0.0 <= prob <= 1.0:
        raise ValueError("aug_config.time_mix_prob must be a number in [0, 1] (got %r)" % (prob,))
    gain = aug.get("time_mix_gain_db", [0.0, 0.0])
    if not isinstance(gain, (list, tuple)) or len(gain) != 2 \
            or any(isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) for v in gain) \
            or gain[0] > gain[1]:
        raise ValueError("aug_config.time_mix_gain_db must be [lo, hi] with lo <= hi, both finite (got %r)" % (gain,))
    return float(prob), float(gain[0]), float(gain[1])


def time_mix_enabled(params):
    """``aug_config.time_mix_augment``, with the refusals of ``time_mix_config``."""
    return time_mix_config(params) is not None


def draw_time_mix(rnd, config, total_filelist, name, comb_draw=None, yaw=None):
    """The draws of one training item, after its own (rotation or swap combination, SpecAug table), from ``rnd`` (the dataset's
    ``random`` module): mixed at all?  If so the mate chunk, the mate's combination (``comb_draw`` "rotate": one of 16, "swap": one
    of ``MIC_SWAP_COMBS``, None: no draw) and the gain.  -> None (unmixed) or (mate name, combination or None, np.float32 gain).
    A mate that is the item itself leaves the item unmixed, after all the draws.  yaw (``yaw_config``; None: no draw, and the
    tuple as above): the mate's yaw is drawn right after its combination (``draw_yaw``) and returned as a fourth element."""
    import numpy as np
    prob, lo, hi = config
    if not rnd.random() < prob:
        return None
    mate = total_filelist[int(rnd.uniform(0, len(total_filelist)))]
    comb = None
    if comb_draw == "rotate":
        comb = int(rnd.uniform(0, 16))
    elif comb_draw == "swap":
        comb = MIC_SWAP_COMBS[int(rnd.uniform(0, 8))]
    phi = draw_yaw(rnd, yaw) if yaw is not None else None
    gain = np.float32(10.0 ** (rnd.uniform(lo, hi) / 20.0))
    if mate == name:
        return None
    return (mate, comb, gain) if yaw is None else (mate, comb, gain, phi)


def merge_labels(a: dict, b: dict):
    """Two label dicts {frame: [[cls, src, az, el], ...]} (each already moved by its own ``rotate_labels``) -> the labels of their
    mixture: the frames of both in ascending order, each frame's list ``a``'s events followed by ``b``'s.  New dict and lists."""
    return {frame: [list(ev) for ev in a.get(frame, [])] + [list(ev) for ev in b.get(frame, [])]
            for frame in sorted(set(a) | set(b))}


# ---- Frequency shift and cutout on the normalised features (``aug_config.freq_shift_augment`` / ``cutout_augment``).  The item's
# table grows from the SpecAug rows (G, 4) to (G + 2, 4): row G the cutout rectangle {t0, t1, f0, f1}, row G + 1 {shift, 0, 0, 0}.
FEATURE_AUG_DEFAULTS = {"freq_shift_prob": 0.5, "freq_shift_max_bins": 5, "cutout_prob": 0.5, "cutout_time_param": 40,
                        "cutout_freq_param": 20}


def feature_aug_config(params):
    """``aug_config.freq_shift_augment`` / ``cutout_augment`` and their keys -> None (both off) or
    (shift_prob or None, shift_max_bins, cutout_prob or None, cutout_time_param, cutout_freq_param): a probability of None is an
    augmentation that is off.  ``freq_shift_prob`` / ``cutout_prob`` (0.5) must be numbers in [0, 1], ``freq_shift_max_bins`` (5)
    an integer in 1..63, ``cutout_time_param`` (40 frames) / ``cutout_freq_param`` (20 mel bins) finite numbers >= 0
    (``ValueError`` naming the key otherwise).  The keys of an augmentation that is off are not read."""
    import math
    aug = params.get("aug_config", {})
    shift_on, cut_on = bool(aug.get("freq_shift_augment", False)), bool(aug.get("cutout_augment", False))
    if not shift_on and not cut_on:
        return None

    def number(key):
        v = aug.get(key, FEATURE_AUG_DEFAULTS[key])
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError("aug_config.%s must be a finite number (got %r)" % (key, v))
        return v

    def prob(key):
        v = number(key)
        if not 0.0 <= v <= 1.0:
            raise ValueError("aug_config.%s must be a number in [0, 1] (got %r)" % (key, v))
        return float(v)

    shift_prob, max_bins, cut_prob, cut_t, cut_f = None, FEATURE_AUG_DEFAULTS["freq_shift_max_bins"], None, 0.0, 0.0
    if shift_on:
        shift_prob = prob("freq_shift_prob")
        max_bins = aug.get("freq_shift_max_bins", max_bins)
        if isinstance(max_bins, bool) or not isinstance(max_bins, int) or not 1 <= max_bins <= 63:
            raise ValueError("aug_config.freq_shift_max_bins must be an integer in 1..63 (got %r)" % (max_bins,))
    if cut_on:
        cut_prob = prob("cutout_prob")
        cut_t, cut_f = number("cutout_time_param"), number("cutout_freq_param")
        for key, v in (("cutout_time_param", cut_t), ("cutout_freq_param", cut_f)):
            if v < 0:
                raise ValueError("aug_config.%s must be >= 0 (got %r)" % (key, v))
    return shift_prob, int(max_bins), cut_prob, float(cut_t), float(cut_f)


def draw_feature_aug(rnd, config, t, f):
    """The LAST draws of one training item (after its rotation or swap, SpecAug table and mixing draws), from ``rnd`` (the
    dataset's ``random`` module), for features of ``t`` frames and ``f`` bins -> (cutout row [t0, t1, f0, f1], shift).  The shift,
    if enabled: ``random() < prob``, then the size 1 + min(int(random() * max_bins), max_bins - 1), then the sign (negative when
    ``random() < 0.5``).  The cutout, if enabled: ``random() < prob``, then the frame range and the bin range by ``SpecAug._range``'s
    formula (value = U * param, start = U * (size - value), [int(start), int(start + value))).  One helper for ``FoaDataset`` and
    both device corpora: the same seed draws the same tables on every training path."""
    shift_prob, max_bins, cut_prob, cut_t, cut_f = config
    shift, row = 0, [0, 0, 0, 0]
    if shift_prob is not None and rnd.random() < shift_prob:
        shift = 1 + min(int(rnd.random() * max_bins), max_bins - 1)
        if rnd.random() < 0.5:
            shift = -shift
    if cut_prob is not None and rnd.random() < cut_prob:
        for k, (param, size) in enumerate(((cut_t, t), (cut_f, f))):
            value = rnd.random() * param
            start = rnd.random() * (size - value)
            row[2 * k], row[2 * k + 1] = int(start), int(start + value)
    return row, shift


def feature_aug_table(spec, cutout, shift):
    """One item's table int32 (G + 2, 4): ``spec`` (G, 4) (the SpecAug draw, or zeros), the cutout row, {shift, 0, 0, 0}."""
    return torch.cat([spec.to(torch.int32).reshape(-1, 4), torch.tensor([list(cutout), [int(shift), 0, 0, 0]], dtype=torch.int32)], 0)


def apply_feature_aug_host(feat, table, groups, shift_groups):
    """The definition of ``adyolo_feat_augment`` in NumPy (exact: data movement and zero fill).  feat (B, T, F, C) float32, table
    int32 (B, G + 2, 4), groups G pairs (q0, q1) of float4 quads, shift_groups one bool per group -> new array.  Per sample, in
    this order: (1) shift: s = clamp(table[b, G + 1, 0], -(F - 1), F - 1); if s != 0 every channel of a group with
    ``shift_groups[g]`` moves along the bin axis, out[t, f] = in[t, src(f)], u = f - s, src = -u (u < 0), 2 (F - 1) - u (u > F - 1),
    u otherwise -- ``np.pad(mode="reflect")`` and a crop (a channel in several shifting groups moves once); (2) the SpecAug
    stripes of rows 0..G-1 as ``adyolo_mask_groups``: frames [t0, t1) x all bins and bins [f0, f1) x all frames of the group's
    channels, t0 = clamp(., 0, T), t1 = clamp(., t0, T), likewise the bins; (3) cutout: row G = {t0, t1, f0, f1}, clamped the same
    way, zeroes [t0, t1) x [f0, f1) in ALL channels; an empty range in either direction masks nothing."""
    import numpy as np
    feat = feat.detach().cpu().numpy() if isinstance(feat, torch.Tensor) else np.asarray(feat)
    table = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    out = np.array(feat, dtype=np.float32, copy=True)
    nb, t, f, c = out.shape
    g = len(groups)
    if table.shape != (nb, g + 2, 4) or len(shift_groups) != g:
        raise ValueError("apply_feature_aug_host: table %s with %d groups, expected (%d, %d, 4)" % (table.shape, g, nb, g + 2))

    def clamp(lo, hi, size):
        lo = min(max(int(lo), 0), size)
        return lo, min(max(int(hi), lo), size)

    bins = np.arange(f)
    for b in range(nb):
        s = min(max(int(table[b, g + 1, 0]), -(f - 1)), f - 1)
        if s != 0:
            u = bins - s
            src = np.where(u < 0, -u, np.where(u > f - 1, 2 * (f - 1) - u, u))
            moving = np.zeros(c, dtype=bool)
            for (q0, q1), on in zip(groups, shift_groups):
                if on:
                    moving[4 * q0:4 * q1] = True
            out[b][:, :, moving] = feat[b][:, src][:, :, moving]
        for (q0, q1), row in zip(groups, table[b, :g]):
            t0, t1 = clamp(row[0], row[1], t)
            f0, f1 = clamp(row[2], row[3], f)
            out[b, t0:t1, :, 4 * q0:4 * q1] = 0.0
            out[b, :, f0:f1, 4 * q0:4 * q1] = 0.0
        t0, t1 = clamp(table[b, g, 0], table[b, g, 1], t)
        f0, f1 = clamp(table[b, g, 2], table[b, g, 3], f)
        out[b, t0:t1, f0:f1, :] = 0.0
    return out


def swap_audio(audio, comb_nos):
    """audio (B, n_samples, 4) float32 on the GPU, comb_nos: B combinations of ``MIC_SWAP_COMBS`` -> the audio with its channels
    permuted (new tensor; csrc/aug.hip ``mic_swap_kernel``).  ``ValueError`` for any other combination, before any launch."""
    src = [mic_swap_source(c) for c in comb_nos]
    if not audio.is_cuda or audio.dtype != torch.float32 or not audio.is_contiguous():
        raise _lib.AdyoloHipError("swap_audio needs contiguous float32 audio (B, n_samples, 4) on the GPU")
    if audio.dim() != 3 or audio.shape[2] != 4 or audio.shape[0] != len(src):
        raise _lib.AdyoloHipError("swap_audio: audio %s with %d combinations, expected (B, n_samples, 4) and B of them"
                                  % (tuple(audio.shape), len(src)))
    from . import ops
    return ops.mic_swap(audio, torch.tensor(src, dtype=torch.int32).reshape(-1, 4).to(audio.device))


class ChannelSwapAug:
    """``RotationAug``'s surface for MIC-format audio: ``augment(audio (T,4) on the GPU, label)`` with one of the eight
    symmetries of the array (``aug_config.channel_swap_augment``; never on validation data)."""

    def __init__(self, params: dict, is_valid: bool):
        self.apply_augment = channel_swap_enabled(params) and not is_valid

    def augment(self, audio, label, comb_no=None):
        if not self.apply_augment:
            return audio, label
        if comb_no is None:
            comb_no = MIC_SWAP_COMBS[int(random.uniform(0, len(MIC_SWAP_COMBS)))]
        return swap_audio(audio.view(1, -1, 4), [comb_no]).view_as(audio), rotate_labels(label, comb_no)


class RotationAug:
    """Same surface as the reference class: ``augment(audio (T,4) on the GPU as (1,T,4) or labels only, label)``."""

    def __init__(self, params: dict, is_valid: bool):
        self.apply_augment = bool(params["aug_config"]["rotation_augment"]) and not is_valid

    def augment(self, audio, label, comb_no=None, phi=None):
        """phi (degrees, optional): the yaw applied after the combination -- on its own where the rotation is off."""
        if phi is not None:
            comb = None
            if self.apply_augment:
                comb = int(random.uniform(0, 16)) if comb_no is None else comb_no
                label = rotate_labels(label, comb)
            return rotate_audio_yaw(audio.view(1, -1, 4), [comb], [phi]).view_as(audio), yaw_labels(label, phi)
        if not self.apply_augment:
            return audio, label
        if comb_no is None:
            comb_no = int(random.uniform(0, 16))
        return rotate_audio(audio.view(1, -1, 4), [comb_no]).view_as(audio), rotate_labels(label, comb_no)


class SpecAug:
    """Feature-wise spec-augmentation (reference src/utils/augmentations.py:6-33) on the GPU feature tensor.

    The reference applies torchaudio 0.10's ``TimeMasking`` / ``FrequencyMasking`` to a (C, T, F) tensor, i.e. (quirk)
    its "time" mask (axis 2) zeroes MEL BINS and its "frequency" mask (axis 1) zeroes FRAMES; both with probability
    ``spec_augment_thresh`` per sample, identity when ``spec_augment`` is false (the default) or on validation data.
    ``mask_along_axis``: value = U(0,1) * mask_param, start = U(0,1) * (size - value), mask [int(start), int(start+value)).
    torchaudio is not installed in this image, so the draw order is restated from its published 0.10 source (parity of the
    random stream unpinned); the masking itself is exact and tested against NumPy slicing.
    ``augment(feat)``: feat (B, T, 64, 8) float32 channels-last on the GPU, masked in place per sample.
    """

    def __init__(self, params: dict, is_valid: bool):
        a = params.get("aug_config", {})
        self.apply_augment = bool(a.get("spec_augment", False)) and not is_valid
        self.thresh = a.get("spec_augment_thresh", 0.5)
        self.time_mask_param = a.get("spec_augment_time_mask_param", 0)
        self.freq_mask_param = a.get("spec_augment_freq_mask_param", 0)

    @staticmethod
    def _range(mask_param, size):
        value = random.random() * mask_param
        start = random.random() * (size - value)
        return int(start), int(start + value)

    def _draw_one(self, t, f):
        """One mask pair, drawn as the reference's ``_mask`` draws it for one spectrogram -> [t0, t1, f0, f1]."""
        r = [0, 0, 0, 0]
        if random.random() <= self.thresh:                           # reference "time_masking": last axis = mel bins
            r[2], r[3] = self._range(self.time_mask_param, f)
        if random.random() <= self.thresh:                           # reference "frequency_masking": axis 1 = frames
            r[0], r[1] = self._range(self.freq_mask_param, t)
        return r

    def draw(self, batch, t, f):
        """-> int32 (batch, 4) host tensor {t0, t1, f0, f1}; empty ranges where a mask is not applied."""
        return torch.tensor([self._draw_one(t, f) for _ in range(batch)], dtype=torch.int32).reshape(batch, 4)

    def draw_groups(self, batch, t, f, groups=2):
        """-> int32 (batch, groups, 4) host tensor: one independent ``draw`` per sample and feature group, sample after sample
        and group after group -- the reference masks each element of ``feature_stack = [MEL, IV]`` with its own draw
        (datasets.py:158-159).  ``draw_groups(b, t, f, 1)[:, 0]`` == ``draw(b, t, f)`` from the same ``random`` state."""
        return torch.tensor([[self._draw_one(t, f) for _ in range(groups)] for _ in range(batch)],
                            dtype=torch.int32).reshape(batch, groups, 4)

    def augment(self, feat, ranges=None):
        if not self.apply_augment:
            return feat
        from . import ops
        b, t, f, _ = feat.shape
        if ranges is None:
            ranges = self.draw(b, t, f)
        return ops.mask_ranges_(feat, ranges.to(feat.device, non_blocking=True).contiguous())
