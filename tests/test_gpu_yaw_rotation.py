"""GPU: the FOA yaw-rotation augmentation (``aug_config.yaw_rotation_augment``), every comparison bit for bit (as int32).
``rotate_audio_yaw`` against the NumPy float32 definition and against the four combinations a quarter turn reproduces;
``adyolo_corpus_gather`` with a yaw table (and mates) against ``pcm16_to_f32`` -> ``rotate_audio_yaw`` (-> ``a + g * m``) at both
offset parities, odd lengths, ``comb = -1`` and bad rows; the AD-YOLO rows and the dense class-wise targets of the yawed label calls
against the host path (``rotate_labels`` -> ``yaw_labels`` -> ``merge_labels`` -> encoder -> collate) at the wraps, at exactly +-180,
on cell bounds, at the poles and under every combination; both device corpora against ``FoaDataset`` through
``train_one_epoch_audio``; and three training steps from either corpus, eagerly and replayed from ONE hipGraph, against the
host-fed epoch from the same seed."""
import random

import numpy as np
import pytest
import torch

from test_gpu_corpus_classwise import _trainer
from test_yaw_rotation_cpu import write_whole_degree_split, yaw_params

pytestmark = pytest.mark.gpu

SR = 24000
C_TRAIN = 12
S = 5000                       # frames of the direct calls' pcm buffer
DEV = "cuda:0"
BAD_ITEM = 2


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    root = tmp_path_factory.mktemp("gpu_yaw_rotation")
    write_whole_degree_split(root, sr=SR, seed=21, nb_classes=C_TRAIN)
    return root


@pytest.fixture(scope="module")
def pcm():
    g = torch.Generator().manual_seed(18)
    return torch.randint(-32768, 32768, (S, 4), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _gain_word(g):
    return int(np.float32(g).view(np.uint32))


def _rows(offs, combs, yaws, gains=None):
    """(B, 8) int64 item rows from offsets, combinations and yaws (offset None: the no-mate row); gains -> word 6."""
    rows = torch.zeros(len(offs), 8, dtype=torch.int64)
    for j, (o, c, p) in enumerate(zip(offs, combs, yaws)):
        if o is None:
            rows[j, 0], rows[j, 4] = -1, -1
            continue
        rows[j, 0], rows[j, 4], rows[j, 7] = o, c, p
        if gains is not None:
            rows[j, 6] = _gain_word(gains[j])
    return rows


def _windows(ops, pcm, offs, n):
    """``pcm16_to_f32`` of the windows, each copied to an aligned buffer of its own first."""
    return ops.pcm16_to_f32(torch.stack([pcm[o:o + n] for o in offs]).contiguous())


# ------------------------------------------------------------------------------------------------------ rotate_audio_yaw
def _host_comb(x, k):
    from adyolo_amd.augmentations import COMBINATIONS
    if k is None or k < 0:
        return x
    (sy, sz, sx), swap = COMBINATIONS[k][:2]
    y, z, xx = x[:, 1] * np.float32(sy), x[:, 2] * np.float32(sz), x[:, 3] * np.float32(sx)
    return np.stack([x[:, 0], xx, z, y] if swap else [x[:, 0], y, z, xx], 1).astype(np.float32)


def test_rotate_audio_yaw_is_the_numpy_definition(ops, pcm):
    from adyolo_amd.augmentations import rotate_audio, rotate_audio_yaw, yaw_audio_host
    n = 1001                                                      # odd: no multiple of any vector width
    audio = _windows(ops, pcm, [0, 1500, 3001], n)
    host = audio.cpu().numpy()
    calls = ([(0, 5), (90, 0), (180, 11)], [(-90, None), (37, 14), (-179, 3)], [(37, 0), (-179, 8), (0, -1)],
             [(-180, 9), (179, 15), (1, 6)])
    for pairs in calls:
        got = rotate_audio_yaw(audio, [k for _, k in pairs], [p for p, _ in pairs])
        assert got.data_ptr() != audio.data_ptr() and tuple(got.shape) == (3, n, 4)
        for b, (phi, k) in enumerate(pairs):
            want = yaw_audio_host(_host_comb(host[b], k), phi)
            assert np.array_equal(got[b].cpu().numpy().view(np.int32), want.view(np.int32)), (phi, k)
    assert torch.equal(_bits(audio.cpu()), torch.from_numpy(host).view(torch.int32))                 # the input is only read
    # a quarter turn is a combination: yaws 0 / 180 / 90 / -90 under combination 0 are combinations 0 / 4 / 8 / 12
    got = rotate_audio_yaw(audio, [0, 0, 0], [0, 180, 90])
    assert torch.equal(_bits(got), _bits(rotate_audio(audio, [0, 4, 8])))
    got = rotate_audio_yaw(audio, [0, 0, 0], [-90, -180, 0])
    assert torch.equal(_bits(got), _bits(rotate_audio(audio, [12, 4, 0])))
    assert torch.equal(_bits(rotate_audio_yaw(audio, [7, 13, 2], [0, 0, 0])), _bits(rotate_audio(audio, [7, 13, 2])))
    from adyolo_amd._lib import AdyoloHipError
    with pytest.raises(AdyoloHipError):
        rotate_audio_yaw(audio, [0, 0], [0, 0, 0])
    with pytest.raises(AdyoloHipError):
        rotate_audio_yaw(audio.cpu(), [0, 0, 0], [0, 0, 0])


def test_rotation_aug_takes_an_optional_yaw(ops, pcm):
    from adyolo_amd.augmentations import RotationAug, rotate_audio_yaw, rotate_labels, yaw_labels
    audio = _windows(ops, pcm, [10], 255)[0]
    label = {0: [[1, 0, 170.0, 10.0]], 4: [[2, 0, -20.5, -5.0]]}
    on = RotationAug({"aug_config": {"rotation_augment": True}}, False)
    off = RotationAug({"aug_config": {"rotation_augment": False}}, False)
    a, lab = on.augment(audio, label, comb_no=9, phi=37)
    assert torch.equal(_bits(a), _bits(rotate_audio_yaw(audio[None], [9], [37])[0])) and lab == yaw_labels(rotate_labels(label, 9), 37)
    a, lab = off.augment(audio, label, comb_no=9, phi=37)         # the rotation off: the yaw on its own
    assert torch.equal(_bits(a), _bits(rotate_audio_yaw(audio[None], [None], [37])[0])) and lab == yaw_labels(label, 37)
    a, lab = off.augment(audio, label)                            # no yaw: today's behaviour
    assert a is audio and lab is label


# ------------------------------------------------------------------------------------------ adyolo_corpus_gather (yaw_tab)
def _gather(ops, pcm, items, n, mates=None):
    """One call -> (out, status word); a guard band behind the output must stay."""
    from adyolo_amd.augmentations import COMBINATIONS
    rot, tab = ops.corpus_rot_table(COMBINATIONS), ops.corpus_yaw_table(DEV)
    b = items.shape[0]
    buf = torch.full((b * n * 4 + 64,), 7.0, device=DEV)
    out = buf[:b * n * 4].view(b, n, 4)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.corpus_gather(pcm, items.to(DEV), rot, out, status, mates=None if mates is None else mates.to(DEV), yaw_tab=tab)
    torch.cuda.synchronize()
    assert bool((buf[b * n * 4:] == 7.0).all())
    return out, int(status.item())


def _gather_reference(ops, pcm, rows, n):
    from adyolo_amd.augmentations import rotate_audio_yaw
    return rotate_audio_yaw(_windows(ops, pcm, rows[:, 0].tolist(), n), rows[:, 4].tolist(), rows[:, 7].tolist())


def test_yaw_table_is_yaw_cos_sin(ops):
    from adyolo_amd.augmentations import yaw_cos_sin
    tab = ops.corpus_yaw_table(DEV).cpu().numpy()
    assert tab.shape == (360, 2) and tab.dtype == np.float32
    for phi in (-180, -179, -90, -1, 0, 1, 37, 90, 179):
        assert tuple(tab[phi + 180].view(np.int32)) == tuple(np.asarray(yaw_cos_sin(phi)).view(np.int32)), phi


@pytest.mark.parametrize("n", [1, 2, 255, 1001])
def test_gather_yaw_is_convert_then_rotate_audio_yaw(ops, pcm, n):
    last = S - n
    offs = [0, last, 1234, 2501, 101, 100, 17, 3000]              # even and odd window offsets, the first and the last window
    assert {o & 1 for o in offs} == {0, 1}
    combs = [5, -1, 15, 8, 0, 3, -1, 12]
    yaws = [37, -179, 0, 90, -180, 179, -90, 1]
    for lo in (0, 4):                                              # B = 4 per call
        items = _rows(offs[lo:lo + 4], combs[lo:lo + 4], yaws[lo:lo + 4])
        out, status = _gather(ops, pcm, items, n)
        assert status == 0
        ref = _gather_reference(ops, pcm, items, n)
        assert torch.equal(_bits(out), _bits(ref)), [j for j in range(4) if not torch.equal(_bits(out[j]), _bits(ref[j]))]
    # a yaw of 0 is the plain gather, bit for bit
    from adyolo_amd.augmentations import COMBINATIONS
    items = _rows(offs[:4], combs[:4], [0] * 4)
    plain = torch.empty(4, n, 4, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.corpus_gather(pcm, items.to(DEV), ops.corpus_rot_table(COMBINATIONS), plain, st)
    out, status = _gather(ops, pcm, items, n)
    assert status == 0 and int(st.item()) == 0 and torch.equal(_bits(out), _bits(plain))
    # a yaw outside [-180, 180), a combination past the last, a window outside the corpus: zeros for that item, the status bit
    good = _rows(offs[:4], combs[:4], yaws[:4])
    ref = _gather_reference(ops, pcm, good, n)
    for word, value in ((7, 180), (7, -181), (7, 1 << 40), (7, -(1 << 40)), (4, 16), (0, last + 1), (0, -1)):
        items = good.clone()
        items[2, word] = value
        out, status = _gather(ops, pcm, items, n)
        assert status == BAD_ITEM == ops.CORPUS_STATUS[1][0], (word, value)
        assert not bool(_bits(out[2]).any()), (word, value)
        for j in (0, 1, 3):
            assert torch.equal(_bits(out[j]), _bits(ref[j])), (word, value, j)


@pytest.mark.parametrize("n", [1, 2, 255, 1001])
def test_gather_yaw_mix_is_two_yawed_gathers_and_a_sum(ops, pcm, n):
    last = S - n
    pairs = [(0, last), (last, 0), (1234, 2501), (2501, 1234), (1233, 2501), (1234, 2502), (100, 101), (101, 100)]
    assert {(o & 1, m & 1) for o, m in pairs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    ca, cm = [5, -1, 15, 8, 0, 3, 12, 9], [0, 12, -1, 3, 7, 14, 1, 10]
    ya, ym = [37, -179, 0, 90, -180, 179, -90, 1], [-37, 0, 123, -90, 91, -1, 45, -180]
    gains = [(1.0, 0.5, float(np.float32(10.0 ** (-3.0 / 20.0))))[k % 3] for k in range(8)]
    assert all(x != y for x, y in zip(ca, cm)) and all(x != y for x, y in zip(ya, ym))
    for lo in (0, 4):
        items = _rows([p[0] for p in pairs[lo:lo + 4]], ca[lo:lo + 4], ya[lo:lo + 4])
        mates = _rows([p[1] for p in pairs[lo:lo + 4]], cm[lo:lo + 4], ym[lo:lo + 4], gains[lo:lo + 4])
        out, status = _gather(ops, pcm, items, n, mates)
        a, m = _gather_reference(ops, pcm, items, n), _gather_reference(ops, pcm, mates, n)
        g = mates[:, 6].to(torch.int32).view(torch.float32).to(DEV)
        ref = a + g[:, None, None] * m
        assert status == 0
        assert torch.equal(_bits(out), _bits(ref)), [j for j in range(4) if not torch.equal(_bits(out[j]), _bits(ref[j]))]
        assert not torch.equal(out, a)
    # an unmixed item between mixed ones has the plain yaw gather's bits; a bad mate (its yaw) zeroes its sample only
    items = _rows([2501, 100, 1234, last], ca[:4], ya[:4])
    mates = _rows([0, None, 101, 1233], cm[:4], ym[:4], gains[:4])
    plain, status = _gather(ops, pcm, items, n)
    assert status == 0
    out, status = _gather(ops, pcm, items, n, mates)
    assert status == 0 and torch.equal(_bits(out[1]), _bits(plain[1])) and not torch.equal(out[0], plain[0])
    for word, value in ((7, 180), (7, -181), (4, 16), (0, last + 1)):
        bad = mates.clone()
        bad[2, word] = value
        got, status = _gather(ops, pcm, items, n, bad)
        assert status == BAD_ITEM and not bool(_bits(got[2]).any()), (word, value)
        for j in (0, 1, 3):
            assert torch.equal(_bits(got[j]), _bits(out[j])), (word, value, j)
    bad_items = items.clone()
    bad_items[3, 7] = 180                                         # a bad item with a good mate is zeroed as well
    got, status = _gather(ops, pcm, bad_items, n, mates)
    assert status == BAD_ITEM and not bool(_bits(got[3]).any()) and torch.equal(_bits(got[0]), _bits(out[0]))
    none = _rows([None] * 4, [0] * 4, [0] * 4)                    # all unmixed: the plain yaw gather, word 7 of a no-mate row unread
    none[:, 7] = 999
    got, status = _gather(ops, pcm, items, n, none)
    assert status == 0 and torch.equal(_bits(got), _bits(plain))


# ------------------------------------------------------------------------------------------ adyolo_corpus_yolo_labels (yaw)
def _ev(cls, az, el=0.0):
    return [cls, 0, az, el]


# (frame offset on the recording's axis, {window-relative frame: events}); the default grid's azimuth cells are bounded at
# -157.5 + 45 k, so a whole yaw reaches a bound only from a half-degree azimuth
CHUNKS = (
    (0, {}),
    (100, {0: [_ev(3, 170.0, 10.0)], 5: [_ev(1, -170.0, -20.0), _ev(2, 143.0, 0.0)], 19: [_ev(4, -143.0, 45.0)],
           20: [_ev(5, 10.0, 10.0)]}),
    (40, {0: [_ev(6, -14.5, 5.0)], 5: [_ev(7, 75.5, 30.0)], 7: [_ev(8, -91.0, -60.0)], 19: [_ev(9, 179.0, 89.0)],
          25: [_ev(10, 1.0, 1.0)]}),
    (7, {5: [_ev(11, 45.0, 0.0), _ev(0, -45.0, 22.5), _ev(11, 135.0, -22.5)], 6: [_ev(1, -135.0, 67.5)],
         19: [_ev(2, 0.0, -67.5), _ev(3, 22.5, 0.0)]}),
)
MAX_EVENTS = 6
# (item chunk, item comb, item yaw, mate chunk or None, mate comb, mate yaw)
BATCHES = (
    [(1, -1, 37, None, 0, 0), (1, -1, -37, None, 0, 0), (2, -1, 37, None, 0, 0)],       # both wraps, 180 and -180, cell bounds
    [(1, 4, 37, 2, 0, -53), (2, 9, -179, 1, -1, 37), (3, 7, 1, None, 0, 0)],            # after a combination; a frame in both
    [(0, 3, 5, 0, 5, -5), (0, 0, 90, 1, 4, -90), (1, 12, 0, 0, 9, 179)],                 # empty sources on either side
    [(3, 12, -180, 3, 2, 179), (2, 15, 90, 3, 8, -90), (1, 0, -37, 1, 0, 37)],           # a chunk with itself under other yaws
)


def _event_table():
    ev, rows = [], []
    for f_off, label in CHUNKS:
        lo = len(ev)
        for fr, evs in label.items():
            ev += [[float(fr + f_off), float(e[0]), e[2], e[3]] for e in evs]
        rows.append((f_off, lo, len(ev) - lo))
    return torch.tensor(ev, dtype=torch.float64), rows


def _label_rows(pairs, rows, mix):
    items, mates = torch.zeros(len(pairs), 8, dtype=torch.int64), torch.zeros(len(pairs), 8, dtype=torch.int64)
    for j, (ca, ka, pa, cb, kb, pb) in enumerate(pairs):
        items[j] = torch.tensor([16 * ca, rows[ca][0], rows[ca][1], rows[ca][2], ka, 0, 0, pa])
        mates[j] = torch.tensor([-1, 0, 0, 0, -1, 0, 0, 0] if cb is None or not mix else
                                [16 * cb, rows[cb][0], rows[cb][1], rows[cb][2], kb, 0, _gain_word(0.5), pb])
    return items, mates


def _moved(chunk, comb, phi):
    from adyolo_amd.augmentations import rotate_labels, yaw_labels
    label = CHUNKS[chunk][1]
    return yaw_labels(label if comb < 0 else rotate_labels(label, comb), phi)


def _merged(pair, mix):
    from adyolo_amd.augmentations import merge_labels
    ca, ka, pa, cb, kb, pb = pair
    return merge_labels(_moved(ca, ka, pa), {} if cb is None or not mix else _moved(cb, kb, pb))


def _yolo_want(pairs, t, mix, skip=()):
    from adyolo_amd.datasets import YoloLabelEncoder, collate_fn
    enc = YoloLabelEncoder()
    labels = [[] if j in skip else enc.get_yolo_label(_merged(p, mix), t) for j, p in enumerate(pairs)]
    if not any(labels):
        return torch.zeros(0, 7)
    return collate_fn([(np.zeros(1, dtype=np.float32), r) for r in labels])[1]


def _yolo_run(ops, events, items, mates, t, cap, mix, yaw=True):
    from adyolo_amd.augmentations import COMBINATIONS
    from adyolo_amd.datasets import YoloLabelEncoder
    enc = YoloLabelEncoder()
    bounds = torch.from_numpy(np.concatenate([enc.az_lb, enc.az_ub, enc.el_lb, enc.el_ub]).astype(np.float64)).to(DEV)
    b = items.shape[0]
    words = ops.corpus_labels_workspace_words(b, MAX_EVENTS, mix=mix)
    ws = torch.full((words + 16,), -77, dtype=torch.int32, device=DEV)
    buf = torch.full((cap * 7 + 64,), 7.0, device=DEV)
    target = buf[:cap * 7].view(cap, 7)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.corpus_yolo_labels(events.to(DEV), items.to(DEV), MAX_EVENTS, t, bounds, (len(enc.az_lb), len(enc.el_lb)),
                           ops.corpus_rot_table(COMBINATIONS), ws, target, count, status, mates=mates.to(DEV) if mix else None,
                           yaw=yaw)
    torch.cuda.synchronize()
    assert bool((buf[cap * 7:] == 7.0).all()) and bool((ws[words:] == -77).all())
    return target.cpu(), int(count.item()), int(status.item())


@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("t", [1, 20])
def test_yolo_labels_yaw_are_the_rows_of_the_host_path(ops, t, mix):
    events, rows = _event_table()
    assert max(r[2] for r in rows) <= MAX_EVENTS
    for pairs in BATCHES:
        items, mates = _label_rows(pairs, rows, mix)
        want = _yolo_want(pairs, t, mix)
        m = want.shape[0]
        target, count, status = _yolo_run(ops, events, items, mates, t, 256, mix)
        assert status == 0 and count == m, (pairs, count, m)
        assert torch.equal(_bits(target[:m]), _bits(want)), pairs
        assert bool((target[m:, 0] == -1).all()) and not bool(target[m:, 1:].any())        # the b = -1 tail
    if t == 20:                                                   # the edges the events were chosen for did occur
        u = _yolo_want(BATCHES[0], t, mix)[:, 5].tolist()
        assert -153.0 in u and 153.0 in u                         # 170 + 37 wraps down, -170 - 37 wraps up
        assert u.count(-180.0) >= 2 and 180.0 not in u            # 143 + 37 = 180 -> -180 (the encoder), -143 - 37 = -180
        assert 22.5 in u and 112.5 in u                           # -14.5 + 37 and 75.5 + 37: on cell bounds of the default grid
        from adyolo_amd.augmentations import yaw_labels
        assert yaw_labels(CHUNKS[1][1], 37)[5][1][2] == 180.0 and yaw_labels(CHUNKS[1][1], -37)[19][0][2] == -180.0
        plain_rows = _yolo_run(ops, events, *_label_rows(BATCHES[0], rows, mix), t, 256, mix, yaw=False)[0]
        assert not torch.equal(plain_rows, _yolo_run(ops, events, *_label_rows(BATCHES[0], rows, mix), t, 256, mix)[0])
    # a yaw of 0 in every row: the rows of the un-yawed call
    pairs = [(ca, ka, 0, cb, kb, 0) for ca, ka, _, cb, kb, _ in BATCHES[1]]
    items, mates = _label_rows(pairs, rows, mix)
    assert [torch.equal(_bits(a), _bits(b)) if isinstance(a, torch.Tensor) else a == b for a, b in
            zip(_yolo_run(ops, events, items, mates, t, 256, mix), _yolo_run(ops, events, items, mates, t, 256, mix, yaw=False))] \
        == [True] * 3
    # a forced small capacity: the overflow bit, the rows up to the capacity correct -- as in the un-yawed calls
    pairs = BATCHES[1]
    items, mates = _label_rows(pairs, rows, mix)
    want = _yolo_want(pairs, t, mix)
    cap = 3
    assert want.shape[0] > cap
    target, count, status = _yolo_run(ops, events, items, mates, t, cap, mix)
    assert status == ops.CORPUS_STATUS[0][0] == 1 and count == want.shape[0]
    assert torch.equal(_bits(target), _bits(want[:cap]))
    # a bad row (more events than max_events, a combination past the last, a yaw outside the range): the bad-item bit, no rows
    # for that item, the others unchanged
    want = _yolo_want(pairs, t, mix, skip={0})
    for table, word, value in ((0, 3, MAX_EVENTS + 1), (0, 4, 16), (0, 7, 180), (0, 7, -181)) + \
            (((1, 7, 180), (1, 7, -181), (1, 3, MAX_EVENTS + 1)) if mix else ()):
        bad = [items.clone(), mates.clone()]
        bad[table][0, word] = value
        target, count, status = _yolo_run(ops, events, bad[0], bad[1], t, 256, mix)
        assert status == BAD_ITEM and count == want.shape[0], (table, word, value)
        assert torch.equal(_bits(target[:count]), _bits(want)) and bool((target[count:, 0] == -1).all())


# ------------------------------------------------------------------------------------- adyolo_corpus_classwise_labels (yaw)
CW_YAWS = (0, 90, -90, -180, 37, -179, 1, 179, -1, 123)          # -180 is the half turn: the legal range is [-180, 180)
CW_CHUNKS = (                    # whole degrees: the poles, elevation 0 (-0.0 under an elevation flip), +-180, signed zeros
    (3, {0: [_ev(0, 30.0, 90.0), _ev(1, -45.0, -90.0), _ev(2, 100.0, 0.0)],
         1: [_ev(3, 180.0, 10.0), _ev(3, -180.0, -10.0), _ev(4, -0.0, 0.0), _ev(0, 0.0, -0.0)],
         2: [_ev(1, 143.0, 45.0), _ev(1, -143.0, -45.0), _ev(1, 179.0, 89.0), _ev(1, 5.0, 5.0), _ev(2, -90.0, 0.0)],
         3: [_ev(4, 90.0, 60.0)]}),
    (50, {0: [_ev(2, -1.0, 0.0), _ev(0, 67.0, -67.0)], 1: [_ev(3, 1.0, 1.0)], 2: [_ev(1, -179.0, -89.0), _ev(4, 45.0, 90.0)]}),
)
CW_C = 5
CW_MAX_EVENTS = 16


@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("t", [3, 4])
def test_classwise_labels_yaw_are_the_host_encoders(ops, t, mix):
    from adyolo_amd.augmentations import COMBINATIONS, merge_labels, rotate_labels, yaw_labels
    from adyolo_amd.corpus import xyz_table
    from adyolo_amd.datasets import CLASSWISE_LABELS, ClasswiseLabelEncoder
    ev, rows = [], []
    for f_off, label in CW_CHUNKS:
        lo = len(ev)
        for fr, evs in label.items():
            ev += [[float(fr + f_off), float(e[0]), e[2], e[3]] for e in evs]
        rows.append((f_off, lo, len(ev) - lo))
    events = torch.tensor(ev, dtype=torch.float64)
    xyz = torch.from_numpy(xyz_table(events[:, 2].numpy(), events[:, 3].numpy())).to(DEV)
    cases = [(k, phi) for k in range(-1, 16) for phi in CW_YAWS]                      # all 16 combinations and comb = -1
    b = len(cases)
    items, mates = torch.zeros(b, 8, dtype=torch.int64), torch.zeros(b, 8, dtype=torch.int64)
    mate_of = []
    for j, (k, phi) in enumerate(cases):
        items[j] = torch.tensor([0, rows[0][0], rows[0][1], rows[0][2], k, 0, 0, phi])
        mk, mphi = (k + 6) % 17 - 1, CW_YAWS[(j * 3 + 1) % len(CW_YAWS)]
        mate_of.append(None if j % 7 == 3 else (mk, mphi))
        mates[j] = torch.tensor([-1, 0, 0, 0, -1, 0, 0, 0] if mate_of[j] is None else
                                [16, rows[1][0], rows[1][1], rows[1][2], mk, 0, _gain_word(1.0), mphi])
    enc = ClasswiseLabelEncoder(CW_C)

    def moved(c, k, phi):
        label = CW_CHUNKS[c][1]
        return yaw_labels(label if k < 0 else rotate_labels(label, k), phi)

    def label_of(j):
        la = moved(0, *cases[j])
        return merge_labels(la, moved(1, *mate_of[j])) if mix and mate_of[j] is not None else la
    rot, yaw_xyz = ops.corpus_rot_table(COMBINATIONS), ops.corpus_yaw_xyz_tables(DEV)
    for loss in ("seddoa", "accdoa", "adpit"):
        shape = ops.corpus_classwise_shape(loss, b, t, CW_C)
        n = int(np.prod(shape))
        buf = torch.full((n + 97,), 7.0, device=DEV)
        target = buf[:n].view(shape)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)

        def run(it, mt):
            buf.fill_(7.0)
            status.zero_()
            ops.corpus_classwise_labels(events.to(DEV), it.to(DEV), xyz, CW_MAX_EVENTS, t, CW_C, loss, target, status,
                                        mates=mt.to(DEV) if mix else None, rot=rot, yaw_xyz=yaw_xyz)
            torch.cuda.synchronize()
            assert bool((buf[n:] == 7.0).all())
            return int(status.item())

        assert run(items, mates) == 0
        got = target.cpu()
        want = torch.stack([getattr(enc, CLASSWISE_LABELS[loss])(label_of(j), t) for j in range(b)])
        diff = [cases[j] for j in range(b) if not torch.equal(_bits(got[j]), _bits(want[j]))]
        assert not diff, (loss, diff[:8])
        if loss == "seddoa":                                      # the edges did occur: z = -0.0 under an elevation flip, kept
            z = want[:, 1, 3 * CW_C + 4].view(torch.int32)
            assert bool((z == -2 ** 31).any()) and bool((z == 0).any())
            assert bool((want[:, 0, CW_C:2 * CW_C] != want[0, 0, CW_C:2 * CW_C]).any())   # the yaw moved x
        # a yaw of 0 everywhere: the bits of the un-yawed call (the table arithmetic against xyz_table)
        zero_i, zero_m = items.clone(), mates.clone()
        zero_i[:, 7] = 0
        zero_m[:, 7] = 0
        assert run(zero_i, zero_m) == 0
        plain = torch.full(shape, 7.0, device=DEV)
        ops.corpus_classwise_labels(events.to(DEV), zero_i.to(DEV), xyz, CW_MAX_EVENTS, t, CW_C, loss, plain, status,
                                    mates=zero_m.to(DEV) if mix else None)
        # (under a combination: without one the host keeps an azimuth of -0.0 as it is, and ``yaw_labels`` makes it -0.0 + 0 = +0.0)
        same = [j for j in range(b) if cases[j][0] >= 0 and (not mix or mate_of[j] is None or mate_of[j][0] >= 0)]
        assert len(same) > b // 2 and int(status.item()) == 0 and torch.equal(_bits(target[same]), _bits(plain[same]))
        # a bad yaw (item; with mix also the mate): that item zeros, the bit, the others unchanged
        for table, value in ((0, 180), (0, -181)) + (((1, 180),) if mix else ()):
            bad = [items.clone(), mates.clone()]
            bad[table][1, 7] = value
            assert mate_of[1] is not None
            assert run(bad[0], bad[1]) == BAD_ITEM
            again = target.cpu()
            assert not bool(again[1].any())
            assert torch.equal(_bits(again[0]), _bits(want[0])) and torch.equal(_bits(again[2:]), _bits(want[2:]))


# ------------------------------------------------------------------- what the merged argument lists refuse, on the host
def test_optional_tables_that_do_not_go_together_are_refused_before_any_launch(ops):
    from adyolo_amd._lib import AdyoloHipError
    from adyolo_amd.augmentations import COMBINATIONS, MIC_SWAP_COMBS, mic_swap_source
    rot, tab = ops.corpus_rot_table(COMBINATIONS), ops.corpus_yaw_table(DEV)
    mic = ops.corpus_mic_table({k: mic_swap_source(k) for k in MIC_SWAP_COMBS})
    pcm = torch.zeros(16, 4, dtype=torch.int16, device=DEV)
    items = _rows([0], [0], [0]).to(DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((1, 2, 4), 7.0, device=DEV)
    for r, kw in ((rot, {"yaw_tab": tab, "mic_src": mic}),         # there is no MIC yaw
                  (None, {"yaw_tab": tab, "mic_src": mic}),
                  (None, {}), (None, {"yaw_tab": tab})):            # neither rot nor mic_src
        with pytest.raises(AdyoloHipError):
            ops.corpus_gather(pcm, items, r, out, status, **kw)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and int(status.item()) == 0, (r is None, sorted(kw))
    events = torch.tensor([[0.0, 1.0, 30.0, 10.0]], dtype=torch.float64, device=DEV)
    xyz = torch.zeros(1, ops.CORPUS_XYZ_SLOTS, 3, device=DEV)
    items = torch.tensor([[0, 0, 0, 1, 0, 0, 0, 37]], dtype=torch.int64, device=DEV)
    target = torch.full(ops.corpus_classwise_shape("accdoa", 1, 2, CW_C), 7.0, device=DEV)
    with pytest.raises(AdyoloHipError):                            # yaw_xyz needs the rotation table
        ops.corpus_classwise_labels(events, items, xyz, CW_MAX_EVENTS, 2, CW_C, "accdoa", target, status,
                                    yaw_xyz=ops.corpus_yaw_xyz_tables(DEV))
    torch.cuda.synchronize()
    assert bool((target == 7.0).all()) and int(status.item()) == 0


# ------------------------------------------------------------------------------------------- corpus against the host path
def _prm(root, loss, mix):
    prm = yaw_params(root, loss, mix=mix, sr=SR, nb_classes=C_TRAIN, nb_iters=3)
    prm["args"]["device"] = DEV
    prm["train_config"].update({"loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
                                "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0})
    prm["aug_config"].update({"spec_augment_thresh": 0.8, "spec_augment_time_mask_param": 30, "spec_augment_freq_mask_param": 40})
    return prm


class _Recorder:
    """What ``train_one_epoch_audio`` needs of a trainer: the device and ``step``; keeps every step's inputs."""

    class _Flat:
        pass

    def __init__(self):
        self.flat, self.graphs, self.steps = self._Flat(), None, []
        self.flat.flat = torch.zeros(1, device=DEV)

    def step(self, audio, target, spec=None):
        self.steps.append((audio.clone(), target.clone(), None if spec is None else spec.clone()))
        return torch.zeros(1, device=audio.device)


@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("loss", ["adyolo", "adpit"])
def test_batches_equal_the_host_path(ops, split, loss, mix):
    from adyolo_amd.corpus import ClasswiseDeviceCorpus, DeviceCorpus, load_chunked_split
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    from adyolo_amd.train import train_one_epoch_audio
    prm = _prm(split, loss, mix)
    seed = 47
    random.seed(seed)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    host = _Recorder()
    for ep in range(2):
        if ep:
            ds.sample_filelist_for_train_iter()
        loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, collate_fn=audio_collate_fn, num_workers=0)
        train_one_epoch_audio(prm, loader, host)
    state = random.getstate()
    hc = load_chunked_split(prm, verify="all")
    random.seed(seed)
    corpus = (DeviceCorpus if loss == "adyolo" else ClasswiseDeviceCorpus)(hc, prm, DEV, rank=0, world=1)
    assert corpus.yaw == 1 and corpus.rotate
    got, yaws = [], set()
    for ep in range(2):
        if ep:
            corpus.sample_filelist_for_train_iter()
        for b0 in range(0, len(corpus), 4):
            drawn = corpus.draw(range(b0, b0 + 4))
            yaws |= set(drawn[0][:, 7].tolist())
            audio, target, spec = corpus.launch(drawn)
            got.append((audio.clone(), target.clone(), spec.clone(), corpus.rows.clone() if loss == "adyolo" else None))
    torch.cuda.synchronize()
    assert random.getstate() == state
    assert len(got) == len(host.steps) == 6 and len(yaws) >= 12
    for (ha, ht, hs), (audio, target, spec, rows) in zip(host.steps, got):
        assert torch.equal(_bits(audio), _bits(ha))
        if loss == "adyolo":
            m = ht.shape[0]
            assert int(rows.item()) == m and m > 0 and tuple(target.shape) == (corpus.cap, 7)
            assert torch.equal(_bits(target[:m].cpu()), _bits(ht.cpu())) and bool((target[m:, 0] == -1).all())
        else:
            assert tuple(target.shape) == tuple(ht.shape) == corpus.target_shape(4)
            assert torch.equal(_bits(target.cpu()), _bits(ht.cpu()))
        assert torch.equal(spec.cpu(), hs.cpu())
    assert int(corpus.status.item()) == 0
    corpus.check()


# ------------------------------------------------------------------------------------------------------------------ epoch
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("loss", ["adyolo", "adpit"])
def test_corpus_epoch_equals_the_host_epoch(ops, split, loss, graph):
    """Three train steps with ``rotation_augment`` + ``yaw_rotation_augment`` (the replayed runs with ``time_mix_augment`` as well)
    from the corpus and from ``FoaDataset`` + ``train_one_epoch_audio``, same seed: the same losses, parameters, Adam moments and
    BatchNorm statistics; replayed: ONE graph recorded, although every batch has other yaws in its item table."""
    from adyolo_amd.corpus import ClasswiseDeviceCorpus, DeviceCorpus, load_chunked_split
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    from adyolo_amd.train import train_one_epoch_audio, train_one_epoch_corpus
    prm = _prm(split, loss, mix=graph)
    seed = 53
    random.seed(seed)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, collate_fn=audio_collate_fn, num_workers=0)
    th = _trainer(graph, prm)
    mean_h = train_one_epoch_audio(prm, loader, th)
    state_h = random.getstate()
    hc = load_chunked_split(prm)
    random.seed(seed)
    corpus = (DeviceCorpus if loss == "adyolo" else ClasswiseDeviceCorpus)(hc, prm, DEV, rank=0, world=1)
    assert corpus.get_filelist() == ds.get_filelist() and corpus.yaw == 1
    tables = []
    draw = corpus.draw
    corpus.draw = lambda idx: tables.append(draw(idx)) or tables[-1]
    tc = _trainer(graph, prm)
    mean_c = train_one_epoch_corpus(prm, corpus, tc)
    torch.cuda.synchronize()
    assert random.getstate() == state_h
    assert len(th.recorded) == len(tc.recorded) == len(tables) == 3
    assert len({tuple(d[0][:, 7].tolist()) for d in tables}) == 3                     # every batch has other yaws
    for i, ((lh, _, _), (lc, _, _)) in enumerate(zip(th.recorded, tc.recorded)):
        assert bool(torch.isfinite(lc)) and torch.equal(lh, lc), (i, float(lh), float(lc))
    assert mean_h == mean_c
    assert torch.equal(th.flat.flat, tc.flat.flat) and bool(torch.isfinite(tc.flat.flat).all())
    assert torch.equal(th.optimizer.exp_avg, tc.optimizer.exp_avg)
    assert torch.equal(th.optimizer.exp_avg_sq, tc.optimizer.exp_avg_sq)
    for (k, a), (_, b) in zip(th.model.named_buffers(), tc.model.named_buffers()):
        assert torch.equal(a, b), k
    if graph:
        g = tc.graphs
        assert g.captures == 1 and g.replays == 2 and g.eager_steps == 1
        (key, ent), = g.entries.items()
        assert tuple(ent.target.shape) == corpus.target_shape(4)
        assert (tc.recorded[2][1], tc.recorded[2][2]) == (ent.audio.data_ptr(), ent.target.data_ptr())   # written in place
