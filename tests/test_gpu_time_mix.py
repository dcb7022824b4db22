"""GPU: the time-domain mixing augmentation (``aug_config.time_mix_augment``), every comparison bit for bit.
``adyolo_corpus_gather`` with mates against two plain gathers and ``a + g * m`` in torch (all parities of the two offsets, the first
and last window on either side, a no-mate and a bad mate between mixed items, both tables); ``adyolo_audio_mix`` in and out of
place; ``adyolo_corpus_yolo_labels`` with mates against ``get_yolo_label(merge_labels(...))`` + ``collate_fn``;
``adyolo_corpus_classwise_labels`` with mates against the three host encoders on the merged dict; both device corpora against
the host-fed path through ``train_one_epoch_audio``; and three training steps from the mixing corpus, eagerly and replayed from one hipGraph."""
import random

import numpy as np
import pytest
import torch

from test_corpus_classwise_cpu import classwise_params, write_classwise_split
from test_gpu_corpus_classwise import _trainer

pytestmark = pytest.mark.gpu

SR = 24000
RECS = (("fold1_room1_mix001", 6.0), ("fold1_room2_mix002", 3.7), ("fold2_room1_mix003", 2.0), ("take_chunk3_mix", 4.0))
C_TRAIN = 12
S = 5000                       # frames of the direct calls' pcm buffer
GAINS = (1.0, 0.5, float(np.float32(10.0 ** (-3.0 / 20.0))))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def mic_split(tmp_path_factory):
    root = tmp_path_factory.mktemp("gpu_time_mix")
    write_classwise_split(root, recordings=RECS, sr=SR, window_s=2, stride_s=1, seed=14, nb_classes=C_TRAIN, audio_dir="mic_dev")
    return root


@pytest.fixture(scope="module")
def pcm():
    g = torch.Generator().manual_seed(8)
    return torch.randint(-32768, 32768, (S, 4), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)


def _prm(root, loss, mix=True):
    prm = classwise_params(root, loss, batch_size=4, nb_iters=3, spec=True, rotation=False, window_s=2, stride_s=1, sr=SR,
                           nb_classes=C_TRAIN)
    prm["args"]["device"] = DEV
    prm["data_config"]["audio_format"] = "mic"
    prm["train_config"].update({"loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
                                "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0})
    prm["aug_config"].update({"channel_swap_augment": True, "spec_augment_thresh": 0.8, "spec_augment_time_mask_param": 30,
                              "spec_augment_freq_mask_param": 40})
    if mix:
        prm["aug_config"].update({"time_mix_augment": True, "time_mix_prob": 0.6, "time_mix_gain_db": [-6.0, 3.0]})
    return prm


def _bits(t):
    return t.contiguous().view(torch.int32)


def _gain_word(g):
    return int(np.float32(g).view(np.uint32))


def _rows(offs, combs, gains=None):
    """(B, 8) int64 item rows from offsets and combinations (offset None: the no-mate row); gains -> word 6."""
    rows = torch.zeros(len(offs), 8, dtype=torch.int64)
    for j, (o, c) in enumerate(zip(offs, combs)):
        if o is None:
            rows[j, 0], rows[j, 4] = -1, -1
            continue
        rows[j, 0], rows[j, 4] = o, c
        if gains is not None:
            rows[j, 6] = _gain_word(gains[j])
    return rows


# -------------------------------------------------------------------------------------------- adyolo_corpus_gather (mates)
def _tables(ops, mic):
    from adyolo_amd.augmentations import COMBINATIONS, MIC_SWAP_COMBS, mic_swap_source
    rot = ops.corpus_rot_table(COMBINATIONS)
    return rot, (ops.corpus_mic_table({k: mic_swap_source(k) for k in MIC_SWAP_COMBS}) if mic else None)


def _plain(ops, pcm, rows, n, mic):
    rot, src = _tables(ops, mic)
    out = torch.empty(rows.shape[0], n, 4, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.corpus_gather(pcm, rows.to(DEV), None if mic else rot, out, status, mic_src=src)
    assert int(status.item()) == 0
    return out


def _mix(ops, pcm, items, mates, n, mic):
    """One call -> (out, status word); a guard band behind the output must stay."""
    rot, src = _tables(ops, mic)
    b = items.shape[0]
    buf = torch.full((b * n * 4 + 64,), 7.0, device=DEV)
    out = buf[:b * n * 4].view(b, n, 4)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.corpus_gather(pcm, items.to(DEV), rot, out, status, mates=mates.to(DEV), mic_src=src)
    torch.cuda.synchronize()
    assert bool((buf[b * n * 4:] == 7.0).all())
    return out, int(status.item())


def _mix_reference(ops, pcm, items, mates, n, mic):
    a = _plain(ops, pcm, items, n, mic)
    m = _plain(ops, pcm, mates, n, mic)
    g = mates[:, 6].to(torch.int32).view(torch.float32).to(DEV)
    return a + g[:, None, None] * m, a


@pytest.mark.parametrize("mic", [False, True], ids=["foa", "mic"])
@pytest.mark.parametrize("n", [1, 2, 255, 1027])
def test_gather_mix_is_two_gathers_and_a_sum(ops, pcm, n, mic):
    from adyolo_amd.augmentations import MIC_SWAP_COMBS
    last = S - n
    pairs = [(0, last), (last, 0), (1234, 2501), (2501, 1234), (1233, 2501), (1234, 2502), (100, 101), (101, 100)]
    assert {(o & 1, m & 1) for o, m in pairs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    if mic:
        ca = [MIC_SWAP_COMBS[k % 8] for k in (1, 0, 5, 2, 7, 3, 4, 6)]
        cm = [MIC_SWAP_COMBS[k % 8] for k in (4, 6, -1, 1, 0, 7, 2, 5)]
        ca[1], cm[2] = -1, -1
    else:
        ca, cm = [5, -1, 15, 8, 0, 3, 12, 9], [0, 12, -1, 3, 7, 14, 1, 10]
    assert all(x != y for x, y in zip(ca, cm))
    gains = [GAINS[k % 3] for k in range(8)]
    for lo in (0, 4):                                              # B = 4 per call
        items = _rows([p[0] for p in pairs[lo:lo + 4]], ca[lo:lo + 4])
        mates = _rows([p[1] for p in pairs[lo:lo + 4]], cm[lo:lo + 4], gains[lo:lo + 4])
        out, status = _mix(ops, pcm, items, mates, n, mic)
        ref, a = _mix_reference(ops, pcm, items, mates, n, mic)
        assert status == 0
        assert torch.equal(_bits(out), _bits(ref)), [j for j in range(4) if not torch.equal(_bits(out[j]), _bits(ref[j]))]
        assert not torch.equal(out, a)                             # the mates did add something
    # a no-mate item and a bad mate between mixed ones
    items = _rows([2501, 100, 1234, last], ca[:4])
    for bad_word, bad_value in ((0, last + 1), (0, -2), (4, 16)) + (((4, 1),) if mic else ()):      # 1: no symmetry of the array
        mates = _rows([0, None, 101, 1233], cm[:4], gains[:4])
        good = mates.clone()
        mates[2, bad_word] = bad_value
        out, status = _mix(ops, pcm, items, mates, n, mic)
        good[2] = good[0]                                          # any valid row: only rows 0 and 3 of the reference are read
        ref, a = _mix_reference(ops, pcm, items, torch.where(good[:, :1] == -1, good[0], good), n, mic)
        assert status == ops.CORPUS_STATUS[1][0] == 2
        assert torch.equal(_bits(out[1]), _bits(a[1]))             # no mate: the plain gather
        assert not bool(_bits(out[2]).any())                       # bad mate: zeros for that sample only
        for j in (0, 3):
            assert torch.equal(_bits(out[j]), _bits(ref[j])), j
    # a bad item with a good mate is zeroed as well; all items without a mate: the plain gather, no status bit
    mates = _rows([0, None, 101, 1233], cm[:4], gains[:4])
    bad_items = items.clone()
    bad_items[3, 0] = last + 1
    out, status = _mix(ops, pcm, bad_items, mates, n, mic)
    assert status == 2 and not bool(_bits(out[3]).any()) and torch.equal(_bits(out[1]), _bits(a[1]))
    out, status = _mix(ops, pcm, items, _rows([None] * 4, [0] * 4), n, mic)
    assert status == 0 and torch.equal(_bits(out), _bits(a))


def test_gather_mix_refusals(ops, pcm):
    from adyolo_amd._lib import AdyoloHipError
    rot, _ = _tables(ops, False)
    items = _rows([0, 10], [0, 1]).to(DEV)
    out = torch.empty(2, 16, 4, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(AdyoloHipError, match="mates"):
        ops.corpus_gather(pcm, items, rot, out, status, mates=items[:1])
    with pytest.raises(AdyoloHipError, match="mates"):
        ops.corpus_gather(pcm, items, rot, out, status, mates=items.to(torch.int32))
    with pytest.raises(AdyoloHipError, match="rotation table"):
        ops.corpus_gather(pcm, items, None, out, status, mates=items)


# ------------------------------------------------------------------------------------------------------- adyolo_audio_mix
@pytest.mark.parametrize("n", [1, 2, 255, 1027])
def test_audio_mix_in_and_out_of_place(ops, n):
    g = torch.Generator().manual_seed(200 + n)
    audio = (torch.rand(3, n, 4, generator=g) * 2 - 1)
    mate = (torch.rand(3, n, 4, generator=g) * 2 - 1)
    special = torch.tensor([0x7FC00001, -0x80000000, -0x3EDCBB, 0x00000001], dtype=torch.int64).to(torch.int32).view(torch.float32)
    audio[1, 0] = special                                          # the unmixed clip: a NaN with a payload, -0.0, ...
    audio[0, n - 1, 1] = -0.0
    mate[1] = float("nan")                                         # never read
    gains = torch.tensor([GAINS[2], 123.0, 0.5])
    mixed = torch.tensor([True, False, True])
    want = torch.where(mixed[:, None, None], audio + gains[:, None, None] * mate, audio)
    want_bits = torch.where(mixed[:, None, None], _bits(want), _bits(audio))
    a, m = audio.to(DEV), mate.to(DEV)
    buf = torch.full((3 * n * 4 + 64,), 7.0, device=DEV)
    out = buf[:3 * n * 4].view(3, n, 4)
    got = ops.audio_mix(a, m, gains.to(DEV), mixed.to(DEV), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and bool((buf[3 * n * 4:] == 7.0).all())
    assert torch.equal(_bits(out).cpu(), want_bits)
    assert torch.equal(_bits(a).cpu(), _bits(audio)) and torch.equal(_bits(m[0]).cpu(), _bits(mate[0]))     # inputs only read
    fresh = ops.audio_mix(a, m, gains.to(DEV), mixed.to(DEV))
    assert fresh.data_ptr() != a.data_ptr() and torch.equal(_bits(fresh).cpu(), want_bits)
    same = ops.audio_mix(a, m, gains.to(DEV), mixed.to(DEV), out=a)                                       # in place
    assert same.data_ptr() == a.data_ptr() and torch.equal(_bits(a).cpu(), want_bits)
    # the device arithmetic is the torch expression on the device as well (product rounded, then the sum)
    a2 = audio.to(DEV)
    assert torch.equal(_bits((a2 + gains.to(DEV)[:, None, None] * m)[0]), _bits(out[0]))


def test_audio_mix_refusals(ops):
    from adyolo_amd._lib import AdyoloHipError
    a = torch.zeros(2, 16, 4, device=DEV)
    gains, mixed = torch.ones(2, device=DEV), torch.ones(2, dtype=torch.bool, device=DEV)
    big = torch.zeros(2 * 16 * 4 + 4, device=DEV)
    lo, hi = big[:128].view(2, 16, 4), big[4:].view(2, 16, 4)         # one frame apart: overlapping, neither in place nor apart
    with pytest.raises(AdyoloHipError, match="overlaps"):
        ops.audio_mix(lo, a, gains, mixed, out=hi)
    with pytest.raises(AdyoloHipError, match="overlaps"):
        ops.audio_mix(a, lo, gains, mixed, out=hi)
    with pytest.raises(AdyoloHipError, match="mixed"):
        ops.audio_mix(a, a.clone(), gains, mixed.to(torch.uint8))
    with pytest.raises(AdyoloHipError, match="gains"):
        ops.audio_mix(a, a.clone(), gains[:1], mixed)
    with pytest.raises(AdyoloHipError):
        ops.audio_mix(a, a.clone()[:, :8], gains, mixed)


# ---------------------------------------------------------------------------------------- adyolo_corpus_yolo_labels (mates)
def _ev(cls, az, el=0.0):
    return [cls, 0, az, el]


CHUNKS = (                       # (frame offset on the recording's axis, {window-relative frame: events}), frames ascending
    (0, {}),
    (100, {0: [_ev(3, 170.0, 10.0)], 5: [_ev(1, -30.0, -20.0), _ev(2, 180.0, 0.0)], 19: [_ev(4, 0.0, 45.0)],
           20: [_ev(5, 10.0, 10.0)]}),
    (40, {0: [_ev(6, -170.0, 5.0)], 5: [_ev(7, 90.0, 30.0)], 7: [_ev(8, -91.0, -60.0)], 19: [_ev(9, 179.0, 89.0)],
          25: [_ev(10, 1.0, 1.0)]}),
    (7, {5: [_ev(11, 45.0, 0.0), _ev(0, -45.0, 22.5), _ev(11, 135.0, -22.5)], 6: [_ev(1, -135.0, 67.5)],
         19: [_ev(2, 0.0, -67.5), _ev(3, 22.5, 0.0)]}),
)
MAX_EVENTS = 6


def _event_table():
    """-> (events float64 (E, 4) {frame, class, az, el}, rows [(frame offset, first event, count)] per chunk)"""
    ev, rows = [], []
    for f_off, label in CHUNKS:
        lo = len(ev)
        for fr, evs in label.items():
            ev += [[float(fr + f_off), float(e[0]), e[2], e[3]] for e in evs]
        rows.append((f_off, lo, len(ev) - lo))
    return torch.tensor(ev, dtype=torch.float64), rows


def _label_rows(pairs, rows):
    """[(item chunk, item comb, mate chunk or None, mate comb)] -> (items, mates) int64 (B, 8)"""
    items, mates = torch.zeros(len(pairs), 8, dtype=torch.int64), torch.zeros(len(pairs), 8, dtype=torch.int64)
    for j, (ca, ka, cb, kb) in enumerate(pairs):
        items[j] = torch.tensor([16 * ca, rows[ca][0], rows[ca][1], rows[ca][2], ka, 0, 0, 0])
        mates[j] = torch.tensor([-1, 0, 0, 0, -1, 0, 0, 0] if cb is None else
                                [16 * cb, rows[cb][0], rows[cb][1], rows[cb][2], kb, 0, _gain_word(0.5), 0])
    return items, mates


def _merged(pair):
    from adyolo_amd.augmentations import merge_labels, rotate_labels
    ca, ka, cb, kb = pair
    la = CHUNKS[ca][1] if ka < 0 else rotate_labels(CHUNKS[ca][1], ka)
    if cb is None:
        return merge_labels(la, {})
    return merge_labels(la, CHUNKS[cb][1] if kb < 0 else rotate_labels(CHUNKS[cb][1], kb))


def _yolo_want(pairs, t, skip=()):
    from adyolo_amd.datasets import YoloLabelEncoder, collate_fn
    enc = YoloLabelEncoder()
    labels = [[] if j in skip else enc.get_yolo_label(_merged(p), t) for j, p in enumerate(pairs)]
    if not any(labels):
        return torch.zeros(0, 7)
    return collate_fn([(np.zeros(1, dtype=np.float32), r) for r in labels])[1]


def _yolo_run(ops, events, items, mates, t, cap):
    from adyolo_amd.augmentations import COMBINATIONS
    from adyolo_amd.datasets import YoloLabelEncoder
    enc = YoloLabelEncoder()
    bounds = torch.from_numpy(np.concatenate([enc.az_lb, enc.az_ub, enc.el_lb, enc.el_ub]).astype(np.float64)).to(DEV)
    b = items.shape[0]
    words = ops.corpus_labels_workspace_words(b, MAX_EVENTS, mix=True)
    assert words == b * 2 * MAX_EVENTS
    ws = torch.full((words + 16,), -77, dtype=torch.int32, device=DEV)
    buf = torch.full((cap * 7 + 64,), 7.0, device=DEV)
    target = buf[:cap * 7].view(cap, 7)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.corpus_yolo_labels(events.to(DEV), items.to(DEV), MAX_EVENTS, t, bounds, (len(enc.az_lb), len(enc.el_lb)),
                           ops.corpus_rot_table(COMBINATIONS), ws, target, count, status, mates=mates.to(DEV))
    torch.cuda.synchronize()
    assert bool((buf[cap * 7:] == 7.0).all()) and bool((ws[words:] == -77).all())
    return target.cpu(), int(count.item()), int(status.item())


BATCHES = (
    [(0, 3, 0, 5), (0, 0, 1, 4), (1, 4, 0, 9)],                  # both empty; only the item empty; only the mate empty
    [(1, 4, 2, 0), (2, -1, 1, -1), (3, 7, None, 0)],             # a frame in both; 170 degrees wraps under 4, not under 0; no mate
    [(3, 12, 3, 2), (2, 15, 3, 8), (1, 0, 1, 0)],                # a chunk with itself under another combination, and under the same
)


@pytest.mark.parametrize("t", [1, 20])
def test_yolo_labels_mix_are_the_rows_of_the_merged_labels(ops, t):
    events, rows = _event_table()
    assert max(r[2] for r in rows) <= MAX_EVENTS
    for pairs in BATCHES:
        items, mates = _label_rows(pairs, rows)
        want = _yolo_want(pairs, t)
        m = want.shape[0]
        target, count, status = _yolo_run(ops, events, items, mates, t, 256)
        assert status == 0 and count == m, (pairs, count, m)
        assert torch.equal(_bits(target[:m]), _bits(want)), pairs
        assert bool((target[m:, 0] == -1).all()) and not bool(target[m:, 1:].any())        # the b = -1 tail
    # the wrap: 170 + 180 under combination 4 is -10, and 170 stays under 0
    if t == 20:
        w = _yolo_want([BATCHES[1][0]], t)
        assert bool((w[:, 5] == -10.0).any()) and bool((_yolo_want([(1, 0, None, 0)], t)[:, 5] == 170.0).any())
        both = _yolo_want([BATCHES[1][0]], t)
        f0 = both[both[:, 1] == 0]
        assert set(f0[:, 4].tolist()) == {3.0, 6.0} and f0[0, 4] == 3.0 and f0[-1, 4] == 6.0  # the item's event first
    # a forced small capacity: the overflow bit, the rows up to the capacity correct
    pairs = BATCHES[1]
    items, mates = _label_rows(pairs, rows)
    want = _yolo_want(pairs, t)
    cap = 3
    assert want.shape[0] > cap
    target, count, status = _yolo_run(ops, events, items, mates, t, cap)
    assert status == ops.CORPUS_STATUS[0][0] == 1 and count == want.shape[0]
    assert torch.equal(_bits(target), _bits(want[:cap]))
    # a mate with more events than max_events: the bad-item bit, no rows for that item, the others unchanged
    bad = mates.clone()
    bad[0, 3] = MAX_EVENTS + 1
    want = _yolo_want(pairs, t, skip={0})
    target, count, status = _yolo_run(ops, events, items, bad, t, 256)
    assert status == 2 and count == want.shape[0]
    assert torch.equal(_bits(target[:count]), _bits(want)) and bool((target[count:, 0] == -1).all())
    # all items unmixed: the rows of the existing call
    from adyolo_amd.augmentations import COMBINATIONS
    from adyolo_amd.datasets import YoloLabelEncoder
    enc = YoloLabelEncoder()
    none = mates.clone()
    none[:] = torch.tensor([-1, 0, 0, 0, -1, 0, 0, 0])
    target, count, status = _yolo_run(ops, events, items, none, t, 256)
    plain = torch.full((256, 7), 7.0, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(ops.corpus_labels_workspace_words(3, MAX_EVENTS), dtype=torch.int32, device=DEV)
    bounds = torch.from_numpy(np.concatenate([enc.az_lb, enc.az_ub, enc.el_lb, enc.el_ub]).astype(np.float64)).to(DEV)
    ops.corpus_yolo_labels(events.to(DEV), items.to(DEV), MAX_EVENTS, t, bounds, (len(enc.az_lb), len(enc.el_lb)),
                           ops.corpus_rot_table(COMBINATIONS), ws, plain, cnt, st)
    assert status == 0 and count == int(cnt.item()) and torch.equal(_bits(target), _bits(plain.cpu()))


# ----------------------------------------------------------------------------------- adyolo_corpus_classwise_labels (mates)
CW_CASES = ((1, 1), (2, 1), (2, 2), (1, 0), (0, 1), (0, 3), (3, 1), (1, 2))     # same-class events (item, mate) in one frame
CW_MAX_EVENTS = 80


def _cw_chunks(n_classes, n_frames):
    """Four chunk pairs (item, mate): frame f of pair j holds case (f + j) % 8 of ``CW_CASES`` in class (5 f + j) % C, plus (C > 1)
    an event of the next class in the item on odd frames and in the mate on frames f % 3 == 0; two frames past the label
    frames hold events too.  Every event has its own angles."""
    k = [0]

    def ev(cls):
        k[0] += 1
        return [cls, 0, float(-175 + (k[0] * 13) % 350), float(-80 + (k[0] * 7) % 160)]
    chunks = []
    for j in range(4):
        a, b = {}, {}
        for f in range(n_frames + 2):
            na, nb = CW_CASES[(f + j) % 8]
            cls = (5 * f + j) % n_classes
            ea, eb = [ev(cls) for _ in range(na)], [ev(cls) for _ in range(nb)]
            if n_classes > 1 and f % 2:
                ea.insert(len(ea) // 2, ev((cls + 1) % n_classes))
            if n_classes > 1 and f % 3 == 0:
                eb.append(ev((cls + 1) % n_classes))
            if ea:
                a[f] = ea
            if eb:
                b[f] = eb
        chunks += [(11 * j, a), (1000 + 3 * j, b)]
    return chunks


@pytest.mark.parametrize("t", [1, 8, 9, 20])
@pytest.mark.parametrize("n_classes", [1, 13])
def test_classwise_labels_mix_are_the_encoders_on_the_merged_labels(ops, n_classes, t):
    from adyolo_amd.augmentations import merge_labels, rotate_labels
    from adyolo_amd.corpus import xyz_table
    from adyolo_amd.datasets import CLASSWISE_LABELS, ClasswiseLabelEncoder
    chunks = _cw_chunks(n_classes, t)
    ev, rows = [], []
    for f_off, label in chunks:
        lo = len(ev)
        for fr, evs in label.items():
            ev += [[float(fr + f_off), float(e[0]), e[2], e[3]] for e in evs]
        rows.append((f_off, lo, len(ev) - lo))
    assert max(r[2] for r in rows) <= CW_MAX_EVENTS
    events = torch.tensor(ev, dtype=torch.float64)
    xyz = torch.from_numpy(xyz_table(events[:, 2].numpy(), events[:, 3].numpy())).to(DEV)
    combs = [(5, 12), (-1, -1), (15, 0), (0, 9)]                  # (item, mate): different slots of the xyz table
    items, mates = torch.zeros(4, 8, dtype=torch.int64), torch.zeros(4, 8, dtype=torch.int64)
    for j in range(4):
        ra, rb = rows[2 * j], rows[2 * j + 1]
        items[j] = torch.tensor([0, ra[0], ra[1], ra[2], combs[j][0], 0, 0, 0])
        mates[j] = torch.tensor([16, rb[0], rb[1], rb[2], combs[j][1], 0, _gain_word(1.0), 0])
    mates[3] = torch.tensor([-1, 0, 0, 0, -1, 0, 0, 0])           # item 3 has no mate
    enc = ClasswiseLabelEncoder(n_classes)

    def rot(label, comb):
        return label if comb < 0 else rotate_labels(label, comb)

    def merged(j, drop=None):
        lb = {} if j == 3 else rot(chunks[2 * j + 1][1], combs[j][1])
        if drop is not None and drop[0] == j:
            lb = {f: [e for i, e in enumerate(evs) if (f, i) != drop[1:]] for f, evs in lb.items()}
        return merge_labels(rot(chunks[2 * j][1], combs[j][0]), lb)

    for loss in ("seddoa", "accdoa", "adpit"):
        shape = ops.corpus_classwise_shape(loss, 4, t, n_classes)
        n = int(np.prod(shape))
        buf = torch.full((n + 97,), 7.0, device=DEV)
        target = buf[:n].view(shape)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)

        def run(it, mt, events=events):
            buf.fill_(7.0)
            status.zero_()
            ops.corpus_classwise_labels(events.to(DEV), it.to(DEV), xyz, CW_MAX_EVENTS, t, n_classes, loss, target, status,
                                        mates=mt.to(DEV))
            torch.cuda.synchronize()
            assert bool((buf[n:] == 7.0).all())
            return int(status.item())

        def want(j, drop=None):
            return getattr(enc, CLASSWISE_LABELS[loss])(merged(j, drop), t)

        assert run(items, mates) == 0
        for j in range(4):
            assert torch.equal(_bits(target[j].cpu()), _bits(want(j))), (loss, j)
        if loss == "adpit":                                       # the count cases did land in all three groups of slots
            got = target[:3].cpu()
            assert bool(got[:, :, 0, 0].any()) or t == 1
            assert bool(got[:, :, 1:3, 0].any()) and bool(got[:, :, 3:, 0].any())
        # the no-mate item equals the existing call on the same row
        plain = torch.full(shape, 7.0, device=DEV)
        ops.corpus_classwise_labels(events.to(DEV), items.to(DEV), xyz, CW_MAX_EVENTS, t, n_classes, loss, plain, status)
        assert int(status.item()) == 0 and torch.equal(_bits(target[3]), _bits(plain[3]))
        assert not torch.equal(target[0], plain[0])
        # a bad mate (more events than max_events, a combination past the last): that item zeros, the others unchanged
        for word, value in ((3, CW_MAX_EVENTS + 1), (4, 16), (2, len(ev) + 1)):
            bad = mates.clone()
            bad[1, word] = value
            assert run(items, bad) == 2
            assert not bool(target[1].any())
            for j in (0, 2, 3):
                assert torch.equal(_bits(target[j].cpu()), _bits(want(j))), (loss, word, j)
        # an event of the mate with a class outside [0, C): dropped, status bit 4
        f_bad = 0
        e_bad = rows[1][1]                                        # the first event of item 0's mate: frame 0, index 0
        assert chunks[1][1][f_bad][0][0] == int(ev[e_bad][1])
        for cls in (n_classes, -1):
            changed = events.clone()
            changed[e_bad, 1] = cls
            assert run(items, mates, changed) == 4
            assert torch.equal(_bits(target[0].cpu()), _bits(want(0, drop=(0, f_bad, 0)))), (loss, cls)
            for j in (1, 2, 3):
                assert torch.equal(_bits(target[j].cpu()), _bits(want(j))), (loss, cls, j)


# ------------------------------------------------------------------------------------------- corpus against the host path
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


@pytest.mark.parametrize("loss", ["adyolo", "adpit"])
def test_batches_equal_the_host_path(ops, mic_split, loss):
    from adyolo_amd.corpus import ClasswiseDeviceCorpus, DeviceCorpus, load_chunked_split
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    from adyolo_amd.train import train_one_epoch_audio
    prm = _prm(mic_split, loss)
    seed = 43
    random.seed(seed)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    host_first_files = list(ds.get_filelist()[:4])
    host = _Recorder()
    mixed = []
    for ep in range(2):
        if ep:
            ds.sample_filelist_for_train_iter()
        loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, collate_fn=audio_collate_fn, num_workers=0)
        train_one_epoch_audio(prm, loader, host)
    state = random.getstate()
    hc = load_chunked_split(prm, verify="all")
    random.seed(seed)
    corpus = (DeviceCorpus if loss == "adyolo" else ClasswiseDeviceCorpus)(hc, prm, DEV, rank=0, world=1)
    assert corpus.swap and corpus.mix == (0.6, -6.0, 3.0)
    got = []
    for ep in range(2):
        if ep:
            corpus.sample_filelist_for_train_iter()
        for b0 in range(0, len(corpus), 4):
            drawn = corpus.draw(range(b0, b0 + 4))
            mixed += (drawn[2][:, 0] != -1).tolist()
            audio, target, spec = corpus.launch(drawn)
            got.append((audio.clone(), target.clone(), spec.clone(), corpus.rows.clone() if loss == "adyolo" else None))
    torch.cuda.synchronize()
    assert random.getstate() == state
    assert len(got) == len(host.steps) == 6
    assert 6 <= sum(mixed) <= 22, mixed
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
    # the mixing does change the batches: without the key the same seed draws no mates and a mixed item has other audio
    random.seed(seed)
    plain = (DeviceCorpus if loss == "adyolo" else ClasswiseDeviceCorpus)(hc, _prm(mic_split, loss, mix=False), DEV, rank=0, world=1)
    assert plain.get_filelist()[:4] == host_first_files and plain.mix is None
    drawn = plain.draw(range(4))
    assert len(drawn) == 2
    audio_off = plain.launch(drawn)[0]
    j = mixed[:4].index(True)
    assert not torch.equal(audio_off[j], got[0][0][j])


# ------------------------------------------------------------------------------------------------------------------ epoch
def test_mixing_corpus_replayed_equals_eager(ops, mic_split):
    """Three steps of ``train_one_epoch_corpus`` at test size from the mixing AD-YOLO corpus (the doubled row capacity), eagerly
    and through ``StepGraphs``: the same losses and parameter bits, one graph recorded."""
    from adyolo_amd.corpus import DeviceCorpus, load_chunked_split
    from adyolo_amd.train import train_one_epoch_corpus
    prm = _prm(mic_split, "adyolo")
    hc = load_chunked_split(prm)
    runs = []
    for graph in (False, True):
        random.seed(37)
        corpus = DeviceCorpus(hc, prm, DEV, rank=0, world=1)
        tr = _trainer(graph, prm, mic=True)
        train_one_epoch_corpus(prm, corpus, tr)
        torch.cuda.synchronize()
        runs.append((tr, corpus))
    (eager, _), (replayed, corpus) = runs
    assert len(eager.recorded) == len(replayed.recorded) == 3
    assert replayed.graphs.captures == 1 and replayed.graphs.replays == 2
    (key, ent), = replayed.graphs.entries.items()
    assert tuple(ent.target.shape) == (corpus.cap, 7)
    for i, ((le, _, _), (lr, _, _)) in enumerate(zip(eager.recorded, replayed.recorded)):
        assert bool(torch.isfinite(le)) and torch.equal(le, lr), (i, float(le), float(lr))
    assert torch.equal(eager.flat.flat, replayed.flat.flat)
    assert torch.equal(eager.optimizer.exp_avg, replayed.optimizer.exp_avg)
    assert bool(torch.isfinite(eager.flat.flat).all())
