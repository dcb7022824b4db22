"""GPU: the MIC channel-swap augmentation's two kernels and its training paths.  ``adyolo_mic_swap`` (csrc/aug.hip) against
tensor indexing on raw 32-bit patterns (NaN payloads, infinities and -0.0 keep their bits); ``adyolo_corpus_gather`` (MIC form)
(csrc/corpus.hip) against ``pcm16_to_f32`` followed by ``swap_audio``, bit for bit, at even and odd offsets, the first and the
last window of the buffer, odd lengths, comb -1 against the FOA gather's comb -1, and a bad item between good ones;
``DeviceCorpus`` / ``ClasswiseDeviceCorpus`` with ``aug_config.channel_swap_augment`` against the host path iterated in the main
process; and BASELINE config 5 at test size with the key on, eagerly and replayed from a hipGraph."""
import random

import pytest
import torch

from test_corpus_classwise_cpu import classwise_params, write_classwise_split
from test_gpu_corpus_classwise import _trainer

pytestmark = pytest.mark.gpu

SR = 24000
RECS = (("fold1_room1_mix001", 6.0), ("fold1_room2_mix002", 3.7), ("fold2_room1_mix003", 2.0), ("take_chunk3_mix", 4.0))
#        5 + 3 + 1 + 3 = 12 chunks of 2 s (1 s stride): 48000 samples, 20 label frames, the test model's shape
C_TRAIN = 12
S = 5000                       # frames of the direct calls' pcm buffer
SPECIAL = (0x7FC00001, -0x3EDCBB, 0x7F800000, -0x800000, -0x80000000, 0x7F800001, 0x00000001, -0x7FFFFFFF)
#          quiet NaN with a payload, a negative NaN (0xffc12345), +inf, -inf, -0.0, a signalling NaN, the two smallest denormals


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def mic_split(tmp_path_factory):
    root = tmp_path_factory.mktemp("gpu_mic_swap")
    write_classwise_split(root, recordings=RECS, sr=SR, window_s=2, stride_s=1, seed=14, nb_classes=C_TRAIN, audio_dir="mic_dev")
    return root


@pytest.fixture(scope="module")
def pcm():
    g = torch.Generator().manual_seed(8)
    return torch.randint(-32768, 32768, (S, 4), generator=g, dtype=torch.int32).to(torch.int16).to("cuda:0")


def _prm(root, loss, swap=True):
    prm = classwise_params(root, loss, batch_size=4, nb_iters=3, spec=True, rotation=False, window_s=2, stride_s=1, sr=SR,
                           nb_classes=C_TRAIN)
    prm["args"]["device"] = "cuda:0"
    prm["data_config"]["audio_format"] = "mic"
    prm["train_config"].update({"optim": "Adam", "lr": 1e-3, "weight_decay": 0.0})
    prm["aug_config"].update({"channel_swap_augment": swap, "spec_augment_thresh": 0.8, "spec_augment_time_mask_param": 30,
                              "spec_augment_freq_mask_param": 40})
    return prm


def _bits(t):
    return t.contiguous().view(torch.int32)


# -------------------------------------------------------------------------------------------------------- adyolo_mic_swap
@pytest.mark.parametrize("n", [1, 2, 255, 1027])
def test_mic_swap_moves_the_bits(ops, n):
    """B = 3, three different combinations per batch, every combination of the set in every batch position; the input is random
    32-bit patterns with the special values in the first frames; a guard band behind the output."""
    from adyolo_amd.augmentations import MIC_SWAP_COMBS, mic_swap_source, swap_audio
    g = torch.Generator().manual_seed(100 + n)
    bits = torch.randint(-2 ** 31, 2 ** 31, (3, n, 4), generator=g, dtype=torch.int64).to(torch.int32)
    flat = bits.view(-1)
    k = min(flat.numel(), len(SPECIAL))
    flat[:k] = torch.tensor(SPECIAL[:k], dtype=torch.int64).to(torch.int32)
    if n > 1:
        bits[1, 1] = torch.tensor(SPECIAL[4:8], dtype=torch.int64).to(torch.int32)
        bits[2, n - 1] = torch.tensor(SPECIAL[:4], dtype=torch.int64).to(torch.int32)
    audio = bits.view(torch.float32).to("cuda:0")
    for i, comb in enumerate(MIC_SWAP_COMBS):
        combs = [comb, MIC_SWAP_COMBS[(i + 1) % 8], MIC_SWAP_COMBS[(i + 3) % 8]]
        assert len(set(combs)) == 3
        want = torch.stack([bits[b][:, list(mic_swap_source(c))] for b, c in enumerate(combs)])
        out = swap_audio(audio, combs)
        assert out.data_ptr() != audio.data_ptr()
        assert torch.equal(_bits(out).cpu(), want), (n, combs)
    # a table value outside 0..3 cannot address outside the frame (the kernel masks it); the output's neighbours stay
    buf = torch.full((3 * n * 4 + 64,), 7.0, device="cuda:0")
    out = buf[:3 * n * 4].view(3, n, 4)
    src = torch.tensor([[4, 5, 6, 7], [3, 2, 1, 0], [-1, -2, -3, -4]], dtype=torch.int32, device="cuda:0")
    ops.mic_swap(audio, src, out=out)
    want = torch.stack([bits[0], bits[1][:, [3, 2, 1, 0]], bits[2][:, [3, 2, 1, 0]]])
    assert torch.equal(_bits(out).cpu(), want) and bool((buf[3 * n * 4:] == 7.0).all())
    assert torch.equal(_bits(audio).cpu(), bits)                      # the input is only read


def test_mic_swap_refusals(ops):
    from adyolo_amd._lib import AdyoloHipError
    from adyolo_amd.augmentations import swap_audio
    audio = torch.zeros(2, 16, 4, device="cuda:0")
    for combs in ([1, 0], [0, 16]):
        with pytest.raises(ValueError, match="symmetry"):
            swap_audio(audio, combs)
    src = torch.zeros(2, 4, dtype=torch.int32, device="cuda:0")
    with pytest.raises(AdyoloHipError, match="overlaps"):
        ops.mic_swap(audio, src, out=audio)
    with pytest.raises(AdyoloHipError):
        ops.mic_swap(audio, src[:1])
    with pytest.raises(AdyoloHipError):
        swap_audio(audio, [0])


# ------------------------------------------------------------------------------------- adyolo_corpus_gather (mic_src)
def _mic_table(ops):
    from adyolo_amd.augmentations import MIC_SWAP_COMBS, mic_swap_source
    return ops.corpus_mic_table({k: mic_swap_source(k) for k in MIC_SWAP_COMBS})


def _gather(ops, pcm, offs, combs, n, foa=False):
    """One call over (offset, combination) items -> (out, status word); checks the guard band behind the output."""
    from adyolo_amd.augmentations import COMBINATIONS
    b = len(offs)
    items = torch.zeros(b, 8, dtype=torch.int64)
    items[:, 0] = torch.tensor(offs)
    items[:, 4] = torch.tensor(combs)
    buf = torch.full((b * n * 4 + 64,), 7.0, device="cuda:0")
    out = buf[:b * n * 4].view(b, n, 4)
    status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    if foa:
        ops.corpus_gather(pcm, items.to("cuda:0"), ops.corpus_rot_table(COMBINATIONS), out, status)
    else:
        ops.corpus_gather(pcm, items.to("cuda:0"), None, out, status, mic_src=_mic_table(ops))
    torch.cuda.synchronize()
    assert bool((buf[b * n * 4:] == 7.0).all())
    return out, int(status.item())


def _reference(ops, pcm, offs, combs, n):
    from adyolo_amd.augmentations import swap_audio
    windows = torch.stack([pcm[o:o + n] for o in offs]).contiguous()
    return swap_audio(ops.pcm16_to_f32(windows), [max(c, 0) for c in combs])       # comb -1: no permutation


@pytest.mark.parametrize("n", [1, 2, 1027, 2048])
def test_gather_mic_is_the_conversion_then_the_swap(ops, pcm, n):
    from adyolo_amd.augmentations import MIC_SWAP_COMBS
    offsets = [0, S - n, 1234, 2501]                                  # the first and the last window, an even and an odd offset
    assert {o & 1 for o in offsets} == {0, 1}
    offs = [o for c in (-1,) + MIC_SWAP_COMBS for o in offsets]
    combs = [c for c in (-1,) + MIC_SWAP_COMBS for _ in offsets]
    out, status = _gather(ops, pcm, offs, combs, n)
    ref = _reference(ops, pcm, offs, combs, n)
    assert status == 0
    assert torch.equal(_bits(out), _bits(ref)), [(o, c) for j, (o, c) in enumerate(zip(offs, combs))
                                                 if not torch.equal(_bits(out[j]), _bits(ref[j]))]
    if n > 1:                                                          # the permutations do move something
        assert not torch.equal(out[len(offsets):2 * len(offsets)], out[2 * len(offsets):3 * len(offsets)])
    plain, status = _gather(ops, pcm, offsets, [-1] * 4, n)
    foa, foa_status = _gather(ops, pcm, offsets, [-1] * 4, n, foa=True)
    assert status == foa_status == 0 and torch.equal(_bits(plain), _bits(foa)) and torch.equal(_bits(plain), _bits(out[:4]))


@pytest.mark.parametrize("bad", [("comb", 1), ("comb", 16), ("off", -1), ("off", "past")], ids=lambda b: "%s_%s" % b)
def test_gather_mic_bad_item_is_zeroed_and_flagged(ops, pcm, bad):
    n = 1027
    offs, combs = [0, 100, 2501, S - n], [3, 9, 14, -1]
    ref = _reference(ops, pcm, offs, combs, n)
    out, status = _gather(ops, pcm, offs, combs, n)
    assert status == 0 and torch.equal(_bits(out), _bits(ref))        # all good: no bit
    word, value = bad
    if word == "comb":
        combs[1] = value
    else:
        offs[1] = S - n + 1 if value == "past" else value
    out, status = _gather(ops, pcm, offs, combs, n)
    assert status == ops.CORPUS_STATUS[1][0] == 2
    assert not bool(_bits(out[1]).any())
    for j in (0, 2, 3):
        assert torch.equal(_bits(out[j]), _bits(ref[j])), j


# ------------------------------------------------------------------------------------------- corpus against the host path
def _host_batches(prm, seed):
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    random.seed(seed)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, collate_fn=audio_collate_fn, num_workers=0)
    return list(loader)


@pytest.mark.parametrize("loss", ["adyolo", "adpit"])
def test_batches_equal_the_host_path(ops, mic_split, loss):
    from adyolo_amd.augmentations import MIC_SWAP_COMBS, swap_audio
    from adyolo_amd.corpus import ClasswiseDeviceCorpus, DeviceCorpus, load_chunked_split
    prm = _prm(mic_split, loss)
    seed = 41
    host = _host_batches(prm, seed)
    state = random.getstate()
    hc = load_chunked_split(prm, verify="all")
    random.seed(seed)
    corpus = (DeviceCorpus if loss == "adyolo" else ClasswiseDeviceCorpus)(hc, prm, "cuda:0", rank=0, world=1)
    assert corpus.swap and not corpus.rotate
    got = []
    for b0 in range(0, len(corpus), 4):
        audio, target, spec = corpus.batch(range(b0, b0 + 4))
        got.append((audio.clone(), target.clone(), spec.clone(), corpus.rows.clone() if loss == "adyolo" else None))
    torch.cuda.synchronize()
    assert random.getstate() == state
    assert len(got) == len(host) == 3
    combs = []
    for (pcm, cmb, tgt, sp), (audio, target, spec, rows) in zip(host, got):
        combs += [int(c) for c in cmb]
        ref = swap_audio(ops.pcm16_to_f32(pcm.to("cuda:0").contiguous()), cmb)
        assert torch.equal(_bits(audio), _bits(ref))
        if loss == "adyolo":
            m = tgt.shape[0]
            assert int(rows.item()) == m and m > 0
            assert torch.equal(_bits(target[:m].cpu()), _bits(tgt)) and bool((target[m:, 0] == -1).all())
        else:
            assert tuple(target.shape) == tuple(tgt.shape) == corpus.target_shape(4)
            assert torch.equal(_bits(target.cpu()), _bits(tgt))
        assert torch.equal(spec.cpu(), sp)
    assert set(combs) <= set(MIC_SWAP_COMBS) and len(set(combs) - {0}) >= 3, combs
    assert int(corpus.status.item()) == 0
    corpus.check()


# ------------------------------------------------------------------------------------------------------------------ epoch
def test_config5_with_channel_swap_replayed_equals_eager(ops, mic_split):
    """BASELINE config 5 at test size (mic_dev, ADPIT, SpecAug, ``MicFeatureExtractor``) with the key on: three steps of
    ``train_one_epoch_corpus``, eagerly and through ``StepGraphs``, end on the same parameter bits; the first batch's audio is
    not the audio of a run without the key from the same seed."""
    from adyolo_amd.corpus import ClasswiseDeviceCorpus, load_chunked_split
    from adyolo_amd.train import train_one_epoch_corpus
    prm = _prm(mic_split, "adpit")
    hc = load_chunked_split(prm)
    runs = []
    for graph in (False, True):
        random.seed(37)
        corpus = ClasswiseDeviceCorpus(hc, prm, "cuda:0", rank=0, world=1)
        tr = _trainer(graph, prm, mic=True)
        train_one_epoch_corpus(prm, corpus, tr)
        torch.cuda.synchronize()
        runs.append(tr)
    eager, replayed = runs
    assert len(eager.recorded) == len(replayed.recorded) == 3
    assert replayed.graphs.captures == 1 and replayed.graphs.replays == 2
    for i, ((le, _, _), (lr, _, _)) in enumerate(zip(eager.recorded, replayed.recorded)):
        assert bool(torch.isfinite(le)) and torch.equal(le, lr), (i, float(le), float(lr))
    assert torch.equal(eager.flat.flat, replayed.flat.flat)
    assert torch.equal(eager.optimizer.exp_avg, replayed.optimizer.exp_avg)
    assert bool(torch.isfinite(eager.flat.flat).all())
    first = []
    for swap in (True, False):
        p = _prm(mic_split, "adpit", swap=swap)
        random.seed(37)
        corpus = ClasswiseDeviceCorpus(hc, p, "cuda:0", rank=0, world=1)
        drawn = corpus.draw(range(4))
        first.append((corpus.get_filelist()[:4], drawn[0][:, 4].tolist(), corpus.launch(drawn)[0].clone()))
    (files_on, combs_on, audio_on), (files_off, combs_off, audio_off) = first
    assert files_on == files_off and combs_off == [-1] * 4 and any(c > 0 for c in combs_on), combs_on
    assert audio_on.shape == audio_off.shape and not torch.equal(audio_on, audio_off)
