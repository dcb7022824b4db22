"""``HostCorpus`` is one structure for every kind of split: the chunked training split, a whole-recording evaluation split, an
inference folder and in-memory recordings with ``rates=``.  Each loader must hand back the same fields, the same 16-frame
stream layout with zeroed alignment tails, and a ``kind`` the device corpora can ask instead of probing for fields."""
import numpy as np
import pytest

import adyolo_amd  # noqa: F401
from adyolo_amd import corpus as C
from test_corpus_cpu import params_for, write_split
from test_eval_corpus_cpu import eval_params, write_eval_split
from test_infer_windows_cpu import SR, infer_params, write_folder

CHUNK_SR = 2410                 # a 2 s window is 4820 samples: no multiple of 16


@pytest.fixture(scope="module")
def splits(tmp_path_factory):
    root = tmp_path_factory.mktemp("host_corpus")
    # one chunk (2 s) and three chunks (4 s) of a 2 s window with a 1 s stride
    write_split(str(root / "train"), recordings=(("fold1_one", 2.0), ("fold1_three", 4.0)), sr=CHUNK_SR, window_s=2, stride_s=1)
    chunked = C.load_chunked_split(params_for(root / "train", window_s=2, stride_s=1, sr=CHUNK_SR), verify="all")
    write_eval_split(str(root / "eval"), clips=(("fold4_a", 48000), ("fold4_b", 48000 + 77)))
    evald = C.load_eval_split(eval_params(root / "eval"), "test", rank=0, world=1, verify="all")
    write_folder(root / "infer", lengths=(("rec_a", 24000 + 77), ("rec_b", 4800)))
    prm = infer_params(root / "infer")
    infer = C.load_infer_split(prm, rank=0, world=1, verify="all")
    rs = np.random.RandomState(5)
    arrays = [rs.randint(-8000, 8000, size=(n, 4)).astype(np.int16) for n in (4800 + 7, 2400 + 5)]
    rated = C.infer_split_from_arrays(["double", "same"], arrays, prm, rates=[2 * SR, SR])         # "double" stays native
    empty = C.infer_split_from_arrays([], [], prm)
    return {"chunked": chunked, "eval": evald, "infer": infer, "rated": rated, "empty": empty}, arrays


def test_every_kind_of_split_is_the_same_structure(splits):
    hcs, arrays = splits
    fields = {name: sorted(vars(hc)) for name, hc in hcs.items()}
    assert all(f == fields["chunked"] for f in fields.values()), fields
    assert len(hcs["chunked"].chunks) == 4 and sorted(hcs["chunked"].lengths.tolist()) == [4820, 4820 + 2 * 2410]
    for name, hc in hcs.items():
        r_n = len(hc.rec_names)
        assert r_n == (0 if name == "empty" else 2)
        assert hc.audio.dtype == np.int16 and hc.audio.shape == (max(int(hc.rec_start[-1]), 16), 4)
        assert hc.rec_start.shape == hc.ev_start.shape == (r_n + 1,) and hc.lengths.shape == (r_n,)
        assert hc.rec_start.dtype == hc.ev_start.dtype == hc.lengths.dtype == np.int64
        assert not (hc.rec_start % 16).any() and hc.rec_start[0] == 0
        assert int(hc.ev_start[-1]) == hc.events.shape[0] and hc.events.shape[1] == 5
        for i in range(r_n):
            s0, room, n = int(hc.rec_start[i]), int(hc.rec_start[i + 1] - hc.rec_start[i]), int(hc.lengths[i])
            assert n <= room < n + 16, (name, i)
            assert not hc.audio[s0 + n:s0 + room].any(), (name, i)           # the alignment tail is int16 zero
        kept = sum(a.nbytes for a in hc.native or () if a is not None)
        assert hc.nbytes() == hc.audio.nbytes + hc.events.nbytes + kept
    assert any(int(n) % 16 for name in ("chunked", "eval", "infer", "rated") for n in hcs[name].lengths)
    assert hcs["empty"].rec_start.tolist() == [0] and hcs["empty"].audio.shape == (16, 4)
    # what the device corpora ask: the kind, and whether recordings wait on the host in their native form
    H = C.HostCorpus
    assert [hcs[k].kind for k in ("chunked", "eval", "infer", "rated", "empty")] == [H.CHUNKED, H.EVAL, H.INFER, H.INFER, H.INFER]
    for name in ("chunked", "eval", "infer", "empty"):
        hc = hcs[name]
        assert hc.native is None and hc.rates is None and hc.kinds is None and hc.native_lengths is None
    rated = hcs["rated"]
    assert rated.native[0] is arrays[0] and rated.native[1] is None and rated.nbytes() > rated.audio.nbytes
    assert rated.rates.tolist() == [2 * SR, SR] and rated.kinds.tolist() == [0, 0]
    assert rated.native_lengths.tolist() == [4807, 2405] and rated.lengths.tolist() == [2404, 2405]
    assert not rated.stream(0).any() and np.array_equal(rated.stream(1), arrays[1])     # a zeroed place; today's bytes
    # the fields a kind does not use hold their empty value
    for name in ("eval", "infer", "rated", "empty"):
        hc = hcs[name]
        assert hc.chunks == {} and hc.chunk_events == {} and hc.stride == 0 and hc.filelist == hc.total_filelist == hc.rec_names
    for name in ("infer", "rated", "empty"):
        hc = hcs[name]
        assert hc.events.shape == (0, 5) and not hc.ev_start.any() and hc.max_events == 0
    assert (hcs["chunked"].rank, hcs["chunked"].world) == (0, 1) and hcs["chunked"].filelist == hcs["chunked"].total_filelist
    assert hcs["chunked"].events.shape[0] > 0 and hcs["eval"].events.shape[0] > 0
    for name, make in (("EvalDeviceCorpus", C.EvalDeviceCorpus), ("InferDeviceCorpus", C.InferDeviceCorpus)):
        with pytest.raises(ValueError, match=name + ".*got the chunked training split"):
            make(hcs["chunked"], eval_params("unused"), device="cpu")
