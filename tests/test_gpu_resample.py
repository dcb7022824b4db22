"""GPU: sample-rate conversion on the device (csrc/resample.hip ``adyolo_resample_pcm``, ``ops.resample_pcm``,
``resample.resample_device``, ``corpus.InferDeviceCorpus`` on a ``load_infer_split(resample=True)`` split) against the NumPy int64
restatement of tests/test_resample_cpu.py.  The arithmetic is integer, so every comparison is ``np.array_equal``: no tolerance.

The launch cases take the tile size from ``ops.RESAMPLE_TILE`` and add, to the recordings of 0, 1, K - 1, K + 1, 255 and 1 031
frames, those whose converted length is one frame short of a tile, a whole tile and one frame more (where the ratio reaches that
length), so that a tile ends before, on and after the edge.  The three ratios: 2 -> 1 (L = 1: one phase, a broadcast tap),
147 -> 80 (the phase wraps within a tile, K = 118) and 2 -> 3 (up-conversion: several outputs read one input); beside them
147 -> 320 (more phases than a tile has frames, and the one standard rate whose tile needs more than 64 KB of LDS, which the
launch asks for by name) and 8 -> 1 (the longest rows, K = 513, and the widest input span)."""
import os

import numpy as np
import pytest
import torch

from test_infer_windows_cpu import SR, infer_params
from test_resample_cpu import ref_convert, ref_plan, ref_resample, write_wav24

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAD_ITEM, NONFINITE = 2, 8
RATIOS = {"2to1": (48000, 24000), "147to80": (44100, 24000), "2to3": (16000, 24000), "147to320": (11025, 24000),
          "8to1": (192000, 24000)}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def plans():
    from adyolo_amd import resample as R
    return {key: R.plan(*rates) for key, rates in RATIOS.items()}


def _sentinel(frames):
    """A loud int16 pattern that differs from frame to frame: what must survive wherever no row writes."""
    i = np.arange(frames * 4, dtype=np.int64).reshape(frames, 4)
    return (((i * 37 + 11) % 4001) + 21000).astype(np.int16)


def _n_out(n, pl):
    return (n * pl["L"] + pl["M"] - 1) // pl["M"]


def _lay_out(arrays, pl, loud):
    """Recordings -> (src stream with one loud frame between neighbours, rows, dst frames): the sources back to back on any
    frame, the destinations on 16-frame boundaries with a gap of 16 frames after each."""
    rows, pieces, s_pos, d_pos = [], [], 0, 16
    for a in arrays:
        n = a.shape[0]
        rows.append((s_pos, n, d_pos, _n_out(n, pl)))
        pieces += [a, np.full((1, 4), loud, dtype=a.dtype)]
        s_pos += n + 1
        d_pos += (_n_out(n, pl) + 15) // 16 * 16 + 16
    return np.ascontiguousarray(np.concatenate(pieces, 0)), rows, d_pos


def _launch(ops, src, rows, pl, dst_frames):
    dst = torch.from_numpy(_sentinel(dst_frames)).to(DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.resample_pcm(torch.from_numpy(src).to(DEV), torch.tensor(rows, dtype=torch.int64, device=DEV),
                           torch.from_numpy(pl["taps"]).to(DEV), pl["M"], pl["centre"], dst, status)
    assert got is dst
    return dst.cpu().numpy(), int(status.item())


def _ref(a, pl):
    return ref_resample(a, pl["L"], pl["M"], pl["K"], pl["centre"], pl["taps"])


# ------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("key", list(RATIOS))
def test_one_launch_over_many_recordings_equals_the_restatement(ops, plans, key):
    pl = plans[key]
    assert np.array_equal(pl["taps"].astype(np.int64), ref_plan(*RATIOS[key])[4])
    tile, k = ops.RESAMPLE_TILE, pl["K"]
    counts = [0, 1, k - 1, k + 1, 255, 1031]
    edges = {}
    for n in range(1, (2 * tile + 2) * pl["M"] // pl["L"] + pl["M"]):       # source lengths whose output ends around a tile edge
        if _n_out(n, pl) in (tile - 1, tile, tile + 1, 2 * tile):
            edges.setdefault(_n_out(n, pl), n)
    assert {tile - 1, tile + 1} <= set(edges) and (pl["L"] > pl["M"] or {tile, 2 * tile} <= set(edges))
    counts += [edges[v] for v in sorted(edges)]
    rs = np.random.RandomState(7)
    arrays = [rs.randint(-8000, 8001, size=(n, 4)).astype(np.int16) for n in counts]
    src, rows, dst_frames = _lay_out(arrays, pl, 30000)
    got, status = _launch(ops, src, rows, pl, dst_frames)
    want = _sentinel(dst_frames)
    for a, (_, _, d_off, d_n) in zip(arrays, rows):
        want[d_off:d_off + d_n] = _ref(a, pl)
    assert status == 0
    for a, (_, n, d_off, d_n) in zip(arrays, rows):
        assert np.array_equal(got[d_off:d_off + d_n], want[d_off:d_off + d_n]), (key, n)
    assert np.array_equal(got, want)                                        # the gaps and tails keep the sentinel


@pytest.mark.parametrize("key", ["2to1", "147to80"])
def test_a_recording_of_more_tiles_than_the_grid_is_wide(ops, plans, key):
    """The launch has at most 1024 workgroups per recording (csrc/resample.hip RS_GRID_X); a longer recording sends some of
    them round the stride loop a second time.  At 2 -> 1 the second tile has the first one's phases and keeps the staged rows;
    at 147 -> 80 it starts on another phase (1024 * 256 * 147 % 80 = 48) and stages them again."""
    pl = plans[key]
    tile, grid = ops.RESAMPLE_TILE, 1024
    n = ((grid + 3) * tile + 5) * pl["M"] // pl["L"]
    assert (grid + 3) * tile < _n_out(n, pl) < (grid + 4) * tile
    x = np.random.RandomState(31).randint(-8000, 8001, size=(n, 4)).astype(np.int16)
    src, rows, dst_frames = _lay_out([x], pl, 30000)
    got, status = _launch(ops, src, rows, pl, dst_frames)
    want = _sentinel(dst_frames)
    want[rows[0][2]:rows[0][2] + rows[0][3]] = _ref(x, pl)
    assert status == 0 and np.array_equal(got, want)


def _float_cases(n, rs):
    x = (rs.randint(-2 ** 23, 2 ** 23, size=(n, 4)) / 2.0 ** 23).astype(np.float32)
    ties = (np.arange(-40, 40, dtype=np.float64) + 0.5) * 2.0 ** -23
    x[100:120] = ties.astype(np.float32).reshape(20, 4)                     # exact halves of the Q23 step: ties to even
    x[300] = (1.0, -1.0, 1.5, -1.5)                                         # the clamp
    x[301] = (np.float32(1.0) - np.float32(2.0 ** -24), 3.0e38, -3.0e38, 1e-45)
    return x


@pytest.mark.parametrize("kind", ["int16", "int32", "float32"])
def test_each_sample_format(ops, plans, kind):
    pl = plans["2to1"]
    rs = np.random.RandomState(9)
    if kind == "int16":
        x = rs.randint(-32768, 32768, size=(1031, 4)).astype(np.int16)
    elif kind == "int32":
        x = rs.randint(-2 ** 31, 2 ** 31, size=(1031, 4)).astype(np.int32)   # low bytes set: the shift is arithmetic and drops them
        x[5] = (-1, -256, -257, 2 ** 31 - 1)
    else:
        x = _float_cases(1031, rs)
    loud = 30000 if kind != "float32" else 0.9
    src, rows, dst_frames = _lay_out([x], pl, loud)
    got, status = _launch(ops, src, rows, pl, dst_frames)
    want = _sentinel(dst_frames)
    want[rows[0][2]:rows[0][2] + rows[0][3]] = _ref(x, pl)
    assert status == 0 and np.array_equal(got, want)
    if kind == "float32":                                                   # one NaN and one Inf: taken as 0, told by the status
        x[400, 2], x[700, 0] = np.nan, -np.inf
        src, rows, dst_frames = _lay_out([x], pl, loud)
        got, status = _launch(ops, src, rows, pl, dst_frames)
        zeroed = x.copy()
        zeroed[400, 2], zeroed[700, 0] = 0.0, 0.0
        want[rows[0][2]:rows[0][2] + rows[0][3]] = _ref(zeroed, pl)
        assert status == NONFINITE and np.array_equal(got, want)
        assert np.array_equal(_ref(zeroed, pl), _ref(x, pl))                # the restatement's own rule says the same


def test_a_full_scale_square_wave_saturates_both_ways(ops, plans):
    pl = plans["147to80"]
    x = np.where((np.arange(2000) // 37) % 2 == 0, 32767, -32767).astype(np.int16)
    x = np.ascontiguousarray(np.repeat(x[:, None], 4, 1))
    want_y = _ref(x, pl)
    assert want_y.max() == 32767 and want_y.min() == -32768                 # the overshoot of the edges meets the clamp
    src, rows, dst_frames = _lay_out([x], pl, 30000)
    got, status = _launch(ops, src, rows, pl, dst_frames)
    assert status == 0 and np.array_equal(got[rows[0][2]:rows[0][2] + rows[0][3]], want_y)


def test_bad_rows_write_nothing_and_set_the_status_bit(ops, plans):
    from adyolo_amd import _lib
    pl = plans["147to80"]
    rs = np.random.RandomState(13)
    arrays = [rs.randint(-8000, 8001, size=(n, 4)).astype(np.int16) for n in (600, 500, 700)]
    src, rows, dst_frames = _lay_out(arrays, pl, 30000)
    s_total = src.shape[0]
    for bad in ((rows[1][0], 500, rows[1][2], rows[1][3] + 1),             # dst frames are not n_out of the src frames
                (rows[1][0], 500, rows[1][2], rows[1][3] - 1),
                (s_total - 499, 500, rows[1][2], rows[1][3]),               # the source runs past its stream
                (-1, 500, rows[1][2], rows[1][3]),
                (rows[1][0], -500, rows[1][2], _n_out(-500, pl)),
                (rows[1][0], 500, dst_frames - rows[1][3] + 1, rows[1][3]),  # the destination runs past its stream
                (rows[1][0], 500, -16, rows[1][3])):
        got, status = _launch(ops, src, [rows[0], bad, rows[2]], pl, dst_frames)
        want = _sentinel(dst_frames)
        for i in (0, 2):
            want[rows[i][2]:rows[i][2] + rows[i][3]] = _ref(arrays[i], pl)
        assert status == BAD_ITEM, bad
        assert np.array_equal(got, want), bad                               # the other rows are right, nothing else is touched
    edge = [(s_total - 500, 500, dst_frames - rows[1][3], rows[1][3])]     # both end with their streams: legal
    got, status = _launch(ops, src, edge, pl, dst_frames)
    assert status == 0 and np.array_equal(got[dst_frames - rows[1][3]:], _ref(src[s_total - 500:], pl))
    # the entry point's own refusals
    dev_src = torch.from_numpy(src).to(DEV)
    taps = torch.from_numpy(pl["taps"]).to(DEV)
    dst = torch.zeros((dst_frames, 4), dtype=torch.int16, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.AdyoloHipError):                                # a source that starts 8 bytes into a 16-byte slot
        ops.resample_pcm(dev_src[1:], table, taps, pl["M"], pl["centre"], dst, status)
    with pytest.raises(_lib.AdyoloHipError):
        ops.resample_pcm(dev_src, table[:0], taps, pl["M"], pl["centre"], dst, status)
    with pytest.raises(_lib.AdyoloHipError):
        ops.resample_pcm(dev_src, table, taps.to(torch.int64), pl["M"], pl["centre"], dst, status)
    args = [dev_src.data_ptr(), 0, s_total, table.data_ptr(), 3, taps.data_ptr(), taps.numel(), pl["L"], pl["M"], pl["K"],
            pl["centre"], dst.data_ptr(), dst_frames, status.data_ptr(), None]
    for pos, value in ((6, taps.numel() - 1), (4, 0), (1, 3), (0, None), (11, None)):      # K L against the table, R, kind, nulls
        broken = list(args)
        broken[pos] = value
        with pytest.raises(_lib.AdyoloHipError):
            _lib.call("adyolo_resample_pcm", *broken)
    assert int(status.item()) == 0 and not dst.any()


# --------------------------------------------------------------------------------------------------------- the whole path
def _chain(root):
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.wrapper import WrapperModel
    prm = infer_params(root, device=DEV)
    torch.manual_seed(8)
    model = WrapperModel((1, 7, 80, 64), (), prm).to(DEV).eval()
    return prm, model, FeatureExtractor(None, DEV), LabelPostProcessor(prm)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """Folder A: one int16 recording at 2 SR, one at SR, one float32 at SR * 147 / 80 and one 24-bit at SR.  Folder B: the same
    recordings converted by the restatement, written as int16 at SR."""
    from scipy.io import wavfile
    rs = np.random.RandomState(23)
    a, b = tmp_path_factory.mktemp("native"), tmp_path_factory.mktemp("converted")
    native = {"r0_double": (2 * SR, rs.randint(-8000, 8001, size=(2 * 60000 + 1, 4)).astype(np.int16)),
              "r1_same": (SR, rs.randint(-8000, 8001, size=(48000, 4)).astype(np.int16)),
              "r2_float": (SR * 147 // 80, (rs.randint(-8000, 8001, size=(66150 + 40, 4)) / 32768.0).astype(np.float32)),
              "r3_24bit": (SR, (rs.randint(-2 ** 21, 2 ** 21, size=(24000 + 9, 4)) << 8).astype(np.int32))}
    converted = {}
    for name, (rate, data) in native.items():
        if data.dtype == np.int32:
            write_wav24(str(a / (name + ".wav")), rate, data)
        else:
            wavfile.write(str(a / (name + ".wav")), rate, data)
        converted[name] = data if (rate == SR and data.dtype == np.int16) else ref_convert(data, rate, SR)
        wavfile.write(str(b / (name + ".wav")), SR, converted[name])
    return a, b, native, converted


def _csv(folder, names):
    assert sorted(os.listdir(folder)) == sorted(n + ".csv" for n in names)
    return {n: open(os.path.join(folder, n + ".csv"), "rb").read() for n in names}


def test_a_folder_of_native_recordings_equals_the_converted_folder(ops, folders, tmp_path):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import InferDeviceCorpus, load_infer_split
    a, b, native, converted = folders
    names = sorted(native)
    prm_a, model, fx, post = _chain(a)
    prm_b = infer_params(b, device=DEV)
    hc_a = load_infer_split(prm_a, rank=0, world=1, verify="all", resample=True, files=names)
    hc_b = load_infer_split(prm_b, rank=0, world=1, verify="all", files=names)
    corp_a = InferDeviceCorpus(hc_a, prm_a, DEV, window_s=2, margin_s=0.4, batch_size=4)
    corp_b = InferDeviceCorpus(hc_b, prm_b, DEV, window_s=2, margin_s=0.4, batch_size=4)
    corp_a.check()
    assert corp_a.lengths == [converted[n].shape[0] for n in corp_a.filelist] and sum(corp_a.label_frames) > 60
    pcm_a, pcm_b = corp_a.pcm.cpu().numpy(), corp_b.pcm.cpu().numpy()
    for i, name in enumerate(corp_a.filelist):                              # each recording and its zero tail, by name
        k = corp_b.filelist.index(name)
        sa, sb = int(hc_a.rec_start[i]), int(hc_b.rec_start[k])
        span = int(hc_a.rec_start[i + 1]) - sa
        assert span == int(hc_b.rec_start[k + 1]) - sb
        assert np.array_equal(pcm_a[sa:sa + span], pcm_b[sb:sb + span]), name
        assert np.array_equal(pcm_a[sa:sa + converted[name].shape[0]], converted[name]), name
    if corp_a.filelist == corp_b.filelist:
        assert np.array_equal(pcm_a, pcm_b) and np.array_equal(corp_a.table_host, corp_b.table_host)
    assert corp_a.nbytes() == corp_b.nbytes()
    out_a, out_b = str(tmp_path / "native"), str(tmp_path / "converted")
    info_a = atest.infer_epoch_corpus(corp_a, model, fx, post, out_a)
    info_b = atest.infer_epoch_corpus(corp_b, model, fx, post, out_b)
    assert info_a == info_b and info_a["recordings"] == 4
    got, want = _csv(out_a, names), _csv(out_b, names)
    assert got == want and sum(len(v) for v in want.values()) > 0
    corp_a.check()


def test_a_non_finite_sample_in_a_folder_stops_the_upload(ops, tmp_path):
    """``infer_epoch_corpus`` clears the status word when a pass begins, so the conversion's bits are read while the corpus is
    built: a float file with a NaN never reaches a pass, and no ``check()`` of the caller is needed for that."""
    from scipy.io import wavfile
    from adyolo_amd import _lib
    from adyolo_amd.corpus import InferDeviceCorpus, infer_split_from_arrays, load_infer_split
    rs = np.random.RandomState(29)
    wavfile.write(str(tmp_path / "fine.wav"), SR, rs.randint(-8000, 8001, size=(4800, 4)).astype(np.int16))
    wavfile.write(str(tmp_path / "fine48.wav"), 2 * SR, rs.randint(-8000, 8001, size=(9600, 4)).astype(np.int16))
    good = (rs.randint(-8000, 8001, size=(8820, 4)) / 32768.0).astype(np.float32)
    bad = good.copy()
    bad[4000, 3] = np.nan
    wavfile.write(str(tmp_path / "holed.wav"), 44100, bad)
    prm = infer_params(tmp_path, device=DEV)
    hc = load_infer_split(prm, rank=0, world=1, verify="all", resample=True)
    with pytest.raises(_lib.AdyoloHipError, match=r"44100 Hz float32 recordings \(holed\).*NaN"):
        InferDeviceCorpus(hc, prm, DEV, window_s=2, margin_s=0.4)
    bad[4000, 3] = -np.inf
    with pytest.raises(_lib.AdyoloHipError, match="holed.*Inf"):
        InferDeviceCorpus(infer_split_from_arrays(["fine", "holed"], [np.zeros((480, 4), dtype=np.int16), bad], prm,
                                                  rates=[SR, 44100]), prm, DEV, window_s=2, margin_s=0.4)
    wavfile.write(str(tmp_path / "holed.wav"), 44100, good)                 # the same folder without the hole goes through
    corp = InferDeviceCorpus(load_infer_split(prm, rank=0, world=1, resample=True), prm, DEV, window_s=2, margin_s=0.4)
    assert int(corp.status.item()) == 0 and corp.lengths[corp.filelist.index("holed")] == 4800


def test_resample_device_gives_the_corpus_bytes(ops, folders):
    from adyolo_amd import resample as R
    from adyolo_amd.corpus import InferDeviceCorpus, infer_split_from_arrays
    _, _, native, converted = folders
    prm = infer_params("unused", device=DEV)
    for name in ("r0_double", "r2_float", "r3_24bit"):
        rate, data = native[name]
        got = R.resample_device(torch.from_numpy(data).to(DEV), rate, SR)
        assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), converted[name]), name
        corp = InferDeviceCorpus(infer_split_from_arrays([name], [data], prm, rates=[rate]), prm, DEV, window_s=2, margin_s=0.4)
        assert np.array_equal(corp.pcm[:got.shape[0]].cpu().numpy(), got.cpu().numpy()) and not corp.pcm[got.shape[0]:].any()
    same = torch.from_numpy(native["r1_same"][1]).to(DEV)
    assert R.resample_device(same, SR, SR) is same
    out = torch.empty((converted["r0_double"].shape[0], 4), dtype=torch.int16, device=DEV)
    assert R.resample_device(torch.from_numpy(native["r0_double"][1]).to(DEV), 2 * SR, SR, out=out) is out
    assert np.array_equal(out.cpu().numpy(), converted["r0_double"])
    bad = native["r2_float"][1][:5000].copy()
    bad[17, 1] = np.nan
    from adyolo_amd import _lib
    with pytest.raises(_lib.AdyoloHipError, match="NaN"):
        R.resample_device(torch.from_numpy(bad).to(DEV), 44100, SR)
