"""GPU: the device selection of the class-wise heads (``ops.classwise_select``, csrc/select.hip ``adyolo_classwise_select``)
on the MI355X, held to bit equality: against the rows of the REAL reference (``postprocess_classwise.npz``), against the host
``select`` on the same decode with every ADPIT case counted, over clips and untrimmed buffers, through its error codes, and
through ``test_epoch_audio`` / ``sweep_conf_thresh`` with ``device_select`` and the device scorer on the ADPIT chain."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, G)
# a sibling test module: pytest puts this directory on sys.path (rootdir insertion, no __init__.py), as for test_gpu_corpus.py
from test_gpu_classwise_eval import _chain_setup, _random_outputs  # noqa: E402

pytestmark = pytest.mark.gpu

LOSSES = ["seddoa", "masked-seddoa", "accdoa", "adpit"]
THRESHOLDS = list(np.arange(0.1, 1.0, 0.1)) + [np.float32(0.7), 0.1 * 3, 1.0]     # float64 scalars, a float32, Python floats
UNIFY = (15.0, 30.0, 45.0)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _post(loss, c, conf=0.5, unify=15.0):
    from adyolo_amd.postprocess import LabelPostProcessor
    return LabelPostProcessor({"args": {"loss": loss}, "data_config": {"nb_classes": c},
                               "train_config": {"conf_thresh": conf, "unify_thresh": unify}})


def _flat(res):
    """{frame: [[class, x, y, z], ...]} -> (N, 5) float32 [frame, class, x, y, z] in dict order."""
    return np.asarray([[fr] + list(r) for fr, rr in res.items() for r in rr], dtype=np.float32).reshape(-1, 5)


def _assert_same_dicts(got, want, msg):
    assert list(got.keys()) == list(want.keys()), msg
    assert [len(v) for v in got.values()] == [len(v) for v in want.values()], msg
    a, b = _flat(got), _flat(want)
    np.testing.assert_array_equal(a[:, :2], b[:, :2], err_msg=msg)
    np.testing.assert_array_equal(_bits(a[:, 2:]), _bits(b[:, 2:]), err_msg=msg)


# ------------------------------------------------------------------------------------------------ 1. reference rows
@pytest.mark.parametrize("c", [12, 13])
@pytest.mark.parametrize("loss", LOSSES)
def test_device_postprocess_matches_the_reference_rows(ops, loss, c):
    """Every key of the fixture the real reference wrote: frame and class equal, xyz bit-equal (the comparison of
    test_gpu_classwise_eval.test_postprocess_on_the_gpu_matches_the_reference_rows, with the selection on the device)."""
    g = np.load(os.path.join(G, "postprocess_classwise.npz"))
    src = "seddoa" if loss == "masked-seddoa" else loss
    out = torch.from_numpy(g["out_%s_C%d" % (src, c)]).cuda()
    pp = _post(loss, c)
    ths = list(g["conf_thresholds"]) + ([] if src == "seddoa" else [float(g["high_thresh"])])
    assert len(ths) >= 9
    seen = 0
    for i, th in enumerate(ths):
        pp.set_conf_thresh(th)
        for u in (g["unify_thresholds"] if src == "adpit" else (None,)):
            key = "rows_%s_C%d_t%d" % (src, c, i) + ("" if u is None else "_u%d" % int(u))
            if u is not None:
                pp.unify_thresh = float(u)
            res = pp.postprocess(out, on_device=True)
            got = np.asarray([[fr] + [float(v) for v in r] for fr, rr in res.items() for r in rr], dtype=np.float64).reshape(-1, 5)
            ref = g[key]
            assert got.shape == ref.shape, key
            np.testing.assert_array_equal(got[:, :2], ref[:, :2], err_msg=key)
            np.testing.assert_array_equal(_bits(got[:, 2:]), _bits(ref[:, 2:]), err_msg=key)
            seen += 1
    assert seen == len(ths) * (3 if src == "adpit" else 1)
    assert seen == len([k for k in g.files if k.startswith("rows_%s_C%d_" % (src, c))])      # no key of the fixture left out


# ------------------------------------------------------------------------------------- 2. device == host, same decode
def _adpit_cases(dec, conf, unify):
    """The six ADPIT cases of ``classwise_select`` on a host decode -> their (frame, class) counts."""
    act, dist = dec[..., 0:3], dec[..., 12:15]
    sed = act > conf
    pair = np.stack([sed[..., 0] & sed[..., 1], sed[..., 1] & sed[..., 2], sed[..., 2] & sed[..., 0]], -1) & (dist < unify)
    n = pair.sum(-1)
    one = n == 1
    return {"no pair, some track active": int(((n == 0) & sed.any(-1)).sum()),
            "pair 01 only": int((one & pair[..., 0]).sum()), "pair 12 only": int((one & pair[..., 1]).sum()),
            "pair 20 only": int((one & pair[..., 2]).sum()), "two pairs": int((n == 2).sum()),
            "three pairs": int((n == 3).sum())}


@pytest.mark.parametrize("c", [12, 13])
@pytest.mark.parametrize("loss", LOSSES)
def test_device_rows_equal_the_host_select_on_the_same_decode(ops, loss, c):
    from adyolo_amd.postprocess import group_rows
    frames = 1237
    out = _random_outputs(loss, c, frames, 3 + c)
    dec = ops.classwise_decode(torch.from_numpy(out).cuda().view(1, frames, -1), c, loss)
    host = dec.cpu().numpy()
    pp = _post(loss, c)
    for u in (UNIFY if loss == "adpit" else (None,)):
        if u is not None:
            pp.unify_thresh = u
        for k, th in enumerate(THRESHOLDS):
            msg = "%s C=%d conf=%r unify=%r" % (loss, c, th, u)
            pp.set_conf_thresh(th)
            if loss == "adpit" and k < 9 and u in (30.0, 45.0):               # every branch is exercised, not just one
                cases = _adpit_cases(host, th, u)
                print(msg, cases)
                assert all(v > 0 for v in cases.values()), (msg, cases)
            want = pp.select(host)
            rows, counts = pp.select_device_rows(dec)
            assert rows.is_cuda and counts.is_cuda and counts.dtype == torch.int32
            assert rows.shape == (sum(len(v) for v in want.values()), 5) and counts.shape == (frames,)
            counts_h = counts.cpu().numpy()
            np.testing.assert_array_equal(counts_h, [len(want.get(f, ())) for f in range(frames)], err_msg=msg)
            rows_h = rows.cpu().numpy()
            np.testing.assert_array_equal(rows_h[:, 0], np.repeat(np.arange(frames), counts_h), err_msg=msg)
            _assert_same_dicts(group_rows(rows_h, counts_h)[0], want, msg)
            if loss != "adpit" and k == 4:                                      # threshold 0.5
                assert 0 < len(rows_h) < frames * c, (msg, len(rows_h))
            if th == 1.0 and loss != "adpit":
                assert len(rows_h) == 0 and want == {}                          # the reference's double test
            elif th == 1.0:                       # adpit: no lone track passes it; every (frame, class) with a pair gives its mean
                cases = _adpit_cases(host, th, u)
                assert len(rows_h) == sum(v for key, v in cases.items() if "pair" in key and not key.startswith("no"))
    pp.set_conf_thresh(0.5)
    assert len(pp.select(host)) > 0


# ---------------------------------------------------------------------------------------------- 3. clips, trimming
@pytest.mark.parametrize("loss", ["accdoa", "adpit"])
def test_clips_and_untrimmed_rows(ops, loss):
    c, t = 13, 211
    decs = [ops.classwise_decode(torch.from_numpy(_random_outputs(loss, c, t, 40 + k)).cuda().view(1, t, -1), c, loss)
            for k in range(3)]
    pp = _post(loss, c, conf=0.4, unify=30.0)
    singles = [pp.select_device(d) for d in decs]
    assert all(len(s) == 1 and len(s[0]) > 0 for s in singles)
    dec3 = torch.cat(decs, 0)
    three = pp.select_device(dec3, n_clips=3)
    assert len(three) == 3
    for k in range(3):
        _assert_same_dicts(three[k], singles[k][0], "clip %d" % k)
        _assert_same_dicts(three[k], pp.select(decs[k].cpu().numpy()), "clip %d against the host" % k)
    rows, counts = pp.select_device_rows(dec3, 3)
    full, counts_full = pp.select_device_rows(dec3, 3, trim=False)
    assert full.shape == (3 * t * c * (3 if loss == "adpit" else 1), 5) and counts_full.shape == (3 * t,)
    assert int(counts_full.sum()) == rows.shape[0] and 0 < rows.shape[0] < full.shape[0]
    assert torch.equal(counts, counts_full)
    np.testing.assert_array_equal(_bits(full[:rows.shape[0]].cpu().numpy()), _bits(rows.cpu().numpy()))
    for n_clips in (2, 4, 0):
        with pytest.raises(ValueError):
            pp.select_device_rows(dec3, n_clips)
        with pytest.raises(ValueError):
            pp.select_device(dec3, n_clips)


# -------------------------------------------------------------------------------------------------- 4. error codes
def test_classwise_select_error_codes(ops):
    from adyolo_amd import _lib
    lib = _lib.load()
    n, c = 4, 12
    torch.manual_seed(7)
    dec = torch.rand(n * c * 16 + 4, device="cuda:0")
    ws = torch.zeros(2 * n * c, device="cuda:0")
    rows = torch.zeros(n * c * 3 * 5, device="cuda:0")
    cnt = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)                         # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = ctypes.c_float
    call = lambda d, w, r, k, nf=n, nc=c, mode=2: lib.adyolo_classwise_select(d, w, r, k, nf, nc, mode, f(0.5), f(15.0), st)  # noqa: E731
    assert call(None, p(ws), p(rows), p(cnt)) == -1
    assert call(p(dec), None, p(rows), p(cnt)) == -1
    assert call(p(dec), p(ws), None, p(cnt)) == -1
    assert call(p(dec), p(ws), p(rows), None) == -1
    assert b"null" in lib.adyolo_last_error()
    assert call(p(dec), p(ws), p(rows), p(cnt), nf=0) == -1
    assert call(p(dec), p(ws), p(rows), p(cnt), nc=0) == -1
    assert call(p(dec), p(ws), p(rows), p(cnt), nf=-3) == -1
    assert b"frames" in lib.adyolo_last_error()
    assert call(p(dec, 4), p(ws), p(rows), p(cnt)) == -1                             # record loads need 16-byte alignment
    assert b"aligned" in lib.adyolo_last_error()
    assert call(p(dec), p(ws), p(rows), p(cnt), mode=3) == -2
    assert call(p(dec), p(ws), p(rows), p(cnt), mode=-1) == -2
    assert b"mode" in lib.adyolo_last_error()
    assert call(p(dec), p(ws), p(rows), p(cnt), nf=(1 << 31) // (3 * c) + 1) == -2  # refused before anything is launched
    assert b"32-bit" in lib.adyolo_last_error()
    torch.cuda.synchronize()
    assert not rows.any() and not cnt.any()                                          # nothing was written by the refused calls
    for mode in (2, 1, 0):
        assert call(p(dec), p(ws), p(rows), p(cnt), mode=mode) == 0
    torch.cuda.synchronize()
    counts = cnt.cpu().numpy()
    assert counts[n] == counts[:n].sum() and 0 < counts[n] < n * c                  # uniform [0, 1) activities at 0.5
    with pytest.raises(_lib.AdyoloHipError):
        ops.classwise_select(torch.zeros(5, 12, 4, device="cuda:0"), 12, "adpit", 0.5, unify=15.0)     # record width
    with pytest.raises(_lib.AdyoloHipError):
        ops.classwise_select(torch.zeros(5, 12, 4, device="cuda:0"), 12, 3, 0.5)                       # unknown mode
    with pytest.raises(ValueError):
        ops.classwise_select(torch.zeros(5, 12, 16, device="cuda:0"), 12, "adpit", 0.5)


# --------------------------------------------------------------------------------------------------------- 5. chain
def _same_folder(a, b, n):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) == n
    size = 0
    for f in os.listdir(a):
        with open(os.path.join(a, f), "rb") as x, open(os.path.join(b, f), "rb") as y:
            data = x.read()
            assert data == y.read(), f
            size += len(data)
    return size


def _scores(res):
    return np.asarray([float(v) for v in res[:5]]), np.asarray(res[5], dtype=np.float64)


@pytest.mark.parametrize("mode", ["eager", "graphs-batched"])
def test_adpit_chain_with_device_selection_and_scoring(ops, tmp_path, mode):
    """``test_epoch_audio(device_select=True, device_scorer=...)`` on the ADPIT chain writes the CSV files of the host-selection
    run of the same mode byte for byte and returns its loss; the device scores equal the host's on that folder; unify_thresh
    is read at call time (the reference sets it on the object between its three test runs)."""
    from adyolo_amd import test as atest
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.features import FeatureExtractor, load_scaler_npz
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import ComputeSELDResults, DeviceSELDScorer
    from adyolo_amd.wrapper import WrapperCriterion
    g = np.load(os.path.join(G, "seld_chain_adpit.npz"))
    prm, model, cdir, clips = _chain_setup(tmp_path, g)
    fx = FeatureExtractor(load_scaler_npz(os.path.join(G, "scaler_DCASE2021.npz")), "cuda:0")
    crit, post = WrapperCriterion(prm), LabelPostProcessor(prm)
    ds = FoaDataset(prm, "test", is_valid=True)
    kw = {} if mode == "eager" else {"batch_size": 4, "forward": ForwardGraphs(model, fx, post, warm_calls=0)}
    dev, host = DeviceSELDScorer(prm, cdir), ComputeSELDResults(prm, cdir)
    sizes = []
    for u in UNIFY:
        post.unify_thresh = u
        out_h, out_d = os.path.join(tmp_path, "host_%d" % u), os.path.join(tmp_path, "dev_%d" % u)
        loss_h = atest.test_epoch_audio(ds, model, fx, crit, post, "cuda:0", out_h, **kw)
        dev.reset()
        loss_d = atest.test_epoch_audio(ds, model, fx, crit, post, "cuda:0", out_d, device_select=True, device_scorer=dev, **kw)
        assert loss_d == loss_h, (u, loss_d, loss_h)
        sizes.append(_same_folder(out_h, out_d, len(clips)))
        assert sizes[-1] > 0
        s, cw = _scores(dev.scores())
        hs, hcw = _scores(host.get_SELD_Results(out_d))
        np.testing.assert_allclose(s, hs, rtol=1e-9, atol=1e-12, err_msg="unify %g" % u)
        np.testing.assert_allclose(cw, hcw, rtol=1e-9, atol=1e-12, err_msg="unify %g" % u)
    print("adpit device chain %s: CSV bytes per unify threshold %s" % (mode, sizes))
    if mode != "eager":
        assert kw["forward"].replays >= 2


# --------------------------------------------------------------------------------------------------------- 6. sweep
def test_adpit_sweep_host_device_select_device_score(ops, tmp_path):
    """``sweep_conf_thresh`` on the ADPIT chain, host / device_select / device_select + device_score: the same new threshold
    and loss, score tables within 1e-9 of the host's, the final output folder byte-identical."""
    from adyolo_amd import test as atest
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.features import FeatureExtractor, load_scaler_npz
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import ComputeSELDResults, DeviceSELDScorer
    from adyolo_amd.wrapper import WrapperCriterion
    g = np.load(os.path.join(G, "seld_chain_adpit.npz"))
    prm, model, cdir, _ = _chain_setup(tmp_path, g)
    fx = FeatureExtractor(load_scaler_npz(os.path.join(G, "scaler_DCASE2021.npz")), "cuda:0")
    crit = WrapperCriterion(prm)
    ds = FoaDataset(prm, "test", is_valid=True)
    names = ds.get_filelist()

    class AudioModel:                          # sweep_conf_thresh feeds ``model(feat)``: here feat is the clip's audio
        def eval(self):
            model.eval()

        def __call__(self, audio):
            return model(fx(audio, channels_last8=True), channels_last8=True)
    batches = []
    for i in range(len(ds)):
        pcm, _, lab = ds[i]
        t = (pcm.shape[0] // 600) * 600
        audio = ops.pcm16_to_f32(torch.from_numpy(np.ascontiguousarray(pcm[:t])).cuda()).view(1, t, 4)
        batches.append((audio, lab.unsqueeze(0)))
    got = {}
    for key, kw in (("host", {}), ("select", {"device_select": True}),
                    ("select_score", {"device_select": True, "device_score": True})):
        post = LabelPostProcessor(prm)
        scorer = DeviceSELDScorer(prm, cdir) if "device_score" in kw else ComputeSELDResults(prm, cdir)
        got[key] = atest.sweep_conf_thresh(batches, names, AudioModel(), crit, post, scorer, "cuda:0",
                                           os.path.join(tmp_path, "sweep_" + key), **kw)
        assert post.get_conf_thresh() == got[key][0]
    new_h, table_h, loss_h = got["host"]
    table_h = np.asarray(table_h, dtype=np.float64)
    assert table_h.shape == (9, 5) and len({tuple(r) for r in table_h}) > 1
    for key in ("select", "select_score"):
        new_d, table_d, loss_d = got[key]
        assert new_d == new_h and loss_d == loss_h, key
        np.testing.assert_allclose(np.asarray(table_d, dtype=np.float64), table_h, rtol=0, atol=1e-9, err_msg=key)
        _same_folder(os.path.join(tmp_path, "sweep_host"), os.path.join(tmp_path, "sweep_" + key), len(names))
