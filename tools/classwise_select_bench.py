"""Host ``postprocess.classwise_select`` against the device selection (``LabelPostProcessor.select_device``) of the class-wise
heads, ADPIT at C = 13 (BASELINE config 5).

  python tools/classwise_select_bench.py [--frames 600] [--reps 7] [--sweep-reps 3] [--out results.json]

* one synthetic 60 s clip (600 frames, C = 13, outputs uniform in [-1, 1), every third frame with two tracks nearly on top of
  each other, decoded by ``ops.classwise_decode``) at thresholds 0.1, 0.5 and 0.9, unify 30 degrees: wall time of ``select`` on
  the host decode and of ``select_device`` on the device decode (kernels + the row copy + grouping), the two alternating, medians;
  the stream time per call of the three selection launches alone (device events around 50 back-to-back calls, launch overhead
  included, median of 7 batches); the rows; the ``classwise_decode`` time measured the same way and the time of the decode's
  page-locked copy to the host (what the host path pays before it can select).  The device rows are checked against the
  host's, bit for bit, before anything is timed;
* ``sweep_conf_thresh`` wall time on the three clips of tests/golden/seld_chain_adpit.npz (the evaluation chain's
  filler-weight model, nine thresholds): host, ``device_select=True``, and ``device_select=True, device_score=True``, the three
  alternating, one warm round, then the median of ``--sweep-reps`` rounds.
Prints one JSON object."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

C = 13
THRESHOLDS = [0.1, 0.5, 0.9]
UNIFY = 30.0


def _params(data_pth=None, nb_classes=C, thresh=0.5, unify=UNIFY):
    prm = {"args": {"device": "cuda:0", "encoder": "se-resnet34", "loss": "adpit"},
           "data_config": {"nb_classes": nb_classes, "sr": 24000, "label_hop_len_s": 0.1},
           "aug_config": {"rotation_augment": False, "spec_augment": False},
           "train_config": {"conf_thresh": thresh, "unify_thresh": unify}}
    if data_pth is not None:
        prm["data_config"]["data_pth"] = data_pth
    return prm


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _events_ms(fn, n=50, batches=7):
    """Stream time per call between two device events around n back-to-back calls, median over the batches (after one warm
    batch).  The calls are enqueued by the host as fast as it can, so whenever the queue drains this includes launch overhead:
    it is the cost of a call on a busy stream, not the sum of the kernels' execution times."""
    ts = []
    for b in range(batches + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        if b:
            ts.append(ev[0].elapsed_time(ev[1]) / n)
    return float(np.median(ts))


def _launches_ms(dec, thresh):
    """``_events_ms`` of the three selection launches alone (no row-total read, no copy)."""
    import ctypes
    from adyolo_amd import _lib, ops
    frames = dec.shape[0]
    ws = torch.empty(_lib.load().adyolo_classwise_select_workspace_words(frames, C, 2), device=dec.device)
    rows = torch.empty(frames * C * 3 * 5, device=dec.device)
    counts = torch.empty(frames + 1, dtype=torch.int32, device=dec.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                      # noqa: E731
    args = (p(dec), p(ws), p(rows), p(counts), frames, C, 2, ops.np_f32_threshold(thresh, ">"),
            ops.np_f32_threshold(UNIFY, "<"), ops._stream())
    return _events_ms(lambda: _lib.call("adyolo_classwise_select", *args))


def synthetic(frames, reps):
    from adyolo_amd import ops
    from adyolo_amd.postprocess import LabelPostProcessor
    rs = np.random.RandomState(0)
    out = rs.uniform(-1.0, 1.0, size=(frames, 9 * C)).astype(np.float32)
    v = out.reshape(frames, 3, 3, C)
    v[::3, 1] = v[::3, 0] + rs.uniform(-0.2, 0.2, size=v[::3, 0].shape).astype(np.float32)
    output = torch.from_numpy(out).cuda().view(1, frames, -1)
    dec = ops.classwise_decode(output, C, "adpit")
    host = ops.to_host(dec).numpy().copy()
    res = {"frames": frames, "classes": C, "unify": UNIFY, "decode_ms": _events_ms(lambda: ops.classwise_decode(output, C, "adpit")),
           "decode_bytes": int(dec.numel() * 4), "rows": []}
    ops.to_host(dec)
    res["decode_to_host_ms"] = 1e3 * float(np.median([_wall(lambda: ops.to_host(dec))[0] for _ in range(reps)]))
    pp = LabelPostProcessor(_params())
    for th in THRESHOLDS:
        pp.set_conf_thresh(th)
        got, ref = pp.select_device(dec)[0], pp.select(host)                        # warm: allocations, pinned buffers
        assert got.keys() == ref.keys()
        a = np.asarray([r for rr in got.values() for r in rr], dtype=np.float32)
        b = np.asarray([r for rr in ref.values() for r in rr], dtype=np.float32)
        assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), "device rows differ from the host's"
        t_dev, t_host = [], []
        for _ in range(reps):                                                       # alternating
            t_host.append(_wall(lambda: pp.select(host))[0])
            t_dev.append(_wall(lambda: pp.select_device(dec))[0])
        r = {"thresh": th, "rows": int(len(a)), "host_ms": 1e3 * float(np.median(t_host)),
             "device_ms": 1e3 * float(np.median(t_dev)), "host_ms_minmax": [1e3 * min(t_host), 1e3 * max(t_host)],
             "device_ms_minmax": [1e3 * min(t_dev), 1e3 * max(t_dev)], "launches_ms": _launches_ms(dec, th)}
        print("adpit %.1f  rows %6d  host %8.3f ms  device %8.3f ms (launches %.4f ms)"
              % (th, r["rows"], r["host_ms"], r["device_ms"], r["launches_ms"]), file=sys.stderr)
        res["rows"].append(r)
    return res


def chain_sweep(reps):
    from scipy.io import wavfile
    from oracle.filler import fill_module_
    from seld_chain_inputs import CLIPS, chain_clip
    from adyolo_amd import ops, test as atest
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.features import FeatureExtractor, load_scaler_npz
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import ComputeSELDResults, DeviceSELDScorer
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    g = np.load(os.path.join(ROOT, "tests", "golden", "seld_chain_adpit.npz"))
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        wdir, cdir = os.path.join(tmp, "foa_dev", "dev-test"), os.path.join(tmp, "metadata_dev", "dev-test")
        os.makedirs(wdir), os.makedirs(cdir)
        for name, seed, n in CLIPS:
            wavfile.write(os.path.join(wdir, name + ".wav"), 24000, chain_clip(seed, n))
            with open(os.path.join(cdir, name + ".csv"), "w") as f:
                for r in g["ref_" + name]:
                    f.write("%d,%d,%d,%d,%d\n" % tuple(int(v) for v in r))
        prm = _params(tmp, nb_classes=12, thresh=float(g["conf_thresh"]), unify=float(g["unify_thresh"]))
        model = WrapperModel((1, 7, 400, 64), (), prm)
        fill_module_(model)
        model = model.to("cuda:0").eval()
        fx = FeatureExtractor(load_scaler_npz(os.path.join(ROOT, "tests", "golden", "scaler_DCASE2021.npz")), "cuda:0")
        crit = WrapperCriterion(prm)
        scorers = {"host": ComputeSELDResults(prm, cdir), "device_select": ComputeSELDResults(prm, cdir),
                   "device_select_score": DeviceSELDScorer(prm, cdir)}
        ds = FoaDataset(prm, "test", is_valid=True)

        class AudioModel:
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
        modes = (("host", {}), ("device_select", {"device_select": True}),
                 ("device_select_score", {"device_select": True, "device_score": True}))
        times = {key: [] for key, _ in modes}
        for rep in range(reps + 1):                                     # round 0 warms every path and is not reported
            for key, kw in modes:
                post = LabelPostProcessor(prm)
                dt, (new, table, _) = _wall(lambda: atest.sweep_conf_thresh(
                    batches, ds.get_filelist(), AudioModel(), crit, post, scorers[key], "cuda:0", os.path.join(tmp, "out"), **kw))
                if rep:
                    times[key].append(dt)
                res["new_thresh_" + key] = float(new)
                res["seld_" + key] = [float(r[4]) for r in table]
        for key, ts in times.items():
            res[key + "_s"] = float(np.median(ts))
            res[key + "_s_minmax"] = [min(ts), max(ts)]
        res["rounds"] = reps
        res["device_select_score_not_slower_than_host"] = bool(res["device_select_score_s"] <= res["host_s"])
        print("adpit sweep: host %.4f s, device_select %.4f s, device_select + device_score %.4f s"
              % (res["host_s"], res["device_select_s"], res["device_select_score_s"]), file=sys.stderr)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweep-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import adyolo_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("classwise_select_bench.py measures the device selection: it needs a GPU")
    res = {"synthetic": synthetic(a.frames, a.reps), "chain_sweep": chain_sweep(a.sweep_reps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
