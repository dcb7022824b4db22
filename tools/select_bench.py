"""Host ``postprocess.nms_decoded`` against the device selection (``LabelPostProcessor.select_device``) of the AD-YOLO head.

  python tools/select_bench.py [--frames 600] [--reps 5] [--out results.json]

* synthetic 60 s clips (600 frames, C = 12, random logits, objectness biases -2 / -1 / 0, decoded by ``ops.yolo_decode``) at
  thresholds 0.1 .. 0.9 and the three nms modes: wall time of ``select`` on the host decode and of ``select_device`` on the
  device decode (kernels + the row copy + grouping), the device time of the selection kernels alone, the rows, and the
  ``yolo_decode`` time of the same clip;
* ``sweep_conf_thresh`` wall time on the three clips of tests/golden/seld_chain.npz (the evaluation chain's filler-weight
  model), host selection against ``device_select=True``.
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

THRESHOLDS = [round(0.1 * i, 1) for i in range(1, 10)]
NMS = ["conn-merge", "soft-merge", "default"]


def _params(nms="conn-merge", thresh=0.5, unify=15.0):
    return {"args": {"device": "cuda:0", "encoder": "se-resnet34", "loss": "adyolo"},
            "data_config": {"nb_classes": 12},
            "train_config": {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
                             "conf_thresh": thresh, "clss_thresh": thresh, "unify_thresh": unify, "nms": nms,
                             "loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0}}}


def _median_wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def _kernels_ms(dec, thresh, nms, n=20):
    """Device time of the three selection launches alone (no row-total read, no copy), per call."""
    import ctypes
    from adyolo_amd import _lib, ops
    frames = dec.shape[0]
    ws = torch.empty(_lib.load().adyolo_yolo_select_workspace_words(frames, 160, 12), device=dec.device)
    rows = torch.empty(frames * 12 * 160 * 5, device=dec.device)
    counts = torch.empty(frames + 1, dtype=torch.int32, device=dec.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                      # noqa: E731
    t = ops.np_f32_threshold(thresh, ">")
    mode = ops.SELECT_MODES.get(nms, 0)
    u = ops.np_f32_threshold(15.0, "<" if mode == 1 else "<=")
    args = (p(dec), p(ws), p(rows), p(counts), frames, 160, 12, t, t, u, t, mode, ops._stream())
    _lib.call("adyolo_yolo_select", *args)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        _lib.call("adyolo_yolo_select", *args)
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / n


def synthetic(frames, reps):
    from adyolo_amd import ops
    from adyolo_amd.postprocess import LabelPostProcessor
    rs = np.random.RandomState(0)
    lg = rs.normal(0.0, 1.5, size=(frames, 160, 15))
    lg[..., 0] += np.asarray([-2.0, -1.0, 0.0])[np.arange(frames) % 3][:, None]
    logit = torch.from_numpy(lg.astype(np.float32)).cuda().view(1, frames, -1)
    dec = ops.yolo_decode(logit, 12)
    host = dec.cpu().numpy()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ops.yolo_decode(logit, 12)
    ev[0].record()
    for _ in range(20):
        ops.yolo_decode(logit, 12)
    ev[1].record()
    torch.cuda.synchronize()
    res = {"frames": frames, "decode_ms": ev[0].elapsed_time(ev[1]) / 20, "rows": []}
    for nms in NMS:
        pp = LabelPostProcessor(_params(nms))
        for th in THRESHOLDS:
            pp.set_conf_thresh(th)
            pp.select_device(dec)                                   # warm: allocations, pinned buffers
            t_dev, got = _median_wall(lambda: pp.select_device(dec), reps)
            t_host, ref = _median_wall(lambda: pp.select(host), 1 if th < 0.3 else reps)
            n = sum(len(v) for v in ref.values())
            assert n == sum(len(v) for v in got[0].values())
            k_ms = _kernels_ms(dec, th, nms)
            res["rows"].append({"nms": nms, "thresh": th, "rows": n, "host_ms": 1e3 * t_host, "device_ms": 1e3 * t_dev,
                                "kernels_ms": k_ms})
            print("%-10s %.1f  rows %7d  host %10.2f ms  device %7.3f ms (kernels %.3f ms)"
                  % (nms, th, n, 1e3 * t_host, 1e3 * t_dev, k_ms), file=sys.stderr)
    return res


def chain_sweep():
    from scipy.io import wavfile
    from oracle.filler import fill_module_
    from seld_chain_inputs import CLIPS, chain_clip
    from adyolo_amd import ops, test as atest
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    from adyolo_amd.features import FeatureExtractor, load_scaler_npz
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import ComputeSELDResults
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    g = np.load(os.path.join(ROOT, "tests", "golden", "seld_chain.npz"))
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        wdir, cdir = os.path.join(tmp, "foa_dev", "dev-test"), os.path.join(tmp, "metadata_dev", "dev-test")
        os.makedirs(wdir), os.makedirs(cdir)
        for name, seed, n in CLIPS:
            wavfile.write(os.path.join(wdir, name + ".wav"), 24000, chain_clip(seed, n))
            with open(os.path.join(cdir, name + ".csv"), "w") as f:
                for r in g["ref_" + name]:
                    f.write("%d,%d,%d,%d,%d\n" % tuple(int(v) for v in r))
        prm = _params(unify=float(g["unify_thresh"]))
        prm["data_config"].update(sr=24000, label_hop_len_s=0.1, data_pth=tmp)
        prm["aug_config"] = {"rotation_augment": False, "spec_augment": False}
        model = WrapperModel((1, 7, 400, 64), (), prm)
        fill_module_(model)
        model = model.to("cuda:0").eval()
        fx = FeatureExtractor(load_scaler_npz(os.path.join(ROOT, "tests", "golden", "scaler_DCASE2021.npz")), "cuda:0")
        crit, scorer = WrapperCriterion(prm), ComputeSELDResults(prm, cdir)
        ds = FoaDataset(prm, "test", is_valid=True)

        class AudioModel:
            def eval(self):
                model.eval()

            def __call__(self, audio):
                return model(fx(audio, channels_last8=True), channels_last8=True)
        batches = []
        for i in range(len(ds)):
            pcm, _, rows = ds[i]
            t = (pcm.shape[0] // 600) * 600
            audio = ops.pcm16_to_f32(torch.from_numpy(np.ascontiguousarray(pcm[:t])).cuda()).view(1, t, 4)
            batches.append((audio, audio_collate_fn([(pcm, 0, rows)])[2]))
        for device_select in (False, True, False, True):                # the second pair is the one reported (warm)
            post = LabelPostProcessor(prm)
            t0 = time.perf_counter()
            new, table, _ = atest.sweep_conf_thresh(batches, ds.get_filelist(), AudioModel(), crit, post, scorer, "cuda:0",
                                                    os.path.join(tmp, "out"), device_select=device_select)
            res["device_s" if device_select else "host_s"] = time.perf_counter() - t0
            res["new_thresh_" + ("device" if device_select else "host")] = float(new)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import adyolo_amd  # noqa: F401
    res = {"synthetic": synthetic(a.frames, a.reps), "chain_sweep": chain_sweep()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
