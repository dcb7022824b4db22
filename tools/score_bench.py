"""Host SELD scoring (CSV files + ``ComputeSELDResults``) against the device scorer (``seld_metrics.DeviceSELDScorer``).

  python tools/score_bench.py [--clips 100] [--frames 600] [--reps 3] [--out results.json]

* a seeded synthetic split: ``--clips`` clips of ``--frames`` frames, C = 12, about 2, 20 and 110 prediction rows per frame
  (random classes and directions, float32), the three reference files of tests/golden/seld_chain.npz repeated.  Host = writing
  the CSV files plus ``get_SELD_Results``; device = ``add_rows`` of the rows already on the device plus ``scores()`` (one
  accumulator copy), end to end with a synchronise; kernels = the ``adyolo_seld_score`` launches alone (device events).  The
  reference is parsed (host) and uploaded (device) once, outside the timings.  The device scores are checked against the
  host's before anything is timed;
* ``sweep_conf_thresh`` wall time on the three clips of seld_chain.npz (the evaluation chain's filler-weight model): host,
  ``device_select=True``, and ``device_select=True, device_score=True``.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

PRM = {"data_config": {"nb_classes": 12, "sr": 24000, "label_hop_len_s": 0.1}}


def _split(tmp, clips, frames, per_frame, seed):
    """Reference folder (seld_chain.npz's three files repeated) and the predictions: rows (N, 5) float32 in frame order and
    counts (clips * frames,) int32."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "seld_chain.npz"))
    refs = [g["ref_" + str(n)] for n in g["names"]]
    ref_dir = os.path.join(tmp, "ref")
    os.makedirs(ref_dir, exist_ok=True)
    names = ["clip%03d" % k for k in range(clips)]
    for k, name in enumerate(names):
        with open(os.path.join(ref_dir, name + ".csv"), "w") as f:
            for r in refs[k % 3]:
                f.write("%d,%d,%d,%d,%d\n" % tuple(int(v) for v in r))
    rng = np.random.default_rng(seed)
    counts = rng.poisson(per_frame, clips * frames).astype(np.int32)
    n = int(counts.sum())
    az, el = rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi / 2, np.pi / 2, n)
    rows = np.zeros((n, 5), dtype=np.float32)
    rows[:, 0] = np.repeat(np.arange(clips * frames), counts) % frames
    rows[:, 1] = rng.integers(0, 12, n)
    rows[:, 2], rows[:, 3], rows[:, 4] = np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)
    return ref_dir, names, rows, counts


def _host(ref_dir, names, dicts, out_dir, scorer):
    from adyolo_amd.postprocess import write_seld_output_file
    from adyolo_amd.test import delete_and_create_folder
    delete_and_create_folder(out_dir)
    for name, d in zip(names, dicts):
        write_seld_output_file(os.path.join(out_dir, name + ".csv"), d)
    return scorer.get_SELD_Results(out_dir)


def _kernels_ms(dev, rows, counts, fids, frames, n=10):
    from adyolo_amd import ops
    status = torch.zeros(1, dtype=torch.int32, device=rows.device)
    ops.seld_score(rows, counts, dev.table, fids, frames, dev._acc, status)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        ops.seld_score(rows, counts, dev.table, fids, frames, dev._acc, status)
    ev[1].record()
    torch.cuda.synchronize()
    ops.seld_status_check(status)
    return ev[0].elapsed_time(ev[1]) / n


def synthetic(clips, frames, reps):
    from adyolo_amd.postprocess import group_rows
    from adyolo_amd.seld_metrics import ComputeSELDResults, DeviceSELDScorer
    res = []
    for per_frame in (2, 20, 110):
        with tempfile.TemporaryDirectory() as tmp:
            ref_dir, names, rows, counts = _split(tmp, clips, frames, per_frame, seed=per_frame)
            dicts = group_rows(rows, counts, clips)
            host_scorer = ComputeSELDResults(PRM, ref_dir)
            t0 = time.perf_counter()
            dev = DeviceSELDScorer(PRM, ref_dir)
            torch.cuda.synchronize()
            upload_s = time.perf_counter() - t0
            rows_d, counts_d = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()

            def device():
                dev.reset()
                dev.add_rows(rows_d, counts_d, names)
                out = dev.scores()
                torch.cuda.synchronize()
                return out
            out_dir = os.path.join(tmp, "out")
            t0 = time.perf_counter()
            h = _host(ref_dir, names, dicts, out_dir, host_scorer)
            host_s = time.perf_counter() - t0
            d = device()
            np.testing.assert_allclose([float(v) for v in d[:5]], [float(v) for v in h[:5]], rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(d[5], h[5], rtol=1e-9, atol=1e-12)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                device()
                ts.append(time.perf_counter() - t0)
            fids = torch.tensor([dev._index[n + ".csv"] for n in names], dtype=torch.int32, device="cuda:0")
            k_ms = _kernels_ms(dev, rows_d, counts_d, fids, frames)
            r = {"rows_per_frame": per_frame, "rows": int(len(rows)), "host_s": host_s, "device_ms": 1e3 * float(np.median(ts)),
                 "kernels_ms": k_ms, "upload_s": upload_s, "seld": float(h[4])}
            print(json.dumps(r), file=sys.stderr)
            res.append(r)
    return res


def chain_sweep():
    from scipy.io import wavfile
    from oracle.filler import fill_module_
    from seld_chain_inputs import CLIPS, chain_clip
    from select_bench import _params
    from adyolo_amd import ops, test as atest
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    from adyolo_amd.features import FeatureExtractor, load_scaler_npz
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import ComputeSELDResults, DeviceSELDScorer
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
            pcm, _, rows = ds[i]
            t = (pcm.shape[0] // 600) * 600
            audio = ops.pcm16_to_f32(torch.from_numpy(np.ascontiguousarray(pcm[:t])).cuda()).view(1, t, 4)
            batches.append((audio, audio_collate_fn([(pcm, 0, rows)])[2]))
        for rep in range(2):                                            # the second round is the one reported (warm)
            for key, kw in (("host", {}), ("device_select", {"device_select": True}),
                            ("device_select_score", {"device_select": True, "device_score": True})):
                post = LabelPostProcessor(prm)
                t0 = time.perf_counter()
                new, table, _ = atest.sweep_conf_thresh(batches, ds.get_filelist(), AudioModel(), crit, post, scorers[key],
                                                        "cuda:0", os.path.join(tmp, "out"), **kw)
                res[key + "_s"] = time.perf_counter() - t0
                res["new_thresh_" + key] = float(new)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=100)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import adyolo_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("score_bench.py measures the device scorer: it needs a GPU")
    res = {"synthetic": synthetic(a.clips, a.frames, a.reps), "chain_sweep": chain_sweep()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
