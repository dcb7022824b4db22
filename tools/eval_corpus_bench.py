"""Evaluation from an HBM-resident split against the host-fed evaluation pass, on a synthetic split written to local disk.

A labelled split in the reference's layout (``foa_dev/dev-test`` + ``metadata_dev/dev-test``: --clips recordings of 60 s of int16
noise, CSVs with ~1 event per label frame, 12 classes) is written to --dir.  With the page cache warm, the SECOND pass of each
of these is timed (the first records the forward graphs):

  host          test_epoch_audio(batch_size, forward=ForwardGraphs, device_select=True, device_scorer=...): per clip one WAV
                read, one CSV parse, the host label encoding, the upload, one criterion call
  corpus        test_epoch_corpus with the same batch size and graphs, output_pth=None (one synchronisation per pass)
  corpus_csv    the same writing the CSV files, as the host pass does
  host_sweep    sweep_conf_thresh(device_select=True, device_score=True) fed clip by clip from audio and targets already on the
                device (its loader is built outside the timing: the forward passes, the per-clip losses, the nine selections
                and the scores are timed, not the file reads)
  corpus_sweep  sweep_conf_thresh_corpus
For each: wall time per clip, host CPU seconds per clip (resource.getrusage of this process) and the mean loss, which must be
the same float on both sides; plus the load (host read + upload) time and the bytes held on the device.

  python tools/eval_corpus_bench.py [--dir /tmp/adyolo_eval_bench] [--clips 48] [--batch 8] [--loss adyolo|seddoa|accdoa|adpit]
                                    [--json out.json] [--keep]
"""
import argparse
import json
import os
import resource
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SR, REC_S = 24000, 60


def write_split(root, n_clips, seed=0, n_classes=12):
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    wdir, cdir = os.path.join(root, "foa_dev", "dev-test"), os.path.join(root, "metadata_dev", "dev-test")
    os.makedirs(wdir, exist_ok=True)
    os.makedirs(cdir, exist_ok=True)
    for r in range(n_clips):
        audio = np.clip(rs.normal(0, 3000, size=(SR * REC_S, 4)), -32768, 32767).astype(np.int16)
        name = "fold4_room%d_mix%03d" % (r % 10, r)
        wavfile.write(os.path.join(wdir, name + ".wav"), SR, audio)
        with open(os.path.join(cdir, name + ".csv"), "w") as fid:
            for f in range(REC_S * 10):
                for s in range(int(rs.choice(3, p=[0.35, 0.45, 0.2])) or (1 if f == REC_S * 10 - 1 else 0)):
                    fid.write("%d,%d,%d,%r,%r\n" % (f, int(rs.randint(n_classes)), s, round(float(rs.uniform(-180, 180)), 1),
                                                  round(float(rs.uniform(-60, 60)), 1)))
    return n_clips * SR * REC_S * 8


def params(root, loss, n_classes):
    from __graft_entry__ import _params
    prm = _params(nb_classes=n_classes)
    prm["args"]["loss"] = loss
    prm["data_config"].update({"data_pth": root, "sr": SR, "label_hop_len_s": 0.1})
    prm["train_config"].update({"conf_thresh": 0.5, "clss_thresh": 0.5, "unify_thresh": 15.0, "nms": "conn-merge"})
    return prm


def cpu_seconds():
    s = resource.getrusage(resource.RUSAGE_SELF)
    return s.ru_utime + s.ru_stime


def timed(run, n_clips):
    torch.cuda.synchronize()
    c0, t0 = cpu_seconds(), time.perf_counter()
    res = run()
    torch.cuda.synchronize()
    t1, c1 = time.perf_counter(), cpu_seconds()
    loss = res[2] if isinstance(res, tuple) else res
    return {"wall_s": round(t1 - t0, 4), "wall_ms_per_clip": round(1e3 * (t1 - t0) / n_clips, 3),
            "cpu_ms_per_clip": round(1e3 * (c1 - c0) / n_clips, 3), "loss": loss}, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=os.path.join("/tmp", "adyolo_eval_bench"))
    ap.add_argument("--clips", type=int, default=48)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--loss", default="adyolo", choices=["adyolo", "seddoa", "accdoa", "adpit"])
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--keep", action="store_true", help="keep the split on disk afterwards")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "eval_corpus_bench needs the GPU"
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops, test as atest
    from adyolo_amd.corpus import EvalDeviceCorpus, load_eval_split
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    shutil.rmtree(a.dir, ignore_errors=True)
    t0 = time.perf_counter()
    nbytes = write_split(a.dir, a.clips, n_classes=a.classes)
    res = {"split": {"clips": a.clips, "seconds_per_clip": REC_S, "wav_bytes": nbytes, "write_s": round(time.perf_counter() - t0, 2)},
           "batch": a.batch, "loss": a.loss, "cpus": len(os.sched_getaffinity(0))}
    print(json.dumps(res), flush=True)
    try:
        prm = params(a.dir, a.loss, a.classes)
        ref = os.path.join(a.dir, "metadata_dev", "dev-test")
        out = os.path.join(a.dir, "out")
        torch.manual_seed(0)
        model = WrapperModel((1, 7, SR * REC_S // 600, 64), (), prm).to("cuda:0").eval()
        fx, crit, post = FeatureExtractor(None, "cuda:0"), WrapperCriterion(prm), LabelPostProcessor(prm)
        fg = ForwardGraphs(model, fx, post, warm_calls=0)
        ds = FoaDataset(prm, "test", is_valid=True, rank=0, world=1)
        n = len(ds)

        t0 = time.perf_counter()
        hs = load_eval_split(prm, "test", rank=0, world=1, verify="sample")
        t1 = time.perf_counter()
        corpus = EvalDeviceCorpus(hs, prm, "cuda:0")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res["load"] = {"host_s": round(t1 - t0, 3), "upload_s": round(t2 - t1, 3), "device_bytes": corpus.nbytes(),
                       "ms_per_clip": round(1e3 * (t2 - t0) / n, 3)}
        print(json.dumps({"load": res["load"]}), flush=True)

        scorer = DeviceSELDScorer(prm, ref, "cuda:0")      # the reference CSVs are parsed and uploaded once, outside the timing

        def host_pass():
            scorer.reset()
            return atest.test_epoch_audio(ds, model, fx, crit, post, "cuda:0", out, batch_size=a.batch, forward=fg,
                                          device_select=True, device_scorer=scorer)

        def corpus_pass(output_pth=None):
            scorer.reset()
            return atest.test_epoch_corpus(corpus, model, fx, crit, post, output_pth, batch_size=a.batch, forward=fg,
                                           device_scorer=scorer)
        for key, run in (("host", host_pass), ("corpus", corpus_pass), ("corpus_csv", lambda: corpus_pass(out))):
            run()
            res[key], _ = timed(run, n)
            print(json.dumps({key: res[key]}), flush=True)
        res["same_loss"] = res["host"]["loss"] == res["corpus"]["loss"] == res["corpus_csv"]["loss"]

        if not a.no_sweep:
            class AudioModel:                      # sweep_conf_thresh feeds ``model(feat)``: here feat is the clip's audio
                def eval(self):
                    model.eval()

                def __call__(self, audio):
                    return fg(audio)[0]
            loader = []
            for i in range(n):
                item = ds[i]
                pcm = torch.from_numpy(np.ascontiguousarray(item[0][:item[0].shape[0] // 600 * 600])).to("cuda:0")
                label = item[2].unsqueeze(0) if isinstance(item[2], torch.Tensor) else audio_collate_fn([item])[2]
                loader.append((ops.pcm16_to_f32(pcm).view(1, -1, 4), label))

            def host_sweep():
                return atest.sweep_conf_thresh(loader, ds.get_filelist(), AudioModel(), crit, LabelPostProcessor(prm), scorer,
                                               "cuda:0", out, device_select=True, device_score=True)

            def corpus_sweep():
                return atest.sweep_conf_thresh_corpus(corpus, model, fx, crit, LabelPostProcessor(prm), scorer, output_pth=out,
                                                      batch_size=a.batch, forward=fg)
            got = {}
            for key, run in (("host_sweep", host_sweep), ("corpus_sweep", corpus_sweep)):
                run()
                res[key], got[key] = timed(run, n)
                print(json.dumps({key: res[key]}), flush=True)
            # (the host sweep runs one clip per forward pass, the corpus sweep --batch: the passes agree to rounding, so a
            #  detection at a threshold can differ; the tests compare the two sweeps at one batching, bit for bit)
            th, tc = (np.asarray(got[k][1], dtype=np.float64) for k in ("host_sweep", "corpus_sweep"))
            res["sweep"] = {"host_thresh": float(got["host_sweep"][0]), "corpus_thresh": float(got["corpus_sweep"][0]),
                            "table_max_abs_diff": float(np.abs(th - tc).max())}
        print(json.dumps(res), flush=True)
    finally:
        if not a.keep:
            shutil.rmtree(a.dir, ignore_errors=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
