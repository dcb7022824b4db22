"""Labelled evaluation through windows against the whole-recording corpus pass, on a synthetic labelled split on local disk.

The folder of tools/infer_bench.py (--recordings int16 noise recordings between 20 and 180 s, at least 12 distinct lengths: more
than ``graph.MAX_GRAPHS``) with a synthetic reference CSV per recording (about 1.5 events per label frame) is written to --dir
as a 'test' split and loaded once (``load_eval_split``).  After one untimed pass each, --repeats passes of

  whole     test_epoch_corpus on EvalDeviceCorpus with ForwardGraphs and a DeviceSELDScorer (--batch clips per pass where
            consecutive lengths are equal: on this folder one clip and one graph per pass, recorded again whenever evicted)
  windowed  test_epoch_windows on EvalWindowCorpus (--window s windows, --margin s margin, --batch windows per pass, one graph)
            with ForwardGraphs and a DeviceSELDScorer

are timed by the host clock around the pass (output_pth=None: each ends in its one device synchronisation); the medians are
reported per recorded second, with the host CPU seconds of a pass (``time.process_time``) and the graphs recorded per pass.

The scorer alone: the rows the windowed pass selects are kept on the device, and ``ops.seld_score_runs`` over all passes of the
split is timed between two device events (median of 20) against ``ops.seld_score`` on the same rows, one whole-recording call
per recording; both into a zeroed accumulator, whose bits are compared.

  python tools/eval_windows_bench.py [--dir DIR] [--recordings 14] [--batch 8] [--window 20] [--margin 2]
                                     [--loss adyolo|seddoa|accdoa|adpit] [--conf 0.3] [--repeats 5] [--json out.json] [--keep]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infer_bench import LENGTHS_S, SR, event_ms, params  # noqa: E402


def write_split(root, lengths_s, n_classes, seed=0):
    """foa_dev/dev-test + metadata_dev/dev-test under root -> recorded samples."""
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    wdir, cdir = os.path.join(root, "foa_dev", "dev-test"), os.path.join(root, "metadata_dev", "dev-test")
    os.makedirs(wdir, exist_ok=True)
    os.makedirs(cdir, exist_ok=True)
    total = 0
    for r, s in enumerate(lengths_s):
        n = int(round(SR * s))
        total += n
        audio = np.clip(rs.normal(0, 3000, size=(n, 4)), -32768, 32767).astype(np.int16)
        wavfile.write(os.path.join(wdir, "rec%03d.wav" % r), SR, audio)
        with open(os.path.join(cdir, "rec%03d.csv" % r), "w") as fid:
            for f in range(n // (SR // 10)):
                for k in range(int(rs.choice(4, p=[0.15, 0.4, 0.3, 0.15]))):
                    fid.write("%d,%d,%d,%d,%d\n" % (f, rs.randint(n_classes), k, rs.randint(-180, 180), rs.randint(-60, 61)))
    return total


def timed_cpu(run, repeats):
    """-> (wall seconds, host CPU seconds) of ``repeats`` passes after one untimed pass."""
    run()
    walls, cpus = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0, c0 = time.perf_counter(), time.process_time()
        run()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        cpus.append(time.process_time() - c0)
    return walls, cpus


def summary(walls, cpus, seconds):
    med = statistics.median(walls)
    return {"wall_s": [round(w, 4) for w in walls], "median_s": round(med, 4), "ms_per_recorded_s": round(1e3 * med / seconds, 4),
            "host_cpu_s": round(statistics.median(cpus), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "adyolo_eval_windows_bench"))
    ap.add_argument("--recordings", type=int, default=14)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--window", type=float, default=20.0)
    ap.add_argument("--margin", type=float, default=2.0)
    ap.add_argument("--loss", default="adyolo", choices=["adyolo", "seddoa", "accdoa", "adpit"])
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--conf", type=float, default=0.3, help="conf_thresh and clss_thresh (random weights: lower it until rows appear)")
    ap.add_argument("--keep", action="store_true", help="keep the folder on disk afterwards")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "eval_windows_bench needs the GPU"
    import adyolo_amd  # noqa: F401
    from adyolo_amd import graph, ops, test as atest
    from adyolo_amd.corpus import EvalDeviceCorpus, EvalWindowCorpus, load_eval_split
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    lengths = [LENGTHS_S[i % len(LENGTHS_S)] for i in range(a.recordings)]
    shutil.rmtree(a.dir, ignore_errors=True)
    res = {"batch": a.batch, "window_s": a.window, "margin_s": a.margin, "loss": a.loss, "conf_thresh": a.conf, "repeats": a.repeats,
           "max_graphs": graph.MAX_GRAPHS, "cpus": len(os.sched_getaffinity(0))}
    try:
        samples = write_split(a.dir, lengths, a.classes)
        seconds = samples / SR
        res["folder"] = {"recordings": len(lengths), "distinct_lengths": len(set(lengths)), "seconds": round(seconds, 1)}
        prm = params(a.dir, a.loss, a.classes, a.window, a.conf)
        ref = os.path.join(a.dir, "metadata_dev", "dev-test")
        torch.manual_seed(0)
        model = WrapperModel((1, 7, int(SR * a.window) // 600, 64), (), prm).to("cuda:0").eval()
        fx, post, crit = FeatureExtractor(None, "cuda:0"), LabelPostProcessor(prm), WrapperCriterion(prm)
        hc = load_eval_split(prm, "test", rank=0, world=1, verify="sample")

        whole = EvalDeviceCorpus(hc, prm, "cuda:0")
        fg_whole = ForwardGraphs(model, fx, post, warm_calls=0)
        sc_whole = DeviceSELDScorer(prm, ref, "cuda:0")
        state = {}

        def whole_pass():
            state["before"] = (fg_whole.captures, fg_whole.evictions)
            sc_whole.reset()
            state["loss"] = atest.test_epoch_corpus(whole, model, fx, crit, post, None, batch_size=a.batch, forward=fg_whole,
                                                    device_scorer=sc_whole)
        res["whole"] = dict(summary(*timed_cpu(whole_pass, a.repeats), seconds), loss=state["loss"],
                            passes=len(whole.batches(a.batch)), graphs_recorded_per_pass=fg_whole.captures - state["before"][0],
                            graphs_evicted_per_pass=fg_whole.evictions - state["before"][1])
        res["whole"]["seld"] = [float(v) for v in sc_whole.scores()[:5]]
        print(json.dumps({"whole": res["whole"]}), flush=True)
        del fg_whole, whole
        torch.cuda.empty_cache()

        corpus = EvalWindowCorpus(hc, prm, "cuda:0", window_s=a.window, margin_s=a.margin, batch_size=a.batch)
        fg = ForwardGraphs(model, fx, post, warm_calls=0)
        sc = DeviceSELDScorer(prm, ref, "cuda:0")

        def windowed_pass():
            state["before"] = fg.captures
            sc.reset()
            state["loss"] = atest.test_epoch_windows(corpus, model, fx, crit, post, None, forward=fg, device_scorer=sc)
        res["windowed"] = dict(summary(*timed_cpu(windowed_pass, a.repeats), seconds), loss=state["loss"], windows=corpus.n_windows,
                               passes=corpus.n_passes, graphs_recorded_per_pass=fg.captures - state["before"],
                               graphs_held=len(fg.entries))
        res["windowed"]["seld"] = [float(v) for v in sc.scores()[:5]]
        res["whole_over_windowed"] = round(res["whole"]["median_s"] / res["windowed"]["median_s"], 2)
        print(json.dumps({"windowed": res["windowed"], "whole_over_windowed": res["whole_over_windowed"]}), flush=True)

        # ------------------------------------------------------------------------------------------------ the scorer alone
        kept, stitched = [], None
        acc = ops.loss_accumulator(corpus.device)
        with torch.no_grad():
            for p in range(corpus.n_passes):
                stitched, run = atest._window_pass(corpus, p, model, fx, crit, post, fg, acc, stitched)
                rows, counts = post.select_device_rows(run, 1, trim=False)
                kept.append((rows.clone(), counts.clone()))
        totals = [int(c.sum().item()) for _, c in kept]
        all_rows = torch.cat([r[:t] for (r, _), t in zip(kept, totals)], 0)
        all_counts = torch.cat([c for _, c in kept], 0)
        ends = torch.cumsum(all_counts, 0).cpu().numpy()
        per_rec = []
        for r, name in enumerate(corpus.get_filelist()):
            f0, f1 = int(corpus.frame_start[r]), int(corpus.frame_start[r + 1])
            r0 = int(ends[f0 - 1]) if f0 else 0
            r1 = int(ends[f1 - 1]) if f1 else 0
            ids = torch.tensor([sc._lookup(name)], dtype=torch.int32, device="cuda:0")
            per_rec.append((all_rows[r0:r1].contiguous(), all_counts[f0:f1].contiguous(), ids, f1 - f0))
        segments = corpus.segments(sc)
        status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        acc_runs, acc_whole = torch.zeros_like(sc._acc), torch.zeros_like(sc._acc)

        def score_runs():
            acc_runs.zero_()
            for (rows, counts), (dev, seg_blocks, _) in zip(kept, segments):
                ops.seld_score_runs(rows, counts, sc.table, dev, seg_blocks, acc_runs, status)

        def score_whole():
            acc_whole.zero_()
            for rows, counts, ids, t in per_rec:
                ops.seld_score(rows, counts, sc.table, ids, t, acc_whole, status)
        res["seld_score_runs"] = dict(event_ms(score_runs, 20), calls=len(kept))
        res["seld_score"] = dict(event_ms(score_whole, 20), calls=len(per_rec))
        res["scorer"] = {"rows": int(sum(totals)), "frames": int(all_counts.numel()), "status": int(status.item()),
                         "same_bits": bool(torch.equal(acc_runs.view(torch.int64), acc_whole.view(torch.int64))),
                         "runs_ms_per_recorded_s": round(res["seld_score_runs"]["median_ms"] / seconds, 6),
                         "whole_ms_per_recorded_s": round(res["seld_score"]["median_ms"] / seconds, 6)}
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
