"""Streaming inference: what the ring gather costs beside the linear one, and what a push costs.

Gather.  ``ops.stream_gather_windows`` against ``ops.corpus_gather_windows`` on the same --windows windows of --window s: the
windows lie --hop s apart in a stream whose last samples a ring of exactly that span holds, its head placed so that the ring
has wrapped and one window straddles the seam; the linear gather reads the same table from the stream laid out linearly.
The two are alternated in one session, --reps times each after an untimed call, between device events; medians with least
and largest, the ratio of the medians, and the rate over the bytes read and written.  The outputs are compared bit for bit.

Stream.  A --seconds s recording of int16 noise pushed hop by hop into ``test.StreamInference`` at window --window s / margin
--margin s, once per hop of --hops, eager and with ``ForwardGraphs``: the host clock around every ``push`` (a push that runs a
pass ends in its one synchronisation), reported as the median, least and largest over the pushes that completed a step, over
those that did not, and the whole stream per recorded second.  Beside the first hop the same recording through
``infer_epoch_corpus`` at batch_size 1 (the file path: the recording in HBM before the clock starts).  The streamed CSV at the
default hop is compared with the file path's, byte for byte.  The weights are random filler: row counts, and with them the
copy of the rows, are not a trained model's.

  python tools/stream_bench.py [--window 20] [--margin 2] [--hops 16,1,0.1] [--seconds 180] [--windows 8] [--hop 16]
                               [--reps 30] [--loss adyolo] [--conf 0.5] [--skip-stream] [--json out.json]
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SR, HOP_LABEL = 24000, 2400
DEV = "cuda:0"


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def gather_bench(a):
    from adyolo_amd import ops
    n, hop = int(SR * a.window), int(SR * a.hop)
    cap = n + (a.windows - 1) * hop                                          # exactly the windows' span
    head = 2 * cap + hop + n // 2                                            # wrapped twice; the seam falls inside a window
    first = head - cap
    rows = [(first + k * hop, n, 0, 0, 0, 0, 0, 0) for k in range(a.windows)]
    seam = head // cap * cap
    assert any(r[0] < seam < r[0] + n for r in rows) and first % 2 == 0 and cap % 2 == 0
    rs = np.random.RandomState(0)
    stream = np.zeros((head, 4), dtype=np.int16)
    stream[first:] = rs.randint(-32768, 32768, size=(cap, 4)).astype(np.int16)
    ring = np.empty((cap, 4), dtype=np.int16)
    ring[(first + np.arange(cap)) % cap] = stream[first:]
    dstream, dring = torch.from_numpy(stream).to(DEV), torch.from_numpy(ring).to(DEV)
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    out_l, out_r = torch.empty((a.windows, n, 4), device=DEV), torch.empty((a.windows, n, 4), device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def linear():
        ops.corpus_gather_windows(dstream, table, out_l, status)

    def ringed():
        ops.stream_gather_windows(dring, head, table, out_r, status)

    linear(), ringed()
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and torch.equal(out_l.view(torch.int32), out_r.view(torch.int32)), "the two gathers differ"
    ms = {"linear": [], "ring": []}
    for _ in range(a.reps):
        for key, run in (("linear", linear), ("ring", ringed)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms[key].append(e0.elapsed_time(e1))
    moved = a.windows * n * (8 + 16)
    res = {k: dict(spread(v), gb_per_s=round(moved / statistics.median(v) / 1e6, 1)) for k, v in ms.items()}
    # two halves of the linear gather's own timings: what two runs of one binary show
    half = len(ms["linear"]) // 2
    res["linear_half_over_half"] = round(statistics.median(ms["linear"][:half]) / statistics.median(ms["linear"][half:]), 4)
    res["ring_over_linear"] = round(res["ring"]["median_ms"] / res["linear"]["median_ms"], 4)
    res["shape"] = {"windows": a.windows, "window_s": a.window, "hop_s": a.hop, "capacity": cap, "bytes": moved}
    return res


def params(folder, loss, n_classes, window_s, conf):
    from __graft_entry__ import _params
    prm = _params(nb_classes=n_classes)
    prm["args"].update({"loss": loss, "infer_pth": folder})
    prm["data_config"].update({"data_pth": folder, "sr": SR, "label_hop_len_s": 0.1, "chunk_window_s": window_s, "chunk_stride_s": 1})
    prm["train_config"].update({"conf_thresh": conf, "clss_thresh": conf, "unify_thresh": 15.0, "nms": "conn-merge"})
    return prm


def stream_bench(a, res):
    from adyolo_amd import test as atest
    from adyolo_amd.corpus import InferDeviceCorpus, StreamDeviceCorpus, infer_split_from_arrays
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.wrapper import WrapperModel
    work = tempfile.mkdtemp(prefix="adyolo_stream_bench")
    prm = params(work, a.loss, a.classes, a.window, a.conf)
    torch.manual_seed(0)
    model = WrapperModel((1, 7, int(SR * a.window) // 600, 64), (), prm).to(DEV).eval()
    fx, post = FeatureExtractor(None, DEV), LabelPostProcessor(prm)
    total = int(SR * a.seconds)
    audio = np.clip(np.random.RandomState(1).normal(0, 3000, size=(total, 4)), -32768, 32767).astype(np.int16)
    hops = [float(h) for h in a.hops.split(",")]
    default_hop = a.window - 2 * a.margin

    # the file path: the recording in HBM, batch_size 1
    corpus = InferDeviceCorpus(infer_split_from_arrays(["rec"], [audio], prm), prm, DEV, window_s=a.window, margin_s=a.margin,
                               batch_size=1)
    file_dir = os.path.join(work, "file")
    res["file_path"] = {}
    for key, fg in (("eager", None), ("graph", ForwardGraphs(model, fx, post, warm_calls=0))):
        walls, info = [], {}
        for k in range(a.repeats + 1):                                       # the first one untimed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = atest.infer_epoch_corpus(corpus, model, fx, post, file_dir, forward=fg)
            torch.cuda.synchronize()
            if k:
                walls.append(1e3 * (time.perf_counter() - t0))
        res["file_path"][key] = dict(spread(walls), ms_per_recorded_s=round(statistics.median(walls) / a.seconds, 4),
                                     ms_per_pass=round(statistics.median(walls) / info["passes"], 3), **info)
    want = open(os.path.join(file_dir, "rec.csv"), "rb").read()
    res["file_path"]["csv_bytes"] = len(want)
    print(json.dumps({"file_path": res["file_path"]}), flush=True)
    del corpus

    res["stream"] = {}
    for hop_s in hops:
        piece = int(round(SR * hop_s))
        sc = StreamDeviceCorpus(prm, DEV, window_s=a.window, margin_s=a.margin, hop_s=hop_s, batch_size=1)
        out = os.path.join(work, "live.csv")
        entry = res["stream"]["%g" % hop_s] = {"hop_frames": sc.hop_frames, "capacity_s": sc.capacity / SR, "push_samples": piece}
        for key, fg in (("eager", None), ("graph", ForwardGraphs(model, fx, post, warm_calls=0))):
            session = atest.StreamInference(sc, model, fx, post, forward=fg, output_file=out)
            for rep in range(2):                                             # the first stream untimed (the graph is recorded)
                session.reset()
                stepped, idle = [], []
                torch.cuda.synchronize()
                t_all = time.perf_counter()
                for at in range(0, total, piece):
                    before = session.passes
                    t0 = time.perf_counter()
                    session.push(audio[at:at + piece])
                    (stepped if session.passes > before else idle).append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                session.close()
                close_ms = 1e3 * (time.perf_counter() - t0)
                torch.cuda.synchronize()
                wall = 1e3 * (time.perf_counter() - t_all)
            entry[key] = {"push_with_step": spread(stepped), "push_without_step": spread(idle) if idle else None,
                          "close_ms": round(close_ms, 3), "passes": session.passes, "stream_ms": round(wall, 2),
                          "ms_per_recorded_s": round(wall / a.seconds, 4)}
            if fg is not None:
                entry[key].update(captures=fg.captures, evictions=fg.evictions)
            if abs(hop_s - default_hop) < 1e-9:
                entry[key]["csv_equals_file_path"] = open(out, "rb").read() == want
                assert entry[key]["csv_equals_file_path"], "the streamed CSV differs from the file path's"
        print(json.dumps({"stream": {"%g" % hop_s: entry}}), flush=True)
        del sc
    shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=20.0)
    ap.add_argument("--margin", type=float, default=2.0)
    ap.add_argument("--hops", default="16,1,0.1", help="the hops (s) the recording is streamed at; each is also the push size")
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--windows", type=int, default=8, help="gather: windows per launch")
    ap.add_argument("--hop", type=float, default=16.0, help="gather: the windows' distance in the stream (s)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3, help="timed passes of the file path")
    ap.add_argument("--loss", default="adyolo", choices=["adyolo", "seddoa", "accdoa", "adpit"])
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--conf", type=float, default=0.5)
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "stream_bench needs the GPU"
    import adyolo_amd  # noqa: F401
    res = {"cpus": len(os.sched_getaffinity(0)), "gather": gather_bench(a)}
    print(json.dumps({"gather": res["gather"]}), flush=True)
    if not a.skip_stream:
        stream_bench(a, res)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
