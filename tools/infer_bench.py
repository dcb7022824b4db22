"""Windowed inference from an HBM-resident folder against the whole-recording inference pass, on synthetic folders on local disk.

Timing.  A folder of --recordings int16 noise recordings between 20 and 180 s with at least 12 distinct lengths (more than
``graph.MAX_GRAPHS``) is written to --dir.  With the page cache warm, after one untimed pass each, --repeats passes of

  whole     test_epoch_audio on FoaDataset('infer') with ForwardGraphs and device_select=True (--batch clips per pass where
            consecutive lengths are equal): per recording one WAV read, one upload and one graph per distinct length, recorded
            again whenever it was evicted
  windowed  infer_epoch_corpus on InferDeviceCorpus (--window s windows, --margin s margin, --batch windows per pass, one graph)

are timed by the host clock around the pass, which ends in a device synchronisation; the medians are reported per recording and
per recorded second, with the load (host read + upload) of the folder apart, and the graphs recorded / evicted in a timed pass.

Agreement.  On --clips clips of 60 s the CSV files of the windowed pass at margins of 0, 1, 2 and 4 s are compared with those of
the whole-clip pass (``test_epoch_audio``, one clip per pass, eager), frame by frame: a frame differs when its rows are not
the same text ("exact"), and when they are not the same detections ("detections": another number of rows, another class, or
a direction more than 1 degree off).  Both shares are split into the frames next to a seam (the last frame one window keeps
and the first the next one keeps) and all other frames.  The weights are random filler: the figures say how far the context a
window lacks moves THIS network's output, and little about a trained model.

Sample-rate conversion.  With --rate HZ the folder is written at that rate and loaded with ``load_infer_split(resample=True)``:
the one ``adyolo_resample_pcm`` launch over all recordings (median of 20 by device events, GB/s over the bytes read and written)
beside the host-to-device copy of the same native bytes in the same session, the load with the conversion in it, and the
windowed pass over the converted folder.  --rate 24000 is the same run without a conversion.

  python tools/infer_bench.py [--dir DIR] [--recordings 14] [--clips 4] [--batch 8] [--window 20] [--margin 2]
                              [--loss adyolo|seddoa|accdoa|adpit] [--conf 0.5] [--repeats 3] [--json out.json] [--keep]
                              [--rate HZ]
"""
import argparse
import json
import math
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

SR = 24000
# seconds: 14 distinct lengths between 20 and 180 s, all whole label hops -- the whole-recording pass takes no other length (a
# recording whose feature frames are no multiple of four is refused by the encoder's pooling; the windowed pass takes any)
LENGTHS_S = (20.0, 31.7, 44.3, 60.0, 72.5, 85.1, 97.0, 110.4, 123.9, 137.2, 150.0, 163.6, 180.0, 41.1, 60.0, 97.0)


def write_folder(root, lengths_s, seed=0, rate=SR):
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    os.makedirs(root, exist_ok=True)
    for r, s in enumerate(lengths_s):
        audio = np.clip(rs.normal(0, 3000, size=(int(round(rate * s)), 4)), -32768, 32767).astype(np.int16)
        wavfile.write(os.path.join(root, "rec%03d.wav" % r), rate, audio)
    return sum(int(round(rate * s)) for s in lengths_s)


def event_ms(run, repeats):
    """Median and range of ``run`` between two device events, after one untimed call."""
    run()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4), "n": len(out)}


def rate_run(a, res, folder, out, lengths):
    """--rate: the folder written at ``a.rate`` Hz, loaded with ``resample=True``.  The conversion launch (all recordings, one
    launch) and the host-to-device copy of the same native bytes (pageable, as the corpus uploads them, and page-locked) by
    device events in one session; the windowed pass over the converted folder as in the plain run."""
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops, resample, test as atest
    from adyolo_amd.corpus import InferDeviceCorpus, load_infer_split
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.wrapper import WrapperModel
    samples = write_folder(folder, lengths, rate=a.rate)
    seconds = samples / a.rate
    res["folder"] = {"recordings": len(lengths), "rate": a.rate, "seconds": round(seconds, 1), "native_bytes": samples * 8}
    prm = params(folder, a.loss, a.classes, a.window, a.conf)
    torch.manual_seed(0)
    model = WrapperModel((1, 7, int(SR * a.window) // 600, 64), (), prm).to("cuda:0").eval()
    fx, post = FeatureExtractor(None, "cuda:0"), LabelPostProcessor(prm)
    t0 = time.perf_counter()
    hs = load_infer_split(prm, rank=0, world=1, verify="sample", resample=True)
    t1 = time.perf_counter()
    corpus = InferDeviceCorpus(hs, prm, "cuda:0", window_s=a.window, margin_s=a.margin, batch_size=a.batch)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res["load"] = {"host_s": round(t1 - t0, 3), "upload_and_convert_s": round(t2 - t1, 3), "device_bytes": corpus.nbytes(),
                   "ms_per_recorded_s": round(1e3 * (t2 - t0) / seconds, 4)}
    if a.rate != SR:
        pl = resample.plan(a.rate, SR)
        stream = np.concatenate(hs.native, 0)
        pos = np.concatenate([[0], np.cumsum(hs.native_lengths)])
        rows = torch.tensor([(int(pos[i]), int(hs.native_lengths[i]), int(hs.rec_start[i]), int(hs.lengths[i]))
                             for i in range(len(hs.native))], dtype=torch.int64, device="cuda:0")
        src, taps = torch.from_numpy(stream).to("cuda:0"), torch.from_numpy(pl["taps"]).to("cuda:0")
        dst, status = torch.zeros_like(corpus.pcm), torch.zeros(1, dtype=torch.int32, device="cuda:0")
        conv = event_ms(lambda: ops.resample_pcm(src, rows, taps, pl["M"], pl["centre"], dst, status), 20)
        assert int(status.item()) == 0 and torch.equal(dst, corpus.pcm), "the timed launch is not the corpus's conversion"
        moved = stream.nbytes + int(hs.lengths.sum()) * 8
        macs = int(hs.lengths.sum()) * 4 * pl["K"]
        res["convert"] = dict(conv, L=pl["L"], M=pl["M"], K=pl["K"], bytes_in=stream.nbytes, bytes_out=int(hs.lengths.sum()) * 8,
                              gb_per_s=round(moved / conv["median_ms"] / 1e6, 1), gmac_per_s=round(macs / conv["median_ms"] / 1e6, 1),
                              ms_per_recorded_s=round(conv["median_ms"] / seconds, 6))
        del src
        hold = torch.empty(stream.shape, dtype=torch.int16, device="cuda:0")
        host = torch.from_numpy(stream)
        res["h2d_pageable"] = dict(event_ms(lambda: hold.copy_(host), 5), bytes=stream.nbytes)
        pinned = host.pin_memory()
        res["h2d_pinned"] = dict(event_ms(lambda: hold.copy_(pinned, non_blocking=True), 5), bytes=stream.nbytes)
        for key in ("h2d_pageable", "h2d_pinned"):
            res[key]["gb_per_s"] = round(stream.nbytes / res[key]["median_ms"] / 1e6, 1)
        res["convert_over_h2d_pinned"] = round(conv["median_ms"] / res["h2d_pinned"]["median_ms"], 3)
        del hold, host, pinned, stream, dst
    print(json.dumps({k: res[k] for k in ("folder", "load", "convert", "h2d_pageable", "h2d_pinned") if k in res}), flush=True)
    fg = ForwardGraphs(model, fx, post, warm_calls=0)
    info = {}
    walls = timed(lambda: info.update(atest.infer_epoch_corpus(corpus, model, fx, post, out, forward=fg)), a.repeats)
    med = statistics.median(walls)
    res["windowed"] = {"wall_s": [round(w, 4) for w in walls], "median_s": round(med, 4),
                       "ms_per_recorded_s": round(1e3 * med / seconds, 4), **info}
    print(json.dumps(res), flush=True)


def params(folder, loss, n_classes, window_s, conf=0.5):
    from __graft_entry__ import _params
    prm = _params(nb_classes=n_classes)
    prm["args"].update({"loss": loss, "infer_pth": folder})
    prm["data_config"].update({"data_pth": folder, "sr": SR, "label_hop_len_s": 0.1, "chunk_window_s": window_s, "chunk_stride_s": 1})
    prm["train_config"].update({"conf_thresh": conf, "clss_thresh": conf, "unify_thresh": 15.0, "nms": "conn-merge"})
    return prm


def timed(run, repeats):
    run()                                                   # untimed: code objects, page-locked buffers, the first recordings
    walls = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    return walls


def read_csvs(folder, names):
    out = {}
    for n in names:
        frames = {}
        with open(os.path.join(folder, n + ".csv")) as fid:
            for line in fid:
                w = line.strip().split(",")
                frames.setdefault(int(w[0]), []).append((line, int(w[1]), [float(v) for v in w[3:6]]))
        out[n] = frames
    return out


def same_detections(a, b, max_deg=1.0):
    if len(a) != len(b):
        return False
    for (_, ca, va), (_, cb, vb) in zip(a, b):
        dot = sum(x * y for x, y in zip(va, vb)) / max(1e-12, math.sqrt(sum(x * x for x in va)) * math.sqrt(sum(y * y for y in vb)))
        if ca != cb or math.degrees(math.acos(max(-1.0, min(1.0, dot)))) > max_deg:
            return False
    return True


def agreement(whole, windowed, names, n_frames, seams):
    """-> shares of differing frames {exact, detections} x {seam, other}, and the frame counts."""
    cnt = {"seam": [0, 0, 0], "other": [0, 0, 0]}          # frames, exact differences, detection differences
    for n in names:
        for f in range(n_frames):
            a, b = whole[n].get(f, []), windowed[n].get(f, [])
            c = cnt["seam" if f in seams else "other"]
            c[0] += 1
            c[1] += [x[0] for x in a] != [x[0] for x in b]
            c[2] += not same_detections(a, b)
    return {k: {"frames": v[0], "exact_share": round(v[1] / max(v[0], 1), 4), "detections_share": round(v[2] / max(v[0], 1), 4)}
            for k, v in cnt.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "adyolo_infer_bench"))
    ap.add_argument("--recordings", type=int, default=14)
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--window", type=float, default=20.0)
    ap.add_argument("--margin", type=float, default=2.0)
    ap.add_argument("--loss", default="adyolo", choices=["adyolo", "seddoa", "accdoa", "adpit"])
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--conf", type=float, default=0.5, help="conf_thresh and clss_thresh (random weights: lower it until rows appear)")
    ap.add_argument("--rate", type=int, default=0, help="write the folder at this rate (Hz) and load it with resample=True: the "
                    "conversion launch against the upload of the same bytes, then the windowed pass (no whole pass, no agreement)")
    ap.add_argument("--keep", action="store_true", help="keep the folders on disk afterwards")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "infer_bench needs the GPU"
    import adyolo_amd  # noqa: F401
    from adyolo_amd import graph, test as atest
    from adyolo_amd.corpus import InferDeviceCorpus, load_infer_split, window_plan
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.wrapper import WrapperModel
    lengths = [LENGTHS_S[i % len(LENGTHS_S)] for i in range(a.recordings)]
    assert len(set(lengths)) >= 12 > graph.MAX_GRAPHS or a.recordings < 12, "the folder is meant to hold more lengths than graphs"
    shutil.rmtree(a.dir, ignore_errors=True)
    folder, clips_dir, out = os.path.join(a.dir, "folder"), os.path.join(a.dir, "clips"), os.path.join(a.dir, "out")
    res = {"batch": a.batch, "window_s": a.window, "margin_s": a.margin, "loss": a.loss, "conf_thresh": a.conf, "repeats": a.repeats,
           "max_graphs": graph.MAX_GRAPHS, "cpus": len(os.sched_getaffinity(0))}
    try:
        if a.rate:
            rate_run(a, res, folder, out, lengths)
            if a.json:
                os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
                with open(a.json, "w") as f:
                    json.dump(res, f, indent=1)
            return
        samples = write_folder(folder, lengths)
        seconds = samples / SR
        res["folder"] = {"recordings": len(lengths), "distinct_lengths": len(set(lengths)), "seconds": round(seconds, 1)}
        prm = params(folder, a.loss, a.classes, a.window, a.conf)
        torch.manual_seed(0)
        model = WrapperModel((1, 7, int(SR * a.window) // 600, 64), (), prm).to("cuda:0").eval()
        fx, post = FeatureExtractor(None, "cuda:0"), LabelPostProcessor(prm)

        # ------------------------------------------------------------------------------------------------------ timing
        ds = FoaDataset(prm, "infer", rank=0, world=1)
        fg_whole = ForwardGraphs(model, fx, post, warm_calls=0)

        def whole_pass():
            whole_pass.before = (fg_whole.captures, fg_whole.evictions)
            atest.test_epoch_audio(ds, model, fx, None, post, "cuda:0", out, batch_size=a.batch, forward=fg_whole, device_select=True)
        walls = timed(whole_pass, a.repeats)
        med = statistics.median(walls)
        res["whole"] = {"wall_s": [round(w, 4) for w in walls], "median_s": round(med, 4),
                        "ms_per_recording": round(1e3 * med / len(lengths), 3), "ms_per_recorded_s": round(1e3 * med / seconds, 4),
                        "graphs_recorded_per_pass": fg_whole.captures - whole_pass.before[0],
                        "graphs_evicted_per_pass": fg_whole.evictions - whole_pass.before[1]}
        print(json.dumps({"whole": res["whole"]}), flush=True)
        del fg_whole
        torch.cuda.empty_cache()

        t0 = time.perf_counter()
        hs = load_infer_split(prm, rank=0, world=1, verify="sample")
        t1 = time.perf_counter()
        corpus = InferDeviceCorpus(hs, prm, "cuda:0", window_s=a.window, margin_s=a.margin, batch_size=a.batch)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res["load"] = {"host_s": round(t1 - t0, 3), "upload_s": round(t2 - t1, 3), "device_bytes": corpus.nbytes(),
                       "ms_per_recorded_s": round(1e3 * (t2 - t0) / seconds, 4)}
        fg = ForwardGraphs(model, fx, post, warm_calls=0)
        info = {}

        def windowed_pass():
            windowed_pass.before = fg.captures
            info.update(atest.infer_epoch_corpus(corpus, model, fx, post, out, forward=fg))
        walls = timed(windowed_pass, a.repeats)
        med = statistics.median(walls)
        res["windowed"] = {"wall_s": [round(w, 4) for w in walls], "median_s": round(med, 4),
                           "ms_per_recording": round(1e3 * med / len(lengths), 3), "ms_per_recorded_s": round(1e3 * med / seconds, 4),
                           "graphs_recorded_per_pass": fg.captures - windowed_pass.before, "graphs_held": len(fg.entries), **info}
        res["whole_over_windowed"] = round(res["whole"]["median_s"] / med, 2)
        print(json.dumps({"load": res["load"], "windowed": res["windowed"]}), flush=True)
        del corpus, hs

        # --------------------------------------------------------------------------------------------------- agreement
        if a.clips > 0:
            write_folder(clips_dir, [60.0] * a.clips, seed=1)
            prm_c = params(clips_dir, a.loss, a.classes, a.window, a.conf)
            ds_c = FoaDataset(prm_c, "infer", rank=0, world=1)
            names = ds_c.get_filelist()
            whole_dir = os.path.join(a.dir, "whole_csv")
            atest.test_epoch_audio(ds_c, model, fx, None, post, "cuda:0", whole_dir, batch_size=1, device_select=True)
            whole = read_csvs(whole_dir, names)
            hs_c = load_infer_split(prm_c, rank=0, world=1)
            wf, hop_s = int(round(a.window * 10)), 0.1
            res["agreement"] = {"clips": a.clips, "frames_with_rows_whole": sum(len(v) for v in whole.values()),
                                "rows_whole": sum(len(r) for v in whole.values() for r in v.values()), "margins": {}}
            for margin in (0.0, 1.0, 2.0, 4.0):
                cor = InferDeviceCorpus(hs_c, prm_c, "cuda:0", window_s=a.window, margin_s=margin, batch_size=a.batch)
                win_dir = os.path.join(a.dir, "win_csv_%g" % margin)
                atest.infer_epoch_corpus(cor, model, fx, post, win_dir, forward=fg)
                plan = window_plan(600, wf, int(round(margin / hop_s)))
                seams = {f for w in plan[1:] for f in (w[2] - 1, w[2])}
                res["agreement"]["margins"]["%g" % margin] = dict(agreement(whole, read_csvs(win_dir, names), names, 600, seams),
                                                                  windows_per_clip=len(plan))
            print(json.dumps({"agreement": res["agreement"]}), flush=True)
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
