"""The device CSV formatter (``ops.csv_format``, ``device_csv=True``) against the host writer, on one MI355X in one process.

All figures are medians of --reps (at least 7) repetitions with the least and the largest next to them; every timed call runs
once beforehand.  Run the tool twice: the difference between the two runs' medians is the spread to read every ratio with.

  format   ``ops.csv_format`` alone, by device events around its launches, on synthetic rows for --clips x 60 s clips (600
           label frames each): no rows; about 1.5 rows per frame (a Poisson draw: a trained model's order of magnitude);
           --dense rows per frame (an untrained head's hundreds).  Beside it, on the same rows in the same process and on the
           host clock: ``device`` = csv_format + the two copies (offsets, then the bytes), and ``host`` = ``to_host_many`` +
           ``group_rows`` + ``write_seld_output_file`` (the files go to --dir).  Bytes and rows are reported.
  corpus   ``test_epoch_corpus`` on the 16 x 60 s split of tools/eval_corpus_bench.py (recorded forward graphs): no files, the
           host writer, ``device_csv=True``; at conf 0.5, where the untrained head selects nothing, and at --rows-conf, where it
           selects its hundreds of rows per frame.  ms per clip, host clock (a pass with files ends in file writes).
  infer    ``infer_epoch_corpus`` on the 14-recording folder of tools/infer_bench.py (20 to 180 s; 20 s windows, 2 s margin, 8
           windows per pass): the host writer and ``device_csv=True`` at the same two thresholds.  ms per recorded second.
  --root   the package of ANOTHER checkout (the parent commit, built) is measured instead: only the default paths -- corpus
           without files and with the host writer, infer with the host writer -- to be set against this tree's figures for
           ``device_csv=False`` from the same session.

  Everything is written to a fresh folder made under --dir, which is removed at the end; --dir itself is left alone.

  python tools/csv_bench.py [--dir /tmp/adyolo_csv_bench] [--clips 8] [--dense 300] [--reps 7] [--rows-conf 0.3]
                            [--skip format,corpus,infer] [--root PATH] [--json out.json]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
T_CLIP = 600


def spread(values, per=1.0):
    return {"median": round(statistics.median(values) / per, 4), "min": round(min(values) / per, 4),
            "max": round(max(values) / per, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=os.path.join("/tmp", "adyolo_csv_bench"))
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--dense", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows-conf", type=float, default=0.3)
    ap.add_argument("--skip", default="")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package is measured")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert a.reps >= 7, "medians of at least 7 repetitions"
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(1, HERE)
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "csv_bench needs the GPU"
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops, test as atest
    from adyolo_amd.postprocess import LabelPostProcessor, group_rows, write_seld_output_file
    assert os.path.abspath(adyolo_amd.__file__).startswith(root), (adyolo_amd.__file__, root)
    has_csv = hasattr(ops, "csv_format")
    skip = set(a.skip.split(",")) | (set() if has_csv else {"format"})
    res = {"root": root, "device_csv": has_csv, "reps": a.reps, "cpus": len(os.sched_getaffinity(0))}
    os.makedirs(a.dir, exist_ok=True)
    a.dir = tempfile.mkdtemp(prefix="run_", dir=a.dir)          # the tool's own folder: nothing else is ever deleted

    def events(run):
        run()
        out = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    def walls(run):
        run()
        out = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return out

    try:
        if "format" not in skip:
            from adyolo_amd.postprocess import csv_segments_clips
            rng = np.random.default_rng(0)
            frames = a.clips * T_CLIP
            names = ["clip%02d" % k for k in range(a.clips)]
            out_dir = os.path.join(a.dir, "format")
            os.makedirs(out_dir)
            table = torch.from_numpy(csv_segments_clips(a.clips, T_CLIP)).to("cuda:0")
            res["format"] = {}
            for key, counts in (("none", np.zeros(frames, dtype=np.int32)), ("poisson1.5", rng.poisson(1.5, frames).astype(np.int32)),
                                ("dense%d" % a.dense, np.full(frames, a.dense, dtype=np.int32))):
                n = int(counts.sum())
                rows = np.zeros((max(n, 1), 5), dtype=np.float32)
                rows[:, 1] = rng.integers(0, 12, len(rows))
                v = rng.standard_normal((len(rows), 3)).astype(np.float32)
                rows[:, 2:] = v / np.linalg.norm(v, axis=1, keepdims=True)
                d_rows, d_counts = torch.from_numpy(rows).to("cuda:0"), torch.from_numpy(counts).to("cuda:0")
                buf = ops.csv_buffers("cuda:0", frames, len(rows), a.clips, len(rows) * ops.CSV_LINE_MAX)
                status = torch.zeros(1, dtype=torch.int32, device="cuda:0")

                def launch():
                    return ops.csv_format(d_rows, d_counts, table, None, buf=buf, status=status)

                def device():
                    out, seg_bytes, _ = launch()
                    seg_h, status_h = ops.to_host_many(seg_bytes, status)
                    ops.csv_status_check(int(status_h[0]))
                    total = int(seg_h[-1])
                    if total:
                        ops.to_host_many(out[:total])
                    return total

                def host():
                    rows_h, counts_h = [t.numpy() for t in ops.to_host_many(d_rows[:n], d_counts)]
                    for name, clip_rows in zip(names, group_rows(rows_h, counts_h, a.clips)):
                        write_seld_output_file(os.path.join(out_dir, name + ".csv"), clip_rows)
                res["format"][key] = {"rows": n, "bytes": device(), "launches_ms": spread(events(launch)),
                                      "device_wall_ms": spread(walls(device)), "host_wall_ms": spread(walls(host))}
                print(json.dumps({key: res["format"][key]}), flush=True)

        if "corpus" not in skip:
            from adyolo_amd.corpus import EvalDeviceCorpus, load_eval_split
            from adyolo_amd.features import FeatureExtractor
            from adyolo_amd.graph import ForwardGraphs
            from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
            from eval_corpus_bench import REC_S, SR, params, write_split
            split = os.path.join(a.dir, "split")
            write_split(split, 16)
            prm = params(split, "adyolo", 12)
            torch.manual_seed(0)
            model = WrapperModel((1, 7, SR * REC_S // 600, 64), (), prm).to("cuda:0").eval()
            fx, crit = FeatureExtractor(None, "cuda:0"), WrapperCriterion(prm)
            corpus = EvalDeviceCorpus(load_eval_split(prm, "test", rank=0, world=1, verify="none"), prm, "cuda:0")
            res["corpus_ms_per_clip"] = {}
            for conf in (0.5, a.rows_conf):
                post = LabelPostProcessor(prm)
                post.set_conf_thresh(conf)
                fg = ForwardGraphs(model, fx, post, warm_calls=0)
                out = os.path.join(a.dir, "corpus_out")
                cases = {"no_files": dict(output_pth=None), "host_writer": dict(output_pth=out)}
                if has_csv:
                    cases["device_csv"] = dict(output_pth=out, device_csv=True)
                got = {}
                for key, kw in cases.items():
                    got[key] = spread(walls(lambda: atest.test_epoch_corpus(corpus, model, fx, crit, post, batch_size=8, forward=fg,
                                                                            **kw)), len(corpus))
                    if kw["output_pth"]:
                        got[key + "_bytes"] = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
                res["corpus_ms_per_clip"]["conf%g" % conf] = got
                print(json.dumps({"corpus conf%g" % conf: got}), flush=True)
            del corpus, model

        if "infer" not in skip:
            from adyolo_amd.corpus import InferDeviceCorpus, load_infer_split
            from adyolo_amd.features import FeatureExtractor
            from adyolo_amd.graph import ForwardGraphs
            from adyolo_amd.wrapper import WrapperModel
            import infer_bench
            folder = os.path.join(a.dir, "folder")
            lengths = [infer_bench.LENGTHS_S[i % len(infer_bench.LENGTHS_S)] for i in range(14)]
            seconds = infer_bench.write_folder(folder, lengths) / infer_bench.SR
            prm = infer_bench.params(folder, "adyolo", 12, 20.0)
            torch.manual_seed(0)
            model = WrapperModel((1, 7, int(infer_bench.SR * 20.0) // 600, 64), (), prm).to("cuda:0").eval()
            fx = FeatureExtractor(None, "cuda:0")
            corpus = InferDeviceCorpus(load_infer_split(prm, rank=0, world=1, verify="sample"), prm, "cuda:0", window_s=20.0,
                                       margin_s=2.0, batch_size=8)
            res["infer_ms_per_recorded_s"] = {"seconds": round(seconds, 1)}
            for conf in (0.5, a.rows_conf):
                post = LabelPostProcessor(prm)
                post.set_conf_thresh(conf)
                fg = ForwardGraphs(model, fx, post, warm_calls=0)
                out = os.path.join(a.dir, "infer_out")
                cases = {"host_writer": {}}
                if has_csv:
                    cases["device_csv"] = dict(device_csv=True)
                got = {}
                for key, kw in cases.items():
                    got[key] = spread(walls(lambda: atest.infer_epoch_corpus(corpus, model, fx, post, out, forward=fg, **kw)), seconds)
                    got[key + "_bytes"] = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
                res["infer_ms_per_recorded_s"]["conf%g" % conf] = got
                print(json.dumps({"infer conf%g" % conf: got}), flush=True)
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
