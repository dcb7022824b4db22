"""Tracks across frames (``ops.track_rows``, csrc/track.hip), timed and illustrated on one MI355X.

All times are medians of --reps repetitions between two device events, with the least and the largest next to them (the
run-to-run spread); the cases of one part are run alternately, repetition by repetition, in one session, after one untimed call
each.

  stages   ``ops.track_rows`` alone (given buffers, trim=False: no allocation, no synchronisation) on --batch clips of 60 s
           (T' = 600), --classes classes, --calls calls between the events: (a) no rows, (b) the rows of
           ``random_tracks`` (tests/test_track_cpu.py: persistent sources with dropouts, jitter and false alarms), (c) the rows
           an untrained model selects at --dense-conf.  Reported per call, with the rows in and out.  The kernels' own times
           (bin / link / emit) come from a run of this part under ``rocprofv3 --kernel-trace --stats`` (kernel names
           track_scan_kernel, track_bin_kernel, track_link_kernel, track_emit_kernel); the link stage's time per frame step is
           its time over T' (every wave walks the T' frames of its clip at the same time).
  epoch    ``test_epoch_corpus(forward=ForwardGraphs, output_pth=None, device_scorer=...)`` on the synthetic split of
           tools/eval_corpus_bench.py, ms per clip, with the argument off and with ``track`` at its defaults, alternately.  With
           --root the package of ANOTHER checkout is measured instead (e.g. the parent commit, which does not know the
           argument): only the plain figure is then reported, to be set against this tree's from the same session.
  value    ER / F / LE / LR / SELD of ``DeviceSELDScorer`` for the raw rows of ``random_tracks`` and for the rows tracked at the
           default keys, against the generator's clean cells.  An illustration on synthetic flicker: it says nothing about a
           trained model and sets no threshold.

  windows  (--windows, or --part windows; not part of ``all``) tracks carried through windows.  (a) ``ops.track_run`` over ONE
           recording of --recording-s seconds cut into the passes of the window plan (--window / --margin seconds, --batch windows
           a pass; ``corpus.window_plan`` and ``corpus.plan_track`` with the scorer's block of 10), all passes between the events
           (given buffers, trim=False, the emitted frames known: no allocation, no synchronisation), against ``ops.track_rows``
           on the same recording whole: ms per recording, the difference per pass, and the link stage's share per frame step
           as the whole figure over the frames.  (b) ``test_epoch_windows`` on the 14-recording split of
           tools/eval_windows_bench.py with ``ForwardGraphs`` and a ``DeviceSELDScorer``, ``tracking`` off and at its defaults,
           alternately, at the configured threshold (an untrained model selects nothing) and at --dense-conf; ms per recorded
           second.  With --root (a checkout that does not know ``tracking``) only the plain figure.

  python tools/track_bench.py [--part stages|epoch|value|windows|all] [--windows] [--dir /tmp/adyolo_track_bench] [--clips 16] [--batch 8]
                              [--reps 7] [--calls 20] [--classes 13] [--dense-conf 0.3] [--root PATH] [--json out.json]
"""
import argparse
import json
import math
import os
import shutil
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
T_CLIP = 600


def spread(values, per=1.0):
    return {"median": round(statistics.median(values) / per, 4), "min": round(min(values) / per, 4),
            "max": round(max(values) / per, 4)}


def windows_part(a, res, alternately, opts, dev):
    """The ``windows`` part (see the module's text)."""
    import numpy as np
    import torch
    import warnings
    from adyolo_amd import ops, test as atest
    from adyolo_amd.corpus import EvalWindowCorpus, load_eval_split, window_plan
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    from eval_windows_bench import LENGTHS_S, SR, params, write_split
    import inspect
    has_run = hasattr(ops, "track_run") and "tracking" in inspect.signature(atest.test_epoch_windows).parameters
    C = a.classes
    res["windows"] = {"track_run": has_run}
    if has_run:
        from adyolo_amd.corpus import plan_track
        from adyolo_amd.postprocess import track_hold
        from test_track_cpu import random_tracks
        frames, wf, mf = int(round(a.recording_s * 10)), int(round(a.window * 10)), int(round(a.margin * 10))
        kept = [w[3] for w in window_plan(frames, wf, mf)]
        bounds = [0] + np.cumsum([sum(kept[k:k + a.batch]) for k in range(0, len(kept), a.batch)]).tolist()
        hold = -(-track_hold(opts["max_gap"], opts["min_len"]) // 10) * 10
        plan = plan_track([0, frames], bounds, hold)
        case = random_tracks(7, 1, frames, C)
        offs = np.concatenate([[0], np.cumsum(case["counts"])])
        rows, counts = torch.from_numpy(case["rows"]).to(dev), torch.from_numpy(case["counts"]).to(dev)
        passes = [(rows[offs[lo]:offs[hi]].contiguous(), counts[lo:hi].contiguous(), torch.from_numpy(seg).to(dev),
                   ops.track_run_buffers(dev, hi - lo, C, hold), n)
                  for lo, hi, seg, n in zip(bounds, bounds[1:], plan["segments_host"], plan["pass_frames"])]
        carry, status = ops.track_carry(dev, C, hold), torch.zeros(1, dtype=torch.int32, device=dev)
        buf = ops.track_buffers(dev, frames, C)

        def carried():
            for _ in range(a.calls):
                for r, c, seg, b, n in passes:
                    ops.track_run(r, c, seg, C, opts, hold, carry, buf=b, status=status, trim=False, emitted=n)

        def whole():
            for _ in range(a.calls):
                ops.track_rows(rows, counts, 1, C, opts, buf=buf, status=status, trim=False)
        t = alternately({"whole": whole, "carried": carried}, a.calls)
        out_whole = int(buf["counts"][frames])
        out_run = sum(int(b["counts"][b["counts"].numel() - 2]) for _, _, _, b, _ in passes)
        res["windows"]["recording"] = {
            "frames": frames, "passes": len(passes), "pass_frames": [int(c.numel()) for _, c, _, _, _ in passes], "hold": hold,
            "rows_in": int(case["counts"].sum()), "rows_out": out_whole, "same_rows_out": out_run == out_whole,
            "ms_per_recording": t, "carry_ms_per_pass": round((t["carried"]["median"] - t["whole"]["median"]) / len(passes), 4),
            "whole_us_per_frame_step": round(1e3 * t["whole"]["median"] / frames, 4),
            "carried_us_per_frame_step": round(1e3 * t["carried"]["median"] / frames, 4)}
        print(json.dumps(res["windows"]["recording"]), flush=True)
    lengths = [LENGTHS_S[i % len(LENGTHS_S)] for i in range(14)]
    seconds = write_split(a.dir, lengths, C) / SR
    prm = params(a.dir, "adyolo", C, a.window, 0.5)
    ref = os.path.join(a.dir, "metadata_dev", "dev-test")
    torch.manual_seed(0)
    model = WrapperModel((1, 7, int(SR * a.window) // 600, 64), (), prm).to(dev).eval()
    fx, post, crit = FeatureExtractor(None, dev), LabelPostProcessor(prm), WrapperCriterion(prm)
    corpus = EvalWindowCorpus(load_eval_split(prm, "test", rank=0, world=1, verify="sample"), prm, dev, window_s=a.window,
                              margin_s=a.margin, batch_size=a.batch)
    fg, scorer = ForwardGraphs(model, fx, post, warm_calls=0), DeviceSELDScorer(prm, ref, dev)

    def epoch(**kw):
        def run():
            scorer.reset()
            return atest.test_epoch_windows(corpus, model, fx, crit, post, None, forward=fg, device_scorer=scorer, **kw)
        return run
    runs = {"plain": epoch()}
    if has_run:
        warnings.simplefilter("ignore")                                        # (the caps of the definition only warn)
        runs["tracked"] = epoch(tracking=opts)
    res["windows"]["split"] = {"recordings": len(lengths), "seconds": round(seconds, 1), "passes": corpus.n_passes}
    res["windows"]["epoch_ms_per_recorded_s"] = alternately(runs, seconds)
    post.set_conf_thresh(a.dense_conf)
    res["windows"]["epoch_dense_ms_per_recorded_s"] = alternately(runs, seconds)
    if has_run:
        res["windows"]["same_loss"] = runs["plain"]() == runs["tracked"]()
    print(json.dumps({k: v for k, v in res["windows"].items() if k != "recording"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["stages", "epoch", "value", "windows", "all"])
    ap.add_argument("--windows", action="store_true", help="the same as --part windows")
    ap.add_argument("--recording-s", type=float, default=180.0)
    ap.add_argument("--window", type=float, default=20.0)
    ap.add_argument("--margin", type=float, default=2.0)
    ap.add_argument("--dir", default=os.path.join("/tmp", "adyolo_track_bench"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--classes", type=int, default=13)
    ap.add_argument("--dense-conf", type=float, default=0.3)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package is measured")
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.windows:
        a.part = "windows"
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(1, HERE)
    sys.path.insert(2, os.path.join(os.path.dirname(HERE), "tests"))
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "track_bench needs the GPU"
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops, test as atest
    from adyolo_amd.corpus import EvalDeviceCorpus, load_eval_split
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    from eval_corpus_bench import REC_S, SR, params, write_split
    assert os.path.abspath(adyolo_amd.__file__).startswith(root), (adyolo_amd.__file__, root)
    has_track = hasattr(ops, "track_rows")
    dev = "cuda:0"
    C = a.classes
    opts = {"gate_deg": 20.0, "max_gap": 2, "min_len": 3, "smooth": 0.5}          # the defaults of augmentations.track_options
    res = {"root": root, "track": has_track, "clips": a.clips, "batch": a.batch, "reps": a.reps, "classes": C}

    def alternately(runs, per=1.0):
        """{name: run} -> {name: spread of ms}: one untimed call each, then --reps rounds over all of them in turn."""
        for run in runs.values():
            run()
        out = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, run in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                out[k].append(e0.elapsed_time(e1))
        return {k: spread(v, per) for k, v in out.items()}

    shutil.rmtree(a.dir, ignore_errors=True)
    try:
        model = corpus = None
        if a.part in ("stages", "epoch", "all"):
            write_split(a.dir, a.clips, n_classes=C)
            prm = params(a.dir, "adyolo", C)
            torch.manual_seed(0)
            model = WrapperModel((1, 7, SR * REC_S // 600, 64), (), prm).to(dev).eval()
            fx, crit, post = FeatureExtractor(None, dev), WrapperCriterion(prm), LabelPostProcessor(prm)
            fg = ForwardGraphs(model, fx, post, warm_calls=0)
            corpus = EvalDeviceCorpus(load_eval_split(prm, "test", rank=0, world=1, verify="none"), prm, dev)
        if has_track and a.part in ("stages", "value", "all"):
            from test_track_cpu import random_tracks
            case = random_tracks(7, a.batch, T_CLIP, C)
        if has_track and a.part in ("stages", "all"):
            frames = a.batch * T_CLIP
            inputs = {"a_no_rows": (torch.zeros(1, 5, device=dev), torch.zeros(frames, dtype=torch.int32, device=dev)),
                      "b_random_tracks": (torch.from_numpy(case["rows"]).to(dev), torch.from_numpy(case["counts"]).to(dev))}
            with torch.no_grad():
                post.set_conf_thresh(a.dense_conf)
                idx = corpus.batches(a.batch)[0]
                dec = atest._corpus_batch(corpus, idx, model, fx, crit, post, fg, ops.loss_accumulator(dev))
                rows, counts = post.select_device_rows(dec, len(idx), trim=False)
                inputs["c_untrained_model"] = (rows.clone(), counts.clone())
                post.set_conf_thresh(prm["train_config"]["conf_thresh"])
            assert inputs["c_untrained_model"][1].numel() == frames
            buf = ops.track_buffers(dev, frames, C)
            status = torch.zeros(1, dtype=torch.int32, device=dev)

            def call(rows, counts):
                def run():
                    for _ in range(a.calls):
                        ops.track_rows(rows, counts, a.batch, C, opts, buf=buf, status=status, trim=False)
                return run
            times = alternately({k: call(*v) for k, v in inputs.items()}, a.calls)
            res["stages"] = {}
            for k, (rows, counts) in inputs.items():
                status.zero_()
                ops.track_rows(rows, counts, a.batch, C, opts, buf=buf, status=status, trim=False)
                res["stages"][k] = {"ms_per_call": times[k], "rows_in": int(counts.sum()), "rows_out": int(buf["counts"][frames]),
                                    "frames": frames, "status": int(status[0])}
            print(json.dumps(res["stages"]), flush=True)
        if a.part in ("epoch", "all"):
            scorer = DeviceSELDScorer(prm, os.path.join(a.dir, "metadata_dev", "dev-test"), dev)

            def epoch(**kw):
                def run():
                    scorer.reset()
                    return atest.test_epoch_corpus(corpus, model, fx, crit, post, None, batch_size=a.batch, forward=fg,
                                                   device_scorer=scorer, **kw)
                return run
            runs = {"plain": epoch()}
            if has_track:
                import warnings
                warnings.simplefilter("ignore")                                # (the caps of the definition only warn)
                runs["tracked"] = epoch(track=opts)
            res["epoch_ms_per_clip"] = alternately(runs, len(corpus))
            if has_track:                                                      # ... and where the untrained model selects rows
                post.set_conf_thresh(a.dense_conf)
                res["epoch_dense_ms_per_clip"] = alternately(runs, len(corpus))
                post.set_conf_thresh(prm["train_config"]["conf_thresh"])
                res["same_loss"] = runs["plain"]() == runs["tracked"]()
            print(json.dumps({k: res[k] for k in res if k.startswith("epoch")}), flush=True)
        if has_track and a.part in ("value", "all"):
            ref = os.path.join(a.dir, "value_ref")
            os.makedirs(ref, exist_ok=True)
            names = ["fold4_room0_clip%03d" % k for k in range(a.batch)]
            lines = {n: [] for n in names}
            for f, c, s, v in case["clean"]:
                az, el = math.degrees(math.atan2(v[1], v[0])), math.degrees(math.atan2(v[2], math.hypot(v[0], v[1])))
                lines[names[f // T_CLIP]].append("%d,%d,%d,%r,%r\n" % (f % T_CLIP, c, s, az, el))
            for n in names:
                with open(os.path.join(ref, n + ".csv"), "w") as fid:
                    fid.writelines(lines[n] or ["%d,0,0,0.0,0.0\n" % (T_CLIP - 1)])
            vprm = {"data_config": {"nb_classes": C, "sr": SR, "label_hop_len_s": 0.1}}
            rows, counts = torch.from_numpy(case["rows"]).to(dev), torch.from_numpy(case["counts"]).to(dev)
            finite = torch.isfinite(rows).all(dim=1)                           # (the scorer refuses the planted NaN row)
            keep = torch.from_numpy(np.repeat(np.arange(len(case["counts"])), case["counts"])).to(dev)[finite]
            raw_rows, raw_counts = rows[finite].contiguous(), torch.bincount(keep, minlength=counts.numel()).int()
            out_rows, out_counts, _ = ops.track_rows(rows, counts, a.batch, C, opts)
            res["value"] = {"rows_raw": int(raw_rows.shape[0]), "rows_tracked": int(out_rows.shape[0]),
                            "clean_cells": len(case["clean"])}
            for key, (r, c) in (("raw", (raw_rows, raw_counts)), ("tracked", (out_rows, out_counts.contiguous()))):
                sc = DeviceSELDScorer(vprm, ref, dev)
                sc.add_rows(r, c, names)
                res["value"][key] = dict(zip(("ER", "F", "LE", "LR", "SELD"), (round(float(v), 4) for v in sc.scores()[:5])))
            print(json.dumps(res["value"]), flush=True)
        if a.part == "windows":
            windows_part(a, res, alternately, opts, dev)
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
