"""Rotation test-time augmentation of the corpus evaluation pass, timed on the synthetic split of tools/eval_corpus_bench.py
(--clips recordings of 60 s of int16 noise; an untrained model, so the figures are costs, not scores).

All times are medians of --reps repetitions between two device events, with the least and the largest next to them (the
run-to-run spread); every pass runs once beforehand (it records the forward graphs).

  plain        test_epoch_corpus(forward=ForwardGraphs, output_pth=None, device_scorer=...) with the argument off: ms per clip.
               With --root the package of ANOTHER checkout is measured instead (one that may not know the argument at all, e.g. the
               parent commit): only this figure is then reported, to be set against this tree's from the same session.
  views8 / 16  the same pass with tta = the first 8 / all 16 combinations: ms per clip, and the merged rows of the pass
  stages       on the first batch, per clip: one view's launch_view + forward + decode + select_device_rows; tta_collect of all 16
               views; tta_merge of the 16-view pool -- at the split's threshold and at --stage-conf, with the rows each pools

  python tools/tta_bench.py [--dir /tmp/adyolo_tta_bench] [--clips 16] [--batch 8] [--reps 7] [--loss adyolo] [--root PATH]
                            [--json out.json]

--windows: the same through windows, on the 14-recording split of tools/eval_windows_bench.py (20 to 180 s, --window s windows
with a --margin s margin, --batch windows per pass, one recorded graph), per recorded second:

  plain        test_epoch_windows(forward=ForwardGraphs, output_pth=None, device_scorer=...) and infer_epoch_corpus (which writes
               its files) with the argument off; with --root these two figures only, from that checkout's package
  gather       ops.corpus_gather_windows against ops.corpus_gather_windows_view (combination 5) on the first pass's table: ms,
               and TB/s over the bytes read (the valid int16 frames) plus the bytes written
  views8 / 16  test_epoch_windows with tta = the first 8 / all 16 combinations, its ratio to the plain pass, and the share of the
               selections, collects and merges in it (timed alone on every view's kept runs) -- at the split's threshold, where
               the untrained model selects nothing, and at each --rows-conf, where its rows fill the pool (a pool too small for
               them is reported as the error the pass raises); the pool is the largest the views allow, 1024 // V rows per frame

  python tools/tta_bench.py --windows [--window 20] [--margin 2] [--rows-conf 0.4,0.3] ...
"""
import argparse
import json
import os
import shutil
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def spread(values, per=1.0):
    return {"median": round(statistics.median(values) / per, 4), "min": round(min(values) / per, 4),
            "max": round(max(values) / per, 4)}


def windows(a, root, res, events):
    """--windows: see the module docstring.  ``adyolo_amd`` is imported (from ``root``) before this is called."""
    import inspect
    import torch
    from adyolo_amd import _lib, ops, test as atest
    from adyolo_amd.corpus import EvalWindowCorpus, InferDeviceCorpus, load_eval_split, load_infer_split
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    from eval_windows_bench import write_split
    from infer_bench import LENGTHS_S, SR, params
    has_tta = "tta" in inspect.signature(atest.test_epoch_windows).parameters
    res.update(tta=has_tta, window_s=a.window, margin_s=a.margin)
    lengths = [LENGTHS_S[i % len(LENGTHS_S)] for i in range(14)]
    seconds = write_split(a.dir, lengths, a.classes) / SR
    res["folder"] = {"recordings": len(lengths), "seconds": round(seconds, 1)}
    prm = params(a.dir, a.loss, a.classes, a.window, 0.5)
    wav_dir, out_dir = os.path.join(a.dir, "foa_dev", "dev-test"), os.path.join(a.dir, "out")
    torch.manual_seed(0)
    model = WrapperModel((1, 7, int(SR * a.window) // 600, 64), (), prm).to("cuda:0").eval()
    fx, crit, post = FeatureExtractor(None, "cuda:0"), WrapperCriterion(prm), LabelPostProcessor(prm)
    fg = ForwardGraphs(model, fx, post, warm_calls=0)
    corpus = EvalWindowCorpus(load_eval_split(prm, "test", rank=0, world=1, verify="none"), prm, "cuda:0", window_s=a.window,
                              margin_s=a.margin, batch_size=a.batch)
    infer = InferDeviceCorpus(load_infer_split(params(wav_dir, a.loss, a.classes, a.window, 0.5), verify="none"), prm, "cuda:0",
                              window_s=a.window, margin_s=a.margin, batch_size=a.batch)
    scorer = DeviceSELDScorer(prm, os.path.join(a.dir, "metadata_dev", "dev-test"), "cuda:0")
    res["passes"], res["n_windows"] = corpus.n_passes, corpus.n_windows

    def epoch(**kw):
        scorer.reset()
        return atest.test_epoch_windows(corpus, model, fx, crit, post, None, forward=fg, device_scorer=scorer, **kw)
    res["plain_ms_per_recorded_s"] = spread(events(epoch), seconds)
    res["infer_ms_per_recorded_s"] = spread(events(lambda: atest.infer_epoch_corpus(infer, model, fx, post, out_dir, forward=fg)),
                                            seconds)
    res["plain_loss"] = epoch()
    print(json.dumps(res), flush=True)
    if not has_tta:
        return
    # the gather: the first pass's table, every window read and written once
    table = corpus.pass_table(0)
    audio = torch.empty((a.batch, corpus.n_samples, 4), device="cuda:0")
    nbytes = int(corpus.table_host[:a.batch, 1].sum()) * 8 + audio.numel() * 4
    for key, run in (("plain", lambda: ops.corpus_gather_windows(corpus.pcm, table, audio, corpus.status)),
                     ("view", lambda: ops.corpus_gather_windows_view(corpus.pcm, table, 5, corpus.rot, audio, corpus.status))):
        ms = spread(events(lambda: [run() for _ in range(50)]), 50)        # 50 launches between the events: one is ~25 us
        res["gather_%s" % key] = {"ms": ms, "bytes": nbytes, "TB_per_s": round(nbytes / (ms["median"] * 1e-3) / 1e12, 3)}
    print(json.dumps({k: res[k] for k in res if k.startswith("gather")}), flush=True)
    conf0 = post.get_conf_thresh()
    for conf in [conf0] + [float(c) for c in a.rows_conf.split(",") if c]:
        post.set_conf_thresh(conf)
        here = res["conf_%g" % conf] = {"plain_ms_per_recorded_s": spread(events(epoch), seconds)}
        for v in (8, 16):
            tta = {"views": list(range(v)), "min_views": (v + 1) // 2, "unify_thresh": 15.0, "max_rows_per_frame": 1024 // v}
            try:
                got = spread(events(lambda: epoch(tta=tta)), seconds)
                here["views%d_ms_per_recorded_s" % v] = got
                here["views%d_over_plain" % v] = round(got["median"] / here["plain_ms_per_recorded_s"]["median"], 2)
                here["views%d_same_loss" % v] = epoch(tta=tta) == res["plain_loss"]
                # the selections, collects and merges alone, on every view's kept runs (what the sweep keeps)
                acc, runs, stitched = ops.loss_accumulator(corpus.device), [], None
                merge = atest._window_merge(tta, post, corpus)
                with torch.no_grad():
                    for p in range(corpus.n_passes):
                        stitched, run = atest._window_pass(corpus, p, model, fx, crit, post, fg, acc, stitched)
                        runs.append([run.clone()] + [atest._window_view(corpus, p, k, model, fx, post, fg, stitched).clone()
                                                     for k in merge.views[1:]])
                    alone = spread(events(lambda: [merge.merged(post, r, 1, trim=False) for r in runs]), seconds)
                    here["views%d_merged_rows" % v] = int(sum(int(merge.merged(post, r, 1, trim=False)[1].sum()) for r in runs))
                here["views%d_select_collect_merge_ms_per_recorded_s" % v] = alone
                here["views%d_merge_share" % v] = round(alone["median"] / got["median"], 3)
                del runs
            except _lib.AdyoloHipError as err:                                 # more rows in a frame than the pool holds
                here["views%d_error" % v] = str(err)
        print(json.dumps({"conf_%g" % conf: here}), flush=True)
    post.set_conf_thresh(conf0)
    res["plain_again_ms_per_recorded_s"] = spread(events(epoch), seconds)   # the spread of one binary within the session


def windows_main(a, root):
    import torch
    res = {"root": root, "windows": True, "batch": a.batch, "reps": a.reps, "loss": a.loss}

    def events(run):
        """ms between two device events around ``run``, --reps times after one untimed call."""
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
    shutil.rmtree(a.dir, ignore_errors=True)
    try:
        windows(a, root, res, events)
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=os.path.join("/tmp", "adyolo_tta_bench"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loss", default="adyolo", choices=["adyolo", "seddoa", "accdoa", "adpit"])
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--rows-per-frame", type=int, default=64)
    ap.add_argument("--stage-conf", type=float, default=0.3, help="the second threshold the stages are timed at")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package is measured")
    ap.add_argument("--windows", action="store_true", help="the windowed loops on the 14-recording split")
    ap.add_argument("--window", type=float, default=20.0)
    ap.add_argument("--margin", type=float, default=2.0)
    ap.add_argument("--rows-conf", default="0.4,0.3", help="--windows: the thresholds at which the untrained head's rows are pooled")
    ap.add_argument("--json")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(1, HERE)
    import torch
    assert torch.cuda.is_available(), "tta_bench needs the GPU"
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
    if a.windows:
        return windows_main(a, root)
    has_tta = hasattr(ops, "tta_merge")
    shutil.rmtree(a.dir, ignore_errors=True)
    write_split(a.dir, a.clips, n_classes=a.classes)
    res = {"root": root, "tta": has_tta, "clips": a.clips, "batch": a.batch, "reps": a.reps, "loss": a.loss}
    try:
        prm = params(a.dir, a.loss, a.classes)
        torch.manual_seed(0)
        model = WrapperModel((1, 7, SR * REC_S // 600, 64), (), prm).to("cuda:0").eval()
        fx, crit, post = FeatureExtractor(None, "cuda:0"), WrapperCriterion(prm), LabelPostProcessor(prm)
        fg = ForwardGraphs(model, fx, post, warm_calls=0)
        corpus = EvalDeviceCorpus(load_eval_split(prm, "test", rank=0, world=1, verify="none"), prm, "cuda:0")
        scorer = DeviceSELDScorer(prm, os.path.join(a.dir, "metadata_dev", "dev-test"), "cuda:0")
        n = len(corpus)

        def events(run):
            """ms between two device events around ``run``, --reps times after one untimed call."""
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

        def epoch(**kw):
            scorer.reset()
            return atest.test_epoch_corpus(corpus, model, fx, crit, post, None, batch_size=a.batch, forward=fg,
                                           device_scorer=scorer, **kw)
        res["plain_ms_per_clip"] = spread(events(epoch), n)
        res["plain_loss"] = epoch()
        print(json.dumps(res), flush=True)
        if has_tta:
            from adyolo_amd import _lib
            for v in (8, 16):
                tta = {"views": list(range(v)), "min_views": (v + 1) // 2, "unify_thresh": 15.0,
                       "max_rows_per_frame": a.rows_per_frame}
                try:
                    res["views%d_ms_per_clip" % v] = spread(events(lambda: epoch(tta=tta)), n)
                    res["views%d_same_loss" % v] = epoch(tta=tta) == res["plain_loss"]
                except _lib.AdyoloHipError as err:                         # e.g. more rows in a frame than the pool holds
                    res["views%d_error" % v] = str(err)
                print(json.dumps({k: res[k] for k in res if k.startswith("views%d" % v)}), flush=True)
            # the stages, on the first batch
            from adyolo_amd.augmentations import view_matrix
            from adyolo_amd.postprocess import tta_cos
            idx = corpus.batches(a.batch)[0]
            b = len(idx)
            views = list(range(16))
            words = [ops.tta_matrix_word(view_matrix(v)) for v in views]
            with torch.no_grad():
                def one_view(v=5):
                    dec = atest._corpus_view(corpus, idx, v, model, fx, post, fg)
                    return post.select_device_rows(dec, b, trim=False)
                res["view_forward_select_ms_per_clip"] = spread(events(one_view), b)
                # the untrained model selects nothing at the split's threshold: the stages are timed on that (empty) pool and
                # again at --stage-conf, where its rows fill the pool
                for conf in (post.get_conf_thresh(), a.stage_conf):
                    post.set_conf_thresh(conf)
                    selected = []
                    for v in views:
                        rows, counts = one_view(v)
                        selected.append((rows.clone(), counts.clone()))
                    frames = selected[0][1].numel()
                    buf = ops.tta_buffers("cuda:0", 16, frames, a.classes, a.rows_per_frame, 8)
                    status = torch.zeros(1, dtype=torch.int32, device="cuda:0")

                    def collect():
                        for k, (rows, counts) in enumerate(selected):
                            ops.tta_collect(rows, counts, k, words[k], a.classes, buf["pool"], buf["pool_counts"], status,
                                            buf["ws"])

                    def merge():
                        return ops.tta_merge(buf["pool"], buf["pool_counts"], a.classes, tta_cos(15.0), 8, status, buf["ws"],
                                             buf["rows"], buf["counts"], trim=False)
                    res["stages_conf_%g" % conf] = {
                        "collect16_ms_per_clip": spread(events(collect), b), "merge16_ms_per_clip": spread(events(merge), b),
                        "selected_rows_view0": int(selected[0][1].sum()), "pooled_rows": int(buf["pool_counts"].sum()),
                        "merged_rows": int(buf["counts"][frames]), "frames": frames, "status": int(status[0])}
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
