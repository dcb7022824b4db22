"""Training from the HBM-resident corpus against the host loader, on a synthetic chunked split written to local disk.

A split in the reference's chunked layout (``foa_dev/dev-train-chunked_20s_1s`` + ``metadata_dev/...``: 60 s recordings of int16
noise cut into 41 overlapping 20 s chunks, chunk CSVs with ~1 event per label frame, 12 classes) is written to --dir.  Then, per
batch size (16 and 64 x 20 s, hipGraph-replayed steps):

  load          load_chunked_split (verify="sample") + DeviceCorpus upload: seconds and bytes held on the device
  batch         gather + label kernels of one batch (DeviceCorpus.launch), device time per batch (events around --iters batches)
  gather        the gather alone on uploaded item tables, device time per launch in us (--iters launches replayed from one
                hipGraph): ``adyolo_corpus_gather`` always, and with --swap its MIC form (``mic_src``) on the same tables
  labels        (class-wise losses) the label kernel alone on an uploaded item table, device time per batch
  replay        the recorded train step alone on fixed inputs (the rate a loader has to keep up with)
  corpus        train_one_epoch_corpus
  host          train_one_epoch_audio over DataLoader(FoaDataset, num_workers=--workers, audio_collate_fn)
For both epochs: the wall time per step over the whole epoch (synchronised at its end; DataLoader start-up included), the
steady interval between step launches from the third step on (both paths keep at most two batches in flight, so this is the
rate the GPU is fed at), and the host CPU seconds per step (resource.getrusage of this process -- the launching thread's waits
on the GPU included -- and of its reaped children, i.e. the DataLoader workers).  Each path runs one warm epoch first (eager
step, capture; page cache).

--loss seddoa | accdoa | adpit trains that class-wise model from a ClasswiseDeviceCorpus instead; --mic writes the split as
``mic_dev`` and trains on the MIC feature set (MicFeatureExtractor: BASELINE config 5 with --loss adpit); --classes sets the event
classes of the split and the model (12 by default: the ACCDOA / ADPIT heads' GEMMs need 3C and 9C in multiples of 4);
--swap (with --mic only) turns ``aug_config.channel_swap_augment`` on instead of ``rotation_augment``: the MIC channel swap;
--labels-only stops after load, batch, gather and labels (no model: any class count, e.g. the 13 of DCASE 2023); --corpus-only
skips the host-loader epochs.  --mix [--prob P] runs every batch size twice, key off ("b16") and with
``aug_config.time_mix_augment`` at probability P ("b16_mix": doubled AD-YOLO row capacity), and adds to the second the time-domain
mixing calls on the same batch: ``adyolo_corpus_gather`` with ``mates`` -- the drawn ones, a mate for every item (prob 1.0) and
none (prob 0.0) -- and the label call with ``mates`` next to the plain one.  --yaw runs every batch size (and with --mix every
mixing run) a second time with ``aug_config.yaw_rotation_augment`` on ("b16_yaw", "b16_yaw_mix"; the split's labels are then
whole degrees, which the class-wise corpus needs) and measures, on the same item tables, the gather with ``yaw_tab`` against the
one without (alone, and with ``mates``) and the label calls with the yaw against the un-yawed ones.

  python tools/corpus_bench.py [--dir /tmp/adyolo_corpus] [--batches 16,64] [--steps 32,8] [--workers 16] [--json out.json]
                               [--loss adyolo|seddoa|accdoa|adpit] [--mic] [--swap] [--classes C] [--labels-only]
                               [--corpus-only] [--mix [--prob P]] [--yaw]
"""
import argparse
import csv
import json
import os
import random
import resource
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SR, WINDOW_S, STRIDE_S, REC_S = 24000, 20, 1, 60


def write_split(root, n_recordings, seed=0, n_classes=12, audio_dir="foa_dev", whole=False):
    """n_recordings x 60 s, chunked as the reference's preprocess.chunk_instance cuts them (60 s: no padding).  whole: the
    angles in whole degrees instead of tenths."""
    nd = 0 if whole else 1
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    sub = "dev-train-chunked_%ds_%ds" % (WINDOW_S, STRIDE_S)
    wdir, cdir = os.path.join(root, audio_dir, sub), os.path.join(root, "metadata_dev", sub)
    os.makedirs(wdir, exist_ok=True)
    os.makedirs(cdir, exist_ok=True)
    win, st, wf, sf = SR * WINDOW_S, SR * STRIDE_S, WINDOW_S * 10, STRIDE_S * 10
    nbytes = 0
    for r in range(n_recordings):
        audio = np.clip(rs.normal(0, 3000, size=(SR * REC_S, 4)), -32768, 32767).astype(np.int16)
        label = {}
        for f in range(REC_S * 10):
            k = rs.choice(3, p=[0.35, 0.45, 0.2])
            if k:
                label[f] = [[int(rs.randint(n_classes)), s, round(float(rs.uniform(-180, 180)), nd), round(float(rs.uniform(-60, 60)), nd)]
                            for s in range(k)]
        for i in range((len(audio) - win) // st + 1):
            name = "fold1_room%d_mix%03d_chunk%03d" % (r % 10, r, i + 1)
            wavfile.write(os.path.join(wdir, name + ".wav"), SR, audio[i * st:i * st + win])
            nbytes += win * 8
            with open(os.path.join(cdir, name + ".csv"), "w", newline="") as fid:
                w = csv.writer(fid)
                for f in range(wf):
                    for ev in label.get(i * sf + f, ()):
                        w.writerow([f] + ev)
    return nbytes


def params(root, batch, steps, loss="adyolo", mic=False, n_classes=12, swap=False, mix=None, yaw=False):
    from __graft_entry__ import _params
    prm = _params(nb_classes=n_classes)
    prm["args"]["loss"] = loss
    prm["data_config"].update({"data_pth": root, "chunk_window_s": WINDOW_S, "chunk_stride_s": STRIDE_S, "sr": SR,
                               "label_hop_len_s": 0.1})
    if mic:
        prm["data_config"]["audio_format"] = "mic"
    prm["train_config"].update({"batch_size": batch, "nb_iters": steps})
    prm["aug_config"] = {"rotation_augment": True, "spec_augment": True, "spec_augment_thresh": 0.5,
                         "spec_augment_time_mask_param": 40, "spec_augment_freq_mask_param": 40}
    if swap:
        prm["aug_config"].update({"rotation_augment": False, "channel_swap_augment": True})
    if mix is not None:
        prm["aug_config"].update({"time_mix_augment": True, "time_mix_prob": mix})
    if yaw:
        prm["aug_config"]["yaw_rotation_augment"] = True
    return prm


def trainer(prm):
    from adyolo_amd.features import FeatureExtractor, MicFeatureExtractor
    from adyolo_amd.train import TrainStep
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    torch.manual_seed(0)
    mic = prm["data_config"].get("audio_format") == "mic"
    model = WrapperModel((1, 10 if mic else 7, SR * WINDOW_S // 600, 64), (), prm).to("cuda:0")
    fx = MicFeatureExtractor(None, "cuda:0") if mic else FeatureExtractor(None, "cuda:0")
    tr = TrainStep(model, WrapperCriterion(prm), fx, prm, graph=True)
    tr.stamps = []
    inner = tr.step

    def step(audio, target, spec=None):
        loss = inner(audio, target, spec)
        tr.stamps.append(time.perf_counter())
        return loss
    tr.step = step
    return tr


def cpu_seconds():
    s, c = resource.getrusage(resource.RUSAGE_SELF), resource.getrusage(resource.RUSAGE_CHILDREN)
    return s.ru_utime + s.ru_stime + c.ru_utime + c.ru_stime


def timed_epoch(run, tr):
    """run() -> one epoch.  -> steps, wall s, steady steps/s, CPU s per step."""
    torch.cuda.synchronize()
    tr.stamps = []
    c0, t0 = cpu_seconds(), time.perf_counter()
    run()
    torch.cuda.synchronize()
    t1, c1 = time.perf_counter(), cpu_seconds()
    n = len(tr.stamps)
    steady = (tr.stamps[-1] - tr.stamps[2]) / (n - 3) if n > 3 else float("nan")
    return {"steps": n, "wall_s": round(t1 - t0, 4), "wall_ms_per_step": round(1e3 * (t1 - t0) / max(n, 1), 3),
            "steady_ms_per_step": round(1e3 * steady, 3), "steady_steps_per_s": round(1.0 / steady, 2),
            "cpu_s_per_step": round((c1 - c0) / max(n, 1), 4)}


def graph_us(launch, iters):
    """launch(i) recorded ``iters`` times in one hipGraph and replayed -> device time per launch in us (the device time rather
    than the rate Python issues launches at)."""
    for i in range(4):
        launch(i)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(iters):
            launch(i)
    graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(5):
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return round(1e3 * best / iters, 2)


def bench_batch(root, batch, steps, workers, iters, loss="adyolo", mic=False, n_classes=12, labels_only=False, swap=False,
                corpus_only=False, mix=None, yaw=False):
    from adyolo_amd import ops
    from adyolo_amd.corpus import ClasswiseDeviceCorpus, DeviceCorpus, load_chunked_split
    from adyolo_amd.datasets import FoaDataset, audio_collate_fn
    from adyolo_amd.train import train_one_epoch_audio, train_one_epoch_corpus
    prm = params(root, batch, steps, loss, mic, n_classes, swap, mix, yaw)
    out = {"batch": batch, "steps_per_epoch": steps}
    if yaw:
        out["yaw"] = True
    if mix is not None:
        out["mix_prob"] = mix
    if loss != "adyolo" or mic:
        out.update(loss=loss, mic=mic, classes=n_classes)
    if swap:
        out["swap"] = True
    t0 = time.perf_counter()
    hc = load_chunked_split(prm, verify="sample")
    t1 = time.perf_counter()
    random.seed(0)
    corpus = DeviceCorpus(hc, prm, "cuda:0") if loss == "adyolo" else ClasswiseDeviceCorpus(hc, prm, "cuda:0")
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out["load"] = {"host_s": round(t1 - t0, 3), "upload_s": round(t2 - t1, 3), "device_bytes": corpus.nbytes(),
                   "files": len(hc.total_filelist), "recordings": len(hc.rec_names)}
    if loss == "adyolo":
        out["load"]["cap_rows"] = corpus.cap
    else:
        out["load"]["target_shape"] = list(corpus.target_shape(batch))
    # gather + labels of one batch
    drawn = [corpus.draw(range(i * batch % len(corpus), i * batch % len(corpus) + batch)) for i in range(4)]
    for d in drawn:
        corpus.launch(d)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        corpus.launch(drawn[i % 4])
    e1.record()
    torch.cuda.synchronize()
    out["batch_ms"] = round(e0.elapsed_time(e1) / iters, 4)
    # the gather alone, on item tables already on the device (with --swap their combinations are the eight symmetries, which
    # both kernels take: the same bytes read and written)
    dev_items = [torch.from_numpy(d[0]).to("cuda:0") for d in drawn]
    audio = torch.empty((batch, corpus.n_samples, 4), dtype=torch.float32, device="cuda:0")
    out["gather_us"] = graph_us(lambda i: ops.corpus_gather(corpus.pcm, dev_items[i % 4], corpus.rot, audio, corpus.status), iters)
    if swap:
        out["gather_mic_us"] = graph_us(lambda i: ops.corpus_gather(corpus.pcm, dev_items[i % 4], None, audio, corpus.status,
                                                                    mic_src=corpus.mic_src), iters)
    if mix is not None:
        # the mixing gather on the same item tables: the drawn mates (prob P), a mate for every item (the next item of the batch,
        # gain 1.0: prob 1.0) and none (prob 0.0)
        one = int(np.float32(1.0).view(np.uint32))
        every, none = [], []
        for d in drawn:
            m = np.roll(d[0], 1, axis=0).copy()
            m[:, 6] = one
            every.append(torch.from_numpy(m).to("cuda:0"))
            m = np.zeros_like(d[0])
            m[:, 0] = m[:, 4] = -1
            none.append(torch.from_numpy(m).to("cuda:0"))
        dev_mates = [torch.from_numpy(d[2]).to("cuda:0") for d in drawn]
        out["mixed_items"] = round(float(np.mean([(d[2][:, 0] != -1).mean() for d in drawn])), 3)
        for key, tabs in (("gather_mix_us", dev_mates), ("gather_mix_p1_us", every), ("gather_mix_p0_us", none)):
            out[key] = graph_us(lambda i: ops.corpus_gather(corpus.pcm, dev_items[i % 4], corpus.rot, audio, corpus.status,
                                                            mates=tabs[i % 4], mic_src=corpus.mic_src), iters)
        gb = batch * corpus.n_samples * (8 + 16) / 1e9                   # int16 frames read + float32 frames written
        out["gather_tb_s"] = round(gb / out["gather_us"] * 1e3, 2)
        out["gather_mix_p1_tb_s"] = round((gb + batch * corpus.n_samples * 8 / 1e9) / out["gather_mix_p1_us"] * 1e3, 2)
        if loss == "adyolo":
            target = torch.empty((corpus.cap, 7), dtype=torch.float32, device="cuda:0")
            rows = torch.empty(1, dtype=torch.int32, device="cuda:0")
            ws = torch.empty(ops.corpus_labels_workspace_words(batch, corpus.max_events, mix=True), dtype=torch.int32,
                             device="cuda:0")
            out["labels_us"] = graph_us(lambda i: ops.corpus_yolo_labels(
                corpus.events, dev_items[i % 4], corpus.max_events, corpus.n_label_frames, corpus.bounds, corpus.grid, corpus.rot,
                ws, target, rows, corpus.status), iters)
            for key, tabs in (("labels_mix_us", dev_mates), ("labels_mix_p1_us", every)):
                out[key] = graph_us(lambda i: ops.corpus_yolo_labels(
                    corpus.events, dev_items[i % 4], corpus.max_events, corpus.n_label_frames, corpus.bounds, corpus.grid,
                    corpus.rot, ws, target, rows, corpus.status, mates=tabs[i % 4]), iters)
            del target, rows, ws
        else:
            target = torch.empty(corpus.target_shape(batch), dtype=torch.float32, device="cuda:0")
            out["labels_us"] = graph_us(lambda i: ops.corpus_classwise_labels(
                corpus.events, dev_items[i % 4], corpus.xyz, corpus.max_events, corpus.n_label_frames, corpus.nb_classes, loss,
                target, corpus.status), iters)
            for key, tabs in (("labels_mix_us", dev_mates), ("labels_mix_p1_us", every)):
                out[key] = graph_us(lambda i: ops.corpus_classwise_labels(
                    corpus.events, dev_items[i % 4], corpus.xyz, corpus.max_events, corpus.n_label_frames, corpus.nb_classes,
                    loss, target, corpus.status, mates=tabs[i % 4]), iters)
            del target
        corpus.check()
    if yaw:
        # the yaw calls on the same tables (word 7 of every row holds its drawn yaw, which the un-yawed calls do not read)
        out["gather_yaw_us"] = graph_us(lambda i: ops.corpus_gather(corpus.pcm, dev_items[i % 4], corpus.rot, audio, corpus.status,
                                                                    yaw_tab=corpus.yaw_tab), iters)
        if mix is not None:
            for key, tabs in (("gather_yaw_mix_us", dev_mates), ("gather_yaw_mix_p1_us", every)):
                out[key] = graph_us(lambda i: ops.corpus_gather(corpus.pcm, dev_items[i % 4], corpus.rot, audio, corpus.status,
                                                                mates=tabs[i % 4], yaw_tab=corpus.yaw_tab), iters)
        target = torch.empty(corpus.target_shape(batch), dtype=torch.float32, device="cuda:0")
        forms = [("labels_us", None, False), ("labels_yaw_us", None, True)]          # key, mates, yaw
        if mix is not None:
            forms += [("labels_mix_us", dev_mates, False), ("labels_yaw_mix_us", dev_mates, True)]
        if loss == "adyolo":
            rows = torch.empty(1, dtype=torch.int32, device="cuda:0")
            ws = torch.empty(ops.corpus_labels_workspace_words(batch, corpus.max_events, mix=True), dtype=torch.int32,
                             device="cuda:0")
            for key, tabs, yawed in forms:
                out[key] = graph_us(lambda i: ops.corpus_yolo_labels(
                    corpus.events, dev_items[i % 4], corpus.max_events, corpus.n_label_frames, corpus.bounds, corpus.grid,
                    corpus.rot, ws, target, rows, corpus.status, mates=None if tabs is None else tabs[i % 4], yaw=yawed), iters)
        else:
            for key, tabs, yawed in forms:
                out[key] = graph_us(lambda i: ops.corpus_classwise_labels(
                    corpus.events, dev_items[i % 4], corpus.xyz, corpus.max_events, corpus.n_label_frames, corpus.nb_classes,
                    loss, target, corpus.status, mates=None if tabs is None else tabs[i % 4], rot=corpus.rot if yawed else None,
                    yaw_xyz=corpus.yaw_xyz if yawed else None), iters)
        del target
        corpus.check()
    del audio
    if loss != "adyolo":
        # the label kernel alone, on item tables already on the device: --iters launches recorded in one hipGraph and
        # replayed, so that the device time is measured rather than the rate Python issues launches at
        target = torch.empty(corpus.target_shape(batch), dtype=torch.float32, device="cuda:0")

        def labels(i):
            ops.corpus_classwise_labels(corpus.events, dev_items[i % 4], corpus.xyz, corpus.max_events, corpus.n_label_frames,
                                        corpus.nb_classes, loss, target, corpus.status)
        for i in range(4):
            labels(i)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for i in range(iters):
                labels(i)
        graph.replay()
        torch.cuda.synchronize()
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        out["labels_ms"] = round(e0.elapsed_time(e1) / iters, 4)
        out["target_mb"] = round(target.numel() * 4 / 2 ** 20, 2)
        del graph, target
        corpus.check()
    if labels_only:
        return out

    tc = trainer(prm)
    for ep in range(2):
        if ep:
            corpus.sample_filelist_for_train_iter()
        r = timed_epoch(lambda: train_one_epoch_corpus(prm, corpus, tc), tc)
    out["corpus"] = r
    out["corpus"]["captures"] = tc.graphs.captures
    # the replayed step alone, on fixed inputs
    audio, target, spec = corpus.batch(range(batch))
    for _ in range(3):
        tc.step(audio, target, spec)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        tc.step(audio, target, spec)
    e1.record()
    torch.cuda.synchronize()
    out["replay_ms"] = round(e0.elapsed_time(e1) / iters, 3)
    del tc, corpus
    torch.cuda.empty_cache()
    if corpus_only:
        return out

    th = trainer(prm)
    random.seed(0)
    ds = FoaDataset(prm, "train")
    for ep in range(2):
        if ep:
            ds.sample_filelist_for_train_iter()
        loader = torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=False, collate_fn=audio_collate_fn,
                                             num_workers=workers, pin_memory=False)
        r = timed_epoch(lambda: train_one_epoch_audio(prm, loader, th), th)
        del loader
    out["host"] = r
    out["host"]["workers"] = workers
    out["host"]["captures"] = th.graphs.captures
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=os.path.join("/tmp", "adyolo_corpus_bench"))
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--steps", default="32,8", help="steps per epoch, one per batch size")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--keep", action="store_true", help="keep the split on disk afterwards")
    ap.add_argument("--json")
    ap.add_argument("--loss", default="adyolo", choices=["adyolo", "seddoa", "accdoa", "adpit"])
    ap.add_argument("--mic", action="store_true", help="a mic_dev split and the MIC feature set")
    ap.add_argument("--classes", type=int, default=12, help="event classes of the split and the model")
    ap.add_argument("--labels-only", action="store_true", help="load, batch and labels timings only (no training epochs)")
    ap.add_argument("--swap", action="store_true", help="MIC channel swap instead of the FOA rotation (needs --mic)")
    ap.add_argument("--corpus-only", action="store_true", help="skip the host-loader epochs")
    ap.add_argument("--mix", action="store_true", help="each batch size with aug_config.time_mix_augment off and on")
    ap.add_argument("--prob", type=float, default=0.5, help="time_mix_prob of the --mix runs")
    ap.add_argument("--yaw", action="store_true", help="each run with aug_config.yaw_rotation_augment off and on (FOA only)")
    a = ap.parse_args()
    if a.swap and not a.mic:
        ap.error("--swap permutes microphone capsules: it needs --mic")
    if a.yaw and a.mic:
        ap.error("--yaw turns the B-format sound field: it is the FOA augmentation (no --mic)")
    n_classes = a.classes
    assert torch.cuda.is_available(), "corpus_bench needs the GPU"
    import adyolo_amd  # noqa: F401
    batches = [int(b) for b in a.batches.split(",")]
    steps = [int(s) for s in a.steps.split(",")]
    steps = (steps * len(batches))[:len(batches)] if len(steps) == 1 else steps
    files = max(b * s for b, s in zip(batches, steps))
    n_rec = -(-files // (REC_S - WINDOW_S + 1))
    shutil.rmtree(a.dir, ignore_errors=True)
    t0 = time.perf_counter()
    nbytes = write_split(a.dir, n_rec, n_classes=n_classes, audio_dir="mic_dev" if a.mic else "foa_dev", whole=a.yaw)
    res = {"split": {"recordings": n_rec, "wav_bytes": nbytes, "write_s": round(time.perf_counter() - t0, 2)},
           "cpus": len(os.sched_getaffinity(0))}
    print(json.dumps(res), flush=True)
    try:
        for b, s in zip(batches, steps):
            r = bench_batch(a.dir, b, s, a.workers, a.iters, a.loss, a.mic, n_classes, a.labels_only, a.swap, a.corpus_only)
            res["b%d" % b] = r
            print(json.dumps(r), flush=True)
            if a.yaw:
                r = bench_batch(a.dir, b, s, a.workers, a.iters, a.loss, a.mic, n_classes, a.labels_only, a.swap, a.corpus_only,
                                yaw=True)
                res["b%d_yaw" % b] = r
                print(json.dumps(r), flush=True)
            if a.mix:
                r = bench_batch(a.dir, b, s, a.workers, a.iters, a.loss, a.mic, n_classes, a.labels_only, a.swap, a.corpus_only,
                                mix=a.prob)
                res["b%d_mix" % b] = r
                print(json.dumps(r), flush=True)
            if a.mix and a.yaw:
                r = bench_batch(a.dir, b, s, a.workers, a.iters, a.loss, a.mic, n_classes, a.labels_only, a.swap, a.corpus_only,
                                mix=a.prob, yaw=True)
                res["b%d_yaw_mix" % b] = r
                print(json.dumps(r), flush=True)
    finally:
        if not a.keep:
            shutil.rmtree(a.dir, ignore_errors=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
