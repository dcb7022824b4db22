"""Evaluation loop.  Mirror of ``test_epoch`` / ``write_seld_output_file`` (/root/reference/src/test.py:26-60):
per file (one full clip, batch 1): eval-mode forward, loss, post-processing (GPU decode + host NMS), one DCASE CSV per
file under ``output_pth``.  The SELD scores come from ``seld_metrics.ComputeSELDResults(ref_dir).get_SELD_Results(output_pth)``."""
import os
import shutil
from itertools import chain

import torch

from .postprocess import group_rows, write_seld_output_file


def delete_and_create_folder(dir_pth):
    if os.path.exists(dir_pth) and os.path.isdir(dir_pth):
        shutil.rmtree(dir_pth)
    os.makedirs(dir_pth, exist_ok=True)


def test_epoch(dataloader, filelist, model, criterion, postprocessor, device, output_pth):
    """dataloader yields (feat (1,7,T,64), label) in the order of ``filelist`` (names without extension)."""
    model.eval()
    delete_and_create_folder(output_pth)
    total = None
    n = 0
    with torch.no_grad():
        for i, (feat, label) in enumerate(dataloader):
            output = model(feat.to(device).float())
            loss = criterion(output, label)
            total = loss.reshape(-1)[:1].clone() if total is None else total + loss.reshape(-1)[:1]
            write_seld_output_file(os.path.join(output_pth, filelist[i] + ".csv"), postprocessor.postprocess(output))
            n = i + 1
    return float(total) / max(n, 1) if total is not None else 0.0


def _sweep_thresholds(postprocessor, thresholds, score):
    """The threshold loop of every sweep: each threshold (default 0.1 .. 0.9) set on the post-processor and scored by
    ``score(k, th, is_last) -> (ER, F, LE, LR, SELD)``; the FIRST one with the lowest SELD score is kept and left set.
    -> (new_thresh, [[ER, F, LE, LR, SELD] per threshold])"""
    if thresholds is None:
        import numpy as np
        thresholds = np.arange(0.1, 1.0, 0.1)
    new_thresh, best, table = postprocessor.get_conf_thresh(), 9999.0, []
    for k, th in enumerate(thresholds):
        postprocessor.set_conf_thresh(th)
        er, f, le, lr, seld = score(k, th, k == len(thresholds) - 1)[:5]
        table.append([er, f, le, lr, seld])
        if seld < best:
            new_thresh, best = th, seld
    postprocessor.set_conf_thresh(new_thresh)
    return new_thresh, table


def sweep_conf_thresh(dataloader, filelist, model, criterion, postprocessor, scorer, device, output_pth,
                      thresholds=None, device_select=False, device_score=False):
    """The reference's periodic threshold reset (src/train.py:178-203): try conf_thresh 0.1 .. 0.9, keep the first one
    with the lowest validation SELD score, leave it set on the post-processor (which rewrites conf AND class threshold,
    datasets.py:532-534).  The reference re-runs the whole validation epoch for each of the nine thresholds; the network
    output does not depend on the threshold, so here the model runs ONCE per file and only the host-side selection/NMS,
    the CSV files and the metrics are redone per threshold -- same files, same scores, a ninth of the forward passes.
    device_select: every file's decode stays on the device (~6 MB per 60 s clip for adyolo, ~0.5 MB for adpit) and the nine
    selections run there (``postprocessor.select_device``: the AD-YOLO NMS or, for the class-wise heads seddoa / masked-seddoa /
    accdoa / adpit, the thresholds and the ADPIT unification); only the selected rows come back to the host.
    device_score: ``scorer`` is a ``seld_metrics.DeviceSELDScorer``; every threshold's rows are scored on the device (device
    rows with device_select, ``add_rows``; host rows otherwise, ``add_dict``) without CSV files, and only the last threshold's
    CSV files are written, so ``output_pth`` ends up as the host sweep leaves it.
    -> (new_thresh, [[ER, F, LE, LR, SELD] per threshold], mean validation loss)"""
    from . import ops
    from .seld_metrics import DeviceSELDScorer
    if device_score and not isinstance(scorer, DeviceSELDScorer):
        raise ValueError("sweep_conf_thresh: device_score=True needs a seld_metrics.DeviceSELDScorer (got %s)"
                         % type(scorer).__name__)
    model.eval()
    decoded, total, n = [], None, 0
    with torch.no_grad():
        for i, (feat, label) in enumerate(dataloader):
            output = model(feat.to(device).float())
            loss = criterion(output, label)
            total = loss.reshape(-1)[:1].clone() if total is None else total + loss.reshape(-1)[:1]
            if device_select:
                if output.shape[0] != 1:
                    raise ValueError("sweep_conf_thresh: one file per batch (B = 1)")
                decoded.append(postprocessor.decode_device(output))
            else:
                decoded.append(postprocessor.decode(output))
            n = i + 1

    def score(k, th, is_last):
        write = not device_score or is_last
        if write:
            delete_and_create_folder(output_pth)
        if device_score:
            scorer.reset()
        for i, dec in enumerate(decoded):
            if device_score and device_select:                  # rows stay on the device; the row total is read to write
                rows, counts = postprocessor.select_device_rows(dec, trim=write)
                scorer.add_rows(rows, counts, [filelist[i]])
                if write:
                    rows = group_rows(*[t.numpy() for t in ops.to_host_many(rows, counts)])[0]
            else:
                rows = postprocessor.select_device(dec)[0] if device_select else postprocessor.select(dec)
                if device_score:
                    scorer.add_dict(filelist[i], rows)
            if write:
                write_seld_output_file(os.path.join(output_pth, filelist[i] + ".csv"), rows)
        return scorer.scores() if device_score else scorer.get_SELD_Results(output_pth)

    new_thresh, table = _sweep_thresholds(postprocessor, thresholds, score)
    return new_thresh, table, (float(total) / max(n, 1) if total is not None else 0.0)


def test_epoch_audio(dataset, model, features, criterion, postprocessor, device, output_pth, batch_size=1, forward=None,
                     device_select=False, device_scorer=None):
    """``test_epoch`` for a raw-audio ``FoaDataset`` split ('valid' / 'test' / 'infer'): int16 audio normalised on the GPU, K1
    features, encoder + head, loss, decode + NMS, one CSV per clip named after the file.  Returns the mean loss (0 for
    'infer', which has no labels).

    batch_size = 1 is the reference's loop (one clip per forward pass, test.py:33-60, train.py:130-133).  In evaluation mode a
    clip's output does not depend on what else is in the batch (BatchNorm uses its running statistics), so consecutive clips of
    EQUAL length may share one forward pass (batch_size > 1: same CSV files; the 60 s clips of a DCASE split all qualify) --
    3 ms per clip at B = 1 against ~1 ms at B = 8 on MI355X.  The loss stays per clip (its normalisers are per call), averaged
    over the clips like the reference's.  forward: optional ``graph.ForwardGraphs`` (K1 + model + decode replayed from a
    hipGraph per clip length); default: eager calls.  device_select: the decoded batch is selected on the device, whatever the
    head (``postprocessor.select_device``: adyolo and the class-wise heads alike, with the post-processor's thresholds as they
    are at the call; launched after the graph replay, not recorded in it) and only the rows come back.
    device_scorer: a ``seld_metrics.DeviceSELDScorer`` the selected rows of every batch are also added to (the device rows
    with device_select); the CSV files are written all the same, and the caller reads ``device_scorer.scores()``.

    Tracking (``test_epoch_corpus(track=...)``) is not taken here: the stage runs on rows that stay on the device, which only
    the corpus passes keep there."""
    from . import ops
    from .datasets import audio_collate_fn

    def select_on_device(dec, clips):
        rows, counts = postprocessor.select_device_rows(dec, len(clips))
        if device_scorer is not None:
            device_scorer.add_rows(rows, counts, clips)
        return group_rows(*[t.numpy() for t in ops.to_host_many(rows, counts)], len(clips))

    model.eval()
    delete_and_create_folder(output_pth)
    total, n = None, 0
    names = dataset.get_filelist()
    i = 0
    with torch.no_grad():
        while i < len(dataset):
            items = []
            for j in range(i, min(i + max(1, int(batch_size)), len(dataset))):
                pcm, _, rows = dataset[j]
                t = (pcm.shape[0] // 600) * 600               # whole hops, like nb_feature_frames in datasets.py:283-286
                if items and t != items[0][1]:
                    break                                     # a clip of another length starts the next batch
                items.append((pcm, t, rows))
            t = items[0][1]
            pcm_b = torch.from_numpy(__import__("numpy").stack([it[0][:t] for it in items])).to(device).contiguous()
            audio = ops.pcm16_to_f32(pcm_b).view(len(items), t, 4)
            decoded = selected = None
            if forward is not None:
                output, dec = forward(audio)
                if dec is not None and device_select:
                    selected = select_on_device(dec, names[i:i + len(items)])
                elif dec is not None:                         # the graph decoded the whole batch: ONE page-locked copy to the host
                    decoded = ops.to_host(dec).numpy()
            else:
                output = model(features(audio, channels_last8=True), channels_last8=True)
            if device_select and selected is None:
                selected = select_on_device(postprocessor.decode_device(output), names[i:i + len(items)])
            for b, (pcm, _, rows) in enumerate(items):
                out_b = output[b:b + 1]
                dense = isinstance(rows, torch.Tensor)          # class-wise losses: (T', ...) label, all zeros for 'infer'
                if (not getattr(dataset, "is_infer", False)) if dense else rows:
                    target = rows.unsqueeze(0) if dense else audio_collate_fn([(pcm, 0, rows)])[2]
                    loss = criterion(out_b, target)
                    total = loss.reshape(-1)[:1].clone() if total is None else total + loss.reshape(-1)[:1]
                    n += 1
                tp = output.shape[1]                          # decoded: [B * T'][...], clip after clip
                if selected is not None:
                    rows_out = selected[b]
                elif decoded is not None:
                    rows_out = postprocessor.select(decoded[b * tp:(b + 1) * tp])
                else:
                    rows_out = postprocessor.postprocess(out_b)
                if device_scorer is not None and selected is None:
                    device_scorer.add_dict(names[i + b], rows_out)
                write_seld_output_file(os.path.join(output_pth, names[i + b] + ".csv"), rows_out)
            i += len(items)
    return float(total) / max(n, 1) if total is not None else 0.0


# ------------------------------------------------------------------------------------- the device loops' shared stages
def _forward_decode(launch, shape, model, features, postprocessor, forward):
    """``launch(audio_out)`` (audio_out: the recorded graph's static input of ``shape`` when ``forward`` has one, so the gather
    writes the graph's input itself; else None) -> the audio, or (audio, target, row_start); then ``forward(audio)`` or the
    eager forward, and ``decode_device`` if nothing decoded yet.  -> (what ``launch`` returned, output, decoded batch: a
    recorded graph's static output when ``forward`` replays one).  No host synchronisation."""
    audio_out = None
    if forward is not None and hasattr(forward, "static_input"):
        audio_out = forward.static_input(shape)
    launched = launch(audio_out)
    audio = launched[0] if isinstance(launched, tuple) else launched
    dec = None
    if forward is not None:
        output, dec = forward(audio)
    else:
        output = model(features(audio, channels_last8=True), channels_last8=True)
    if dec is None:
        dec = postprocessor.decode_device(output)
    return launched, output, dec


def _accumulate_loss(acc, criterion, output, target, row_start, n):
    """The losses of the batch's first ``n`` items (clips, or windows of a pass) into the device accumulator ``acc``."""
    from . import ops
    if row_start is not None:                              # AD-YOLO: every item's loss in one call, normalised per item; one
        cfg = getattr(criterion, "loss", criterion).cfg    # without rows is left out
        ops.adyolo_loss_per_clip(output.contiguous(), target, row_start, cfg["nb_classes"], cfg["grid"], cfg["anchors"],
                                 cfg["thr"], cfg["gains"], cfg["grid_size"], cfg["g_overlap"], acc=acc)
    else:                                                  # class-wise heads: the existing entry point on each item's slice
        for k in range(n):
            ops.loss_accumulate(acc, criterion(output[k:k + 1], target[k:k + 1]).reshape(1))


def _corpus_batch(corpus, idx, model, features, criterion, postprocessor, forward, acc, comb=None):
    """One batch of an HBM-resident evaluation split: ``launch`` -> forward (+ decode) -> the per-clip losses into ``acc``.
    comb: a further view of the batch instead (rotation test-time augmentation): ``launch_view`` into the same graph input, no
    labels, no loss.  -> the decoded batch.  No host synchronisation."""
    launch = (lambda out: corpus.launch(idx, out)) if comb is None else (lambda out: corpus.launch_view(idx, comb, out))
    launched, output, dec = _forward_decode(launch, (len(idx), corpus.n_hops[idx[0]], 4), model, features, postprocessor, forward)
    if comb is None:
        _accumulate_loss(acc, criterion, output, launched[1], launched[2], len(idx))
    return dec


def _corpus_view(corpus, idx, comb, model, features, postprocessor, forward):
    """View ``comb`` of the batch ``_corpus_batch`` ran -> the decoded batch."""
    return _corpus_batch(corpus, idx, model, features, None, postprocessor, forward, None, comb)


def _window_pass(corpus, p, model, features, criterion, postprocessor, forward, acc, stitched, comb=None):
    """One pass of a windowed loop: ``launch`` -> forward (+ decode) -> the window losses into ``acc`` (criterion=None, the
    inference corpus: audio only, no loss) -> ``decode_stitch`` -> (``stitched``, which is made on the first pass and handed
    back; the pass's run of decoded frames, a view of it).  comb: a further view of the pass instead (rotation test-time
    augmentation): ``launch_view`` into the same graph input, no labels, no loss, the same pass table into the same
    ``stitched`` -- the caller has selected the previous view's run before this one is made.  No host synchronisation."""
    from . import ops
    b, wf = corpus.batch_size, corpus.window_frames
    launch = (lambda out: corpus.launch(p, out)) if comb is None else (lambda out: corpus.launch_view(p, comb, out))
    launched, output, dec = _forward_decode(launch, (b, corpus.n_samples, 4), model, features, postprocessor, forward)
    if dec.shape[0] != b * wf:
        raise ValueError("%s: %d decoded frames from %d windows of %d label frames (the model's frame rate is not the label "
                         "hop's)" % (type(corpus).__name__, dec.shape[0], b, wf))
    if comb is None and criterion is not None:
        _accumulate_loss(acc, criterion, output, launched[1], launched[2], corpus.windows_in_pass(p))
    if stitched is None:
        stitched = torch.empty_like(dec)
    ops.decode_stitch(dec, corpus.pass_table(p), wf, corpus.pass_base[p], stitched, corpus.status)
    return stitched, stitched[:corpus.pass_frames[p]]


def _window_view(corpus, p, comb, model, features, postprocessor, forward, stitched):
    """View ``comb`` of the pass ``_window_pass`` ran -> the pass's run under the view."""
    return _window_pass(corpus, p, model, features, None, postprocessor, forward, None, stitched, comb)[1]


class _ViewMerge:
    """The device half of rotation test-time augmentation for the corpus loops: every view's selected rows collected
    (``ops.tta_collect``), then merged (``ops.tta_merge``) into rows and counts in the selection's own layout.  tta: the list of
    views (``augmentations.tta_views``; the other keys at their defaults) or the dict of ``augmentations.tta_options``.  The
    buffers are made once per batch shape; ``status`` collects the ADYOLO_TTA_* bits of the pass.  max_frames (the windowed
    loops, whose runs differ in length from pass to pass): ONE set of buffers for a run of that many frames, made by the
    first merge; a shorter run works in views of it."""

    def __init__(self, tta, postprocessor, device, max_frames=None):
        from .augmentations import tta_options, view_matrix
        from .postprocess import tta_cos
        from . import ops
        opt = tta if isinstance(tta, dict) else tta_options({}, views=tta, postprocessor=postprocessor)
        self.views, self.min_views, self.rows_per_frame = list(opt["views"]), opt["min_views"], opt["max_rows_per_frame"]
        self.cos_t = tta_cos(opt["unify_thresh"])
        self.words = [ops.tta_matrix_word(view_matrix(v)) for v in self.views]
        self.nb_classes = postprocessor.nb_classes
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self._buffers = {}
        self.max_frames, self._longest = None if max_frames is None else int(max_frames), None

    def _buffers_for(self, frames):
        """The buffers of a batch of ``frames`` frames: their own allocation, or with ``max_frames`` views of the one made for
        the longest run (the same layouts over fewer frames; the workspace and the rows as they are)."""
        from . import ops
        buf = self._buffers.get(frames)
        if buf is not None:
            return buf
        v, p = len(self.views), self.rows_per_frame
        if self.max_frames is None:
            buf = ops.tta_buffers(self.status.device, v, frames, self.nb_classes, p, self.min_views)
        else:
            if not 0 < frames <= self.max_frames:
                raise ValueError("_ViewMerge: a run of %d frames with buffers for %d" % (frames, self.max_frames))
            if self._longest is None:
                self._longest = ops.tta_buffers(self.status.device, v, self.max_frames, self.nb_classes, p, self.min_views)
            big = self._longest
            buf = {"pool": big["pool"].view(-1)[:v * frames * p * 4].view(v, frames, p, 4),
                   "pool_counts": big["pool_counts"].view(-1)[:v * frames].view(v, frames),
                   "ws": big["ws"], "rows": big["rows"], "counts": big["counts"][:frames + 1]}
        self._buffers[frames] = buf
        return buf

    def merged(self, postprocessor, decoded_views, n_clips, trim):
        """decoded_views: an iterable of every view's decoded batch, in the order of ``views`` (each is selected before the next
        is asked for: a recorded graph's output is reused) -> the merged (rows, counts)."""
        from . import ops
        buf = None
        for k, dec in enumerate(decoded_views):
            rows, counts = postprocessor.select_device_rows(dec, n_clips, trim=False)
            if buf is None:
                buf = self._buffers_for(counts.numel())
            ops.tta_collect(rows, counts, k, self.words[k], self.nb_classes, buf["pool"], buf["pool_counts"], self.status,
                            buf["ws"])
        return ops.tta_merge(buf["pool"], buf["pool_counts"], self.nb_classes, self.cos_t, self.min_views, self.status, buf["ws"],
                             buf["rows"], buf["counts"], trim=trim)


def _window_merge(tta, postprocessor, corpus):
    """The ``_ViewMerge`` of a windowed loop: its pool and workspace made once, for the longest run of the split."""
    return _ViewMerge(tta, postprocessor, corpus.device, max_frames=max(corpus.pass_frames))


def _track_opts(track, name):
    missing = [k for k in ("gate_deg", "max_gap", "min_len", "smooth") if k not in track]
    if missing:
        raise ValueError("%s: %r lacks %s (augmentations.track_options makes the dict)" % (name, track, missing))
    return dict(track)


class _Tracker:
    """The device half of tracking for the corpus loops: a batch's selected (or merged) rows linked into tracks
    (``LabelPostProcessor.track_device_rows``).  track: the dict of ``augmentations.track_options``.  The buffers are made once
    per batch shape; ``status`` collects the ADYOLO_TRACK_* bits of the pass."""

    def __init__(self, track, device):
        self.opts = _track_opts(track, "track")
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self._buffers = {}

    def tracked(self, postprocessor, rows, counts, n_clips, trim, p=None):
        """-> (rows', counts', ids) of the batch."""
        from . import ops
        key = counts.numel()
        buf = self._buffers.get(key)
        if buf is None:
            buf = self._buffers[key] = ops.track_buffers(self.status.device, key, postprocessor.nb_classes)
        return postprocessor.track_device_rows(rows, counts, n_clips, self.opts, buf=buf, status=self.status, trim=trim)


class _RunTracker:
    """The device half of tracking through windows: every pass's selected rows linked into tracks with the state carried from
    pass to pass (``LabelPostProcessor.track_device_run``), after ``corpus.track_plan(tracking)``.  tracking: the dict of
    ``augmentations.track_options``.  The buffers are made once per run length, the carry once; ``status`` collects the
    ADYOLO_TRACK_* bits.  ``reset()`` empties the carry: before a split is walked again from its first pass."""

    def __init__(self, tracking, corpus):
        self.opts = _track_opts(tracking, "tracking")
        self.plan = corpus.track_plan(self.opts)
        self.hold = self.plan["hold"]
        self.status = torch.zeros(1, dtype=torch.int32, device=corpus.device)
        self.carry = None
        self._buffers = {}

    def reset(self):
        if self.carry is not None:
            self.carry.zero_()

    def tracked(self, postprocessor, rows, counts, n_clips, trim, p):
        """Pass ``p``'s selected (rows, counts) of its one run -> (rows', counts', ids) of the frames the pass emits
        (``plan['pass_frames'][p]`` of them, none for a pass that holds all its frames back, from ``plan['pass_base'][p]`` on
        the common axis)."""
        from . import ops
        if self.carry is None:
            self.carry = ops.track_carry(self.status.device, postprocessor.nb_classes, self.hold)
        key = counts.numel()
        buf = self._buffers.get(key)
        if buf is None:
            buf = self._buffers[key] = ops.track_run_buffers(self.status.device, key, postprocessor.nb_classes, self.hold)
        return postprocessor.track_device_run(rows, counts, self.plan["segments"][p], self.opts, self.hold, self.carry, buf=buf,
                                              status=self.status, trim=trim, emitted=self.plan["pass_frames"][p])


def _further_views(merge):
    return () if merge is None else merge.views[1:]


def _select_rows(postprocessor, dec, more, merge, tracker, n_clips, trim, p=None):
    """The rows of a batch of ``n_clips`` clips, or of pass ``p``'s one run: ``dec`` (view 0's decoded frames) selected -- or,
    with ``merge``, selected, parked and merged with the further views' that the iterable ``more`` yields ONE AT A TIME (a
    recorded graph's output and the stitch buffer are reused, so a view is made only when the one before it is parked) --
    then, with ``tracker``, linked into tracks.  Only the last stage that runs trims (reads the row total: a
    synchronisation); the others hand their capacity buffers on.  -> (rows, counts, ids: None without a tracker)"""
    if merge is None:
        rows, counts = postprocessor.select_device_rows(dec, n_clips, trim=trim and tracker is None)
    else:
        rows, counts = merge.merged(postprocessor, chain((dec,), more), n_clips, trim=trim and tracker is None)
    if tracker is None:
        return rows, counts, None
    return tracker.tracked(postprocessor, rows, counts, n_clips, trim, p)


def _read_status(corpus, acc=None, merge=None, tracker=None):
    """The one synchronisation that ends a walk over the split: the corpus status word and, when they are there, the loss
    accumulator {sum, count} and the status words of the view merge and the tracker, in ONE copy; every word checked.
    -> the mean loss (with ``acc``)."""
    from . import ops
    parts = {"loss": acc, "corpus": corpus.status, "tta": None if merge is None else merge.status,
             "track": None if tracker is None else tracker.status}
    parts = {k: t for k, t in parts.items() if t is not None}
    host = dict(zip(parts, ops.to_host_many(*parts.values())))
    corpus.check(int(host["corpus"][0]))
    if merge is not None:
        ops.tta_status_check(int(host["tta"][0]))
    if tracker is not None:
        ops.track_status_check(int(host["track"][0]))
    if acc is None:
        return None
    total, n = host["loss"][0], int(host["loss"][1])
    return float(total) / max(n, 1) if n else 0.0


def _csv_flag(device_csv, name):
    if not isinstance(device_csv, bool):
        raise ValueError("%s: device_csv must be True or False (got %r)" % (name, device_csv))
    return device_csv


class _CsvWriter:
    """The device half of ``device_csv=True``: a batch's or pass's rows formatted into the bytes of their CSV files on the
    device (``ops.csv_format``: ``postprocess.format_rows`` byte for byte), then two copies -- the segment offsets with the
    status word, then exactly the bytes -- where the host writer reads the row total and then copies the rows.  The rows come
    UNTRIMMED (nothing reads their total).  The workspaces are made once per shape; every segment table is uploaded once,
    from page-locked memory without a synchronisation -- the windowed loops' all together before the first pass; the byte buffer holds a call's row capacity at the longest line, which no call outgrows, or 64 MiB (256 bytes per frame
    if that is more) where that is less: it then grows to the largest total seen, and the call that outgrows it is
    formatted again -- one more read, which a walk over a split pays a handful of times at most."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._ws, self._tables, self._out, self._pinned = {}, {}, None, []

    def _bytes(self, n):
        return torch.empty(max(16, (n + 15) // 16 * 16), dtype=torch.uint8, device=self.device)

    def start(self, output_pth, names):
        """Every file of the split, empty: a windowed loop appends to them pass by pass, and a recording without rows keeps
        its empty file."""
        for name in names:
            open(os.path.join(output_pth, name + ".csv"), "wb").close()

    def _upload(self, pinned):
        """The one host-to-device copy of the writer: page-locked and ``non_blocking``, so it never synchronises the stream
        (a blocking copy from pageable memory would, behind the whole pass)."""
        return pinned.to(self.device, non_blocking=True)

    def tables(self, tables):
        """The segment tables (K, 2) int32 that are not on the device yet -> there, all in ONE page-locked upload.  The windowed
        loops call it with every pass's table before their first pass (``_csv_run_tables``)."""
        import numpy as np
        new = {}
        for t in tables:
            t = np.ascontiguousarray(t, dtype=np.int32)
            if t.tobytes() not in self._tables:
                new.setdefault(t.tobytes(), t)
        if not new:
            return
        pinned = torch.from_numpy(np.concatenate(list(new.values()))).pin_memory()
        self._pinned.append(pinned)                              # (alive until the copy has run: as long as the writer)
        dev, at = self._upload(pinned), 0
        for key, t in new.items():
            self._tables[key] = dev[at:at + len(t)]
            at += len(t)

    def forget(self):
        """Drop the uploaded segment tables: a live stream has a new one per pass, used once.  After a ``fetch``, which has
        synchronised behind the upload and the kernel that read the table."""
        self._tables.clear()
        del self._pinned[:]

    def fetch(self, rows, counts, table, ids=None):
        """-> (the bytes of the call on the host, a uint8 array valid until the next fetch; seg_bytes as a list)"""
        from . import ops
        key = table.tobytes()
        if key not in self._tables:                              # (the clip loops: once per batch shape)
            self.tables([table])
        seg = self._tables[key]
        frames, n_rows, k = counts.numel(), rows.shape[0], len(table)
        ws = self._ws.get((frames, n_rows, k))
        if ws is None:
            ws = self._ws[(frames, n_rows, k)] = ops.csv_buffers(self.device, frames, n_rows, k, 0)
        floor = min(n_rows * ops.CSV_LINE_MAX, max(64 << 20, 256 * frames))
        if self._out is None or self._out.numel() < floor:
            self._out = self._bytes(floor)
        while True:
            buf = {"ws": ws["ws"], "seg_bytes": ws["seg_bytes"], "out": self._out}
            out, seg_bytes, _ = ops.csv_format(rows, counts, seg, ids, buf=buf, status=self.status)
            seg_h, status_h = ops.to_host_many(seg_bytes, self.status)
            word, seg_h = int(status_h[0]), seg_h.tolist()
            if word != ops.CSV_OVERFLOW:
                break
            self._out = self._bytes(1 << (seg_h[-1] - 1).bit_length())
            self.status.zero_()
        ops.csv_status_check(word)
        if not seg_h[-1]:
            return b"", seg_h
        return ops.to_host_many(out[:seg_h[-1]])[0].numpy(), seg_h


def _write_rows(output_pth, names, rows, counts, ids=None, csv=None):
    """Selected device rows of ``len(names)`` clips (trimmed to their total) -> one CSV per clip.  ids: the rows' track ids
    (tracking is on), written into the track column.  csv: the ``_CsvWriter`` of ``device_csv=True`` (the rows untrimmed): the
    files' bytes come formatted from the device."""
    from . import ops
    if csv is not None:
        from .postprocess import csv_segments_clips
        data, at = csv.fetch(rows, counts, csv_segments_clips(len(names), counts.numel() // len(names)), ids)
        for k, name in enumerate(names):
            with open(os.path.join(output_pth, name + ".csv"), "wb") as f:
                f.write(data[at[k]:at[k + 1]])
        return
    if ids is None:
        rows_h, counts_h = [t.numpy() for t in ops.to_host_many(rows, counts)]
        for name, clip_rows in zip(names, group_rows(rows_h, counts_h, len(names))):
            write_seld_output_file(os.path.join(output_pth, name + ".csv"), clip_rows)
        return
    from .postprocess import track_groups
    rows_h, counts_h, ids_h = [t.numpy() for t in ops.to_host_many(rows, counts, ids)]
    for name, clip_rows, clip_ids in zip(names, group_rows(rows_h, counts_h, len(names)),
                                         track_groups(ids_h, counts_h, len(names))):
        write_seld_output_file(os.path.join(output_pth, name + ".csv"), clip_rows, clip_ids)


def _write_pass(corpus, base, rows, counts, ids, outs, out_ids, csv=None, output_pth=None, names=None):
    """The rows (trimmed) of a pass's run, which starts at ``base`` on the common axis -> the host in one copy, onto each
    recording's own frame axis in ``outs``.  ids: the rows' track ids (tracking is on), which go to ``out_ids`` {frame of the
    recording: [id, ...]} per recording, parallel to ``outs``.  csv: the ``_CsvWriter`` of ``device_csv=True`` (the rows
    untrimmed): the run's bytes come formatted from the device and each recording's span is appended to its file under
    ``output_pth`` (a recording's passes come in frame order); ``outs`` / ``out_ids`` are not touched."""
    import numpy as np
    from . import ops
    from .corpus import split_pass_rows
    if csv is not None:
        from .postprocess import csv_segments_run
        r0, table = csv_segments_run(base, counts.numel(), corpus.frame_start)
        data, at = csv.fetch(rows, counts, table, ids)
        for k in range(len(table)):
            if at[k + 1] > at[k]:
                with open(os.path.join(output_pth, names[r0 + k] + ".csv"), "ab") as f:
                    f.write(data[at[k]:at[k + 1]])
        return
    rows_h, counts_h, *ids_h = [t.numpy() for t in ops.to_host_many(*(t for t in (rows, counts, ids) if t is not None))]
    for r, found in split_pass_rows(rows_h, counts_h, base, corpus.frame_start).items():
        outs[r].update(found)                                                # (a recording's passes come in frame order)
    if ids is None:
        return
    ends = np.cumsum(counts_h.astype(np.int64))
    ids_h = ids_h[0].tolist()
    for f in np.flatnonzero(counts_h).tolist():
        r = int(np.searchsorted(corpus.frame_start, base + f, "right")) - 1
        out_ids[r][base + f - int(corpus.frame_start[r])] = ids_h[int(ends[f]) - int(counts_h[f]):int(ends[f])]


def _csv_run_tables(csv, corpus, tracker, base):
    """Before a windowed loop's first pass: the segment table of every pass that emits frames (``_write_pass`` asks for the
    same ones), uploaded together, so that no pass uploads anything."""
    if csv is None:
        return
    from .postprocess import csv_segments_run
    frames = corpus.pass_frames if tracker is None else tracker.plan["pass_frames"]
    csv.tables([csv_segments_run(int(base[p]), int(frames[p]), corpus.frame_start)[1]
                for p in range(corpus.n_passes) if int(frames[p]) > 0])


def _write_recordings(output_pth, names, outs, out_ids=None, csv=None):
    if csv is not None:                                          # (``_CsvWriter.start`` made the files, the passes filled them)
        return
    for k, (name, rows) in enumerate(zip(names, outs)):
        write_seld_output_file(os.path.join(output_pth, name + ".csv"), rows, None if out_ids is None else out_ids[k])


# ------------------------------------------------------------------------------------------------ whole clips from HBM
def test_epoch_corpus(corpus, model, features, criterion, postprocessor, output_pth=None, batch_size=8, forward=None,
                      device_scorer=None, tta=None, track=None, device_csv=False):
    """``test_epoch_audio(device_select=True)`` from an HBM-resident split (``corpus.EvalDeviceCorpus``): the same batches,
    the same mean of per-clip losses (float32 adds in file order, clips without AD-YOLO rows left out), the same selected rows
    into ``device_scorer`` and, with ``output_pth``, the same CSV files -- but no WAV read, no CSV parse, no host label
    encoding and no audio or target upload: per batch ``corpus.launch`` -> ``forward(audio)`` (``graph.ForwardGraphs``; default
    the eager forward + ``decode_device``) -> the per-clip loss on the device (``ops.adyolo_loss_per_clip``, or the class-wise
    loss per slice) -> ``select_device_rows`` -> ``device_scorer.add_rows``.  output_pth=None: nothing is written and the
    pass synchronises ONCE, at its end, to read the loss accumulator and the corpus status word together; with output_pth
    every batch's rows are copied to the host (one synchronisation each).  Returns the mean loss.

    tta (rotation test-time augmentation): None, or the views of ``augmentations.tta_views`` (a list of combinations starting
    with 0, or the dict of ``augmentations.tta_options`` with the other keys).  Every batch then also runs under each further
    view -- ``corpus.launch_view`` into the same graph input, forward, decode, selection -- and the rows that go to the scorer
    and the files are the views' rows turned back and merged on the device (``postprocess.merge_view_rows``; csrc/select.hip).
    View 0 is the plain pass, so the loss is the plain pass's, the same float; the status word of the merge is read with the
    loss (an overflow raises, naming the key to enlarge).

    track (tracks across frames): None, or the dict of ``augmentations.track_options``.  Every batch's rows -- the merged ones
    with ``tta`` -- are then linked per (clip, class) into tracks on the device (``postprocess.track_rows``; csrc/track.hip):
    directions smoothed, short gaps filled, short tracks dropped.  The tracked rows go to the scorer and the files, whose
    third column carries the track ids; the loss is the plain pass's.  The status word is read with the loss (the caps of the
    definition only warn).  None leaves the pass exactly as it is.

    device_csv (with output_pth): True formats every batch's rows into the bytes of their files ON THE DEVICE
    (``ops.csv_format``, csrc/csv.hip: ``postprocess.format_rows``, the bytes ``write_seld_output_file`` writes) -- no row is
    copied, grouped or formatted on the host; per batch the segment offsets and then the bytes are copied (two
    synchronisations, as the host writer's row total and rows) and each file's span is written.  The same files, byte for
    byte, with ``tta``, ``track`` and ``device_scorer`` alike.  False leaves every call, copy and byte as it is."""
    from . import ops
    csv = _CsvWriter(corpus.device) if _csv_flag(device_csv, "test_epoch_corpus") and output_pth is not None else None
    model.eval()
    if output_pth is not None:
        delete_and_create_folder(output_pth)
    names = corpus.get_filelist()
    corpus.reset_status()
    acc = ops.loss_accumulator(corpus.device)
    merge = _ViewMerge(tta, postprocessor, corpus.device) if tta is not None else None
    tracker = _Tracker(track, corpus.device) if track is not None else None
    with torch.no_grad():
        for idx in corpus.batches(batch_size):
            clips = [names[i] for i in idx]
            dec = _corpus_batch(corpus, idx, model, features, criterion, postprocessor, forward, acc)
            more = (_corpus_view(corpus, idx, v, model, features, postprocessor, forward) for v in _further_views(merge))
            rows, counts, ids = _select_rows(postprocessor, dec, more, merge, tracker, len(clips),
                                             output_pth is not None and csv is None)
            if device_scorer is not None:
                device_scorer.add_rows(rows, counts, clips)
            if output_pth is not None:
                _write_rows(output_pth, clips, rows, counts, ids, csv)
    return _read_status(corpus, acc, merge, tracker)


def sweep_conf_thresh_corpus(corpus, model, features, criterion, postprocessor, scorer, thresholds=None, output_pth=None,
                             batch_size=8, forward=None, tta=None, track=None, device_csv=False):
    """``sweep_conf_thresh(device_select=True, device_score=True)`` from an HBM-resident split: ONE forward pass per batch,
    every batch's decode kept on the device, then per threshold the selections and the device scores (``scorer``: a
    ``seld_metrics.DeviceSELDScorer``); the chosen threshold is left set on the post-processor.  With ``output_pth`` the last
    threshold's CSV files are written, as the host sweep leaves them.  Clips without AD-YOLO rows are left out of the mean
    loss (the host sweep cannot take them at all).  -> (new_thresh, [[ER, F, LE, LR, SELD] per threshold], mean loss)

    tta, track: as ``test_epoch_corpus``, redone per threshold: every VIEW's decode of every batch is kept on the device, and
    each threshold selects, collects and merges them again and links the rows before they are scored and written.  The loss
    and the corpus status word are read after the forward phase; the status words of the merge and the tracker once, in one
    copy, after the last threshold.  device_csv: as ``test_epoch_corpus``, for the last threshold's files."""
    from .seld_metrics import DeviceSELDScorer
    _csv_flag(device_csv, "sweep_conf_thresh_corpus")
    if not isinstance(scorer, DeviceSELDScorer):
        raise ValueError("sweep_conf_thresh_corpus needs a seld_metrics.DeviceSELDScorer (got %s)" % type(scorer).__name__)
    from . import ops
    model.eval()
    names = corpus.get_filelist()
    corpus.reset_status()
    acc = ops.loss_accumulator(corpus.device)
    decoded = []
    csv = _CsvWriter(corpus.device) if device_csv and output_pth is not None else None
    merge = _ViewMerge(tta, postprocessor, corpus.device) if tta is not None else None
    tracker = _Tracker(track, corpus.device) if track is not None else None
    with torch.no_grad():
        for idx in corpus.batches(batch_size):
            dec = _corpus_batch(corpus, idx, model, features, criterion, postprocessor, forward, acc)
            views = [dec.clone() if forward is not None else dec]                                     # (a graph's output is reused)
            views += [_corpus_view(corpus, idx, v, model, features, postprocessor, forward).clone() for v in _further_views(merge)]
            decoded.append(([names[i] for i in idx], views))
    loss = _read_status(corpus, acc)

    def score(k, th, is_last):
        write = is_last and output_pth is not None
        if write:
            delete_and_create_folder(output_pth)
        scorer.reset()
        for clips, views in decoded:
            rows, counts, ids = _select_rows(postprocessor, views[0], views[1:], merge, tracker, len(clips),
                                             write and csv is None)
            scorer.add_rows(rows, counts, clips)
            if write:
                _write_rows(output_pth, clips, rows, counts, ids, csv)
        return scorer.scores()

    new_thresh, table = _sweep_thresholds(postprocessor, thresholds, score)
    if merge is not None or tracker is not None:
        _read_status(corpus, None, merge, tracker)
    return new_thresh, table, loss


# ------------------------------------------------------------------------------------- recordings of any length, in windows
def infer_epoch_corpus(corpus, model, features, postprocessor, output_pth, forward=None, tracking=None, tta=None,
                       device_csv=False):
    """Inference on recordings of any length from an HBM-resident folder (``corpus.InferDeviceCorpus``): every recording cut
    into overlapping windows of one shape, the windows run ``corpus.batch_size`` at a time -- so the whole folder has ONE input
    shape and, with ``forward`` (``graph.ForwardGraphs``), one recorded graph.  Per pass: ``adyolo_corpus_gather_windows`` (into
    the graph's static input when there is one) -> ``forward(audio)`` or the eager forward + ``decode_device`` ->
    ``adyolo_decode_stitch`` (each window's frames that have context on both sides, compacted into one run) ->
    ``select_device_rows`` on the run (both selections work frame by frame) -> the rows and counts to the host, where
    ``corpus.split_pass_rows`` puts them on each recording's own frame axis.  One CSV per recording, named after the file, empty
    for a recording without rows or without a label frame.  No audio crosses PCIe; nothing is uploaded per pass.
    -> {'recordings', 'windows', 'passes', 'frames'}.

    Tracking (``tracking``) and tta: as ``test_epoch_windows`` (``postprocess.track_run`` with the state carried from pass to
    pass; the views merged, then linked), without labels, loss and scorer: the emitted rows go to the files only, with one
    synchronisation per pass as without them, and the status words of the merge and the tracker are read with the corpus's in
    the one copy at the end.  None leaves every call, allocation, synchronisation and bit as it is.

    device_csv: as ``test_epoch_windows``."""
    csv = _CsvWriter(corpus.device) if _csv_flag(device_csv, "infer_epoch_corpus") else None
    model.eval()
    delete_and_create_folder(output_pth)
    names = corpus.get_filelist()
    if csv is not None:
        csv.start(output_pth, names)
    corpus.reset_status()
    outs = [{} for _ in names]
    merge = _window_merge(tta, postprocessor, corpus) if tta is not None and corpus.n_passes else None
    tracker = _RunTracker(tracking, corpus) if tracking is not None else None
    out_ids = [{} for _ in names] if tracker is not None else None
    base = corpus.pass_base if tracker is None else tracker.plan["pass_base"]
    _csv_run_tables(csv, corpus, tracker, base)
    stitched = None
    with torch.no_grad():
        for p in range(corpus.n_passes):
            stitched, run = _window_pass(corpus, p, model, features, None, postprocessor, forward, None, stitched)
            more = (_window_view(corpus, p, v, model, features, postprocessor, forward, stitched) for v in _further_views(merge))
            rows, counts, ids = _select_rows(postprocessor, run, more, merge, tracker, 1, csv is None, p)
            if counts.numel():                                               # (a tracked pass may hold all its frames back)
                _write_pass(corpus, base[p], rows, counts, ids, outs, out_ids, csv, output_pth, names)
    _read_status(corpus, None, merge, tracker)
    _write_recordings(output_pth, names, outs, out_ids, csv)
    return {"recordings": len(names), "windows": corpus.n_windows, "passes": corpus.n_passes,
            "frames": int(corpus.frame_start[-1])}


def test_epoch_windows(corpus, model, features, criterion, postprocessor, output_pth=None, forward=None, device_scorer=None,
                       tracking=None, tta=None, device_csv=False):
    """Labelled evaluation of recordings of ANY length from an HBM-resident split (``corpus.EvalWindowCorpus``): every recording
    cut into overlapping windows of one shape, ``corpus.batch_size`` windows per pass -- one input shape for the whole split
    and, with ``forward`` (``graph.ForwardGraphs``), one recorded graph.  Per pass: ``corpus.launch`` (audio into the graph's
    static input when there is one, the windows' labels) -> forward + decode -> the window losses into a device accumulator
    -> ``adyolo_decode_stitch`` (the kept frames of the pass as one run) -> ``select_device_rows`` on the run ->
    ``device_scorer.add_run`` (``adyolo_seld_score_runs``: the run scored in segments, one per recording it touches; a
    recording whose segments have all been added holds the accumulator bits of one whole-recording ``add_rows``).

    THE LOSS is the training chunks' definition, not the reference's per-recording one: the mean over the windows, in window
    order in float32, of the loss of each window's full ``window_frames`` frames, margins included (AD-YOLO:
    ``adyolo_loss_per_clip`` with a window for a clip -- a window without AD-YOLO rows is left out, as a clip without rows is
    in ``test_epoch_corpus``; class-wise heads: the criterion on each window's slice).  A frame that two windows overlap on
    counts in both, a short recording's window is padded with silence and no events.  It equals the reference's loss only
    where every recording is exactly one window long.

    output_pth=None: nothing is written and the pass synchronises ONCE, at its end: one ``to_host_many`` of the loss
    accumulator and the corpus status word (the scorer's status is read by its ``scores()``).  With output_pth the rows of
    every pass go to the host (one synchronisation each) and one CSV is written per recording (``corpus.split_pass_rows``),
    empty for a recording without rows or without a label frame.  Returns the mean loss.

    Tracking (``tracking``: None, or the dict of ``augmentations.track_options``): every pass's selected rows are linked into
    tracks on the device with the state carried from pass to pass (``postprocess.track_run``; csrc/track.hip
    ``adyolo_track_run``), so a recording cut by any number of passes gets the rows and ids ``postprocess.track_rows`` gives on
    it whole, bit for bit.  A pass then emits its frames without the last D of a recording that goes on in the next pass -- a
    gap fill or the erasure of a short track can still reach them -- and with the D it held back before
    (``corpus.track_plan``, D = ``postprocess.track_hold``).  The emitted rows go to the scorer (its segment tables on the
    emitted bounds) and to the files, whose third column carries the track ids; the status word is read in the one
    end-of-pass copy (the caps of the definition only warn).  None leaves every call, allocation and bit as it is.

    tta (rotation test-time augmentation): None, or what ``test_epoch_corpus`` takes (a list of views starting with 0, or the
    dict of ``augmentations.tta_options``).  View 0 is the plain pass: labels, loss -- the same float as without views --
    and stitch.  Every further view of a pass is ``corpus.launch_view`` into the same static input, the forward pass, the
    decode and ``adyolo_decode_stitch`` with the same pass table; each view's run is selected and parked
    (``ops.tta_collect``) before the next one overwrites the graph's output and the stitch buffer, and after the last the
    views are merged per frame (``ops.tta_merge``; ``postprocess.merge_view_rows`` bit for bit -- per frame, so it does not
    matter where the passes cut the axis).  The merged rows take the selection's place everywhere: the scorer, the files
    and, with ``tracking``, the link (merge, then link, as on whole clips).  The pool and the workspace are allocated once,
    for the longest run of the split; the merge's status word is read in the one end-of-pass copy (an overflow raises,
    naming ``tta_max_rows_per_frame``).  None leaves every call, allocation, synchronisation and bit as it is.

    device_csv (with output_pth): True formats every pass's emitted rows into the bytes of their files ON THE DEVICE
    (``ops.csv_format``, csrc/csv.hip: ``postprocess.format_rows``, the bytes ``write_seld_output_file`` writes; the run split
    at the recording boundaries by ``postprocess.csv_segments_run``).  Every recording's file is made empty first and each
    pass appends its spans (a recording's passes come in frame order): no row is copied, split or formatted on the host,
    and per pass the segment offsets and then the bytes are copied (two synchronisations, as the host writer's row total and
    rows).  The same files, byte for byte, with ``tta``, ``tracking`` and ``device_scorer`` alike.  False leaves every call,
    copy and byte as it is."""
    from . import ops
    csv = _CsvWriter(corpus.device) if _csv_flag(device_csv, "test_epoch_windows") and output_pth is not None else None
    model.eval()
    if output_pth is not None:
        delete_and_create_folder(output_pth)
    names = corpus.get_filelist()
    if csv is not None:
        csv.start(output_pth, names)
    corpus.reset_status()
    acc = ops.loss_accumulator(corpus.device)
    merge = _window_merge(tta, postprocessor, corpus) if tta is not None else None
    tracker = _RunTracker(tracking, corpus) if tracking is not None else None
    bounds = None if tracker is None else tracker.plan["bounds"]
    segments = corpus.segments(device_scorer, bounds=bounds) if device_scorer is not None else None
    outs = [{} for _ in names]
    out_ids = [{} for _ in names] if tracker is not None else None
    base = corpus.pass_base if tracker is None else tracker.plan["pass_base"]
    _csv_run_tables(csv, corpus, tracker, base)
    stitched = None
    with torch.no_grad():
        for p in range(corpus.n_passes):
            stitched, run = _window_pass(corpus, p, model, features, criterion, postprocessor, forward, acc, stitched)
            more = (_window_view(corpus, p, v, model, features, postprocessor, forward, stitched) for v in _further_views(merge))
            rows, counts, ids = _select_rows(postprocessor, run, more, merge, tracker, 1,
                                             output_pth is not None and csv is None, p)
            if not counts.numel():                                           # a tracked pass that holds all its frames back
                continue
            if device_scorer is not None:
                device_scorer.add_run(rows, counts, segments[p])
            if output_pth is not None:
                _write_pass(corpus, base[p], rows, counts, ids, outs, out_ids, csv, output_pth, names)
    if output_pth is not None:
        _write_recordings(output_pth, names, outs, out_ids, csv)
    return _read_status(corpus, acc, merge, tracker)


def sweep_conf_thresh_windows(corpus, model, features, criterion, postprocessor, scorer, thresholds=None, output_pth=None,
                              forward=None, tracking=None, tta=None, device_csv=False):
    """``sweep_conf_thresh_corpus`` through windows (``corpus.EvalWindowCorpus``): ONE forward pass per window pass, every
    pass's stitched run kept (cloned) on the device, then per threshold ``scorer.reset()``, the selection of every run and
    ``scorer.add_run``; the chosen threshold is left set on the post-processor.  With ``output_pth`` the last threshold's CSV
    files are written.  The loss is ``test_epoch_windows``'s.  -> (new_thresh, [[ER, F, LE, LR, SELD] per threshold], mean loss)

    Tracking (``tracking``) and tta: as ``test_epoch_windows`` (``postprocess.track_run``), redone per threshold.  Every VIEW's
    stitched run of every pass is kept (cloned) on the device -- passes x views x run frames x the decode's record, i.e.
    views x (the split's label frames) x record x 4 bytes, against one such axis without views -- and each threshold empties
    the tracker's carry with the scorer, then selects, collects, merges and links the runs again; the last threshold's
    emitted rows also go to the files.  The loss and the corpus status word are read after the forward phase; the status
    words of the merge and the tracker once, in one copy, after the last threshold.  None leaves every call, allocation and
    bit as it is.  device_csv: as ``test_epoch_windows``, for the last threshold's files (the folder is then emptied before
    the last threshold's passes, not after them)."""
    from .seld_metrics import DeviceSELDScorer
    _csv_flag(device_csv, "sweep_conf_thresh_windows")
    if not isinstance(scorer, DeviceSELDScorer):
        raise ValueError("sweep_conf_thresh_windows needs a seld_metrics.DeviceSELDScorer (got %s)" % type(scorer).__name__)
    from . import ops
    model.eval()
    names = corpus.get_filelist()
    corpus.reset_status()
    acc = ops.loss_accumulator(corpus.device)
    merge = _window_merge(tta, postprocessor, corpus) if tta is not None else None
    tracker = _RunTracker(tracking, corpus) if tracking is not None else None
    segments = corpus.segments(scorer, bounds=None if tracker is None else tracker.plan["bounds"])
    base = corpus.pass_base if tracker is None else tracker.plan["pass_base"]
    runs, stitched = [], None
    csv = _CsvWriter(corpus.device) if device_csv and output_pth is not None else None
    _csv_run_tables(csv, corpus, tracker, base)
    with torch.no_grad():
        for p in range(corpus.n_passes):
            stitched, run = _window_pass(corpus, p, model, features, criterion, postprocessor, forward, acc, stitched)
            views = [run.clone()]                                            # (the stitch buffer is reused)
            views += [_window_view(corpus, p, v, model, features, postprocessor, forward, stitched).clone()
                      for v in _further_views(merge)]
            runs.append(views)
    loss = _read_status(corpus, acc)

    def score(k, th, is_last):
        write = is_last and output_pth is not None
        outs =[{} for _ in names]
        out_ids = [{} for _ in names] if tracker is not None else None
        scorer.reset()
        if tracker is not None:
            tracker.reset()
        if write and csv is not None:
            delete_and_create_folder(output_pth)
            csv.start(output_pth, names)
        for p, views in enumerate(runs):
            rows, counts, ids = _select_rows(postprocessor, views[0], views[1:], merge, tracker, 1, write and csv is None, p)
            if not counts.numel():
                continue
            scorer.add_run(rows, counts, segments[p])
            if write:
                _write_pass(corpus, base[p], rows, counts, ids, outs, out_ids, csv, output_pth, names)
        if write and csv is None:
            delete_and_create_folder(output_pth)
            _write_recordings(output_pth, names, outs, out_ids)
        return scorer.scores()

    new_thresh, table = _sweep_thresholds(postprocessor, thresholds, score)
    if merge is not None or tracker is not None:
        _read_status(corpus, None, merge, tracker)
    return new_thresh, table, loss


def score_output_folder(params, ref_dir, output_pth, is_jackknife=False):
    """The three score sets the reference prints for one evaluated folder (src/test.py:104-133): all frames, frames with
    overlapping events ("class-independent polyphony") and frames with overlapping events of one class
    ("class-homogenous polyphony").  -> {'all' | 'polyphony' | 'homogenous': (ER, F, LE, LR, SELD, classwise)}."""
    from .seld_metrics import ComputeSELDResults, ComputeSELDResultsFromEventOverlap
    return {
        "all": ComputeSELDResults(params, ref_dir).get_SELD_Results(output_pth, is_jackknife),
        "polyphony": ComputeSELDResultsFromEventOverlap(params, ref_dir).get_SELD_Results(output_pth, is_jackknife),
        "homogenous": ComputeSELDResultsFromEventOverlap(params, ref_dir, classwise_overlap_test=True)
        .get_SELD_Results(output_pth, is_jackknife),
    }


# ------------------------------------------------------------------------------------------------------ a live stream
class _StreamTracker:
    """The device half of tracking through a live stream: ``_RunTracker`` without a plan made in advance.  Every pass is ONE
    segment {0, n, continues = not the first pass, open = the stream goes on}; the hold is ``track_hold`` itself, one carry.
    The emitted frames follow from the frames walked so far: the carried held frames, then the pass's without the newly held
    ones.  ``open`` is set by the session before each pass; ``base`` is then the first emitted frame on the stream's axis."""

    def __init__(self, tracking, device):
        from .postprocess import track_hold
        self.opts = _track_opts(tracking, "tracking")
        self.hold = track_hold(self.opts["max_gap"], self.opts["min_len"])
        self.device = torch.device(device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.carry, self._buffers, self._segments = None, {}, {}
        self.walked, self.open, self.base = 0, True, 0

    def reset(self):
        if self.carry is not None:
            self.carry.zero_()
        self.walked, self.open, self.base = 0, True, 0
        self.status.zero_()

    def _segment(self, key):
        """The one-row segment table on the device: uploaded once per (frames, continues, open), from page-locked memory."""
        seg = self._segments.get(key)
        if seg is None:
            pinned = torch.tensor([[0, key[0], key[1], key[2]]], dtype=torch.int32).pin_memory()
            seg = self._segments[key] = (pinned.to(self.device, non_blocking=True), pinned)
        return seg[0]

    def tracked(self, postprocessor, rows, counts, n_clips, trim, p=None):
        from . import ops
        if self.carry is None:
            self.carry = ops.track_carry(self.device, postprocessor.nb_classes, self.hold)
        n = counts.numel()
        buf = self._buffers.get(n)
        if buf is None:
            buf = self._buffers[n] = ops.track_run_buffers(self.device, n, postprocessor.nb_classes, self.hold)
        held = min(self.hold, self.walked)
        emitted = held + n - (min(self.hold, self.walked + n) if self.open else 0)
        self.base = self.walked - held
        seg = self._segment((n, int(self.walked > 0), int(self.open)))
        self.walked += n
        return postprocessor.track_device_run(rows, counts, seg, self.opts, self.hold, self.carry, buf=buf, status=self.status,
                                              trim=trim, emitted=emitted)


class StreamInference:
    """Inference on ONE live stream (``corpus.StreamDeviceCorpus``): push audio as it comes, get the detections of the frames
    that have become final.  A recording pushed in any pieces and closed gives, byte for byte, the CSV file
    ``infer_epoch_corpus`` writes for it (with the default hop, at ``batch_size`` 1: the same windows; tracking, tta and
    device_csv alike).

        session = StreamInference(corpus, model, features, postprocessor, forward=ForwardGraphs(...), output_file="live.csv")
        rows, ids = session.push(pcm)            # int16 (n, 4), any n
        rows, ids = session.close()

    ``push`` appends the samples and runs every runnable pass -> ({frame: [[class, x, y, z], ...]}, {frame: [id, ...]} or None
    without tracking) of the frames that became final: frames on the stream's own axis, ascending, never revised later.  A push
    larger than the ring's free space is taken in slices between the passes.  A push that completes no window copies the
    samples and returns empties, with no synchronisation.  ``close`` runs the closing window (the tracker's segment not open,
    so its carry is flushed), returns the rest and checks the status words of the corpus, the merge and the tracker in one
    copy.  ``frames_final``: the frames final so far.  ``reset()``: a new stream -- the corpus, the tracker's carry and ids,
    the output file -- in the same buffers and graphs.

    Per pass: ``_forward_decode`` (the ring gather into the graph's static input when ``forward`` has one) ->
    ``ops.decode_stitch`` -> ``_select_rows`` (tta: the further views through ``_ViewMerge``; tracking: ``track_device_run``
    with one segment and one carry), then ONE host synchronisation, the copy of the rows, as in ``infer_epoch_corpus``.  All
    passes of a stream have one shape: ``forward`` records one graph.

    Latency (``corpus.stream_plan``): a frame is final at most margin + hop after it was pushed, with tracking a further
    ``postprocess.track_hold`` frames later; the rest on ``close``.

    output_file: every pass appends its lines (the format of ``write_seld_output_file``).  device_csv=True (needs
    output_file): the lines are formatted on the device (``_CsvWriter``) and go to the file only -- ``push`` and ``close``
    then return empty dicts, nothing else is copied."""

    def __init__(self, corpus, model, features, postprocessor, forward=None, tracking=None, tta=None, device_csv=False,
                 output_file=None):
        if _csv_flag(device_csv, "StreamInference") and output_file is None:
            raise ValueError("StreamInference: device_csv=True formats the lines of output_file; none was given")
        self.corpus, self.model, self.features, self.postprocessor, self.forward = corpus, model, features, postprocessor, forward
        self.output_file = output_file
        self.csv = _CsvWriter(corpus.device) if device_csv else None
        self.merge = None
        if tta is not None:
            self.merge = _ViewMerge(tta, postprocessor, corpus.device, max_frames=corpus.batch_size * corpus.window_frames)
        self.tracker = _StreamTracker(tracking, corpus.device) if tracking is not None else None
        self._stitched = None
        model.eval()
        self.reset()

    def reset(self):
        self.corpus.reset()
        if self.tracker is not None:
            self.tracker.reset()
        if self.merge is not None:
            self.merge.status.zero_()
        self.frames_final, self.passes = 0, 0
        if self.output_file is not None:
            open(self.output_file, "wb").close()

    def _view(self, comb):
        """One view of the pass (None: ``launch``, the next pass itself) -> the pass's run of decoded frames, stitched."""
        from . import ops
        c = self.corpus
        b, wf = c.batch_size, c.window_frames
        launch = c.launch if comb is None else (lambda out: c.launch_view(comb, out))
        _, _, dec = _forward_decode(launch, (b, c.n_samples, 4), self.model, self.features, self.postprocessor, self.forward)
        if dec.shape[0] != b * wf:
            raise ValueError("StreamInference: %d decoded frames from %d windows of %d label frames (the model's frame rate is "
                             "not the label hop's)" % (dec.shape[0], b, wf))
        if self._stitched is None:
            self._stitched = torch.empty_like(dec)
        ops.decode_stitch(dec, c.pass_table, wf, c.pass_base, self._stitched, c.status)
        return self._stitched[:c.pass_frames]

    def _pass(self, rows_out, ids_out):
        from . import ops
        c, tracker = self.corpus, self.tracker
        run = self._view(None)
        if tracker is not None:
            tracker.open = not c.pass_closing
        more = (self._view(v) for v in _further_views(self.merge))
        rows, counts, ids = _select_rows(self.postprocessor, run, more, self.merge, tracker, 1, self.csv is None)
        self.passes += 1
        base = c.pass_base if tracker is None else tracker.base
        n = counts.numel()
        if not n:                                                            # (a tracked pass may hold all its frames back)
            return
        self.frames_final = base + n
        if self.csv is not None:
            import numpy as np
            data, at = self.csv.fetch(rows, counts, np.asarray([[0, base]], dtype=np.int32), ids)
            self.csv.forget()                            # (one table per pass, used once: a stream has no end to plan for)
            if at[1] > at[0]:
                with open(self.output_file, "ab") as f:
                    f.write(data[at[0]:at[1]])
            return
        rows_h, counts_h, *ids_h = [t.numpy() for t in ops.to_host_many(*(t for t in (rows, counts, ids) if t is not None))]
        found = {base + f: v for f, v in group_rows(rows_h, counts_h, 1)[0].items()}
        found_ids = None
        if ids is not None:
            from .postprocess import track_groups
            found_ids = {base + f: v for f, v in track_groups(ids_h[0], counts_h, 1)[0].items()}
            ids_out.update(found_ids)
        rows_out.update(found)
        if self.output_file is not None and found:
            write_seld_output_file(self.output_file, found, found_ids, mode="a")

    def _run(self, closing, rows_out, ids_out):
        n = self.corpus.runnable(closing)
        with torch.no_grad():
            for _ in range(n):
                self._pass(rows_out, ids_out)
        return n

    def push(self, pcm):
        import numpy as np
        if torch.is_tensor(pcm):
            pcm = pcm.numpy()
        rows_out, ids_out = {}, ({} if self.tracker is not None else None)
        at, total = 0, int(np.shape(pcm)[0])
        while True:
            took = self.corpus.append(pcm[at:])
            at += took
            ran = self._run(False, rows_out, ids_out)
            if at >= total:
                return rows_out, ids_out
            if not took and not ran:                                         # (the ring's smallest size rules this out)
                raise RuntimeError("StreamInference.push: the ring is full and no window is runnable")

    def close(self):
        rows_out, ids_out = {}, ({} if self.tracker is not None else None)
        self._run(True, rows_out, ids_out)
        self.frames_final = self.corpus.frames
        _read_status(self.corpus, None, self.merge, self.tracker)
        return rows_out, ids_out
