"""DCASE SELD evaluation (ER / F / LE / LR / SELD score), host NumPy.

Mirror of ``ComputeSELDResults`` / ``SELDMetrics`` (/root/reference/src/utils/seld_metrics.py:188-519; itself adapted
from the DCASE challenge baseline, README.md:156): location-sensitive detection (20 degree threshold) and
class-sensitive localisation over 1-second segments with Hungarian track association, macro-averaged over classes.
This is the CPU evaluator that turns the CSV files written by ``test_epoch`` into the scores the reference prints; it is
host logic on tiny data, restated here so that SELD parity can be checked
without the reference.  Reference quirks kept: the number of frames of a recording is ``max(frame index)`` of its
reference CSV (seld_metrics.py:398); a class matched in no common frame books ``nb_pred`` (not ``nb_ref``) false
negatives (:339-342); LE of a class without matches is 180.
"""
import math
import os

import numpy as np
from scipy.optimize import linear_sum_assignment

EPS = np.finfo(float).eps


def load_output_format_file(path):
    """seld_metrics.py:13-33: rows ``frame,class,source,az,el`` (polar) or ``frame,class,source,x,y,z``."""
    out = {}
    with open(path, "r") as f:
        for line in f:
            w = line.strip().split(",")
            if len(w) < 5:
                continue
            out.setdefault(int(w[0]), []).append([int(w[1]), int(w[2])] + [float(v) for v in w[3:]])
    return out


def cartesian_to_polar(d):
    """seld_metrics.py:67-80."""
    out = {}
    for frame, vals in d.items():
        out[frame] = [[v[0], v[1], math.atan2(v[3], v[2]) * 180 / math.pi,
                       math.atan2(v[4], math.sqrt(v[2] ** 2 + v[3] ** 2)) * 180 / math.pi] for v in vals]
    return out


def _great_circle_deg(az1, el1, az2, el2):
    d = np.sin(el1) * np.sin(el2) + np.cos(el1) * np.cos(el2) * np.cos(np.abs(az1 - az2))
    return np.arccos(np.clip(d, -1, 1)) * 180 / np.pi


def segment(labels, max_frames, frames_per_block):
    """seld_metrics.py:478-519 -> {block: {class: {frame_in_block: [[src, az, el], ...]}}} (insertion ordered)."""
    nb_blocks = int(math.ceil(max_frames / float(frames_per_block)))
    out = {b: {} for b in range(nb_blocks)}
    for start in range(0, max_frames, frames_per_block):
        blk = out[start // frames_per_block]
        for fr in range(start, start + frames_per_block):
            for v in labels.get(fr, ()):
                blk.setdefault(v[0], {}).setdefault(fr - start, []).append(v[1:])
    return out


class SELDScorer:
    def __init__(self, nb_classes, doa_threshold=20.0):
        c = nb_classes
        self.nb_classes, self.thr = c, doa_threshold
        self.TP, self.FP, self.FP_spatial, self.FN, self.Nref = (np.zeros(c) for _ in range(5))
        self.total_DE, self.DE_TP, self.DE_FP, self.DE_FN = (np.zeros(c) for _ in range(4))
        self.S = self.D = self.I = 0

    def update(self, pred, ref):
        """pred / ref: outputs of ``segment`` for one recording (seld_metrics.py:289-395)."""
        for blk in range(len(ref)):
            loc_fn = loc_fp = 0
            pb, rb = pred.get(blk, {}), ref[blk]
            for c in range(self.nb_classes):
                n_ref = max(len(v) for v in rb[c].values()) if c in rb else None
                n_pred = max(len(v) for v in pb[c].values()) if c in pb else None
                if n_ref is not None:
                    self.Nref[c] += n_ref
                if c in rb and c in pb:
                    tracks = {}
                    for fr, ref_vals in rb[c].items():
                        if fr not in pb[c]:
                            continue
                        g = np.asarray(ref_vals, dtype=float)[:, 1:] * np.pi / 180.0
                        p = np.asarray(pb[c][fr], dtype=float)[:, 1:] * np.pi / 180.0
                        cost = _great_circle_deg(g[:, None, 0], g[:, None, 1], p[None, :, 0], p[None, :, 1])
                        ri, ci = linear_sum_assignment(cost)
                        for r, cc in zip(ri, ci):
                            tracks.setdefault(int(r), []).append(cost[r, cc])
                    if not tracks:
                        loc_fn += n_pred
                        self.FN[c] += n_pred
                        self.DE_FN[c] += n_pred
                    else:
                        for dists in tracks.values():
                            avg = sum(dists) / len(dists)
                            self.total_DE[c] += avg
                            self.DE_TP[c] += 1
                            if avg <= self.thr:
                                self.TP[c] += 1
                            else:
                                loc_fp += 1
                                self.FP_spatial[c] += 1
                        if n_pred > n_ref:
                            loc_fp += n_pred - n_ref
                            self.FP[c] += n_pred - n_ref
                            self.DE_FP[c] += n_pred - n_ref
                        elif n_pred < n_ref:
                            loc_fn += n_ref - n_pred
                            self.FN[c] += n_ref - n_pred
                            self.DE_FN[c] += n_ref - n_pred
                elif c in rb:
                    loc_fn += n_ref
                    self.FN[c] += n_ref
                    self.DE_FN[c] += n_ref
                elif c in pb:
                    loc_fp += n_pred
                    self.FP[c] += n_pred
                    self.DE_FP[c] += n_pred
            self.S += min(loc_fp, loc_fn)
            self.D += max(0, loc_fn - loc_fp)
            self.I += max(0, loc_fp - loc_fn)

    def accumulator(self):
        """The counts as one vector [9 * C + 3]: TP, FP, FP_spatial, FN, Nref, total_DE, DE_TP, DE_FP, DE_FN (C each), S, D, I
        -- the layout of ``DeviceSELDScorer``'s per-file accumulators."""
        return np.concatenate([self.TP, self.FP, self.FP_spatial, self.FN, self.Nref, self.total_DE, self.DE_TP, self.DE_FP,
                               self.DE_FN, np.asarray([self.S, self.D, self.I], dtype=float)])

    def scores(self):
        """Macro average (seld_metrics.py:260-287) -> ER, F, LE, LR, SELD, classwise (5, C)."""
        return macro_average(self.accumulator(), self.nb_classes)


def macro_average(acc, nb_classes):
    """ER, F, LE, LR, SELD (class macro averages) and the classwise table (5, C) of one accumulator vector
    (``SELDScorer.accumulator`` layout; seld_metrics.py:260-287)."""
    a = np.asarray(acc, dtype=np.float64)
    tp, fp, fp_spatial, fn, nref, total_de, de_tp, de_fp, de_fn = a[:9 * nb_classes].reshape(9, nb_classes)
    s, d, i = a[9 * nb_classes:9 * nb_classes + 3]
    er = (s + d + i) / (nref.sum() + EPS)
    f = tp / (EPS + tp + fp_spatial + 0.5 * (fp + fn))
    le = total_de / (de_tp + EPS)
    le[de_tp == 0] = 180.0
    lr = de_tp / (EPS + de_tp + de_fn)
    er_c = np.repeat(er, nb_classes)
    seld = np.mean([er_c, 1 - f, le / 180, 1 - lr], 0)
    classwise = np.array([er_c, f, le, lr, seld])
    return er, f.mean(), le.mean(), lr.mean(), seld.mean(), classwise


def jackknife_from_accumulators(acc, nb_classes):
    """``get_SELD_Results(..., is_jackknife=True)`` from per-file accumulators (n_files, 9 C + 3), one row per file in the
    order the host would visit the files: leave-one-file-out sums, the same intervals, and the reference quirk of
    ``ComputeSELDResults._jackknife`` (the point values are those of the LAST leave-one-out pass)."""
    acc = np.asarray(acc, dtype=np.float64)
    er, f, le, lr, seld, cw = macro_average(acc.sum(0), nb_classes)
    global_values = [er, f, le, lr, seld] + cw.reshape(-1).tolist()
    partial, last = [], None
    for k in range(len(acc)):
        last = macro_average(np.delete(acc, k, 0).sum(0), nb_classes)
        partial.append([last[0], last[1], last[2], last[3], last[4]] + last[5].reshape(-1).tolist())
    partial = np.asarray(partial)
    conf = [jackknife_estimation(global_values[i], partial[:, i], 0.05)[3] for i in range(len(global_values))]
    return ([last[0], conf[0]], [last[1], conf[1]], [last[2], conf[2]], [last[3], conf[3]], [last[4], conf[4]],
            [last[5], np.array(conf)[5:].reshape(5, nb_classes, 2)])


def jackknife_estimation(global_value, partial_estimates, significance_level=0.05):
    """seld_metrics.py:149-186: bias-corrected jackknife estimate, bias, standard error and the t-test confidence interval
    of a statistic from its leave-one-out estimates."""
    from scipy import stats
    partial_estimates = np.asarray(partial_estimates, dtype=float)
    mean_jack = np.mean(partial_estimates)
    n = len(partial_estimates)
    bias = (n - 1) * (mean_jack - global_value)
    std_err = np.sqrt((n - 1) * np.mean((partial_estimates - mean_jack) * (partial_estimates - mean_jack), axis=0))
    estimate = global_value - bias
    if not (0 < significance_level < 1):
        raise ValueError("confidence level must be in (0, 1).")
    t_value = stats.t.ppf(1 - significance_level / 2, n - 1)
    return estimate, bias, std_err, estimate + t_value * np.array((-std_err, std_err))


class ComputeSELDResults(object):
    """``ComputeSELDResults(params, ref_files_folder).get_SELD_Results(pred_files_path[, is_jackknife])`` like the reference
    (seld_metrics.py:374-476)."""

    def __init__(self, params, ref_files_folder=None):
        dc = params["data_config"]
        self._nb_classes = dc["nb_classes"]
        self._fpb = int(dc["sr"] / float(int(dc["sr"] * dc["label_hop_len_s"])))
        self._ref = {}
        for name in os.listdir(ref_files_folder):
            gt = load_output_format_file(os.path.join(ref_files_folder, name))
            nb = max(list(gt.keys()))
            self._ref[name] = (segment(gt, nb, self._fpb), nb)

    def _pred_labels(self, pred_files_path, name):
        """Segmented predictions of one file, or None when the file does not take part in this evaluation."""
        pred = cartesian_to_polar(load_output_format_file(os.path.join(pred_files_path, name)))
        return segment(pred, self._ref[name][1], self._fpb)

    def get_SELD_Results(self, pred_files_path, is_jackknife=False):
        scorer = SELDScorer(self._nb_classes, 20.0)
        kept = {}
        for name in os.listdir(pred_files_path):
            labels = self._pred_labels(pred_files_path, name)
            if labels is None:
                continue
            scorer.update(labels, self._ref[name][0])
            kept[name] = labels
        out = scorer.scores()
        if not is_jackknife:
            return out
        return self._jackknife(out, kept)

    def _jackknife(self, global_scores, kept):
        """Leave-one-file-out confidence intervals (seld_metrics.py:441-476 / :640-676).  Reference quirk kept: the point
        values returned next to the intervals are those of the LAST leave-one-out pass (the loop reuses the variable
        names of the global scores), not the global scores; the intervals themselves are built around the global ones."""
        er, f, le, lr, seld, cw = global_scores
        global_values = [er, f, le, lr, seld] + cw.reshape(-1).tolist()
        partial, last = [], global_scores
        names = list(kept.keys())
        for leave in names:
            scorer = SELDScorer(self._nb_classes, 20.0)
            for name in names:
                if name != leave:
                    scorer.update(kept[name], self._ref[name][0])
            last = scorer.scores()
            partial.append([last[0], last[1], last[2], last[3], last[4]] + last[5].reshape(-1).tolist())
        partial = np.asarray(partial)
        conf = [jackknife_estimation(global_values[i], partial[:, i], 0.05)[3] for i in range(len(global_values))]
        return ([last[0], conf[0]], [last[1], conf[1]], [last[2], conf[2]], [last[3], conf[3]], [last[4], conf[4]],
                [last[5], np.array(conf)[5:].reshape(5, self._nb_classes, 2)])


class ComputeSELDResultsFromEventOverlap(ComputeSELDResults):
    """Scores restricted to the reference frames with overlapping events (seld_metrics.py:522-717; printed by the
    reference's test.py:125-133 as "class-independent polyphony" and, with ``classwise_overlap_test=True``, as
    "class-homogenous polyphony"): a frame counts when it holds more than one event (or more than one event of the SAME
    class); reference files without such a frame are left out, predictions are cut down to those frames, the recording
    length stays ``max(frame index)`` of the full reference file."""

    def __init__(self, params, ref_files_folder=None, use_polar_format=True, classwise_overlap_test=False):
        if not use_polar_format:
            raise NotImplementedError("cartesian reference format (seld_metrics.py:547-548) is not used by the reference's callers")
        dc = params["data_config"]
        self._nb_classes = dc["nb_classes"]
        self._fpb = int(dc["sr"] / float(int(dc["sr"] * dc["label_hop_len_s"])))
        self._ref, self._ov_frames = {}, {}
        for name in os.listdir(ref_files_folder):
            gt = load_output_format_file(os.path.join(ref_files_folder, name))
            nb = max(list(gt.keys()))
            keep = {}
            for frame, events in gt.items():
                if classwise_overlap_test:
                    cnt = np.zeros(self._nb_classes)
                    for ev in events:
                        cnt[ev[0]] += 1
                    hit = cnt.max() > 1
                else:
                    hit = len(events) > 1
                if hit:
                    keep[frame] = events
            self._ov_frames[name] = list(keep.keys())
            if keep:
                self._ref[name] = (segment(keep, nb, self._fpb), nb)
        self.nb_overlap_files = len(self._ref)
        self.nb_overlap_frames = sum(len(v) for v in self._ov_frames.values())

    def _pred_labels(self, pred_files_path, name):
        if name not in self._ref:
            return None
        pred = cartesian_to_polar(load_output_format_file(os.path.join(pred_files_path, name)))
        pred = {fr: pred[fr] for fr in self._ov_frames[name] if fr in pred}
        return segment(pred, self._ref[name][1], self._fpb)


def overlap_frames(gt, nb_classes, classwise_overlap_test=False):
    """The frames of a reference {frame: events} that ``ComputeSELDResultsFromEventOverlap`` keeps, in dict order: more than
    one event, or (classwise_overlap_test) more than one event of the same class."""
    keep = []
    for frame, events in gt.items():
        if classwise_overlap_test:
            cnt = np.zeros(nb_classes)
            for ev in events:
                cnt[ev[0]] += 1
            hit = cnt.max() > 1
        else:
            hit = len(events) > 1
        if hit:
            keep.append(frame)
    return keep


MAX_REF_PER_FRAME_CLASS = 8                       # ADYOLO_SELD_MAX_REF


def pack_reference(refs, nb_classes, frames_per_block, keep_frames=None):
    """Reference files -> the host arrays of the device table (adyolo_hip.h, ``adyolo_seld_score``).
    refs: [(gt {frame: [[class, source, az, el], ...]}, length)], length = max(frame index) of the full file.
    keep_frames: None, or per file the frames whose events (and predictions) are scored.
    -> dict of file_info (n_files, 2) int32 [first table frame, blocks], ref_off (frames * C + 1,) int32, ref_ev (n, 3)
    float64 [az rad, sin el, cos el], keep (frames,) int32 or None.  Only frames < blocks * frames_per_block are held, blocks =
    ceil(length / frames_per_block): the last started block is complete, later frames are not scored (``segment``).  Raises
    ValueError for more than MAX_REF_PER_FRAME_CLASS events of one class in one scored frame."""
    c = nb_classes
    info, keys, ang, keep = [], [], [], []
    base = 0
    for k, (gt, length) in enumerate(refs):
        blocks = int(math.ceil(length / float(frames_per_block)))
        n = blocks * frames_per_block
        kept = None if keep_frames is None else set(keep_frames[k])
        if keep_frames is not None:
            m = np.zeros(n, dtype=np.int32)
            for fr in kept:
                if 0 <= fr < n:
                    m[fr] = 1
            keep.append(m)
        for fr in range(n):
            if kept is not None and fr not in kept:
                continue
            for ev in gt.get(fr, ()):
                if 0 <= int(ev[0]) < c:
                    keys.append((base + fr) * c + int(ev[0]))
                    ang.append(ev[-2:])
        info.append((base, blocks))
        base += n
    keys = np.asarray(keys, dtype=np.int64)
    cnt = np.bincount(keys, minlength=base * c) if len(keys) else np.zeros(base * c, dtype=np.int64)
    if len(cnt) and cnt.max() > MAX_REF_PER_FRAME_CLASS:
        cell = int(np.argmax(cnt))
        raise ValueError("device SELD scoring: %d reference events of class %d in one frame, at most %d"
                         % (int(cnt.max()), cell % c, MAX_REF_PER_FRAME_CLASS))
    order = np.argsort(keys, kind="stable")                         # frame, class; reference order within them
    deg = np.asarray(ang, dtype=np.float64).reshape(-1, 2)[order]
    rad = deg * np.pi / 180.0                                       # what SELDScorer.update does to the reference angles
    ev = np.stack([rad[:, 0], np.sin(rad[:, 1]), np.cos(rad[:, 1])], axis=1) if len(rad) else np.zeros((0, 3))
    off = np.zeros(base * c + 1, dtype=np.int64)
    off[1:] = np.cumsum(cnt)
    if keep_frames is not None:
        keep = np.concatenate(keep).astype(np.int32) if keep else np.zeros(0, dtype=np.int32)
    return {"file_info": np.asarray(info, dtype=np.int32).reshape(-1, 2), "ref_off": off.astype(np.int32),
            "ref_ev": np.ascontiguousarray(ev, dtype=np.float64), "keep": keep if keep_frames is not None else None}


def run_segments(label_frames, bounds):
    """Recordings of ``label_frames`` frames each, laid end to end on one frame axis, scored in runs: run p holds the frames
    [bounds[p], bounds[p + 1]) of that axis (bounds ascending from 0 to the total: the pass boundaries of a windowed
    evaluation) -> per run an int64 array (S, 5) of {recording, f0, r0, n, last}: the recordings the run holds frames of, in
    order -- f0 the first of them on the recording's own axis, r0 its place in the run, n their number, last = 1 when the run
    holds the recording's final frame.  A recording without any frame gets one row {r, 0, r0, 0, 1} in the run that holds the
    next recording's first frame, or in the last run when no frame follows.  Every recording has exactly one last row."""
    frames = np.asarray(label_frames, dtype=np.int64).reshape(-1)
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1)
    start = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    if len(bounds) < 2 or bounds[0] != 0 or bounds[-1] != start[-1] or (np.diff(bounds) <= 0).any() or (frames < 0).any():
        raise ValueError("run_segments: bounds %s do not cut the %d frames of the recordings into runs"
                         % (bounds.tolist(), int(start[-1])))
    out = []
    for p in range(len(bounds) - 1):
        lo, hi = int(bounds[p]), int(bounds[p + 1])
        final = p == len(bounds) - 2
        rows = []
        # the recordings that start before the run's end and end after its start, and the empty ones that start inside it
        for r in range(int(np.searchsorted(start[1:], lo, "left")), len(frames)):
            s, e = int(start[r]), int(start[r + 1])
            if s >= hi and not (final and s == e == hi):
                break
            if s == e:
                if lo <= s < hi or (final and s == hi):
                    rows.append((r, 0, s - lo, 0, 1))
            elif e > lo:
                a, b = max(s, lo), min(e, hi)
                rows.append((r, a - s, a - lo, b - a, int(b == e)))
        out.append(np.asarray(rows, dtype=np.int64).reshape(-1, 5))
    return out


class SELDRefTable:
    """A packed reference table (``pack_reference``) on a device, the ``table`` argument of ``ops.seld_score``."""

    def __init__(self, packed, nb_classes, frames_per_block, device, doa_threshold=20.0):
        import torch
        self.nb_classes, self.frames_per_block, self.doa_threshold = nb_classes, frames_per_block, doa_threshold
        self.n_files = len(packed["file_info"])
        self.max_blocks = max(1, int(packed["file_info"][:, 1].max()) if self.n_files else 1)

        def up(a, dtype):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(device=device, dtype=dtype)
        self.file_info = up(packed["file_info"], torch.int32)
        self.ref_off = up(packed["ref_off"], torch.int32)
        self.ref_ev = up(packed["ref_ev"], torch.float64)
        self.keep = None if packed["keep"] is None else up(packed["keep"], torch.int32)


class DeviceSELDScorer:
    """``ComputeSELDResults`` (overlap=None) or ``ComputeSELDResultsFromEventOverlap`` (overlap="polyphony": frames with more
    than one event; "homogenous": more than one event of one class) on the device (csrc/seld.hip, ``ops.seld_score``): the
    reference CSVs are parsed and uploaded once; predictions are added as device rows (``add_rows``, what
    ``LabelPostProcessor.select_device_rows`` returns) or host dicts (``add_dict``) into per-file float64 accumulators on the
    device; ``scores()`` copies them once and returns what ``get_SELD_Results`` returns on the CSV files of the same rows.
    Every added file counts, rows or not (an empty CSV file); a file added twice counts twice.  Names without a reference
    raise KeyError (overlap=None) or are skipped (the overlap variants), like the host; the overlap variants also skip the
    files without overlapping frames.  A skipped clip of an ``add_rows`` batch is scored against an empty table entry that
    nothing reads."""

    def __init__(self, params, ref_files_folder, device="cuda:0", overlap=None):
        if overlap not in (None, "polyphony", "homogenous"):
            raise ValueError("overlap must be None, 'polyphony' or 'homogenous' (got %r)" % (overlap,))
        dc = params["data_config"]
        self.nb_classes = c = dc["nb_classes"]
        self._fpb = int(dc["sr"] / float(int(dc["sr"] * dc["label_hop_len_s"])))
        self.overlap, self.device = overlap, device
        refs, keeps, self.names = [], [], []
        n_ov_frames = 0
        for name in os.listdir(ref_files_folder):
            gt = load_output_format_file(os.path.join(ref_files_folder, name))
            nb = max(list(gt.keys()))
            if overlap is not None:
                kept = overlap_frames(gt, c, overlap == "homogenous")
                n_ov_frames += len(kept)
                if not kept:
                    continue
                keeps.append(kept)
            refs.append((gt, nb))
            self.names.append(name)
        if overlap is not None:
            self.nb_overlap_files, self.nb_overlap_frames = len(self.names), n_ov_frames
        self._index = {name: k for k, name in enumerate(self.names)}
        self._skip = len(self.names)                               # the empty entry: no blocks, never counted
        refs.append(({}, 0))
        keeps.append([])
        packed = pack_reference(refs, c, self._fpb, keeps if overlap is not None else None)
        self._frames = (packed["file_info"][:, 1].astype(np.int64) * self._fpb).tolist()
        self.table = SELDRefTable(packed, c, self._fpb, device)
        self._ids = {}
        self.reset()

    def reset(self):
        """Forget every added file."""
        import torch
        self._acc = torch.zeros(self.table.n_files, 9 * self.nb_classes + 3, dtype=torch.float64, device=self.device)
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._order = []                                           # file indices, each once, in the order first added

    def _lookup(self, name):
        """Table index of a prediction file name (with or without .csv); the empty entry for a file the overlap variants skip."""
        key = name if name.endswith(".csv") else name + ".csv"
        if key not in self._index:
            if self.overlap is None:
                raise KeyError(key)
            return self._skip
        return self._index[key]

    def _score(self, rows, counts, ids, t_clip):
        import torch
        from . import ops
        key = tuple(ids)
        dev = self._ids.get(key)
        if dev is None:
            if len(self._ids) >= 64:
                self._ids.clear()
            dev = self._ids[key] = torch.tensor(ids, dtype=torch.int32).to(self.device, non_blocking=True)
        ops.seld_score(rows, counts, self.table, dev, t_clip, self._acc, self._status)
        seen = set(self._order)
        for k in ids:
            if k != self._skip and k not in seen:
                self._order.append(k)
                seen.add(k)

    def add_rows(self, rows, counts, names):
        """rows (N, 5) [frame, class, x, y, z] and counts (len(names) * T',) int32 on the device for len(names) clips of T'
        frames (names as ``FoaDataset.get_filelist()`` gives them); rows past counts.sum() are not read.  No synchronisation."""
        ids = [self._lookup(n) for n in names]
        if not names or counts.numel() % len(names):
            raise ValueError("add_rows: %d frame counts for %d clips" % (counts.numel(), len(names)))
        self._score(rows, counts.reshape(-1), ids, counts.numel() // len(names))

    def segment_tables(self, names, label_frames, bounds):
        """The segment tables of a windowed evaluation (``run_segments``) for THIS scorer's reference table: recordings
        ``names`` (as ``get_filelist()`` gives them) of ``label_frames`` frames each, scored in runs cut at ``bounds`` -> one
        table per run for ``add_run``, uploaded here, once.  Names go through ``_lookup``: one without a reference raises
        KeyError (overlap=None) or maps to the empty entry (the overlap variants), as in ``add_rows``."""
        import torch
        ids = [self._lookup(n) for n in names]
        if len(ids) != len(label_frames):
            raise ValueError("segment_tables: %d names for %d recordings" % (len(ids), len(label_frames)))
        fpb, tables = self._fpb, []
        for seg in run_segments(label_frames, bounds):
            rows = np.zeros((len(seg), 8), dtype=np.int32)                 # ADYOLO_SELD_RUN_WORDS
            rows[:, 0] = [ids[r] for r in seg[:, 0].tolist()]
            rows[:, 1:5] = seg[:, 1:5]
            blocks = np.asarray([self._frames[k] // fpb for k in rows[:, 0].tolist()], dtype=np.int64)
            b1 = np.where(seg[:, 4] != 0, blocks, np.minimum((seg[:, 1] + seg[:, 3]) // fpb, blocks))
            seg_blocks = max(1, int((b1 - seg[:, 1] // fpb).max())) if len(seg) else 1
            dev = torch.from_numpy(rows).to(self.device) if len(seg) else None
            tables.append((dev, seg_blocks, rows[:, 0].tolist()))
        return tables

    def add_run(self, rows, counts, segments):
        """rows (N, 5) and counts (run frames,) int32 on the device for ONE stitched run of frames (``select_device_rows(run, 1,
        trim=False)``) and the run's entry of ``segment_tables``: every segment's blocks are added to its file's accumulators
        (``ops.seld_score_runs``); a file whose ordered segments have all been added holds the bits ``add_rows`` on the whole
        recording leaves.  No synchronisation."""
        from . import ops
        dev, seg_blocks, ids = segments
        if dev is None:
            return
        ops.seld_score_runs(rows, counts.reshape(-1), self.table, dev, seg_blocks, self._acc, self._status)
        seen = set(self._order)
        for k in ids:
            if k != self._skip and k not in seen:
                self._order.append(k)
                seen.add(k)

    def add_dict(self, name, labels):
        """Host rows {frame: [[class, x, y, z], ...]} of one file (what ``LabelPostProcessor.select`` returns); uploaded in
        float64, so they score exactly as the CSV file of the same rows would."""
        import torch
        k = self._lookup(name)
        if k == self._skip:
            return
        t = max(1, self._frames[k])
        frames = sorted(int(fr) for fr in labels if 0 <= int(fr) < t)
        counts = np.zeros(t, dtype=np.int32)
        vals = []
        for fr in frames:
            counts[fr] = len(labels[fr])
            vals.extend([float(fr)] + [float(v) for v in r[:4]] for r in labels[fr])
        rows = torch.from_numpy(np.asarray(vals, dtype=np.float64).reshape(-1, 5)).to(self.device)
        self._score(rows, torch.from_numpy(counts).to(self.device), [k], t)

    def accumulators(self):
        """(files added, 9 C + 3) float64 on the host, one row per file in the order first added, and their names.  Raises
        ``AdyoloHipError`` when a call has failed on the device (e.g. more than 1024 predictions of one frame and class)."""
        from . import ops
        ops.seld_status_check(self._status)
        acc = ops.to_host(self._acc).numpy()
        return acc[self._order].copy(), [self.names[k] for k in self._order]

    def scores(self, is_jackknife=False):
        """What ``get_SELD_Results(pred_folder, is_jackknife)`` returns for the added files (jackknife: files left out in the
        order they were first added)."""
        acc, _ = self.accumulators()
        if is_jackknife:
            return jackknife_from_accumulators(acc, self.nb_classes)
        return macro_average(acc.sum(0), self.nb_classes)
