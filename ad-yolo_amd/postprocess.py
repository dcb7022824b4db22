"""Inference post-processing of the AD-YOLO output: decode (GPU kernel) -> confidence / class thresholds -> per-class
connectivity soft-merge NMS (host) -> {frame: [[class, x, y, z], ...]} and the DCASE CSV writer.

Mirror of ``LabelPostProcessor`` for ``--loss adyolo`` (/root/reference/src/datasets.py:485-534, ``get_yolo_output``
:741-855, helpers :858-919) and ``write_seld_output_file`` (/root/reference/src/test.py:26-30).  The decode is the same
arithmetic as the loss (csrc/loss.hip ``yolo_decode_kernel``); the NMS is tiny, data dependent and stays on the host
(NumPy float32), exactly where the reference runs it (``postprocessor.postprocess(output.detach().cpu())``, test.py:52).
Like the reference it handles one clip at a time (B = 1, datasets.py:752-753).  Opt-in, ``select_device`` /
``postprocess(on_device=True)`` run the thresholds and the NMS on the GPU too (csrc/select.hip ``adyolo_yolo_select``, the same
rows in the same order) and copy only the selected rows to the host.

The class-wise heads (``--loss seddoa | masked-seddoa | accdoa | adpit``, ``get_seddoa_output`` / ``get_accdoa_output`` /
``get_adpit_output``, datasets.py:536-739) follow the same split: a threshold-free GPU decode (csrc/losses.hip
``adyolo_classwise_decode``: per (frame, class) the track activities, their xyz and, for adpit, the pair distances), then a
vectorised host ``select`` per threshold (``classwise_select``).  Opt-in here too, ``select_device`` /
``postprocess(on_device=True)`` run the thresholds and the ADPIT unification on the GPU (csrc/select.hip
``adyolo_classwise_select``: the same rows, bit for bit) and copy only the selected rows to the host.
"""
import math

import numpy as np

F32 = np.float32


def _ang_dist_deg(a, b):
    """datasets.py:858-871 (acos argument clipped to [-1, 1])."""
    a, b = np.deg2rad(a).astype(F32), np.deg2rad(b).astype(F32)
    d = np.sin(a[..., 1]) * np.sin(b[..., 1]) + np.cos(a[..., 1]) * np.cos(b[..., 1]) * np.cos(np.abs(a[..., 0] - b[..., 0]))
    return np.rad2deg(np.arccos(np.clip(d, -1, 1))).astype(F32)


def _to_xyz(uv):
    r = np.deg2rad(uv).astype(F32)
    return np.stack([np.cos(r[:, 0]) * np.cos(r[:, 1]), np.sin(r[:, 0]) * np.cos(r[:, 1]), np.sin(r[:, 1])], axis=1).astype(F32)


def _single(rows):
    """datasets.py:874-890: rows [cls, conf, U, V] -> [cls, x, y, z]."""
    return np.concatenate([rows[:, :1], _to_xyz(rows[:, 2:4])], axis=1)


def _voted(rows, thresh):
    """datasets.py:893-919: confidence-weighted vote of one cluster (weights = softmax(exp(conf^2 / thresh)))."""
    e = np.exp(rows[:, 1].astype(F32) ** 2 / F32(thresh)).astype(F32)
    w = np.exp(e - e.max())
    w = (w / w.sum()).astype(F32)
    v = (_to_xyz(rows[:, 2:4]) * w[:, None]).sum(axis=0, keepdims=True)
    v = v / np.sqrt((v ** 2).sum())
    return np.concatenate([rows[:1, :1], v.astype(F32)], axis=1)


def nms_frame(det, nms, unify_thresh, clss_thresh):
    """det: (K, 4) [class, class_conf, U, V] sorted by descending class_conf -> list of [class, x, y, z]."""
    out = []
    for cls in np.unique(det[:, 0]):
        rows = det[det[:, 0] == cls]
        if len(rows) == 1:
            out.append(_single(rows))
            continue
        if nms == "conn-merge":
            dist = _ang_dist_deg(rows[None, :, 2:4].repeat(len(rows), 0), rows[:, None, 2:4].repeat(len(rows), 1))
            ref = dist < unify_thresh
            while rows.shape[0]:
                prev = np.zeros(len(rows), dtype=bool)
                cur = ref[0].copy()
                while not (prev == cur).all():
                    if cur.sum() == 1:
                        break
                    prev = cur.copy()
                    cur |= ref[cur].sum(axis=0).astype(bool)
                out.append(_voted(rows[cur], clss_thresh))
                rows = rows[~cur]
                ref = ref[~cur][:, ~cur]
        elif nms == "soft-merge":
            reference = rows.copy()
            while rows.shape[0]:
                d = _ang_dist_deg(rows[:1, 2:4], reference[:, 2:4])
                out.append(_voted(reference[d <= unify_thresh], clss_thresh))
                if len(rows) == 1:
                    break
                d = _ang_dist_deg(rows[:1, 2:4], rows[1:, 2:4])
                rows = rows[1:][d > unify_thresh]
        else:
            while rows.shape[0]:
                out.append(_single(rows[:1]))
                if len(rows) == 1:
                    break
                d = _ang_dist_deg(rows[:1, 2:4], rows[1:, 2:4])
                rows = rows[1:][d > unify_thresh]
    return np.concatenate(out, axis=0).tolist() if out else []


def nms_decoded(decoded, nb_classes, conf_thresh, clss_thresh, unify_thresh, nms="conn-merge"):
    """decoded: (T, Gaz, Gel, A, C+3) float32 [conf, class_conf x C, U, V] -> {frame: [[class, x, y, z], ...]}."""
    t = decoded.shape[0]
    flat = np.asarray(decoded, dtype=F32).reshape(t, -1, nb_classes + 3)
    out = {}
    for frame in range(t):
        fo = flat[frame]
        fo = fo[fo[:, 0] > conf_thresh]
        if len(fo) == 0:
            continue
        i, j = np.nonzero(fo[:, 1:nb_classes + 1] > clss_thresh)
        det = np.concatenate([j.astype(F32)[:, None], fo[:, 1:nb_classes + 1][i, j][:, None], fo[i, -2:]], axis=1)
        det = det[np.argsort(-det[:, 1], kind="stable")]
        res = nms_frame(det, nms, unify_thresh, clss_thresh)
        if len(res):
            out[frame] = res
    return out


CLASSWISE = ("seddoa", "masked-seddoa", "accdoa", "adpit")


def _above(act, thresh):
    """The reference's double test: ``sed = act > thresh`` and then ``sed[f][c] > thresh`` on the BOOLEAN (True counts as 1),
    so a threshold >= 1 keeps nothing that passes through it."""
    return (act > thresh).astype(F32) > thresh


def classwise_select(decoded, loss, conf_thresh, unify_thresh=None):
    """Host half of the class-wise post-processing on a decode [T][C][rec] (``adyolo_classwise_decode``) ->
    {frame: [[class, x, y, z], ...]}: frames ascending, classes ascending, and for adpit within one class the case order of
    ``get_adpit_output`` (datasets.py:661-739).  Two tracks are one event when both are active (activity > conf_thresh) and
    their angular distance is below unify_thresh; per class:
      * no such pair: every active track (double test), in track order;
      * exactly one pair: the third track (double test), then the mean of the pair, (a + b) / 2;
      * two or three pairs: the mean of all three, ((a + b) + c) / 3.
    The means are float32, like the reference's arithmetic on the float32 output."""
    dec = np.asarray(decoded, dtype=F32)
    t, c = dec.shape[0], dec.shape[1]
    if loss != "adpit":
        keep = _above(dec[..., 0], conf_thresh)
        rows = np.concatenate([np.broadcast_to(np.arange(c, dtype=F32)[None, :, None], (t, c, 1)), dec[..., 1:4]], axis=-1)
        fr, cl = np.nonzero(keep)
        return _group(fr, rows[fr, cl])
    act, xyz, dist = dec[..., 0:3], dec[..., 3:12].reshape(t, c, 3, 3), dec[..., 12:15]
    sed = act > conf_thresh
    q = _above(act, conf_thresh)
    pair = np.stack([sed[..., 0] & sed[..., 1], sed[..., 1] & sed[..., 2], sed[..., 2] & sed[..., 0]], -1) & (dist < unify_thresh)
    n = pair.sum(-1)
    one = n == 1
    p01, p12, p20 = (pair[..., k] & one for k in range(3))
    a, b, d = xyz[..., 0, :], xyz[..., 1, :], xyz[..., 2, :]
    # up to three rows per (frame, class), in the reference's order: slot 0, slot 1, slot 2
    slot_ok = np.zeros((t, c, 3), dtype=bool)
    slot_xyz = np.zeros((t, c, 3, 3), dtype=F32)
    zero = n == 0
    slot_ok[..., 0] = (zero & q[..., 0]) | (p01 & q[..., 2]) | (p12 & q[..., 0]) | (p20 & q[..., 1]) | (n >= 2)
    slot_xyz[..., 0, :] = np.select([zero[..., None] | p12[..., None], p01[..., None], p20[..., None]], [a, d, b],
                                    ((a + b) + d) / F32(3))
    slot_ok[..., 1] = (zero & q[..., 1]) | one
    slot_xyz[..., 1, :] = np.select([zero[..., None], p01[..., None], p12[..., None]], [b, (a + b) / F32(2), (b + d) / F32(2)],
                                    (d + a) / F32(2))
    slot_ok[..., 2] = zero & q[..., 2]
    slot_xyz[..., 2, :] = d
    fr, cl, sl = np.nonzero(slot_ok)
    rows = np.concatenate([cl.astype(F32)[:, None], slot_xyz[fr, cl, sl]], axis=1)
    return _group(fr, rows)


def _group(frames, rows):
    """rows (N, 4) float32 with ascending ``frames`` (N,) -> {frame: [[class, x, y, z], ...]}."""
    out = {}
    if len(frames) == 0:
        return out
    starts = np.flatnonzero(np.r_[True, frames[1:] != frames[:-1]])
    ends = np.r_[starts[1:], len(frames)]
    vals = rows.tolist()
    for s, e in zip(starts.tolist(), ends.tolist()):
        out[int(frames[s])] = vals[s:e]
    return out


def group_rows(rows, counts, n_clips=1):
    """Host half of ``LabelPostProcessor.select_device``: rows (N, 5) [frame, class, x, y, z] in frame order and counts
    (frames,) rows per frame, frames = n_clips * T' clip after clip -> one {frame of the clip: [[class, x, y, z], ...]} per
    clip, the shape ``select`` returns."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    rows = np.asarray(rows, dtype=F32).reshape(-1, 5)
    if n_clips < 1 or len(counts) % n_clips or int(counts.sum()) != len(rows):
        raise ValueError("group_rows: %d rows, %d frame counts summing to %d, %d clips"
                         % (len(rows), len(counts), int(counts.sum()), n_clips))
    t = len(counts) // n_clips
    ends = np.cumsum(counts)
    frames = np.flatnonzero(counts)
    clip, local = np.divmod(frames, max(t, 1))
    vals = rows[:, 1:].tolist()
    outs = [{} for _ in range(n_clips)]
    for c, f, s, e in zip(clip.tolist(), local.tolist(), (ends[frames] - counts[frames]).tolist(), ends[frames].tolist()):
        outs[c][f] = vals[s:e]
    return outs


# ---- Rotation test-time augmentation: the host definition of csrc/select.hip ``adyolo_tta_collect`` / ``adyolo_tta_merge``.
TTA_ROWS_OVERFLOW, TTA_CAND_OVERFLOW, TTA_BAD_VECTOR, TTA_BAD_ROWS = 1, 2, 4, 8     # ADYOLO_TTA_* in adyolo_hip.h
TTA_MAX_CANDIDATES = 1024                                                          # ADYOLO_SELECT_MAX_N


def tta_cos(unify_thresh):
    """The membership threshold of ``merge_view_rows``: float32(cos(radians(unify_thresh))), computed once on the host."""
    return F32(math.cos(math.radians(float(unify_thresh))))


def _norm3(v):
    """sqrt((x*x + y*y) + z*z) of float32 rows (N, 3), every operation rounded."""
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def _merge_frame(cls, view, p, cos_t, min_views):
    """The merged rows [[class, x, y, z], ...] of one frame and its status bits.  cls (N,) float32, view (N,) view index,
    p (N, 3) float32 vectors already turned back, in candidate order."""
    status = 0
    with np.errstate(all="ignore"):
        norm = _norm3(p)
        good = np.isfinite(norm) & (norm > 0)
        if not good.all():
            status |= TTA_BAD_VECTOR
        cls, view = cls[good], view[good]
        u = (p[good] / norm[good, None]).astype(F32)
    out = []
    for c in np.unique(cls):
        idx = np.flatnonzero(cls == c)
        if len(idx) > TTA_MAX_CANDIDATES:
            status |= TTA_CAND_OVERFLOW
            continue
        uc, vc = u[idx], view[idx]
        near = ((uc[:, None, 0] * uc[None, :, 0] + uc[:, None, 1] * uc[None, :, 1]) + uc[:, None, 2] * uc[None, :, 2]) > cos_t
        cluster = np.full(len(idx), -1)
        n_clusters = 0
        for seed in range(len(idx)):
            if cluster[seed] >= 0:
                continue
            cluster[seed] = n_clusters
            front = [seed]
            while front:                                           # breadth first; the component does not depend on the order
                reach = near[front].any(axis=0) & (cluster < 0)
                cluster[reach] = n_clusters
                front = np.flatnonzero(reach).tolist()
            n_clusters += 1
        for k in range(n_clusters):
            memb = np.flatnonzero(cluster == k)
            if len(set(vc[memb].tolist())) < min_views:
                continue
            s = np.cumsum(uc[memb], axis=0, dtype=F32)[-1:]        # a running float32 sum, in candidate order
            with np.errstate(all="ignore"):
                out.append([float(c)] + (s[0] / _norm3(s)[0]).astype(F32).tolist())
    return out, status


def merge_view_rows(per_view, views, unify_thresh, min_views=None, max_rows_per_frame=None):
    """Rotation test-time augmentation, the host definition: the selections of the SAME clips under the combinations ``views``
    (``augmentations.COMBINATIONS``; view 0 the unrotated clip) -> one selection and the status bits of the call.

    per_view: one selection per view, either {frame: [[class, x, y, z], ...]} (what ``select`` returns; the result is such a
    dict) or (rows (N, 5) [frame, class, x, y, z], counts (frames,)) arrays (what ``select_device_rows`` returns; the result is
    such a pair, float32 rows and int32 counts).  Everything is float32, every operation rounded (no contraction):
      * candidates of a (frame, class): views ascending, within a view the order its selection wrote them; a view gives at most
        ``max_rows_per_frame`` rows per frame (None: all), its first ones (``TTA_ROWS_OVERFLOW``);
      * a candidate's vector is p = M^T xyz, M = ``augmentations.view_matrix(view)`` (p_i = M[j][i] * xyz[j] for the one j with
        M[j][i] != 0: exact); u = p / sqrt((px*px + py*py) + pz*pz); a zero or non-finite norm drops it (``TTA_BAD_VECTOR``);
      * two candidates are neighbours when (ua.x*ub.x + ua.y*ub.y) + ua.z*ub.z > ``tta_cos(unify_thresh)``; the clusters are
        the connected components, seeded at the lowest unassigned candidate and written in seed order (``nms_frame``'s
        conn-merge discipline); more than ``TTA_MAX_CANDIDATES`` candidates leave the (frame, class) empty
        (``TTA_CAND_OVERFLOW``);
      * a cluster is kept when at least ``min_views`` (default a majority, (V + 1) // 2) DISTINCT views have a member in it;
        its row is [class, s / |s|], s the members' u summed in candidate order, |s| by the expression above.
    Frames ascend, classes ascend within a frame, clusters come in seed order within a class."""
    from .augmentations import view_matrix
    n_views = len(views)
    if n_views < 1 or len(per_view) != n_views:
        raise ValueError("merge_view_rows: %d selections for %d views" % (len(per_view), n_views))
    min_views = (n_views + 1) // 2 if min_views is None else int(min_views)
    if not 1 <= min_views <= n_views:
        raise ValueError("merge_view_rows: min_views %d with %d views" % (min_views, n_views))
    arrays = not isinstance(per_view[0], dict)
    n_frames = None
    if arrays:
        n_frames = len(np.asarray(per_view[0][1]).reshape(-1))
        per_view = [group_rows(np.asarray(r, dtype=F32).reshape(-1, 5)[:int(np.asarray(c).sum())], c)[0] for r, c in per_view]
    turn = []                                                      # per view: the source axis and the sign of each component
    for v in views:
        m = view_matrix(v)
        src = np.abs(m).argmax(axis=0)
        turn.append((src, m[src, np.arange(3)].astype(F32)))
    cos_t = tta_cos(unify_thresh)
    status, out = 0, {}
    for frame in sorted(set().union(*[set(d) for d in per_view])):
        cls, view, vec = [], [], []
        for k, d in enumerate(per_view):
            rows = np.asarray(d.get(frame, []), dtype=F32).reshape(-1, 4)
            if max_rows_per_frame is not None and len(rows) > max_rows_per_frame:
                status |= TTA_ROWS_OVERFLOW
                rows = rows[:max_rows_per_frame]
            src, sign = turn[k]
            cls.append(rows[:, 0])
            view.append(np.full(len(rows), k))
            vec.append(rows[:, 1:4][:, src] * sign[None, :])
        merged, bits = _merge_frame(np.concatenate(cls), np.concatenate(view), np.concatenate(vec).astype(F32), cos_t, min_views)
        status |= bits
        if merged:
            out[frame] = merged
    if not arrays:
        return out, status
    counts = np.zeros(n_frames, dtype=np.int32)
    rows = []
    for frame in sorted(out):
        counts[frame] = len(out[frame])
        rows += [[float(frame)] + r for r in out[frame]]
    return (np.asarray(rows, dtype=F32).reshape(-1, 5), counts), status


# ---- Tracks: the host definition of csrc/track.hip ``adyolo_track_rows``.
TRACK_DET_OVERFLOW, TRACK_SLOT_OVERFLOW, TRACK_BAD_VECTOR, TRACK_BAD_ROWS = 1, 2, 4, 8     # ADYOLO_TRACK_* in adyolo_hip.h
TRACK_SLOTS = 8                                                    # ADYOLO_TRACK_SLOTS: concurrent tracks per clip and class
TRACK_MAX_DET = 64                                                 # ADYOLO_TRACK_MAX_DET: detections per frame and class


def track_cos(gate_deg):
    """The association gate of ``track_rows``: float32(cos(radians(gate_deg))), computed once on the host."""
    return F32(math.cos(math.radians(float(gate_deg))))


def _unit3(v):
    """v / sqrt((x*x + y*y) + z*z) of one float32 vector, every operation rounded."""
    return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def track_candidates(rows, counts, nb_classes):
    """Step 1 of ``track_rows``: {(frame, class): unit vectors (n <= TRACK_MAX_DET, 3) in row order} and the status bits.
    frame is the index on the counts axis; the rows' own frame column is not read."""
    rows = np.asarray(rows, dtype=F32).reshape(-1, 5)
    counts = np.asarray(counts).astype(np.int64).reshape(-1)
    offs = np.cumsum(counts) - counts
    bad = (counts < 0) | (offs < 0) | (offs + counts > len(rows))  # such a frame has no rows
    status = TRACK_BAD_ROWS if bad.any() else 0
    cand = {}
    for f in np.flatnonzero(~bad & (counts > 0)).tolist():
        r = rows[offs[f]:offs[f] + counts[f]]
        cls = r[:, 1]
        with np.errstate(all="ignore"):
            ok = (cls >= 0) & (cls < nb_classes) & (cls == np.floor(cls))
        if not ok.all():                                           # no (frame, class) owns such a row
            status |= TRACK_BAD_ROWS
        for c in np.unique(cls[ok]).tolist():
            p = r[cls == c][:, 2:5]
            if len(p) > TRACK_MAX_DET:
                status |= TRACK_DET_OVERFLOW
                p = p[:TRACK_MAX_DET]
            with np.errstate(all="ignore"):
                norm = _norm3(p)
                good = np.isfinite(norm) & (norm > 0)
                if not good.all():
                    status |= TRACK_BAD_VECTOR
                u = (p[good] / norm[good, None]).astype(F32)
            if len(u):
                cand[(f, int(c))] = u
    return cand, status


def track_rows(rows, counts, n_clips, nb_classes, gate_deg, max_gap, min_len, smooth, trace=None):
    """Link selected rows into tracks across frames, the host definition (csrc/track.hip matches it bit for bit): rows (N, 5)
    [frame, class, x, y, z] and counts (n_clips * T',) rows per frame, clip after clip (``select_device_rows`` /
    ``merge_view_rows``) -> ((rows', counts'), track_ids (N',) int32, status) in the same layout, the frame column the index on
    the counts axis.  Everything is float32, every operation rounded (no contraction).  cos_g = ``track_cos(gate_deg)``,
    a = float32(smooth), b = float32(1) - a.  Every (clip, class) on its own, ``TRACK_SLOTS`` slots that are empty or hold a
    track {id, s (unit vector), first, last, hits}, next_id = 0; for frame t = 0 .. T' - 1:
      1. candidates: the rows of the class in the frame in row order, the first ``TRACK_MAX_DET`` of them
         (``TRACK_DET_OVERFLOW``); u = p / sqrt((px*px + py*py) + pz*pz), a zero or non-finite norm drops it
         (``TRACK_BAD_VECTOR``);
      2. expire: every occupied slot with t - last - 1 > max_gap is closed; closing a track with hits < min_len erases its
         cells in frames first .. last of the slot;
      3. associate: dot(k, j) = (s.x*u.x + s.y*u.y) + s.z*u.z, eligible when dot > cos_g; greedy rounds over the unmatched
         slots and candidates take the eligible pair with the largest dot (ties: the lowest slot, then the lowest candidate);
      4. update each matched (k, j): m = unit((s * b) + (u * a)); with gap = t - last - 1, for g = 1 .. gap, w = float32(g) /
         float32(gap + 1), cell (last + g, class, k) = unit((s * (float32(1) - w)) + (m * w)) with the track's id; then cell
         (t, class, k) = m, s = m, last = t, hits += 1 (filled frames are no hits);
      5. open: the unmatched candidates in candidate order take the lowest empty slot each (one closed in step 2 of this frame
         included): s = u, first = last = t, hits = 1, id = next_id++, cell (t, class, k) = u; without an empty slot the
         candidate is dropped (``TRACK_SLOT_OVERFLOW``).
    After the last frame every slot is closed (short tracks are pruned there too).  Output: frames ascend, classes ascend within
    a frame, slots ascend within a class; a track's id is the order in which it was opened within its (clip, class), pruned
    tracks included.  ``TRACK_BAD_ROWS``: counts negative or running past the rows (such a frame has no rows), or a class that
    is no integer in [0, nb_classes) (such a row is skipped).  trace: a dict that receives what happened on the way, for tests:
    {'opened', 'pruned', 'pruned_fills' (filled cells erased with their track), 'filled', 'reused' (slots closed in step 2 and
    opened again in step 5 of the same frame)}."""
    n_clips, nb_classes, max_gap, min_len = int(n_clips), int(nb_classes), int(max_gap), int(min_len)
    n_frames = len(np.asarray(counts).reshape(-1))
    if n_clips < 1 or n_frames < 1 or n_frames % n_clips or nb_classes < 1:
        raise ValueError("track_rows: %d frame counts, %d clips, %d classes" % (n_frames, n_clips, nb_classes))
    cos_g, a = track_cos(gate_deg), F32(smooth)
    if max_gap < 0 or min_len < 1 or not 0 < float(gate_deg) < 90 or not 0 < cos_g < 1 or not 0 < a <= 1:
        raise ValueError("track_rows: gate_deg %r, max_gap %r, min_len %r, smooth %r" % (gate_deg, max_gap, min_len, smooth))
    b = F32(F32(1) - a)
    t_clip = n_frames // n_clips
    cand, status = track_candidates(rows, counts, nb_classes)
    active = {}                                                    # (clip, class) -> its frames with candidates
    for f, c in sorted(cand):
        active.setdefault((f // t_clip, c), []).append(f)
    cells = {}                                                     # (frame, class, slot) -> (unit vector, id)
    seen = {"opened": 0, "pruned": 0, "pruned_fills": 0, "filled": 0, "reused": 0}
    for (clip, c), frames in active.items():
        f0 = clip * t_clip
        slots = [None] * TRACK_SLOTS                               # None or [id, s, first, last, hits]
        next_id = 0

        def close(k):
            _, _, first, last, hits = slots[k]
            if hits < min_len:
                gone = sum(cells.pop((f0 + t, c, k), None) is not None for t in range(first, last + 1))
                seen["pruned"] += 1
                seen["pruned_fills"] += gone - hits
            slots[k] = None

        for t in range(frames[0] - f0, t_clip):
            u = cand.get((f0 + t, c))
            if u is None and not any(slots):
                if f0 + t > frames[-1]:
                    break
                continue
            expired = set()
            for k in range(TRACK_SLOTS):                           # 2. expire
                if slots[k] is not None and t - slots[k][3] - 1 > max_gap:
                    close(k)
                    expired.add(k)
            if u is None:
                continue
            occ = [k for k in range(TRACK_SLOTS) if slots[k] is not None]
            cand_free = np.ones(len(u), dtype=bool)
            if occ:                                                # 3. associate
                s = np.stack([slots[k][1] for k in occ])
                dot = (s[:, None, 0] * u[None, :, 0] + s[:, None, 1] * u[None, :, 1]) + s[:, None, 2] * u[None, :, 2]
                val = np.where(dot > cos_g, dot, F32(-np.inf))
                while True:
                    at = int(np.argmax(val))                       # row-major: the lowest slot, then the lowest candidate
                    i, j = divmod(at, len(u))
                    if not val[i, j] > -np.inf:
                        break
                    val[i, :] = -np.inf
                    val[:, j] = -np.inf
                    cand_free[j] = False
                    trk = slots[occ[i]]                            # 4. update
                    k, sk, last = occ[i], trk[1], trk[3]
                    m = _unit3((sk * b) + (u[j] * a))
                    gap = t - last - 1
                    for g in range(1, gap + 1):
                        w = F32(g) / F32(gap + 1)
                        cells[(f0 + last + g, c, k)] = (_unit3((sk * (F32(1) - w)) + (m * w)), trk[0])
                    seen["filled"] += gap
                    cells[(f0 + t, c, k)] = (m, trk[0])
                    trk[1], trk[3], trk[4] = m, t, trk[4] + 1
            for j in np.flatnonzero(cand_free).tolist():           # 5. open
                k = next((k for k in range(TRACK_SLOTS) if slots[k] is None), None)
                if k is None:
                    status |= TRACK_SLOT_OVERFLOW
                    break
                slots[k] = [next_id, u[j], t, t, 1]
                cells[(f0 + t, c, k)] = (u[j], next_id)
                next_id += 1
                seen["opened"] += 1
                seen["reused"] += k in expired
        for k in range(TRACK_SLOTS):
            if slots[k] is not None:
                close(k)
    keys = sorted(cells)
    out = np.zeros((len(keys), 5), dtype=F32)
    ids = np.zeros(len(keys), dtype=np.int32)
    out_counts = np.zeros(n_frames, dtype=np.int32)
    for n, key in enumerate(keys):
        vec, tid = cells[key]
        out[n, 0], out[n, 1], out[n, 2:5], ids[n] = key[0], key[1], vec, tid
        out_counts[key[0]] += 1
    if trace is not None:
        trace.update(seen)
    return (out, out_counts), ids, status


def track_groups(ids, counts, n_clips=1):
    """The ids of ``track_rows`` grouped like ``group_rows`` groups its rows: one {frame of the clip: [id, ...]} per clip, what
    ``write_seld_output_file(tracks=...)`` takes."""
    ids = np.asarray(ids).reshape(-1).tolist()
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if n_clips < 1 or len(counts) % n_clips or int(counts.sum()) != len(ids):
        raise ValueError("track_groups: %d ids, %d frame counts summing to %d, %d clips"
                         % (len(ids), len(counts), int(counts.sum()), n_clips))
    t = len(counts) // n_clips
    ends = np.cumsum(counts)
    outs = [{} for _ in range(n_clips)]
    for f in np.flatnonzero(counts).tolist():
        outs[f // t][f % t] = ids[ends[f] - counts[f]:ends[f]]
    return outs


# ---- Tracks through windows: the host definition of csrc/track.hip ``adyolo_track_run``.
def track_hold(max_gap, min_len):
    """H: how many frames behind the frame being walked ``track_rows`` can still write.  Step 4 fills at most max_gap frames
    back.  A track that can still be erased has at most min_len - 1 hits, at most max_gap + 1 frames apart, and is closed in
    frame last + max_gap + 2: t - first <= (min_len - 1) * (max_gap + 1) + 1.  With min_len 1 nothing is erased and H is max_gap.
    Once the frames [0, e) of a recording are walked, every cell of a frame < e - H is final."""
    max_gap, min_len = int(max_gap), int(min_len)
    if max_gap < 0 or min_len < 1:
        raise ValueError("track_hold: max_gap %r, min_len %r" % (max_gap, min_len))
    return max_gap if min_len == 1 else (min_len - 1) * (max_gap + 1) + 1


def track_run(rows, counts, segments, nb_classes, gate_deg, max_gap, min_len, smooth, hold, carry, trace=None):
    """``track_rows`` on one run of frames of a stream of recordings, the state carried from run to run: a recording linked
    through any number of runs gives, concatenated, the rows, counts and ids of ``track_rows(n_clips=1)`` on it whole, bit for
    bit.  rows (N, 5) / counts (run frames,) as ``track_rows`` takes them.  segments: int (S, 4), one row per recording the run
    holds frames of, {first frame in the run, frames (>= 1), continues, open}: the rows tile the run in order; ``continues``
    (row 0 only): the recording's earlier frames were walked by the call that returned ``carry``; ``open`` (the last row
    only): the recording goes on in the next run.  hold: D >= ``track_hold(max_gap, min_len)`` frames (not checked here: every
    write is, see below).  carry: None (nothing to continue) or what the previous call returned.
      * A continuing segment starts from the carried slots and next_id, its time running on from the carried frames; every other
        segment starts empty at its first frame.  Per frame: steps 1 to 5 of ``track_rows``.
      * A segment that is not open closes every slot at its end, as a clip's end does.  An open one keeps its slots, next_id and
        the cells of its last min(D, frames walked so far in the recording) frames -- the held frames -- for the carry.
      * Emitted: the carried held frames first (they are final now or held again), then the run's frames without the newly held
        ones.  counts' runs over the emitted frames and rows' frame column is the index on that axis.
    A write -- a gap fill or an erasure -- made while frame t is walked (t = the end for the closing there) that lands before
    frame t - D raises AssertionError: D was smaller than the reach of these parameters.
    -> ((rows', counts'), ids, status, carry').  carry' is empty when the last segment is not open; continuing from an empty
    carry is starting fresh.  trace: as ``track_rows``, and {'carried_fills': gap fills written into held frames of an earlier
    call, 'carried_prunes': erased cells that were held frames of an earlier call}."""
    nb_classes, max_gap, min_len, hold = int(nb_classes), int(max_gap), int(min_len), int(hold)
    counts = np.asarray(counts).reshape(-1)
    run_frames = len(counts)
    seg = np.asarray(segments, dtype=np.int64).reshape(-1, 4)
    cos_g, a = track_cos(gate_deg), F32(smooth)
    if max_gap < 0 or min_len < 1 or not 0 < float(gate_deg) < 90 or not 0 < cos_g < 1 or not 0 < a <= 1 or hold < 0:
        raise ValueError("track_run: gate_deg %r, max_gap %r, min_len %r, smooth %r, hold %r"
                         % (gate_deg, max_gap, min_len, smooth, hold))
    ends = seg[:, 0] + seg[:, 1]
    if run_frames < 1 or nb_classes < 1 or len(seg) < 1 or seg[0, 0] != 0 or (seg[:, 1] < 1).any() or ends[-1] != run_frames \
            or (seg[1:, 0] != ends[:-1]).any() or not np.isin(seg[:, 2:], (0, 1)).all() or seg[1:, 2].any() or seg[:-1, 3].any():
        raise ValueError("track_run: segments %s do not tile %d frames (continues on row 0, open on the last row only)"
                         % (seg.tolist(), run_frames))
    if carry is not None and (carry["hold"] != hold or carry["nb_classes"] != nb_classes):
        raise ValueError("track_run: the carry was made with hold %d and %d classes" % (carry["hold"], carry["nb_classes"]))
    b = F32(F32(1) - a)
    cand, status = track_candidates(rows, counts, nb_classes)
    seen = {"opened": 0, "pruned": 0, "pruned_fills": 0, "filled": 0, "reused": 0, "carried_fills": 0, "carried_prunes": 0}
    empty = {"hold": hold, "nb_classes": nb_classes, "walked": 0, "held": 0, "slots": {}, "next_id": {}, "cells": {}}
    carry = empty if carry is None else carry
    cells = {}                                                     # (frame of the run, class, slot) -> (unit vector, id)
    held_in = carry["held"] if seg[0, 2] else 0
    out_carry = empty
    for r0, n, cont, is_open in seg.tolist():
        walked = carry["walked"] if cont else 0                    # the recording's frames before local frame 0
        if cont:                                                   # (r0 == 0: the held frames sit at run frames -held .. -1)
            cells.update(carry["cells"])
        keep = {"hold": hold, "nb_classes": nb_classes, "walked": walked + n, "held": min(hold, walked + n), "slots": {},
                "next_id": {}, "cells": {}}
        for c in range(nb_classes):
            slots = [None] * TRACK_SLOTS
            next_id = 0
            if cont:
                slots = [None if s is None else [s[0], s[1], s[2] - walked, s[3] - walked, s[4]]
                         for s in carry["slots"].get(c, slots)]
                next_id = carry["next_id"].get(c, 0)

            def held_line(f, t):
                if f < t - hold:
                    raise AssertionError("track_run: a write at frame %d while frame %d is walked reaches past the hold of %d "
                                         "frames (track_hold(%d, %d) = %d)" % (f, t, hold, max_gap, min_len,
                                                                                track_hold(max_gap, min_len)))

            def close(k, t):
                _, _, first, last, hits = slots[k]
                if hits < min_len:
                    gone = 0
                    held_line(first, t)                            # (the track's first hit: the farthest cell it owns)
                    for f in range(first, last + 1):
                        if cells.pop((r0 + f, c, k), None) is not None:
                            gone += 1
                            seen["carried_prunes"] += f < 0
                    seen["pruned"] += 1
                    seen["pruned_fills"] += gone - hits
                slots[k] = None

            for t in range(n):
                u = cand.get((r0 + t, c))
                if u is None and not any(slots):
                    continue
                expired = set()
                for k in range(TRACK_SLOTS):                       # 2. expire
                    if slots[k] is not None and t - slots[k][3] - 1 > max_gap:
                        close(k, t)
                        expired.add(k)
                if u is None:
                    continue
                occ = [k for k in range(TRACK_SLOTS) if slots[k] is not None]
                cand_free = np.ones(len(u), dtype=bool)
                if occ:                                            # 3. associate
                    s = np.stack([slots[k][1] for k in occ])
                    dot = (s[:, None, 0] * u[None, :, 0] + s[:, None, 1] * u[None, :, 1]) + s[:, None, 2] * u[None, :, 2]
                    val = np.where(dot > cos_g, dot, F32(-np.inf))
                    while True:
                        at = int(np.argmax(val))
                        i, j = divmod(at, len(u))
                        if not val[i, j] > -np.inf:
                            break
                        val[i, :] = -np.inf
                        val[:, j] = -np.inf
                        cand_free[j] = False
                        trk = slots[occ[i]]                        # 4. update
                        k, sk, last = occ[i], trk[1], trk[3]
                        m = _unit3((sk * b) + (u[j] * a))
                        gap = t - last - 1
                        for g in range(1, gap + 1):
                            w = F32(g) / F32(gap + 1)
                            held_line(last + g, t)
                            cells[(r0 + last + g, c, k)] = (_unit3((sk * (F32(1) - w)) + (m * w)), trk[0])
                            seen["carried_fills"] += last + g < 0
                        seen["filled"] += gap
                        cells[(r0 + t, c, k)] = (m, trk[0])
                        trk[1], trk[3], trk[4] = m, t, trk[4] + 1
                for j in np.flatnonzero(cand_free).tolist():       # 5. open
                    k = next((k for k in range(TRACK_SLOTS) if slots[k] is None), None)
                    if k is None:
                        status |= TRACK_SLOT_OVERFLOW
                        break
                    slots[k] = [next_id, u[j], t, t, 1]
                    cells[(r0 + t, c, k)] = (u[j], next_id)
                    next_id += 1
                    seen["opened"] += 1
                    seen["reused"] += k in expired
            if is_open:
                keep["slots"][c] = [None if s is None else [s[0], s[1], s[2] + walked, s[3] + walked, s[4]] for s in slots]
                keep["next_id"][c] = next_id
            else:
                for k in range(TRACK_SLOTS):
                    if slots[k] is not None:
                        close(k, n)
        if is_open:                                                # the newly held frames leave the run for the carry
            for key in [key for key in cells if key[0] >= run_frames - keep["held"]]:
                keep["cells"][(key[0] - run_frames, key[1], key[2])] = cells.pop(key)
            out_carry = keep
    n_emit = held_in + run_frames - out_carry["held"]
    keys = sorted(cells)
    out = np.zeros((len(keys), 5), dtype=F32)
    ids = np.zeros(len(keys), dtype=np.int32)
    out_counts = np.zeros(n_emit, dtype=np.int32)
    for i, key in enumerate(keys):
        vec, tid = cells[key]
        out[i, 0], out[i, 1], out[i, 2:5], ids[i] = key[0] + held_in, key[1], vec, tid
        out_counts[key[0] + held_in] += 1
    if trace is not None:
        trace.update(seen)
    return (out, out_counts), ids, status, out_carry


class LabelPostProcessor:
    """``LabelPostProcessor(params).postprocess(output)`` for the adyolo head (decode + NMS) and the class-wise heads
    (``--loss seddoa | masked-seddoa | accdoa | adpit``); ``output`` (1, T', K) on the GPU."""

    def __init__(self, params):
        tc = params["train_config"]
        self.nb_classes = params["data_config"]["nb_classes"]
        self.loss = params["args"]["loss"]
        self.conf_thresh = tc["conf_thresh"]
        if self.loss in CLASSWISE:
            # unify_thresh: read at select time (the reference's test.py:96-98 sets it on the object between runs)
            self.unify_thresh = tc.get("unify_thresh") if self.loss == "adpit" else None
            return
        if self.loss != "adyolo":
            raise NotImplementedError("postprocess: {}".format(self.loss))
        self.grid_size = [float(v) for v in tc["grid_size"]]
        self.nb_anchors = int(tc["nb_anchors"])
        self.nb_grids = (int(math.ceil(360.0 / self.grid_size[0])), int(math.ceil(180.0 / self.grid_size[1])))
        self.conf_thresh = tc["conf_thresh"]
        self.clss_thresh = tc["clss_thresh"]
        self.unify_thresh = tc["unify_thresh"]
        self.g_overlap = tc["g_overlap"]
        self.nms = tc["nms"]

    def get_conf_thresh(self):
        return self.conf_thresh

    def set_conf_thresh(self, thresh):          # datasets.py:532-534 rewrites both thresholds
        self.conf_thresh = thresh
        self.clss_thresh = thresh

    def decode_device(self, output):
        """The GPU decode of (B, T', K) network outputs as a device tensor, clip after clip along its first axis (B * T'
        frames): adyolo [frames][Gaz][Gel][A][C+3], class-wise [frames][C][rec] (``adyolo_classwise_decode``).  What ``select``
        reads; ``graph.ForwardGraphs`` records it with the forward pass."""
        from . import ops
        if self.loss in CLASSWISE:
            return ops.classwise_decode(output.contiguous(), self.nb_classes, self.loss)
        return ops.yolo_decode(output.contiguous(), self.nb_classes, self.nb_grids, self.nb_anchors, self.grid_size,
                               self.g_overlap)

    def decode(self, output, borrow=False):
        """GPU half of ``postprocess`` (threshold-free): logits (1, T', K) -> decoded predictions as a host array.
        borrow: return a view of the page-locked staging buffer (valid until the next decode of that shape) instead of a copy."""
        from . import ops
        if output.shape[0] != 1:
            raise ValueError("postprocess handles one clip at a time (B = 1), like the reference (datasets.py:752-753)")
        host = ops.to_host(self.decode_device(output)).numpy()
        return host if borrow else host.copy()

    def select(self, decoded):
        """Host half on a ``decode`` result: adyolo -- confidence / class thresholds + NMS; class-wise -- ``classwise_select``
        with the current conf_thresh and unify_thresh."""
        if self.loss in CLASSWISE:
            return classwise_select(decoded, self.loss, self.conf_thresh, self.unify_thresh)
        return nms_decoded(decoded, self.nb_classes, self.conf_thresh, self.clss_thresh, self.unify_thresh, self.nms)

    def select_device_rows(self, decoded_dev, n_clips=1, trim=True):
        """``select`` on the device (adyolo: ``ops.yolo_select``; class-wise heads: ``ops.classwise_select`` with the current
        conf_thresh and unify_thresh; the same rows in the same order) on a ``decode_device`` result of n_clips clips ->
        (rows (N, 5) [frame, class, x, y, z], counts (n_clips * T',) int32, clip after clip), both on the device.
        trim=False: no synchronisation, rows is the capacity buffer of which the first counts.sum() are written (what
        ``seld_metrics.DeviceSELDScorer.add_rows`` takes).  There is no host implementation behind this name: a class-wise
        decode that is not on a HIP device raises NotImplementedError (``select`` is the host path)."""
        from . import ops
        if self.loss in CLASSWISE and not getattr(decoded_dev, "is_cuda", False):
            raise NotImplementedError("select_device: the class-wise heads select on a HIP device only (the host path is "
                                      "select / classwise_select)")
        if n_clips < 1 or decoded_dev.shape[0] % n_clips:
            raise ValueError("select_device_rows: %d frames for %d clips" % (decoded_dev.shape[0], n_clips))
        if self.loss in CLASSWISE:
            return ops.classwise_select(decoded_dev, self.nb_classes, self.loss, self.conf_thresh, self.unify_thresh, trim=trim)
        return ops.yolo_select(decoded_dev, self.nb_classes, self.conf_thresh, self.clss_thresh, self.unify_thresh, self.nms,
                               trim=trim)

    def track_device_rows(self, rows, counts, n_clips, opts, buf=None, status=None, trim=True):
        """``track_rows`` on the device (``ops.track_rows``; the same rows, counts and ids bit for bit) on what
        ``select_device_rows`` or the test-time-augmentation merge returns for n_clips clips -> (rows', counts', ids), all on
        the device.  opts: ``augmentations.track_options``; buf / status / trim as ``ops.track_rows``."""
        from . import ops
        return ops.track_rows(rows, counts, n_clips, self.nb_classes, opts, buf=buf, status=status, trim=trim)

    def track_device_run(self, rows, counts, segments, opts, hold, carry, buf=None, status=None, trim=True, emitted=None):
        """``track_run`` on the device (``ops.track_run``; the same rows, counts and ids bit for bit) on what
        ``select_device_rows`` returns for one stitched run of a windowed pass -> (rows', counts', ids) of the emitted frames,
        all on the device.  segments / hold: ``corpus.track_plan``; carry: ``ops.track_carry``; the rest as ``ops.track_run``."""
        from . import ops
        return ops.track_run(rows, counts, segments, self.nb_classes, opts, hold, carry, buf=buf, status=status, trim=trim,
                             emitted=emitted)

    def select_device(self, decoded_dev, n_clips=1):
        """``select_device_rows`` -> one {frame: [[class, x, y, z], ...]} per clip.  Only the selected rows and the per-frame
        counts are copied to the host."""
        from . import ops
        rows, counts = self.select_device_rows(decoded_dev, n_clips)
        rows_h, counts_h = ops.to_host_many(rows, counts)
        return group_rows(rows_h.numpy(), counts_h.numpy(), n_clips)

    def postprocess(self, output, on_device=False):
        """on_device: the selection too runs on the GPU (``select_device``); default: ``select`` on the host."""
        if on_device:
            if output.shape[0] != 1:
                raise ValueError("postprocess handles one clip at a time (B = 1), like the reference (datasets.py:752-753)")
            return self.select_device(self.decode_device(output))[0]
        return self.select(self.decode(output, borrow=True))       # consumed at once: no second host copy


def write_seld_output_file(file_pth, output: dict, tracks=None, mode="w"):
    """reference test.py:26-30: rows ``frame,class,0,x,y,z``.  tracks: {frame: [id, ...]} parallel to ``output``
    (``track_groups`` of the ids ``track_rows`` returns): the third column, the DCASE track index, is the row's id instead
    of 0.  mode: "a" appends the rows to the file (a live stream's frames as they become final)."""
    with open(file_pth, mode) as f:
        for frame_idx in output.keys():
            ids = None if tracks is None else tracks[frame_idx]
            if ids is not None and len(ids) != len(output[frame_idx]):
                raise ValueError("write_seld_output_file: frame %r has %d rows and %d track ids"
                                 % (frame_idx, len(output[frame_idx]), len(ids)))
            for n, [class_idx, x, y, z] in enumerate(output[frame_idx]):
                f.write("{},{},{},{},{},{}\n".format(int(frame_idx), int(class_idx), 0 if ids is None else int(ids[n]),
                                                     float(x), float(y), float(z)))


# ---- The CSV files as bytes: the host definition of csrc/csv.hip ``adyolo_csv_format``.
CSV_OVERFLOW, CSV_BAD_COUNTS, CSV_BAD_VALUE, CSV_BAD_TABLE = 1, 2, 4, 8                         # ADYOLO_CSV_* in adyolo_hip.h
CSV_LINE_MAX = 110                                                                 # CSVF_LINE_MAX in csrc/csv_format.hpp


def csv_segments_clips(n_clips, t_clip):
    """The segment table of ``format_rows`` for a batch of whole clips, clip after clip on the counts axis: [(k * T', 0)]."""
    n_clips, t_clip = int(n_clips), int(t_clip)
    if n_clips < 1 or t_clip < 0:
        raise ValueError("csv_segments_clips: %d clips of %d frames" % (n_clips, t_clip))
    return np.stack([np.arange(n_clips, dtype=np.int64) * t_clip, np.zeros(n_clips, dtype=np.int64)], 1).astype(np.int32)


def csv_segments_run(base_frame, n_frames, frame_start):
    """The segment table of ``format_rows`` for a run of ``n_frames`` frames that starts at ``base_frame`` on the axis of all
    recordings laid end to end (frame_start (R + 1,): each recording's first frame there): one row per recording from the one
    that holds ``base_frame`` to the one that holds the run's last frame -- a recording without frames between them has an
    empty segment -- the split ``corpus.split_pass_rows`` makes.  -> (the first recording's index, table (K, 2) int32)"""
    frame_start = np.asarray(frame_start, dtype=np.int64).reshape(-1)
    base_frame, n_frames = int(base_frame), int(n_frames)
    if n_frames < 1 or base_frame < 0 or base_frame + n_frames > int(frame_start[-1]):
        raise ValueError("csv_segments_run: frames [%d, %d) of %d" % (base_frame, base_frame + n_frames, int(frame_start[-1])))
    r0 = int(np.searchsorted(frame_start, base_frame, "right")) - 1
    r1 = int(np.searchsorted(frame_start, base_frame + n_frames - 1, "right")) - 1
    first = frame_start[r0:r1 + 1]
    table = np.stack([np.maximum(first - base_frame, 0), np.maximum(base_frame - first, 0)], 1)
    return r0, table.astype(np.int32)


def format_rows(rows, counts, segments, ids=None):
    """The bytes ``write_seld_output_file`` writes for one call's rows, all files of the call in one string: rows (N, 5)
    [frame, class, x, y, z] in frame order, counts (frames,) rows per frame, ids (N,) track ids or None (0).  segments (K, 2)
    int: {first frame of the segment on the counts axis, the number that frame has in its file}, ascending, the first at
    frame 0 (``csv_segments_clips`` / ``csv_segments_run``); a segment is one file's span.  A line is
    ``frame,class,id,x,y,z\\n`` by the writer's own format expression: the frame number from the frame's POSITION on the
    counts axis and its segment (``rows[:, 0]`` is not read), int(class), int(id), repr(float(float32)) thrice.
    -> (bytes, seg_bytes (K + 1,) int64: where each segment's bytes start, the total last)
    ``ValueError``: counts that are negative or do not sum to the rows, a table that is not as above, a class that is not
    finite or not within int32, a negative id (csrc/csv.hip reports the same with a status bit)."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    rows = np.asarray(rows, dtype=F32).reshape(-1, 5)
    seg = np.asarray(segments, dtype=np.int64)
    if (counts < 0).any() or int(counts.sum()) != len(rows):
        raise ValueError("format_rows: %d rows, %d frame counts summing to %d" % (len(rows), len(counts), int(counts.sum())))
    if seg.ndim != 2 or seg.shape[1] != 2 or len(seg) < 1 or seg[0, 0] != 0 or (np.diff(seg[:, 0]) < 0).any() \
            or (seg[:, 1] < 0).any() or seg[-1, 0] > len(counts) or (seg[:, 1] + len(counts) - seg[:, 0] - 1 >= 2 ** 31).any():
        raise ValueError("format_rows: segments %r are not (K, 2) {first frame, its number}, ascending from frame 0, numbers within int32" % (seg,))
    if ids is not None:
        ids = np.asarray(ids).reshape(-1)
        if len(ids) != len(rows) or (ids < 0).any():
            raise ValueError("format_rows: %d ids for %d rows, or a negative id" % (len(ids), len(rows)))
        ids = ids.tolist()
    cls = rows[:, 1]
    if not (np.isfinite(cls).all() and (np.abs(cls) < 2.0 ** 31).all()):
        raise ValueError("format_rows: a class that is not finite or not within int32")
    frame_of = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    k_of = np.searchsorted(seg[:, 0], frame_of, "right") - 1
    number = (seg[k_of, 1] + frame_of - seg[k_of, 0]).tolist()
    ends = np.concatenate([[0], np.cumsum(counts)])
    first_row = ends[np.minimum(seg[:, 0], len(counts))]              # the first row at or behind each segment's start
    lines, at, total = [], np.zeros(len(rows) + 1, dtype=np.int64), 0
    for n, (_, class_idx, x, y, z) in enumerate(rows.tolist()):
        line = "{},{},{},{},{},{}\n".format(int(number[n]), int(class_idx), 0 if ids is None else int(ids[n]),
                                            float(x), float(y), float(z))
        lines.append(line)
        at[n] = total
        total += len(line)
    at[len(rows)] = total
    return "".join(lines).encode("ascii"), np.concatenate([at[first_row], [total]]).astype(np.int64)
