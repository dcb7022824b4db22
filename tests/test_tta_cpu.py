"""CPU: the host half of rotation test-time augmentation -- the view matrices derived from ``rotate_labels``
(``augmentations.view_matrix``), the configuration keys (``tta_views`` / ``tta_options``) and the host definition of the merge
(``postprocess.merge_view_rows``) on hand-built rows.  ``random_views`` is the generator the GPU test (test_gpu_tta.py) feeds to
the kernels; here it is checked against its own redraw cap with the host definition alone."""
import math

import numpy as np
import pytest

import adyolo_amd  # noqa: F401
from adyolo_amd.augmentations import (COMBINATIONS, MIC_SWAP_COMBS, rotate_labels, tta_options, tta_views, view_matrix)
from adyolo_amd.postprocess import (TTA_BAD_VECTOR, TTA_CAND_OVERFLOW, TTA_ROWS_OVERFLOW, merge_view_rows, tta_cos)

F32 = np.float32


def direction(az, el):
    a, e = math.radians(az), math.radians(el)
    return np.array([math.cos(a) * math.cos(e), math.sin(a) * math.cos(e), math.sin(e)])


def seen_by(view, d):
    """A direction of the recording's frame as view ``view`` (a combination) sees it, float32."""
    return (view_matrix(view).astype(np.float64) @ np.asarray(d, dtype=np.float64)).astype(F32)


def angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return math.degrees(math.acos(max(-1.0, min(1.0, float(a @ b) / float(np.linalg.norm(a) * np.linalg.norm(b))))))


# ------------------------------------------------------------------------------------------------------------ view tables
def test_view_matrix_is_a_signed_permutation():
    for k in range(len(COMBINATIONS)):
        m = view_matrix(k)
        assert m.shape == (3, 3) and m.dtype == np.float32
        assert set(np.unique(m).tolist()) <= {-1.0, 0.0, 1.0}
        assert (np.abs(m).sum(axis=0) == 1).all() and (np.abs(m).sum(axis=1) == 1).all()
        assert np.array_equal(m @ m.T, np.eye(3, dtype=np.float32))             # the inverse is the transpose
    assert np.array_equal(view_matrix(0), np.eye(3, dtype=np.float32))
    assert len({view_matrix(k).tobytes() for k in range(16)}) == 16
    for bad in (-1, 16, 1.5, True):
        with pytest.raises(ValueError):
            view_matrix(bad)


def test_view_matrix_moves_directions_as_rotate_labels_moves_them():
    for k in range(len(COMBINATIONS)):
        m = view_matrix(k).astype(np.float64)
        for az in range(-180, 181, 15):
            for el in range(-90, 91, 15):
                ev = rotate_labels({0: [[0, 0, az, el]]}, k)[0][0]
                assert np.abs(direction(ev[2], ev[3]) - m @ direction(az, el)).max() <= 1e-6, (k, az, el)


def test_tta_views_and_options_parse_their_keys():
    def prm(test=None, train=None, fmt=None, loss="adyolo"):
        p = {"args": {"loss": loss}, "data_config": {}, "train_config": {"unify_thresh": 20.0}}
        if fmt:
            p["data_config"]["audio_format"] = fmt
        if test is not None:
            p["test_config"] = test
        p["train_config"].update(train or {})
        return p
    assert tta_views(prm()) is None and tta_options(prm()) is None
    assert tta_views(prm({"tta_views": None})) is None
    assert tta_views(prm({"tta_views": "all"})) == list(range(16))
    assert tta_views(prm({"tta_views": "all"}, fmt="mic")) == list(MIC_SWAP_COMBS)
    assert tta_views(prm(train={"tta_views": [3, 5]})) == [0, 3, 5]
    assert tta_views(prm({"tta_views": [7, 0, 7, 2]}, train={"tta_views": "all"})) == [0, 7, 2]      # test_config first
    assert tta_views(prm({"tta_views": [3, 14]}, fmt="mic")) == [0, 3, 14]
    for bad in ("some", 3, [16], [-1], [1.0], [True], [[1]]):
        with pytest.raises(ValueError, match="tta_views"):
            tta_views(prm({"tta_views": bad}))
    with pytest.raises(ValueError, match="symmetry"):
        tta_views(prm({"tta_views": [1]}, fmt="mic"))
    opt = tta_options(prm({"tta_views": [1, 2, 3]}))
    assert opt == {"views": [0, 1, 2, 3], "min_views": 2, "unify_thresh": 20.0, "max_rows_per_frame": 64}
    assert tta_options(prm({"tta_views": "all"}))["min_views"] == 8
    assert tta_options(prm({"tta_views": [1]}, loss="accdoa"))["unify_thresh"] == 15.0
    assert tta_options(prm({"tta_views": [1], "tta_unify_thresh": 7.5, "tta_min_views": 1, "tta_max_rows_per_frame": 8})) == \
        {"views": [0, 1], "min_views": 1, "unify_thresh": 7.5, "max_rows_per_frame": 8}
    for key, values in (("tta_min_views", (0, 3, 1.0, True)), ("tta_unify_thresh", (0, -1.0, 181, "x", float("nan"))),
                        ("tta_max_rows_per_frame", (0, 1025, 2.0, True))):
        for bad in values:
            with pytest.raises(ValueError, match=key):
                tta_options(prm({"tta_views": [1], key: bad}))
    with pytest.raises(ValueError):
        tta_options(prm(), views=[1, 2])                                       # view 0 comes first


# ------------------------------------------------------------------------------------------------------------ the merge
ROWS = {0: [(2, 10.0, 5.0), (2, 100.0, -40.0), (7, -170.0, 60.0)], 3: [(0, 45.0, 0.0)], 4: [(1, 0.0, 89.0), (1, 0.0, -89.0)]}


def test_copies_of_one_row_set_merge_back_to_it():
    views = list(range(16))
    per_view = [{f: [[c] + seen_by(v, direction(az, el)).tolist() for c, az, el in rows] for f, rows in ROWS.items()} for v in views]
    for min_views in (None, 1, 16):
        out, status = merge_view_rows(per_view, views, 15.0, min_views)
        assert status == 0 and list(out) == [0, 3, 4]
        for f, rows in ROWS.items():
            assert [r[0] for r in out[f]] == [float(c) for c, _, _ in rows]
            for got, (_, az, el) in zip(out[f], rows):
                assert np.abs(np.asarray(got[1:]) - direction(az, el)).max() <= 1e-6
                assert all(isinstance(v, float) and F32(v) == v for v in got)


def test_support_counts_distinct_views():
    a, near_a, b = direction(30, 10), direction(33, 12), direction(-120, -20)
    views = [0, 5, 10]
    per_view = [{1: [[4.0] + seen_by(0, a).tolist(), [4.0] + seen_by(0, near_a).tolist(), [4.0] + seen_by(0, b).tolist()]},
                {1: [[4.0] + seen_by(5, b).tolist()]},
                {}]
    out, status = merge_view_rows(per_view, views, 15.0, 2)
    # the two rows of view 0 around ``a`` are ONE view: support 1, dropped; ``b`` has views 0 and 5
    assert status == 0 and list(out) == [1] and len(out[1]) == 1 and angle_deg(out[1][0][1:], b) < 1e-3
    out, _ = merge_view_rows(per_view, views, 15.0, 1)
    assert len(out[1]) == 2 and angle_deg(out[1][0][1:], direction(31.5, 11)) < 0.5 and angle_deg(out[1][1][1:], b) < 1e-3
    out, _ = merge_view_rows(per_view, views, 15.0, 3)
    assert out == {}
    assert merge_view_rows(per_view, views, 15.0)[0] == merge_view_rows(per_view, views, 15.0, 2)[0]      # a majority


def test_a_chain_is_one_component_and_the_order_is_frames_classes_seeds():
    chain = [direction(0, 0), direction(20, 0), direction(10, 0)]               # A - C are 20 degrees apart, B joins them
    assert angle_deg(chain[0], chain[1]) > 15 > angle_deg(chain[0], chain[2])
    far = direction(-90, 45)
    per_view = [{9: [[5.0] + far.tolist()] + [[5.0] + d.tolist() for d in chain] + [[1.0] + far.tolist()],
                 2: [[3.0] + chain[0].tolist()]}]
    out, status = merge_view_rows(per_view, [0], 15.0, 1)
    assert status == 0 and list(out) == [2, 9]
    assert [r[0] for r in out[9]] == [1.0, 5.0, 5.0]                             # classes ascend, then the seeds
    assert angle_deg(out[9][1][1:], far) < 1e-3 and angle_deg(out[9][2][1:], direction(10, 0)) < 1e-3
    p = np.asarray(chain, dtype=F32)
    u = p / np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])[:, None]
    s = np.cumsum(u, axis=0, dtype=F32)[-1]
    n = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
    assert out[9][2][1:] == (s / n).tolist()                                     # the members summed in candidate order


def test_bad_vectors_and_overflows_are_reported():
    d = direction(10, 20).astype(F32).tolist()
    per_view = [{0: [[1.0, 0.0, 0.0, 0.0], [1.0] + d, [2.0, float("nan"), 0.0, 1.0], [2.0, float("inf"), 0.0, 0.0]]}, {0: [[1.0] + d]}]
    out, status = merge_view_rows(per_view, [0, 0], 15.0, 2)
    assert status == TTA_BAD_VECTOR and list(out) == [0] and [r[0] for r in out[0]] == [1.0]
    # rows per frame: the first ones are kept
    many = [{0: [[0.0] + direction(20 * i, 0).astype(F32).tolist() for i in range(5)]}]
    out, status = merge_view_rows(many, [0], 15.0, 1, max_rows_per_frame=3)
    assert status == TTA_ROWS_OVERFLOW and len(out[0]) == 3
    out, status = merge_view_rows(many, [0], 15.0, 1, max_rows_per_frame=5)
    assert status == 0 and len(out[0]) == 5
    crowd = [{0: [[0.0] + d] * 1025, 1: [[0.0] + d] * 1024}]
    out, status = merge_view_rows(crowd, [0], 15.0, 1)
    assert status == TTA_CAND_OVERFLOW and list(out) == [1] and len(out[1]) == 1
    with pytest.raises(ValueError):
        merge_view_rows(per_view, [0], 15.0)
    with pytest.raises(ValueError):
        merge_view_rows(per_view, [0, 0], 15.0, 3)


# ------------------------------------------------------------------------------------------------------------ the generator
def _unit_vectors(frame_rows, views):
    """(class, unit vector) of every row of one frame as ``merge_view_rows`` forms them."""
    cls, vec = [], []
    for v, rows in zip(views, frame_rows):
        m = view_matrix(v)
        src = np.abs(m).argmax(axis=0)
        r = np.asarray(rows, dtype=F32).reshape(-1, 4)
        cls.append(r[:, 0])
        vec.append(r[:, 1:4][:, src] * m[src, np.arange(3)][None, :])
    cls, p = np.concatenate(cls), np.concatenate(vec).astype(F32)
    n = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    return cls, p / n[:, None]


def most_candidates(per_view, cap):
    """The largest number of candidates of one (frame, class), each view giving its first ``cap`` rows of a frame."""
    seen = {}
    for rows, counts in per_view:
        at = 0
        for f, n in enumerate(counts.tolist()):
            for c in rows[at:at + min(n, cap), 1].tolist():
                seen[(f, c)] = seen.get((f, c), 0) + 1
            at += n
    return max(seen.values())


def boundary_margin(frame_rows, views, cos_t):
    """The least |dot - cos_t| over the pairs of one frame and class (inf without a pair)."""
    cls, u = _unit_vectors(frame_rows, views)
    best = np.inf
    for c in np.unique(cls):
        uc = u[cls == c]
        if len(uc) > 1:
            dots = ((uc[:, None, 0] * uc[None, :, 0] + uc[:, None, 1] * uc[None, :, 1]) + uc[:, None, 2] * uc[None, :, 2])
            best = min(best, float(np.abs(dots[np.triu_indices(len(uc), 1)].astype(np.float64) - float(cos_t)).min()))
    return best


def _draw_frame(rs, nb_classes, views, unify, crowd=0, rows_in_view1=None):
    """One frame's rows per view, each view's in class order: 0-3 sources seen by most views with a jitter of a few degrees
    and any length (an ACCDOA vector is not a unit vector), stray rows of single views, and on request ``crowd`` rows per view
    of ONE class around three directions, or exactly ``rows_in_view1`` rows in view 1."""
    per_view = [[] for _ in views]

    def jitter(d, deg):
        w = rs.randn(3)
        w -= (w @ d) * d
        w /= np.linalg.norm(w)
        t = math.radians(rs.uniform(0, deg))
        return (math.cos(t) * d + math.sin(t) * w) * rs.uniform(0.4, 1.6)

    def any_direction():
        d = rs.randn(3)
        return d / np.linalg.norm(d)
    sources = [(int(rs.randint(nb_classes)), any_direction(), 0) for _ in range(int(rs.choice(4, p=[0.3, 0.3, 0.25, 0.15])))]
    if crowd:
        cls = int(rs.randint(nb_classes))
        sources += [(cls, any_direction(), crowd // 3) for _ in range(3)]
    for k, v in enumerate(views):
        for cls, d, n in sources:
            for _ in range(n or int(rs.rand() < 0.8)):
                per_view[k].append([float(cls)] + seen_by(v, jitter(d, 0.6 * unify)).tolist())
        if rs.rand() < 0.2:
            per_view[k].append([float(rs.randint(nb_classes))] + seen_by(v, any_direction()).tolist())
    if rows_in_view1 is not None:
        rows = per_view[1][:rows_in_view1]
        while len(rows) < rows_in_view1:
            rows.append([float(rs.randint(nb_classes))] + seen_by(views[1], any_direction() * rs.uniform(0.4, 1.6)).tolist())
        per_view[1] = rows
    return [sorted(rows, key=lambda r: r[0]) for rows in per_view]             # (stable: the draw order within a class)


def random_views(seed, frames, nb_classes, views, unify=15.0, rows_cap=None):
    """-> (per_view [(rows (N, 5) float32, counts (frames,) int32)], frames redrawn).  A frame with a pair of one class whose dot
    product lies within 1e-6 of ``tta_cos(unify)`` is drawn again.  With frames >= 3: frame 1 holds more than 64 candidates of one
    class; with ``rows_cap`` = P also, view 1 has exactly P rows in frame 0 and P + 1 in the last frame."""
    rs = np.random.RandomState(seed)
    cos_t = tta_cos(unify)
    out = [([], np.zeros(frames, dtype=np.int32)) for _ in views]
    redrawn = 0
    for f in range(frames):
        special = {}
        if frames >= 3 and f == 1:
            special = {"crowd": 3 * (64 // (3 * len(views)) + 2)}
        elif frames >= 3 and rows_cap is not None and f in (0, frames - 1):
            special = {"rows_in_view1": rows_cap + (f != 0)}
        for attempt in range(100):
            frame_rows = _draw_frame(rs, nb_classes, views, unify, **special)
            if boundary_margin(frame_rows, views, cos_t) > 1e-6:
                break
            redrawn += attempt == 0
        else:
            raise AssertionError("random_views: frame %d keeps a pair on the threshold" % f)
        for k, rows in enumerate(frame_rows):
            out[k][0].extend([float(f)] + r for r in rows)
            out[k][1][f] = len(rows)
    return [(np.asarray(r, dtype=F32).reshape(-1, 5), c) for r, c in out], redrawn


# (frames, classes, views, P): every frame count, class count and view count the kernels are tested at
CONFIGS = ((1, 3, [0, 9], 64), (63, 13, [0, 1, 2, 3, 4, 5, 6, 7], 20), (130, 3, list(range(16)), 12), (130, 13, [0, 15], 40),
           (63, 3, list(range(16)), 64), (1, 13, [0, 2, 4, 6, 8, 10, 12, 14], 12))


def test_generator_stays_inside_its_redraw_cap():
    for k, (frames, nb_classes, views, cap) in enumerate(CONFIGS):
        per_view, redrawn = random_views(40 + k, frames, nb_classes, views, rows_cap=cap)
        assert redrawn <= frames // 100, (k, redrawn)                          # no more than 1 % of the frames
        assert all(len(r) == int(c.sum()) and c.shape == (frames,) for r, c in per_view)
        dicts = [{} for _ in views]
        for d, (rows, counts) in zip(dicts, per_view):
            at = 0
            for f, n in enumerate(counts.tolist()):
                if n:
                    d[f] = rows[at:at + n, 1:].tolist()
                at += n
        cos_t = tta_cos(15.0)
        for f in range(frames):
            assert boundary_margin([d.get(f, []) for d in dicts], views, cos_t) > 1e-6
        if frames >= 3:
            assert per_view[1][1][0] == cap and per_view[1][1][-1] == cap + 1
            assert most_candidates(per_view, cap) > 64 and min(int(c.min()) for _, c in per_view) == 0
        # the two input forms give one result
        (rows, counts), status = merge_view_rows(per_view, views, 15.0, max_rows_per_frame=cap)
        out, status_d = merge_view_rows(dicts, views, 15.0, max_rows_per_frame=cap)
        assert status == status_d == (TTA_ROWS_OVERFLOW if frames >= 3 else 0)
        assert rows.dtype == np.float32 and counts.dtype == np.int32 and int(counts.sum()) == len(rows) > 0
        assert [int(f) for f in np.flatnonzero(counts)] == sorted(out)
        at = 0
        for f in sorted(out):
            assert rows[at:at + counts[f], 1:].tolist() == out[f] and (rows[at:at + counts[f], 0] == f).all()
            at += counts[f]
