"""Oracle (test infrastructure): the detection stage of evaluation -- the AD-YOLO decode (csrc/loss.hip ``yolo_decode_kernel``,
K8b) and the selection (csrc/select.hip ``yolo_select_kernel`` / ``select_scan_kernel`` / ``select_compact_kernel``, K8c) --
stated in NumPy float64, and the builders of the decoded tensors on which tests/test_select_stage_cpu.py and
tests/test_gpu_select_stage.py compare the kernels with it.

``decode64`` is ``oracle.postprocess.decode`` with every operation in float64.  ``select64`` states
``postprocess.nms_decoded`` in float64 without importing it: strict ``>`` filter, stable descending order by class confidence,
per class ``_single`` for one row and otherwise conn-merge (connected components of dist < unify, seeded at the lowest
unassigned rank), soft-merge (greedy; the seed's cluster is every row of the class with dist <= unify, removed ones too) or the
plain greedy suppression, and the vote softmax(exp(c^2 / t)).

The builders return float32 decoded tensors [frames][N][C + 3] (conf, class confidences, U, V in degrees) that are handed to
``ops.yolo_select`` directly, so N is free up to 1024, together with what the case must satisfy.  A case may be used only if no
candidate pair stands near the unify threshold (``margin``): a float32 distance that falls on the other side of it would
change the clusters, which is a property of the input, not an error of a kernel."""
import itertools

import numpy as np

F32 = np.float32
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ decode
def decode64(logit, nb_classes, grid=(8, 4), anchors=5, grid_size=(45.0, 45.0), g_overlap=0.5):
    """logit [...][G * A * (C + 3)] float32 -> (decoded [T][Gaz][Gel][A][C + 3], un-wrapped U, un-clamped V [T][Gaz][Gel][A]),
    all float64.  The V clamp's upper end is the float32 value the product clamps to, float32(90 - 1e-7)."""
    ch = nb_classes + 3
    x = np.asarray(logit, dtype=np.float64).reshape(-1, grid[0], grid[1], anchors, ch)
    out = np.empty_like(x)
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-x[..., :nb_classes + 1]))
    out[..., 0] = sig[..., 0]
    out[..., 1:nb_classes + 1] = sig[..., 1:] * sig[..., :1]
    span = 0.5 + float(g_overlap)
    gi = np.arange(grid[0], dtype=np.float64)[None, :, None, None]
    gj = np.arange(grid[1], dtype=np.float64)[None, None, :, None]
    u_raw = np.tanh(x[..., -2]) * span * float(grid_size[0]) + (gi * float(grid_size[0]) - 180.0 + float(grid_size[0]) * 0.5)
    v_raw = np.tanh(x[..., -1]) * span * float(grid_size[1]) + (gj * float(grid_size[1]) - 90.0 + float(grid_size[1]) * 0.5)
    v = np.clip(v_raw, -90.0, float(F32(90.0 - 1e-7)))
    u = np.where(u_raw >= 180.0, u_raw - 360.0, u_raw)
    u = np.where(u < -180.0, u + 360.0, u)
    out[..., -2], out[..., -1] = u, v
    return out, u_raw, v_raw


# Gaz, Gel, A, C, grid size, g_overlap
DECODE_GEOMS = ((8, 4, 5, 12, (45.0, 45.0), 0.5), (8, 4, 5, 13, (45.0, 45.0), 0.0), (1, 1, 1, 1, (360.0, 180.0), 0.5),
                (3, 5, 2, 4, (120.0, 36.0), 0.25))
DECODE_FRAMES = (1, 7)
DECODE_LARGE = (6554, (8, 4, 5, 1, (45.0, 45.0), 0.5))             # 6554 x 160 anchors: past the grid cap of 4096 x 256
LADDER = (5.5, -5.5, 7.0, -7.0, 9.0, -9.0, 12.0, -12.0, 15.0, -15.0)    # between the drawn logits and the planted ones
PLANTED = (17.0, -17.0, 30.0, -30.0, 88.0, -88.0, 104.0, -104.0, np.inf, -np.inf)


def plant_positions(grid, anchors):
    """(gi, gj, a) of the first and last anchor of the first and last cell."""
    return sorted({(0, 0, 0), (0, 0, anchors - 1), (grid[0] - 1, grid[1] - 1, 0), (grid[0] - 1, grid[1] - 1, anchors - 1)})


def decode_logits(frames, nb_classes, grid, anchors, seed, planted_frames=None):
    """N(0, 2) logits (variance 2) [1][frames][G * A * (C + 3)] float32 with the PLANTED values in every channel of the planted positions of
    the frames ``planted_frames`` (default: the first and the last), cycling through PLANTED over frame, position and channel,
    and the LADDER values in every channel of the anchors of one middle cell, at most half of that cell's anchors over the
    frames (before the planting, which wins a shared anchor).
    -> (logits, planted [frames][Gaz][Gel][A] bool)."""
    rs = np.random.RandomState(seed)
    ch = nb_classes + 3
    x = rs.normal(0.0, np.sqrt(2.0), size=(frames, grid[0], grid[1], anchors, ch)).astype(F32)
    planted = np.zeros(x.shape[:-1], dtype=bool)
    gi, gj = grid[0] // 2, grid[1] // 2        # the tanh and sigmoid tails that variance 2 hardly draws, in a cell whose
    for i, val in enumerate(LADDER[:frames * anchors // 2]):   # saturated U and V stay clear of +-180 and +-90; at most half
        f, a = (i // anchors) % frames, i % anchors
        x[f, gi, gj, a, :] = val
    k = 0
    for f in (sorted({0, frames - 1}) if planted_frames is None else planted_frames):
        for p, (gi, gj, a) in enumerate(plant_positions(grid, anchors)):
            for c in range(ch):
                x[f, gi, gj, a, c] = PLANTED[(k + 3 * p + c) % len(PLANTED)]
            planted[f, gi, gj, a] = True
            k += 1
    return x.reshape(1, frames, -1), planted


def saturated_logits(nb_classes, grid, anchors):
    """[1][len(PLANTED)][G * A * (C + 3)] float32: zero logits, and in frame k every channel of every planted position set to
    PLANTED[k]."""
    ch = nb_classes + 3
    x = np.zeros((len(PLANTED), grid[0], grid[1], anchors, ch), dtype=F32)
    for k, val in enumerate(PLANTED):
        for gi, gj, a in plant_positions(grid, anchors):
            x[k, gi, gj, a, :] = val
    return x.reshape(1, len(PLANTED), -1)


def branch_keep(u_raw, v_raw, logit5, tol=1e-3):
    """The elements of U and V that a value comparison may use: the float64 un-wrapped U farther than ``tol`` degrees from
    +-180 and the un-clamped V farther than ``tol`` from +-90, where a float32 evaluation may legitimately take the other
    branch.  An angle logit with |x| >= 30 stays in: tanh is exactly +-1 there in float32 and float64 alike, so both evaluate
    the same exactly representable sum.  (+-17 does not: the float64 tanh is 1 - 3.4e-15 there, the float32 one is 1, so at
    g_overlap 0 the float64 U of the last cell stays a hair below 180 where every float32 evaluation wraps.  Such planted
    elements are left out like any other; ``decode_share`` counts them apart.)  logit5: the logits [T][Gaz][Gel][A][C + 3]."""
    sat_u, sat_v = np.abs(logit5[..., -2]) >= 30.0, np.abs(logit5[..., -1]) >= 30.0
    keep_u = (np.minimum(np.abs(u_raw - 180.0), np.abs(u_raw + 180.0)) >= tol) | sat_u
    keep_v = (np.minimum(np.abs(v_raw - 90.0), np.abs(v_raw + 90.0)) >= tol) | sat_v
    return keep_u, keep_v


def decode_share(keep_u, keep_v, planted, logit5):
    """(share of the elements outside the planted positions that ``branch_keep`` leaves out, number of planted elements left
    out, whether each of those is a +-17 angle logit -- the one planted value that saturates in float32 only)."""
    free = ~planted
    share = ((~keep_u & free).sum() + (~keep_v & free).sum()) / float(max(1, 2 * free.sum()))
    out_u, out_v = ~keep_u & planted, ~keep_v & planted
    only17 = bool((np.abs(logit5[..., -2][out_u]) == 17.0).all() and (np.abs(logit5[..., -1][out_v]) == 17.0).all())
    return float(share), int(out_u.sum() + out_v.sum()), only17


# --------------------------------------------------------------------------------------------------------- selection
def np_threshold(t):
    """The float64 value t' with (x > t') == (x > t) for a float32 array x under NumPy's promotion: a Python float and a
    float32 scalar are rounded to float32 first, a float64 NumPy scalar is compared as it is."""
    return float(F32(t)) if np.result_type(F32, t) == F32 else float(t)


def dist64(u, v):
    """Pairwise angular distance in degrees of directions (u, v) in degrees, float64 (postprocess._ang_dist_deg's formula)."""
    ru, rv = np.deg2rad(np.asarray(u, dtype=np.float64)), np.deg2rad(np.asarray(v, dtype=np.float64))
    d = (np.sin(rv)[:, None] * np.sin(rv)[None, :]
         + np.cos(rv)[:, None] * np.cos(rv)[None, :] * np.cos(np.abs(ru[:, None] - ru[None, :])))
    return np.rad2deg(np.arccos(np.clip(d, -1.0, 1.0)))


def dist32(u, v):
    """The same in NumPy float32, operation by operation as postprocess._ang_dist_deg evaluates it."""
    ru, rv = np.deg2rad(np.asarray(u, dtype=F32)).astype(F32), np.deg2rad(np.asarray(v, dtype=F32)).astype(F32)
    d = (np.sin(rv)[:, None] * np.sin(rv)[None, :]
         + np.cos(rv)[:, None] * np.cos(rv)[None, :] * np.cos(np.abs(ru[:, None] - ru[None, :])))
    return np.rad2deg(np.arccos(np.clip(d, -1, 1))).astype(F32)


def xyz64(u, v):
    ru, rv = np.deg2rad(np.asarray(u, dtype=np.float64)), np.deg2rad(np.asarray(v, dtype=np.float64))
    return np.stack([np.cos(ru) * np.cos(rv), np.sin(ru) * np.cos(rv), np.sin(rv)], axis=-1)


def vote64(conf, xyz, t):
    """(voted unit vector, e_max, norm of the un-normalised vote) of one cluster; t: the vote temperature (float32 value)."""
    e = np.exp(np.asarray(conf, dtype=np.float64) ** 2 / t)
    w = np.exp(e - e.max())
    w = w / w.sum()
    v = (xyz * w[:, None]).sum(axis=0)
    n = float(np.sqrt((v ** 2).sum()))
    return v / n, float(e.max()), n


def _candidates(flat, nb_classes, conf_t, clss_t):
    """Per (frame, class) with candidates: the anchor indices in rank order (stable, descending class confidence)."""
    ok = (flat[:, :, :1] > conf_t) & (flat[:, :, 1:nb_classes + 1] > clss_t)            # [T][N][C]
    fr, an, cl = np.nonzero(ok)
    order = np.lexsort((an, cl, fr))
    fr, an, cl = fr[order], an[order], cl[order]
    if len(fr) == 0:
        return
    cut = np.flatnonzero(np.r_[True, (fr[1:] != fr[:-1]) | (cl[1:] != cl[:-1]), True])
    for s, e in zip(cut[:-1].tolist(), cut[1:].tolist()):
        a = an[s:e]
        if e - s > 1:
            a = a[np.argsort(-flat[fr[s], a, 1 + cl[s]], kind="stable")]
        yield int(fr[s]), int(cl[s]), a


def clusters64(d, unify, nms):
    """The clusters of rows 0 .. K-1 (rank order) with pairwise distances d: lists of rank indices, in seed order."""
    k = d.shape[0]
    out = []
    if nms == "conn-merge":
        near = d < unify
        comp = np.full(k, -1)
        for seed in range(k):
            if comp[seed] >= 0:
                continue
            comp[seed] = len(out)
            front = np.zeros(k, dtype=bool)
            front[seed] = True
            while front.any():
                front = near[front].any(axis=0) & (comp < 0)
                comp[front] = len(out)
            out.append(np.flatnonzero(comp == len(out)))
        return out
    left = np.ones(k, dtype=bool)
    for seed in range(k):
        if not left[seed]:
            continue
        within = d[seed] <= unify
        within[seed] = True
        if nms == "soft-merge":
            out.append(np.flatnonzero(within))
        else:
            out.append(np.asarray([seed]))
        left &= ~within
    return out


def select64(decoded, nb_classes, conf_t, clss_t, unify, nms, vote_t=None):
    """decoded [frames][...][C + 3] -> (rows (R, 5) float64 [frame, class, x, y, z] in the order of postprocess.nms_decoded,
    diag) with diag a dict of arrays over the rows: ``voted`` (False: written alone, not normalised), ``k_cluster``, ``e_max``,
    ``norm`` (1 for a row written alone) and the list ``members`` of each row's anchor indices.  The thresholds compare as NumPy
    compares them with a float32 array; vote_t defaults to the class threshold (rounded to float32, as the product votes)."""
    flat = np.asarray(decoded, dtype=np.float64).reshape(np.shape(decoded)[0], -1, nb_classes + 3)
    ct, kt, un = np_threshold(conf_t), np_threshold(clss_t), float(unify)
    t = float(F32(clss_t if vote_t is None else vote_t))
    rows, voted, kc, em, nr, members = [], [], [], [], [], []

    def put(fr, cl, xyz, is_voted, k, e, n, memb):
        rows.append([fr, cl, xyz[0], xyz[1], xyz[2]])
        voted.append(is_voted), kc.append(k), em.append(e), nr.append(n), members.append(memb)

    for fr, cl, an in _candidates(flat, nb_classes, ct, kt):
        u, v, conf = flat[fr, an, -2], flat[fr, an, -1], flat[fr, an, 1 + cl]
        p = xyz64(u, v)
        if len(an) == 1:
            put(fr, cl, p[0], False, 1, float(np.exp(conf[0] ** 2 / t)), 1.0, an)
            continue
        for memb in clusters64(dist64(u, v), un, nms):
            if nms in ("conn-merge", "soft-merge"):
                x, e, n = vote64(conf[memb], p[memb], t)
                put(fr, cl, x, True, len(memb), e, n, an[memb])
            else:
                put(fr, cl, p[memb[0]], False, 1, float(np.exp(conf[memb[0]] ** 2 / t)), 1.0, an[memb])
    diag = {"voted": np.asarray(voted, dtype=bool), "k_cluster": np.asarray(kc, dtype=np.float64),
            "e_max": np.asarray(em, dtype=np.float64), "norm": np.asarray(nr, dtype=np.float64), "members": members}
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), 5), diag


def vote_bound(diag):
    """Per row and component: |x - x64| <= (16 e_max + K_cluster + 16) * 2^-24 / norm.  The float32 exponents exp(c^2 / t) carry
    a few units of relative error, that many units times e_max of absolute error in the softmax argument and so of relative
    error in the weights; the weighted sum adds K_cluster roundings; the unit vectors, the maximum and the normalisation a few
    more; dividing by the vote's norm scales all of it."""
    b = (16.0 * diag["e_max"] + diag["k_cluster"] + 16.0) * U24 / diag["norm"]
    return np.repeat(b[:, None], 3, axis=1)


def margin(decoded, nb_classes, conf_t, clss_t, unify):
    """(smallest |dist64 - unify| over the pairs of different candidates of one frame and class, largest |dist32 - dist64| over
    them, largest float32 distance of a candidate from itself).  A case may be used if the first is at least
    max(1e-3, 16 * the second) degrees; the third must stay below unify, since soft-merge finds the seed in its own cluster by
    that distance."""
    flat64 = np.asarray(decoded, dtype=np.float64).reshape(np.shape(decoded)[0], -1, nb_classes + 3)
    m, dd, own = np.inf, 0.0, 0.0
    for fr, cl, an in _candidates(flat64, nb_classes, np_threshold(conf_t), np_threshold(clss_t)):
        if len(an) < 2:
            continue
        d6, d3 = dist64(flat64[fr, an, -2], flat64[fr, an, -1]), dist32(flat64[fr, an, -2], flat64[fr, an, -1]).astype(np.float64)
        off = ~np.eye(len(an), dtype=bool)
        m = min(m, float(np.abs(d6 - unify)[off].min()))
        dd = max(dd, float(np.abs(d3 - d6)[off].max()))
        own = max(own, float(np.diag(d3).max()))
    return m, dd, own


def growth64(decoded, nb_classes, conf_t, clss_t, unify):
    """The breadth-first growth of conn-merge in every (frame, class) with candidates, in rank space as the kernel grows it:
    per component grown -> (generations, largest frontier, most lane words (rank // 64) that one frontier's rows come from)."""
    flat = np.asarray(decoded, dtype=np.float64).reshape(np.shape(decoded)[0], -1, nb_classes + 3)
    out = []
    for fr, cl, an in _candidates(flat, nb_classes, np_threshold(conf_t), np_threshold(clss_t)):
        near = dist64(flat[fr, an, -2], flat[fr, an, -1]) < unify
        seen = np.zeros(len(an), dtype=bool)
        for seed in range(len(an)):
            if seen[seed]:
                continue
            front = np.zeros(len(an), dtype=bool)
            front[seed] = seen[seed] = True
            gen = big = words = 0
            while front.any():
                front = near[front].any(axis=0) & ~seen
                seen |= front
                if front.any():
                    gen += 1
                    big = max(big, int(front.sum()))
                    words = max(words, len(np.unique(np.flatnonzero(front) // 64)))
            out.append((gen, big, words))
    return out


def margin_ok(decoded, nb_classes, conf_t, clss_t, unify):
    m, dd, own = margin(decoded, nb_classes, conf_t, clss_t, unify)
    return m >= max(1e-3, 16.0 * dd) and own < unify


# ----------------------------------------------------------------------------------------------------------- builders
PASS_CONF, FAIL_CONF = 0.99, 0.0          # objectness of a passing / a failing anchor (thresholds 0.3 and 0.5)
CONF_LO, CONF_HI = 0.55, 0.95             # class confidences of the passing rows: above every threshold used


def _blank(frames, n, c, rs):
    """A decoded tensor none of whose anchors passes the objectness test; the class scores would pass, the directions are
    drawn near the equator band the cases use, so an anchor let through by mistake changes the result."""
    dec = np.zeros((frames, n, c + 3), dtype=F32)
    dec[..., 0] = FAIL_CONF
    dec[..., 1:c + 1] = 0.9
    dec[..., -2] = rs.uniform(-170.0, 170.0, size=(frames, n))
    dec[..., -1] = rs.uniform(-60.0, 60.0, size=(frames, n))
    return dec


def _circle(k, step, lat, start=-170.0):
    """k directions on the circle of latitude ``lat``, neighbours ``step`` degrees of great-circle distance apart."""
    daz = 2.0 * np.rad2deg(np.arcsin(np.sin(np.deg2rad(step) / 2.0) / np.cos(np.deg2rad(lat))))
    assert start + k * daz < 180.0 - 2.0 * step, "the chain must not close round the circle"
    return start + daz * np.arange(k), np.full(k, lat)


def chain(K, N, step, unify, seed, lat=0.0, conf=(CONF_LO, CONF_HI)):
    """2 frames x 2 classes, N anchors; slots (0, 0), (1, 0) and (1, 1) hold K passing rows on a circle of latitude, ``step``
    apart (step < unify: one component; a row is near its floor(unify / step) neighbours on either side, so a breadth-first
    frontier holds up to twice that many rows), at K scattered anchors; slot (0, 1) is empty.  The class confidences, spread
    over ``conf``, are distinct and permuted against the position, differently in every slot, so ranks hop between the lane
    words.  The other N - K anchors fail the objectness test.
    -> (decoded [2][N][5], info)."""
    assert 1 <= K <= N and step < unify
    rs = np.random.RandomState(seed)
    dec = _blank(2, N, 2, rs)
    u, v = _circle(K, step, lat)
    for f in range(2):
        an = np.sort(rs.choice(N, size=K, replace=False))
        dec[f, an, 0] = PASS_CONF
        dec[f, an, -2], dec[f, an, -1] = u, v
        for c in range(2):
            dec[f, an, 1 + c] = np.linspace(conf[0], conf[1], K)[rs.permutation(K)] if (f, c) != (0, 1) else 0.0
    info = {"K": K, "N": N, "C": 2, "unify": unify, "slots": 3, "conn_rows": 3, "max_cluster": K}
    return dec, info


def singles(K, N, seed):
    """1 frame, C = K classes, N anchors: class c has exactly one candidate, at a scattered anchor (``_single`` in every mode).
    -> (decoded [1][N][K + 3], info)."""
    rs = np.random.RandomState(seed)
    dec = _blank(1, N, K, rs)
    an = rs.choice(N, size=K, replace=False)                       # class c sits at anchor an[c]: not in anchor order
    dec[0, an, 1:K + 1] = 0.0
    dec[0, an, 0] = PASS_CONF
    dec[0, an, 1 + np.arange(K)] = np.linspace(CONF_LO, CONF_HI, K)[rs.permutation(K)]
    return dec, {"K": 1, "N": N, "C": K, "rows": K}


def _spread(k):
    """k directions pairwise more than 3.5 degrees apart and none opposite another: a 32 x 32 lattice, latitudes -62 .. 65.1,
    11.25 degrees of azimuth."""
    assert k <= 1024
    i = np.arange(k)
    return -175.0 + 11.25 * (i % 32), -62.0 + 4.1 * (i // 32)


TIES_UNIFY = 2.0


def ties(K, N, block):
    """1 frame, 1 class, N anchors, K passing rows at scattered anchors whose class confidences are equal in runs of ``block``
    candidates (in anchor order); the first run is cut short so that every 64-row boundary lies inside a run; block >= K: all
    equal, at 1.0 (a saturated sigmoid).  The run values are permuted, so rank order is not anchor order.  The directions are
    pairwise farther apart than TIES_UNIFY, so every mode writes one row per candidate and the output order is the rank order.
    -> (decoded [1][N][4], info); info['order']: the anchors in the order the rows must come."""
    rs = np.random.RandomState(1000 + K + block)
    dec = _blank(1, N, 1, rs)
    an = np.sort(rs.choice(N, size=K, replace=False))
    run = np.zeros(K, dtype=np.int64)
    if block < K:                           # the first run is cut short so that no run starts on a multiple of 64
        off = next(o % block for o in range(block // 2, block // 2 + block)
                   if all((edge + o) % block for edge in range(64, K, 64)))
        run = (np.arange(K) + off) // block
    nrun = int(run.max()) + 1
    vals = np.asarray([1.0]) if nrun == 1 else np.linspace(CONF_LO, CONF_HI, nrun)[rs.permutation(nrun)]
    u, v = _spread(K)
    pos = rs.permutation(K)
    dec[0, an, 0] = 1.0 if nrun == 1 else PASS_CONF
    dec[0, an, 1] = vals[run]
    dec[0, an, -2], dec[0, an, -1] = u[pos], v[pos]
    conf = dec[0, an, 1]
    order = an[np.lexsort((np.arange(K), -conf.astype(np.float64)))]
    return dec, {"K": K, "N": N, "C": 1, "unify": TIES_UNIFY, "rows": K, "order": order, "runs": nrun}


TRIPLE_UNIFY = 10.0


def triple():
    """6 frames, 1 class, N = 5: three passing rows A, B, C on the equator, A-B and B-C 8 degrees apart (within unify = 10),
    A-C 16 (not); frame p gives the ranks in the p-th permutation of (A, B, C), frame 0 being A > B > C.  With an end row
    ranked first conn-merge gives one row, soft-merge {first, B} then {B, other end} (B was removed, and is counted again),
    default the two ends; with B ranked first every mode gives one row.
    -> (decoded [6][5][4], info); info['expect'][nms][frame]: the clusters as tuples of anchor indices, in output order."""
    rs = np.random.RandomState(3)
    dec = _blank(6, 5, 1, rs)
    anchors = np.asarray([3, 0, 4])                                 # A, B, C: not in anchor order
    confs = (0.62, 0.60, 0.58)                                      # close: every member carries weight in the vote
    expect = {"conn-merge": [], "soft-merge": [], "default": []}
    for f, perm in enumerate(itertools.permutations(range(3))):     # perm[r]: the point ranked r
        dec[f, anchors, 0] = PASS_CONF
        dec[f, anchors, -2], dec[f, anchors, -1] = np.asarray([-8.0, 0.0, 8.0]), 5.0
        for r, p in enumerate(perm):
            dec[f, anchors[p], 1] = confs[r]
        a = [int(anchors[p]) for p in perm]
        expect["conn-merge"].append([tuple(a)])
        if perm[0] == 1:
            expect["soft-merge"].append([tuple(a)])
            expect["default"].append([(a[0],)])
        else:
            b, other = int(anchors[1]), int(anchors[2 - perm[0]])
            expect["soft-merge"].append([(a[0], b), tuple(x for x in a[1:] if x in (b, other))])
            expect["default"].append([(a[0],), (other,)])
    return dec, {"K": 3, "N": 5, "C": 1, "unify": TRIPLE_UNIFY, "expect": expect}


SQUARE_UNIFY = 5.0


def square():
    """2 frames, 1 class, N = 6: four passing rows at the corners of a square of 4 degrees (sides within unify = 5, diagonals
    5.7 not) with class confidences 0.58 .. 0.62, in two rank orders.  conn-merge votes over all four, soft-merge over a seed
    and its two neighbours (an L, whose mean is not at the seed): no member stands at its cluster's mean and every member
    carries weight, so one member more or less moves the vote far.  -> (decoded [2][6][4], info)."""
    rs = np.random.RandomState(4)
    dec = _blank(2, 6, 1, rs)
    anchors = np.asarray([4, 1, 5, 0])
    for f, confs in enumerate(((0.62, 0.61, 0.59, 0.58), (0.59, 0.62, 0.58, 0.61))):
        dec[f, anchors, 0] = PASS_CONF
        dec[f, anchors, 1] = confs
        dec[f, anchors, -2], dec[f, anchors, -1] = np.asarray([20.0, 24.0, 24.0, 20.0]), np.asarray([-2.0, -2.0, 2.0, 2.0])
    return dec, {"K": 4, "N": 6, "C": 1, "unify": SQUARE_UNIFY}


def at_threshold(thresholds=(0.3, 0.5)):
    """1 frame, 1 class: per threshold t six rows far apart from each other -- the objectness at float32(t), one nextafter below
    and one above it (class confidence 0.9), then the class confidence at those three values (objectness 0.99).
    -> (decoded [1][6 * len(thresholds)][4], info); info['values'][i]: (objectness, class confidence) of anchor i as float64."""
    n = 6 * len(thresholds)
    dec = np.zeros((1, n, 4), dtype=F32)
    u, v = _spread(n)
    dec[0, :, -2], dec[0, :, -1] = u, v
    for k, t in enumerate(thresholds):
        t32 = F32(t)
        three = [np.nextafter(t32, F32(0)), t32, np.nextafter(t32, F32(1))]
        for j, val in enumerate(three):
            dec[0, 6 * k + j, 0], dec[0, 6 * k + j, 1] = val, 0.9
            dec[0, 6 * k + 3 + j, 0], dec[0, 6 * k + 3 + j, 1] = PASS_CONF, val
    return dec, {"N": n, "C": 1, "unify": TIES_UNIFY, "values": dec[0, :, :2].astype(np.float64)}


PATTERNS = ("empty", "first", "last", "alternating", "full")


def pattern_mask(n_slots, pattern):
    on = np.zeros(n_slots, dtype=bool)
    if pattern == "first":
        on[0] = True
    elif pattern == "last":
        on[-1] = True
    elif pattern == "alternating":
        on[::2] = True
    elif pattern == "full":
        on[:] = True
    else:
        assert pattern == "empty"
    return on


def slots(frames, C, N, pattern):
    """frames x C slots of N anchors for the scan and the compaction: a slot that the count pattern switches on holds
    1 + slot % N candidates, pairwise farther apart than TIES_UNIFY, so every mode writes that many rows into it.
    -> (decoded [frames][N][C + 3], info); info['counts']: the rows of every slot."""
    on = pattern_mask(frames * C, pattern).reshape(frames, C)
    want = np.where(on, 1 + np.arange(frames * C).reshape(frames, C) % N, 0)
    dec = np.zeros((frames, N, C + 3), dtype=F32)
    u, v = _spread(N)
    dec[..., 0] = PASS_CONF
    dec[..., -2] = u[None, :] + 0.001 * (np.arange(frames) % 1000)[:, None]        # rows of different frames differ
    dec[..., -1] = v[None, :]
    conf = np.linspace(CONF_HI, CONF_LO, N)                                         # anchor n ranks n-th
    for c in range(C):
        dec[..., 1 + c] = np.where(np.arange(N)[None, :] < want[:, c, None], conf[None, :], 0.0)
    return dec, {"N": N, "C": C, "unify": TIES_UNIFY, "counts": want.reshape(-1)}


WORD_EDGES = ((2, 5), (63, 64), (64, 64), (65, 65), (65, 160), (128, 128), (129, 1000), (1023, 1024), (1024, 1024))
TIES = ((130, 160, 3), (1024, 1024, 64), (1024, 1024, 1024))
SCAN_SHAPES = ((1366, 3, 4), (1025, 1, 4))                          # 4098 slots: past the compaction's grid; 1025: chunk 2
THRESHOLDS = (0.3, 0.5)


def cases():
    """name -> builder of every selection case of tests/test_gpu_select_stage.py (tests/test_select_stage_cpu.py holds each to
    its conditions)."""
    out = {}
    for k, n in WORD_EDGES:
        out["chain K=%d N=%d" % (k, n)] = lambda k=k, n=n: chain(k, n, 0.3, 0.5, seed=k + n)
        out["singles K=%d N=%d" % (k, n)] = lambda k=k, n=n: singles(k, n, seed=k + n)
    out["deep K=200 step 0.8"] = lambda: chain(200, 1024, 0.8, 1.0, seed=11, lat=30.0)
    out["deep K=200 step 0.3"] = lambda: chain(200, 1024, 0.3, 1.0, seed=12)       # +-3 neighbours: frontiers of up to 6 rows
    out["square"] = square
    for k, n, b in TIES:
        out["ties K=%d N=%d block=%d" % (k, n, b)] = lambda k=k, n=n, b=b: ties(k, n, b)
    out["triple"] = triple
    out["at_threshold"] = at_threshold
    for f, c, n in SCAN_SHAPES:
        for pat in PATTERNS:
            out["slots %dx%dx%d %s" % (f, c, n, pat)] = lambda f=f, c=c, n=n, pat=pat: slots(f, c, n, pat)
    return out


# ------------------------------------------------------------------------------------------- class-wise records (K8e)
def classwise_records(frames, C, pattern, seed):
    """seddoa / accdoa decode records [frames][C][4] (activity, x, y, z) whose slots above 0.5 follow the count pattern."""
    rs = np.random.RandomState(seed)
    on = pattern_mask(frames * C, pattern).reshape(frames, C)
    rec = rs.uniform(-1.0, 1.0, size=(frames, C, 4)).astype(F32)
    rec[..., 0] = np.where(on, rs.uniform(0.6, 0.99, size=(frames, C)), rs.uniform(0.01, 0.4, size=(frames, C)))
    return rec


def adpit_records(conf_t, unify, seed, copies=3):
    """ADPIT decode records [copies * 64][1][16] (three activities, three xyz, the three pair distances, one pad): every
    combination of the three track activities above / not above conf_t and the three pair distances below / not below unify
    occurs ``copies`` times, in a shuffled order.  The activities reach above 1 where conf_t >= 1 asks for it."""
    rs = np.random.RandomState(seed)
    codes = rs.permutation(np.repeat(np.arange(64), copies))
    rec = np.zeros((len(codes), 1, 16), dtype=F32)
    rec[:, 0, 3:12] = rs.uniform(-1.0, 1.0, size=(len(codes), 9))
    for k in range(3):
        act_on = (codes >> k) & 1
        near = (codes >> (3 + k)) & 1
        rec[:, 0, k] = np.where(act_on, conf_t + rs.uniform(0.05, 0.4, size=len(codes)), conf_t - rs.uniform(0.05, 0.4, size=len(codes)))
        rec[:, 0, 12 + k] = np.where(near, unify - rs.uniform(0.5, 5.0, size=len(codes)), unify + rs.uniform(0.5, 5.0, size=len(codes)))
    return rec


def adpit_codes(rec, conf_t, unify):
    """The combination every record realises: bit k the activity of track k > conf_t, bit 3 + k the k-th pair distance <
    unify (float32 compares, the thresholds as NumPy takes them)."""
    ct, un = np_threshold(conf_t), np_threshold(unify)
    r = rec.astype(np.float64)
    code = np.zeros(r.shape[:2], dtype=np.int64)
    for k in range(3):
        code |= (r[..., k] > ct).astype(np.int64) << k
        code |= (r[..., 12 + k] < un).astype(np.int64) << (3 + k)
    return code


# ------------------------------------------------------------------------------------------------------------ checks
NMS = ("conn-merge", "soft-merge", "default")


def flat_rows(res):
    """{frame: [[class, x, y, z], ...]} (what the host path returns) -> (R, 5) float64 [frame, class, x, y, z] in dict order."""
    rows = [[fr] + [float(v) for v in d] for fr, dets in res.items() for d in dets]
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), 5)


def check_rows(what, got, ref, diag, host32, collect=None):
    """got (R, 5) against select64's rows: frame and class columns, count and order equal; xyz of the voted rows within
    ``vote_bound`` (``checks.sum_check``), xyz of the rows written alone under ``checks.value_check`` with the float32 host rows
    as the float32 evaluation.  Prints the figures of both; -> (worst err / bound of the voted rows, err of the rows written
    alone), None where there are no such rows."""
    import torch
    from oracle.checks import sum_check, value_check
    run = collect if collect is not None else (lambda check, *a, **kw: check(*a, **kw))
    got, host32 = np.asarray(got, dtype=np.float64).reshape(-1, 5), np.asarray(host32, dtype=np.float64).reshape(-1, 5)
    assert got.shape == ref.shape, "%s: %d rows, float64 statement %d" % (what, len(got), len(ref))
    assert host32.shape == ref.shape, "%s: host %d rows, float64 statement %d" % (what, len(host32), len(ref))
    np.testing.assert_array_equal(got[:, :2], ref[:, :2], err_msg=what)
    np.testing.assert_array_equal(host32[:, :2], ref[:, :2], err_msg=what + " (host)")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))                          # noqa: E731
    v = diag["voted"]
    worst = alone = None
    if v.any():
        worst = run(sum_check, what + ", voted", t(got[v, 2:]), t(ref[v, 2:]), t(vote_bound(diag)[v]))
    if (~v).any():
        alone = run(value_check, what + ", alone", t(got[~v, 2:]), t(ref[~v, 2:]), t(host32[~v, 2:]))
    return worst, alone
