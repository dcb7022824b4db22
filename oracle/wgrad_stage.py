"""Oracle (test infrastructure): cases, inputs, float64 references and the checker of the 3x3 weight-gradient tests (K2-wgrad:
``conv3x3_wgrad_kernel<TW>`` and ``stem_wgrad_kernel`` in csrc/conv.hip, ``wino_wgrad_kernel<NT,RAGGED>`` in csrc/wino.hip,
``wino4_wgrad_kernel<AFF,NB>`` in csrc/wino4w.hip, with their slab-reduce and finish kernels).  tests/test_wgrad_stage_cpu.py pins
everything here on the CPU, tests/test_gpu_wgrad_stage.py compares the kernels with it.

``plan(form, N, H, W, Cin, Cout)`` restates the host work split of a launch (``wgrad_splits``, ``wino_wgrad_geometry``,
``wino4_wgrad_geometry``) independently; the GPU module asserts it against ``adyolo_wgrad_plan`` on every case, so what
``branches`` says a case exercises is a statement about the code that runs.  ``CASES`` are small shapes that together reach every
named branch of every form (``coverage`` asserts it), among them the geometries of the three older tests of
tests/test_gpu_kernels.py.

Layouts: x [N][H][W][Cin], dy [N][H][W][Cout] (channels last), dw [Cout][Cin_real][3][3].  ``build`` gives x of order 1 with a
non-zero mean, dy of order 1e-2 and a handful of isolated values about 1e3 x the rms (``spike_rows``: image corners, last row and
column, the rows either side of every work boundary of the plan, first and last row of every sample), in x and in dy: a dropped,
doubled or cross-sample row then moves dw by orders of magnitude more than rounding can.

The bound, entry-wise and a priori (u = 2^-24):

    |got - ref| <= c(form) * u * S

S is the contraction evaluated on absolute values in float64 -- for the direct and the stem kernel sum |dy| |x'| over the pixels of
the tap; for the two Winograd forms the absolute-value evaluation of the algorithm itself,
|G|^T [ sum_tiles (|B^T| |d| |B|) (.) (|A| |e| |A^T|) ] |G| with the matrices of wino.hip (F(2x2)) and wino4_common.hpp / wino4w.hip
(F(4x4), points 0, +-3/4, +-3/2, infinity): the transforms cancel, so the plain sum |dy| |x| is smaller than what the kernel's
roundings are relative to.  |x'| = |x| |scale| + |shift| under the affine (the direct kernel may round the product and the sum
separately).  c counts the roundings a term can meet on its way into dw, one (1 + delta) each, |delta| <= u:

    c = n + t_x + t_dy + 1 (the product) + r + 1 (the slab sum, in double, rounded once) + t_G + (2 under the affine)

    n     the float32 terms one accumulator sums in the longest workgroup of the plan:
          direct  items_per_split_max * (256 / 4)      a wave's share of each 256-pixel tile
          stem    ceil(rows per workgroup / 4) * W     a wave takes every fourth row
          wino2   items_per_split_max * seg * 8        eight tiles of a strip per tile row
          wino4   items_per_split_max * seg * 8        eight tiles of a pair of runs per step
    t_x   the depth of the input transform: 0 | 0 | 2 (one addition per direction) | 4 (two fused operations per direction)
    t_dy  the same for dy: 0 | 0 | 2 | 6 (a6v: three deep per direction)
    r     the additions that join the four waves' accumulators: 3 | 3 | 0 | 0
    t_G   G^T . G: 0 | 0 | 4 (two additions per direction in float32) | 1 (in double, rounded once)

Any order of summation stays inside n u sum |terms| to first order; the slack between n - 1 and n covers the second order for
n < 2^20.  Nothing here is fitted to a kernel's result.

``emulate`` is a float32 model of each algorithm (direct, F(2x2) domain, F(4x4) domain; float32 transforms, products and
accumulation in a fixed order): the CPU module shows that ``check`` passes it -- the bound is loose enough for a correct
implementation -- and that the mutations of ``MUTATIONS`` applied to the float64 reference exceed it -- tight enough."""
import functools

import numpy as np
import torch

U = 2.0 ** -24
F32 = np.float32
SENT = np.float32(-777.25)
GUARD = 64                                   # sentinel floats in front of and behind dw
FORMS = ("direct", "stem", "wino2", "wino4")
FORM_ID = {"direct": 0, "stem": 1, "wino2": 2, "wino4": 3}
KERNEL = {"direct": "conv3x3_wgrad_kernel", "stem": "conv3x3_wgrad_kernel", "wino2": "wino_wgrad_kernel",
          "wino4": "wino4_wgrad_kernel"}


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------ plans
def _deal(p):
    p["items_per_split_max"] = cdiv(p["nitems"], p["nsplit"])
    p["items_per_split_min"] = p["nitems"] // p["nsplit"]
    return p


def plan(form, n, h, w, cin, cout):
    """The work split of one launch.  Keys: supported, nsplit (workgroups per channel block = slabs), nitems, nseg, seg, last_seg,
    items_per_split_max / _min, and per form tw (direct), nblk / rows / per (stem), nt / ragged / tiles_h (wino2), nb / npairs /
    nruns (wino4)."""
    assert form in FORMS
    if form in ("direct", "stem"):
        ok = cout % 32 == 0 and (cin == 8 or cin % 32 == 0)
        if form == "stem":
            ok = ok and cin == 8 and cout == 32 and n * h < 2 ** 31
        if not ok:
            return {"form": form, "supported": False}
        tw = 32 if w >= 32 else 16
        th = 256 // tw
        ntiles = n * cdiv(h, th) * cdiv(w, tw)
        blocks = (cout // 32) * cdiv(cin, 32)
        nsplit = min(max(1024 // blocks, 1), ntiles)
        if form == "direct":
            return _deal({"form": form, "supported": True, "nsplit": nsplit, "nitems": ntiles, "nseg": 1, "seg": th, "last_seg": th,
                          "tw": tw, "th": th, "ragged": h % th != 0 or w % tw != 0})
        nblk = min(nsplit, 512)
        rows = n * h
        per = cdiv(rows, nblk)
        used = cdiv(rows, per)
        return {"form": form, "supported": True, "nsplit": nsplit, "nblk": nblk, "nitems": rows, "rows": rows, "per": per, "nseg": 1,
                "seg": per, "last_seg": rows - (used - 1) * per, "used": used, "tw": 64,
                "items_per_split_max": per, "items_per_split_min": rows - (used - 1) * per if used == nblk else 0}
    if form == "wino2":
        if cin % 32 or cout % 32 or h * w * max(cin, cout) * 4 >= 2 ** 31:
            return {"form": form, "supported": False}
        nt = 2 if cout % 64 == 0 else 1
        tiles_h, tiles_w = cdiv(h, 2), cdiv(w, 16)
        pairs = (cout // (32 * nt)) * (cin // 32)
        nsplit0 = max(512 // pairs, 1)
        strips = n * tiles_w
        best = None
        for want in range(1, tiles_h // 4 + 2):
            seg = cdiv(tiles_h, want)
            seg += seg & 1
            seg = max(seg, 8)
            nseg = cdiv(tiles_h, seg)
            nitems = strips * nseg
            nsplit = min(nitems, nsplit0)
            cost = cdiv(nitems, nsplit) * (0.5 * seg + 1.5)
            if best is None or cost < best[0] - 1e-9:
                best = (cost, seg, nseg, nsplit)
            if seg == 8:
                break
        _, seg, nseg, nsplit = best
        return _deal({"form": form, "supported": True, "nsplit": nsplit, "nitems": strips * nseg, "nseg": nseg, "seg": seg,
                      "last_seg": tiles_h - (nseg - 1) * seg, "nt": nt, "ragged": w % 16 != 0 or h % 2 != 0, "tiles_h": tiles_h,
                      "strips": strips})
    ok = cin % 32 == 0 and cout % 32 == 0 and (w % 16 == 0 or w in (4, 8)) and h % 4 == 0 and h >= 8
    ok = ok and n * h * w * max(cin, cout) * 4 < 2 ** 31
    if not ok:
        return {"form": form, "supported": False}
    nruns = n * (w // 16) if w >= 16 else cdiv(n, 16 // w)
    npairs = (nruns + 1) // 2
    nblk = (cout // (64 if cout % 64 == 0 else 32)) * (cin // 32)
    nsplit = max(256 // nblk, 1)
    steps = h // 4
    best, nseg, seg = None, 1, steps
    for c in range(1, (steps // 8 if steps >= 16 else 1) + 1):
        ss = cdiv(steps, c)
        ns = cdiv(steps, ss)
        items = npairs * ns
        cost = cdiv(items, min(nsplit, items)) * (ss + 2)
        if best is None or cost < best:
            best, nseg, seg = cost, ns, ss
    nitems = npairs * nseg
    return _deal({"form": form, "supported": True, "nsplit": min(nsplit, nitems), "nitems": nitems, "nseg": nseg, "seg": seg,
                  "last_seg": steps - (nseg - 1) * seg, "nb": 2 if cout % 64 == 0 else 1, "npairs": npairs, "nruns": nruns,
                  "channel_blocks": nblk})


def plan_out8(p):
    """What ``adyolo_wgrad_plan`` reports for the launch of ``p``."""
    if not p["supported"]:
        return [0] * 8
    f = p["form"]
    width = {"direct": 1, "stem": 1, "wino2": p.get("nt"), "wino4": p.get("nb")}[f]
    return [p["nsplit"], p["nitems"], p["nseg"], p["seg"], width, p["tw"] if f in ("direct", "stem") else 16,
            p["nblk"] if f == "stem" else 0, 1]


def row_boundaries(case):
    """Image rows r (0 < r < H) at which one work item of the plan ends and the next begins (stem: rows of the whole batch,
    N * H of them, at which a workgroup's run ends)."""
    p = case_plan(case)
    f, h = case["form"], case["h"]
    if f == "direct":
        return list(range(p["th"], h, p["th"]))
    if f == "stem":
        return list(range(p["per"], p["rows"], p["per"]))
    per_row = 2 if f == "wino2" else 4
    return [s * p["seg"] * per_row for s in range(1, p["nseg"])]


# --------------------------------------------------------------------------------------------------------------- branches
ALL_BRANCHES = {
    "direct": {"tw16", "tw32", "ragged", "not_ragged", "image_smaller_than_tile", "one_item_per_split", "several_items_even",
               "several_items_uneven", "several_items_ragged", "affine", "no_affine", "cin_real_lt_cin"},
    "stem": {"nblk_capped", "nblk_not_capped", "rows_per_workgroup_not_multiple_of_4", "rows_per_workgroup_multiple_of_4",
             "chunk_spans_two_samples", "workgroup_without_rows", "w_lt_64", "w_eq_64", "w_gt_64", "w_not_multiple_of_64",
             "cin_real_lt_cin", "no_affine"},
    "wino2": {"nt1", "nt2", "ragged", "not_ragged", "one_segment", "several_segments", "short_last_segment",
              "image_shorter_than_min_segment", "odd_tile_rows_in_segment", "one_item_per_split", "several_items_even",
              "several_items_uneven", "several_items_nt1", "several_items_nt2", "several_items_ragged", "several_items_affine",
              "affine", "no_affine", "cin_real_lt_cin"},
    "wino4": {"nb1", "nb2", "one_segment", "several_segments", "short_last_segment", "one_item_per_split", "several_items_even",
              "several_items_uneven", "several_items_nb1", "several_items_nb2", "several_items_short_last_segment",
              "several_items_affine", "half_empty_last_pair", "last_segment_of_one_step", "w4", "w8", "w16", "w32", "w48", "w64", "affine", "no_affine",
              "cin_real_lt_cin"},
}


def branches(p, affine, cin_real, case=None):
    """The named branches a launch with plan ``p`` exercises (``case``: its shape, for the branches that depend on H and W)."""
    f = p["form"]
    out = set()
    out.add("affine" if affine else "no_affine")
    cin = case["cin"] if case else None
    if case and cin_real < cin:
        out.add("cin_real_lt_cin")
    several = p["items_per_split_max"] > 1
    if f != "stem":
        if not several:
            out.add("one_item_per_split")
        elif p["items_per_split_max"] == p["items_per_split_min"]:
            out.add("several_items_even")
        else:
            out.add("several_items_uneven")
    if f == "direct":
        out.add("tw%d" % p["tw"])
        out.add("ragged" if p["ragged"] else "not_ragged")
        if several and p["ragged"]:
            out.add("several_items_ragged")
        if case and case["h"] < p["th"] and case["w"] < p["tw"]:
            out.add("image_smaller_than_tile")
    elif f == "stem":
        out.add("nblk_capped" if p["nsplit"] > 512 else "nblk_not_capped")
        out.add("rows_per_workgroup_multiple_of_4" if p["per"] % 4 == 0 else "rows_per_workgroup_not_multiple_of_4")
        if p["used"] < p["nblk"]:
            out.add("workgroup_without_rows")
        if case:
            h, w = case["h"], case["w"]
            # a four-row chunk r0 + 4 c .. + 3 of a workgroup's run holds rows of two samples
            if any((r0 + 4 * c) // h != min(r0 + 4 * c + 3, min(p["rows"], r0 + p["per"]) - 1) // h
                   for r0 in range(0, p["rows"], p["per"]) for c in range(cdiv(min(p["per"], p["rows"] - r0), 4))):
                out.add("chunk_spans_two_samples")
            out.add("w_lt_64" if w < 64 else "w_eq_64" if w == 64 else "w_gt_64")
            if w % 64:
                out.add("w_not_multiple_of_64")
    elif f == "wino2":
        out.add("nt%d" % p["nt"])
        out.add("ragged" if p["ragged"] else "not_ragged")
        out.add("one_segment" if p["nseg"] == 1 else "several_segments")
        if p["nseg"] > 1 and p["last_seg"] < p["seg"]:
            out.add("short_last_segment")
        if p["tiles_h"] < 8:
            out.add("image_shorter_than_min_segment")
        if p["last_seg"] % 2 or (p["nseg"] > 1 and p["seg"] % 2):
            out.add("odd_tile_rows_in_segment")
        if several:
            out.add("several_items_nt%d" % p["nt"])
            if p["ragged"]:
                out.add("several_items_ragged")
            if affine:
                out.add("several_items_affine")
    else:
        out.add("nb%d" % p["nb"])
        out.add("one_segment" if p["nseg"] == 1 else "several_segments")
        short = p["nseg"] > 1 and p["last_seg"] < p["seg"]
        if short:
            out.add("short_last_segment")
        if short and p["last_seg"] == 1:
            out.add("last_segment_of_one_step")
        if p["nruns"] % 2:
            out.add("half_empty_last_pair")
        if case and case["w"] in (4, 8, 16, 32, 48, 64):
            out.add("w%d" % case["w"])
        if several:
            out.add("several_items_nb%d" % p["nb"])
            if short:
                out.add("several_items_short_last_segment")
            if affine:
                out.add("several_items_affine")
    return out


# ------------------------------------------------------------------------------------------------------------------ cases
def make_case(form, n, h, w, cin, cout, affine=False, cin_real=None):
    cin_real = cin if cin_real is None else cin_real
    name = "%s_%dx%dx%d_c%d_%d%s%s" % (form, n, h, w, cin, cout, "_aff" if affine else "",
                                       "_real%d" % cin_real if cin_real != cin else "")
    return {"form": form, "n": n, "h": h, "w": w, "cin": cin, "cout": cout, "affine": bool(affine), "cin_real": cin_real,
            "name": name, "seed": 9000 + 131 * n + 17 * h + 7 * w + cin + 3 * cout + FORM_ID[form]}


def case_plan(case):
    return plan(case["form"], case["n"], case["h"], case["w"], case["cin"], case["cout"])


def case_branches(case):
    return branches(case_plan(case), case["affine"], case["cin_real"], case)


def _older_geometries():
    """The shapes of test_conv3x3_dgrad_wgrad, test_wino4_wgrad_every_geometry and test_conv3x3_fused_affine_mask_stats
    (tests/test_gpu_kernels.py), through every kernel that takes them there."""
    out = []
    dgrad = [(2, 16, 64, 32, 32), (2, 13, 32, 32, 64), (1, 18, 16, 64, 128), (1, 9, 16, 256, 256), (3, 40, 64, 32, 32),
             (2, 150, 24, 32, 64), (1, 67, 37, 64, 32), (6, 132, 16, 256, 256), (2, 21, 19, 96, 32)]
    for s in dgrad:
        out.append(make_case("direct", *s))
        out.append(make_case("wino2", *s))
        if plan("wino4", *s)["supported"]:
            out.append(make_case("wino4", *s))
    for s in [(2, 20, 64), (3, 11, 37), (1, 5, 64), (5, 3, 6)]:
        out.append(make_case("stem", s[0], s[1], s[2], 8, 32, cin_real=7))
    w4 = [(2, 8, 16, 32, 64, 0), (1, 8, 16, 32, 64, 1), (3, 40, 16, 64, 64, 1), (5, 36, 32, 64, 128, 1), (2, 64, 32, 32, 64, 0),
          (1, 100, 48, 32, 64, 1), (2, 24, 64, 64, 64, 0), (4, 300, 32, 64, 64, 1), (3, 28, 16, 96, 192, 1), (2, 64, 64, 32, 32, 1),
          (3, 20, 48, 64, 32, 0), (1, 12, 16, 32, 96, 1), (5, 36, 4, 64, 64, 1), (7, 64, 4, 128, 128, 0), (3, 40, 8, 64, 128, 0),
          (2, 24, 8, 64, 64, 1), (9, 16, 4, 32, 32, 1)]
    for s in w4:
        out.append(make_case("wino4", *s[:5], affine=s[5]))
    for s in [(2, 20, 64, 32, 32), (3, 17, 16, 64, 128), (2, 9, 32, 32, 64), (2, 37, 16, 128, 64)]:
        out.append(make_case("direct", *s, affine=True))
        out.append(make_case("wino2", *s, affine=True))
        if plan("wino4", *s)["supported"]:
            out.append(make_case("wino4", *s, affine=True))
    return out


def _edge_cases():
    """Found with ``plan``: the branches the older geometries do not reach."""
    c = make_case
    return [
        # F(4x4): several items per workgroup
        c("wino4", 18, 16, 16, 256, 256),                     # 9 items on 8 splits (uneven), NB = 2
        c("wino4", 6, 64, 16, 512, 512, affine=True),         # 6 items on 2 splits, two segments, even deal
        c("wino4", 40, 16, 4, 512, 512),                      # narrow runs, 5 items on 2 splits
        c("wino4", 9, 32, 16, 256, 512, affine=True),         # 5 items on 4 splits
        c("wino4", 5, 68, 16, 512, 512, affine=True),         # segments of 9 and 8 steps, 6 items on 2 splits, half-empty last pair
        c("wino4", 12, 16, 16, 256, 480),                     # NB = 1: 15 x 8 channel blocks, 6 items on 2 splits
        c("wino4", 5, 72, 16, 512, 288, affine=True),         # NB = 1, two segments, 6 items on 1 split
        c("wino4", 2, 16, 32, 32, 32, cin_real=10),           # the MIC stem: 10 real channels of 32
        c("wino4", 2, 292, 16, 32, 32),                       # 73 steps = 8 x 9 + 1: the last segment is a single step (NB = 1)
        c("wino4", 1, 292, 16, 64, 64, affine=True),          # the same with NB = 2 and half a pair
        # F(2x2): several items per workgroup with NT = 1, ragged, with the affine
        c("wino2", 40, 16, 16, 256, 96, affine=True),         # NT = 1, 40 strips on 21 splits
        c("wino2", 9, 21, 40, 256, 96),                       # NT = 1, ragged, 27 items on 21 splits
        c("wino2", 9, 33, 19, 256, 256, affine=True),         # NT = 2, ragged, affine, segments of 10 and 7: 36 items on 16 splits
        c("wino2", 24, 18, 16, 256, 256, affine=True),        # NT = 2, affine, 24 items on 16 splits
        c("wino2", 32, 16, 16, 256, 256),                     # even deal: 32 items on 16 splits
        c("wino2", 2, 70, 16, 32, 32),                        # several segments, the last one shorter
        c("wino2", 2, 16, 32, 32, 64, cin_real=10),           # the MIC stem
        c("wino2", 1, 6, 5, 32, 32),                          # image shorter than a segment and narrower than a strip
        # direct: several tiles per workgroup, ragged; an image smaller than a tile
        c("direct", 7, 37, 45, 256, 256, affine=True),        # 70 tiles on 16 splits
        c("direct", 32, 16, 16, 256, 256),                    # TW = 16, 32 tiles on 16 splits: an even deal
        c("direct", 2, 5, 9, 32, 32),                         # smaller than one tile
        c("direct", 2, 16, 32, 32, 64, cin_real=10),          # the MIC stem through the direct kernel
        c("direct", 2, 12, 20, 8, 32, affine=True, cin_real=7),  # the 8-channel stem with an affine: not the stem kernel's
        # stem: the 512-workgroup cap
        c("stem", 4, 1043, 32, 8, 32, cin_real=7),            # 524 tiles -> capped, 9 rows per workgroup, ragged rows
        c("stem", 2, 688, 80, 8, 32, cin_real=7),             # 516 tiles -> capped, W > 64 and not a multiple of 64
        c("stem", 3, 64, 128, 8, 32, cin_real=7),             # rows per workgroup a multiple of 4, W a multiple of 64
    ]


@functools.lru_cache(maxsize=None)
def _cases():
    seen, out = set(), []
    for cs in _older_geometries() + _edge_cases():
        if cs["name"] not in seen:
            seen.add(cs["name"])
            out.append(cs)
    return tuple(out)


CASES = _cases()


def cases(form=None):
    return [c for c in CASES if form is None or c["form"] == form]


MAX_ELEMENTS = 4 * 2 ** 20 + 2 ** 18            # "about 4 M" elements in a case's larger tensor


def coverage():
    """Asserts that CASES reach every named branch of every form, that every case is supported and small.  -> {form: {branch:
    [case names]}}"""
    table = {}
    for f in FORMS:
        got = {}
        for cs in cases(f):
            p = case_plan(cs)
            assert p["supported"], cs["name"]
            assert cs["n"] * cs["h"] * cs["w"] * max(cs["cin"], cs["cout"]) <= MAX_ELEMENTS, cs["name"]
            for b in case_branches(cs):
                got.setdefault(b, []).append(cs["name"])
        missing = ALL_BRANCHES[f] - set(got)
        extra = set(got) - ALL_BRANCHES[f]
        assert not missing and not extra, "%s: missing %s, unknown %s" % (f, sorted(missing), sorted(extra))
        table[f] = got
    return table


# ----------------------------------------------------------------------------------------------------------------- inputs
def spike_rows(case):
    """[(sample, row)]: first and last row of every sample and the rows either side of every work boundary of the plan (at most
    the first and last three boundaries of a sample; the stem's boundaries are rows of the whole batch)."""
    n, h = case["n"], case["h"]
    rows = set()
    for s in range(n):
        rows.add((s, 0))
        rows.add((s, h - 1))
    bnd = row_boundaries(case)
    bnd = bnd if len(bnd) <= 6 else bnd[:3] + bnd[-3:]
    if case["form"] == "stem":
        for g in bnd:
            for r in (g - 1, g):
                rows.add((r // h, r % h))
    else:
        for s in range(n):
            for r in bnd:
                rows.add((s, r - 1))
                rows.add((s, r))
    return sorted(rows)


def build(case):
    """-> dict x, dy (float32, channels last), scale, shift (float32 [Cin]; used only under the affine), spikes [(sample, row)]."""
    rng = np.random.default_rng(case["seed"])
    n, h, w, cin, cout = (case[k] for k in ("n", "h", "w", "cin", "cout"))
    x = (rng.standard_normal((n, h, w, cin)) * 0.7 + 0.3).astype(F32)
    dy = (rng.standard_normal((n, h, w, cout)) * 1e-2).astype(F32)
    spikes = spike_rows(case)
    for s, r in spikes:
        for col in {0, w - 1, int(rng.integers(0, w))}:       # the corners, the last column and one place in between
            x[s, r, col, int(rng.integers(0, case["cin_real"]))] = F32(rng.choice((-1.0, 1.0)) * 1e3)
            dy[s, r, col, int(rng.integers(0, cout))] = F32(rng.choice((-1.0, 1.0)) * 10.0)
    scale = (rng.random(cin) + 0.5).astype(F32)
    shift = rng.standard_normal(cin).astype(F32)
    return {"x": x, "dy": dy, "scale": scale, "shift": shift, "spikes": spikes}


def _affine64(case, inp, absolute=False, pad_value_shift=False):
    """x seen through the affine, float64 torch [N][Cin][H + 2][W + 2] with the zero padding applied AFTER the affine
    (pad_value_shift: the mutation that applies the shift to the padding)."""
    x = torch.from_numpy(inp["x"]).double()
    if case["affine"]:
        sc, sh = torch.from_numpy(inp["scale"]).double(), torch.from_numpy(inp["shift"]).double()
        x = x.abs() * sc.abs() + sh.abs() if absolute else x * sc + sh
    elif absolute:
        x = x.abs()
    x = x.permute(0, 3, 1, 2)
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    if pad_value_shift and case["affine"]:
        sh = torch.from_numpy(inp["shift"]).double()[None, :, None, None]
        border = torch.ones_like(xp)
        border[:, :, 1:-1, 1:-1] = 0
        xp = xp + border * sh
    return xp


def _dy64(inp, absolute=False):
    d = torch.from_numpy(inp["dy"]).double().permute(0, 3, 1, 2)
    return d.abs() if absolute else d


def _wgrad64(xp, dy, cin, cout):
    """float64 weight gradient of the 3x3 convolution from an already padded input."""
    return torch.nn.grad.conv2d_weight(xp.contiguous(), (cout, cin, 3, 3), dy.contiguous(), padding=0)


def reference(case, inp, pad_value_shift=False):
    """float64 dw [Cout][Cin_real][3][3] by ``torch.nn.grad.conv2d_weight`` on x * scale + shift, zero padding after the affine."""
    dw = _wgrad64(_affine64(case, inp, pad_value_shift=pad_value_shift), _dy64(inp), case["cin"], case["cout"])
    return dw[:, :case["cin_real"]].contiguous().numpy()


# Winograd matrices.  F(2x2, 3x3): wino.hip; F(4x4, 3x3), points 0, +-3/4, +-3/2, infinity: wino4_common.hpp, wino4w.hip
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
A2M = np.array([[1, 0], [1, 1], [1, -1], [0, -1]], dtype=np.float64)
G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
_a, _b = 0.75, 1.5
_a2, _b2 = _a * _a, _b * _b
BT4 = np.array([[_a2 * _b2, 0, -(_a2 + _b2), 0, 1, 0], [0, -_a * _b2, -_b2, _a, 1, 0], [0, _a * _b2, -_b2, -_a, 1, 0],
                [0, -_b * _a2, -_a2, _b, 1, 0], [0, _b * _a2, -_a2, -_b, 1, 0], [0, _a2 * _b2, 0, -(_a2 + _b2), 0, 1]])
A4M = np.array([[1, 0, 0, 0], [1, _a, _a2, _a ** 3], [1, -_a, _a2, -_a ** 3], [1, _b, _b2, _b ** 3], [1, -_b, _b2, -_b ** 3],
                [0, 0, 0, 1]])
_na, _nb = 2 * _a2 * (_a2 - _b2), 2 * _b2 * (_b2 - _a2)
G4 = np.array([[1 / (_a2 * _b2), 0, 0], [1 / _na, _a / _na, _a2 / _na], [1 / _na, -_a / _na, _a2 / _na], [1 / _nb, _b / _nb, _b2 / _nb],
               [1 / _nb, -_b / _nb, _b2 / _nb], [0, 0, 1]])
WINO = {"wino2": (2, BT2, A2M, G2), "wino4": (4, BT4, A4M, G4)}


def winograd_wgrad(xp, dy, m, bt, am, g, dtype=torch.float64, chunk_rows=None):
    """dw = G^T [ sum over m x m output tiles (B^T d B) (.) (A e A^T) ] G with the given matrices, on torch tensors
    xp [N][Cin][H + 2][W + 2] (padded) and dy [N][Cout][H][W]; arithmetic in ``dtype``.  chunk_rows: accumulate tile row by tile
    row (a fixed order, for the float32 emulation) instead of in one contraction.  -> [Cout][Cin][3][3]"""
    n, cin, hp, wp = xp.shape
    h, w = hp - 2, wp - 2
    th, tw = cdiv(h, m), cdiv(w, m)
    xp = torch.nn.functional.pad(xp, (0, tw * m - w, 0, th * m - h)).to(dtype)
    dy = torch.nn.functional.pad(dy, (0, tw * m - w, 0, th * m - h)).to(dtype)
    bt, am, g = (torch.as_tensor(a).to(dtype) for a in (bt, am, g))
    d = xp.unfold(2, m + 2, m).unfold(3, m + 2, m)                       # [N][Cin][th][tw][m+2][m+2]
    e = dy.unfold(2, m, m).unfold(3, m, m)                               # [N][Cout][th][tw][m][m]
    p = m + 2
    du = torch.zeros(p, p, cin, dy.shape[1], dtype=dtype)
    step = th if chunk_rows is None else chunk_rows
    for t0 in range(0, th, step):
        v = torch.einsum("ai,nchwij,bj->abnhwc", bt, d[:, :, t0:t0 + step], bt).reshape(p, p, -1, cin)
        ee = torch.einsum("ai,nohwij,bj->abnhwo", am, e[:, :, t0:t0 + step], am).reshape(p, p, -1, dy.shape[1])
        du = du + torch.matmul(v.transpose(2, 3), ee)
    return torch.einsum("ak,abco,bl->ockl", g, du, g)


def magnitude(case, inp):
    """S of the bound, float64 [Cout][Cin_real][3][3]."""
    xp, dy = _affine64(case, inp, absolute=True), _dy64(inp, absolute=True)
    if case["form"] in ("direct", "stem"):
        s = _wgrad64(xp, dy, case["cin"], case["cout"])
    else:
        m, bt, am, g = WINO[case["form"]]
        s = winograd_wgrad(xp, dy, m, np.abs(bt), np.abs(am), np.abs(g))
    return s[:, :case["cin_real"]].contiguous().numpy()


def roundings(case):
    """c(form) of the bound: see the module's docstring."""
    p = case_plan(case)
    f = case["form"]
    if f == "direct":
        c = p["items_per_split_max"] * 64 + 0 + 0 + 1 + 3 + 1 + 0
    elif f == "stem":
        c = cdiv(p["per"], 4) * case["w"] + 0 + 0 + 1 + 3 + 1 + 0
    elif f == "wino2":
        c = p["items_per_split_max"] * p["seg"] * 8 + 2 + 2 + 1 + 0 + 1 + 4
    else:
        c = p["items_per_split_max"] * p["seg"] * 8 + 4 + 6 + 1 + 0 + 1 + 1
    return c + (2 if case["affine"] else 0)


def bound(case, inp):
    return roundings(case) * U * magnitude(case, inp)


@functools.lru_cache(maxsize=None)
def prepared(name):
    """(case, inputs, reference, bound) of a case of CASES by name, computed once and shared (treat as read-only)."""
    case = next(c for c in _cases() if c["name"] == name)
    inp = build(case)
    return case, inp, reference(case, inp), bound(case, inp)


# ------------------------------------------------------------------------------------------------------------------ check
def dw_floats(case):
    return case["cout"] * case["cin_real"] * 9


def new_dw_buffer(case):
    """The output buffer of a case: GUARD sentinels, Cout * Cin_real * 9 floats of NaN (the kernel must write every one),
    GUARD sentinels."""
    buf = np.full(2 * GUARD + dw_floats(case), SENT, dtype=F32)
    buf[GUARD:GUARD + dw_floats(case)] = np.nan
    return buf


def check(case, ref, bnd, dwbuf):
    """dwbuf: the whole output buffer after the call.  Guard words bitwise unchanged, no NaN in dw, every element within its
    bound.  -> worst err / bound"""
    out = np.asarray(dwbuf, dtype=F32).reshape(-1)
    nf = dw_floats(case)
    assert out.size == 2 * GUARD + nf, "%s: output buffer of %d floats" % (case["name"], out.size)
    guard = np.concatenate([out[:GUARD], out[GUARD + nf:]])
    changed = guard.view(np.int32) != SENT.view(np.int32)
    assert not changed.any(), "%s: %d guard words beside dw changed" % (case["name"], int(changed.sum()))
    got = out[GUARD:GUARD + nf].astype(np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), "%s: %d of %d elements of dw are not finite" % (case["name"], int((~np.isfinite(got)).sum()), nf)
    err = np.abs(got - ref)
    ratio = float((err / bnd).max())
    assert (err <= bnd).all(), "%s: %d of %d elements over the bound, worst err / bound %.3f (err %.3e)" % (
        case["name"], int((err > bnd).sum()), nf, ratio, float(err.max()))
    return ratio


# -------------------------------------------------------------------------------------------------------------- emulation
def emulate(case, inp, algorithm):
    """float32 model of one algorithm ("direct", "wino2", "wino4") on the case's inputs, whatever kernel the case names: float32
    affine, transforms, products and sums, accumulated image row by image row / tile row by tile row.  -> the output buffer"""
    x = torch.from_numpy(inp["x"])
    if case["affine"]:
        x = x * torch.from_numpy(inp["scale"]) + torch.from_numpy(inp["shift"])
    xp = torch.nn.functional.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1)).contiguous()
    dy = torch.from_numpy(inp["dy"]).permute(0, 3, 1, 2).contiguous()
    cin, cout, h, w = case["cin"], case["cout"], case["h"], case["w"]
    if algorithm == "direct":
        dw = torch.zeros(cout, cin, 3, 3, dtype=torch.float32)
        for r in range(h):
            for ky in range(3):
                for kx in range(3):
                    dw[:, :, ky, kx] += torch.einsum("now,ncw->oc", dy[:, :, r, :], xp[:, :, r + ky, kx:kx + w])
    else:
        m, bt, am, g = WINO[algorithm]
        dw = winograd_wgrad(xp, dy, m, bt, am, g, dtype=torch.float32, chunk_rows=1)
    buf = new_dw_buffer(case)
    buf[GUARD:GUARD + dw_floats(case)] = dw[:, :case["cin_real"]].contiguous().numpy().reshape(-1)
    return buf


# -------------------------------------------------------------------------------------------------------------- mutations
MUTATIONS = ("drop_boundary_row", "row_twice", "halo_from_neighbouring_sample", "shift_on_padding", "write_padded_channels")


def _row_contribution(case, inp, sample, row):
    """What the products of dy row (sample, row) add to dw: float64 [Cout][Cin_real][3][3]."""
    xp = _affine64(case, inp)[sample:sample + 1, :, row:row + 3, :]
    dy = _dy64(inp)[sample:sample + 1, :, row:row + 1, :]
    return _wgrad64(xp, dy, case["cin"], case["cout"])[:, :case["cin_real"]].numpy()


def mutation_row(case, inp):
    """The (sample, row) the row mutations act on: a row next to a work boundary of the plan where there is one, else the last
    row of the last sample (every such row carries spikes)."""
    bnd = row_boundaries(case)
    if bnd and case["form"] == "stem":
        return bnd[0] // case["h"], bnd[0] % case["h"]
    if bnd:
        return case["n"] - 1, bnd[-1]
    return case["n"] - 1, case["h"] - 1


def mutate(case, inp, ref, what):
    """The output buffer a kernel with the named fault would leave, built from the float64 reference; None where the mutation
    does not apply to the case."""
    assert what in MUTATIONS
    dw = ref
    buf = new_dw_buffer(case)
    if what in ("drop_boundary_row", "row_twice"):
        s, r = mutation_row(case, inp)
        dw = ref + (-1.0 if what == "drop_boundary_row" else 1.0) * _row_contribution(case, inp, s, r)
    elif what == "halo_from_neighbouring_sample":
        # row -1 of sample s reads the last row of sample s - 1 (of itself in a batch of one) instead of the padding
        s = case["n"] - 1
        xa = _affine64(case, inp)
        halo = torch.zeros_like(xa[:1, :, :3, :])
        halo[0, :, 0, :] = xa[(s - 1) % case["n"], :, case["h"], :]
        dy = _dy64(inp)[s:s + 1, :, 0:1, :]
        dw = ref + _wgrad64(halo, dy, case["cin"], case["cout"])[:, :case["cin_real"]].numpy()
    elif what == "shift_on_padding":
        if not case["affine"]:
            return None
        dw = reference(case, inp, pad_value_shift=True)
    elif what == "write_padded_channels":
        if case["cin_real"] == case["cin"]:
            return None
        full = _wgrad64(_affine64(case, inp), _dy64(inp), case["cin"], case["cout"]).numpy().astype(F32).reshape(-1)
        nf = dw_floats(case)
        room = min(full.size, nf + GUARD)
        buf[GUARD:GUARD + room] = full[:room]                      # [Cout][Cin][9] written where [Cout][Cin_real][9] belongs
        return buf
    buf[GUARD:GUARD + dw_floats(case)] = dw.astype(F32).reshape(-1)
    return buf
