"""Oracle (test infrastructure): cases, inputs, float64 references, the bound and the checker of the 3x3 forward / data-gradient
tests (K2-fwd: ``conv3x3_fwd_kernel<KC,BN,TW>`` and ``stem_fwd_kernel`` in csrc/conv.hip, ``wino_fwd_kernel<NT,ONE>`` in
csrc/wino.hip, ``wino4_fwd_kernel<TC,AFF>`` in csrc/wino4.hip and the persistent ``wino4p_fwd_kernel<TC,AFF,EPI,NB,BRES,FULL,MKM>``
of csrc/wino4p.hpp).  tests/test_fwd_stage_cpu.py pins everything here on the CPU, tests/test_gpu_fwd_stage.py compares the kernels
with it.

``plan(form, N, H, W, Cin, Cout, operands, mask_bits, affine, ncus)`` restates the host decisions of a launch independently
(``conv3x3_fwd_variant``, ``wino_fwd_geometry``, ``wino4_fwd_geometry``, ``adyolo_wino4_fwd_form``, ``wino4p_variant``); the GPU
module asserts it against ``adyolo_conv_fwd_plan`` on every case, so what ``branches`` says a case exercises is a statement about
the code that runs.  For the persistent kernel ``walks`` lists the patches every workgroup takes, in order:
sp = (slot + k * slots) * xcd_div + xcd / ncb, k = 0, 1, ...; the branches of a walk (its length, the deal, where the next patch
lies, whether it is ragged) are read off that list.  ``CASES`` reach every named branch of every form at 256 CUs (``coverage``).

Layouts: x [N][H][W][Cin], y [N][H][W][Cout] (channels last), stats [2][patches][Cout].  A launch computes
y = relu?( conv3x3(x') + bias + addend * (addend_mask > 0) ), x' = x * scale + shift on in-image pixels (the padding stays 0), with
the filter of a layer (forward pack) or the flipped, transposed filter (data-gradient pack: the float64 reference is the autograd
gradient).  stats[0][p] = sum over the pixels of patch p of t = y * (stat_mask > 0), stats[1][p] = sum t * t, or
sum t * (aux - mean) * invstd with stat_aux.

The bound, element-wise and a priori (u = 2^-24):

    |got - ref| <= c * u * S

S is the algorithm the form runs evaluated on absolute values in float64: direct and stem sum |x'| |w| over the nine taps and Cin;
the Winograd forms |A^T| [ sum_cin (|G| |g| |G^T|) (.) (|B^T| |d| |B|) ] |A| with the kernels' own matrices (F(2x2): wino.hip;
F(4x4): points 0, +-3/4, +-3/2, infinity, wino4_common.hpp) -- the transforms cancel, so the plain sum |x| |w| is smaller than what
the kernel's roundings are relative to; |x'| = |x| |scale| + |shift| under the affine; plus |bias| and |addend| where they are added.
c counts the roundings a term can meet on its way into y, one (1 + delta) each, |delta| <= u (``roundings``):

    c = n + 1 (the product) + t_d + t_g + t_o + e + (2 under the affine)

    n     the float32 terms one accumulator sums: 9 Cin (direct, stem: Cin = 8), Cin (both Winograd forms: one GEMM per position)
    t_d   depth of the data transform B^T d B: 0 | 2 (F(2x2): one addition per direction) | 4 (F(4x4): bt6, two fused operations
          per direction: fma(P2, c0, fma(-S2, c2, c4)), fma(PA, o12, e12) of o12 = fma(-B2, c1, c3))
    t_g   the filter transform G g G^T: 0 | 4 (float32, two additions per direction; the halvings are exact) | 1 (in double,
          rounded to float32 once: wino4_pack_one)
    t_o   depth of the output transform A^T M A: 0 | 4 (two additions per direction) | 6 (at4: three deep per direction --
          s12 = m1 + m2, m0 + s12, + s34;  d34, fma(B3, d34, m5), fma(A3, d12, .))
    e     the epilogue's additions: 1 for the bias, 1 for the addend

Any order of summation stays inside n u sum |terms| to first order.  Nothing here is fitted to a kernel's result.

``emulate_conv`` is a float32 model of each algorithm; the CPU module shows that ``check`` passes it on every case and that every fault
of ``MUTATIONS`` planted into it exceeds the bound."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import seresnet as onet
from oracle.checks import sum_check
from oracle.wgrad_stage import A2M, A4M, BT2, BT4, G2, G4, MAX_ELEMENTS, cdiv

U = 2.0 ** -24
F32 = np.float32
SENT = np.float32(-777.25)
GUARD = 64                                   # sentinel floats in front of and behind y and stats
FORMS = ("direct", "stem", "wino2", "wino4")
FORM_ID = {"direct": 0, "stem": 1, "wino2": 2, "wino4": 3}
KERNEL_NAME = {0: None, 1: "conv3x3_fwd_kernel", 2: "stem_fwd_kernel", 3: "wino_fwd_kernel", 4: "wino4_fwd_kernel",
               5: "wino4p_fwd_kernel"}
# ADYOLO_W4_* operand bits (include/adyolo_hip.h)
STATS, ADDEND, ADDEND_MASK, STAT_AUX, STAT_MASK, BIAS = 1, 2, 4, 8, 16, 32
PERSISTENT_SETS = (0, 1, 2, 9, 15, 27, 31)      # ADYOLO_W4P_BUILT, csrc/wino4p_launch.hpp
WMAXC = 512
PLAN_KEYS = ("kernel", "ph", "pw", "patches_h", "patches_w", "nsp", "nb", "ncb", "xcd_div", "grid_x", "grid_y", "slots", "tc", "aff",
             "one", "kc", "bn", "tw", "bres", "full", "mkm", "narrow")


# ------------------------------------------------------------------------------------------------------------------ plans
def w4_form(cout, operands, mask_bits):
    """``adyolo_wino4_fwd_form`` with both switches on: 2 persistent, 1 one-patch, 0 none."""
    if cout <= 0 or cout % 32:
        return 0
    nb = 2 if cout % 64 == 0 else 1
    ncb = cout // (32 * nb)
    bits_ok = (not operands & ADDEND_MASK or mask_bits & 1) and (not operands & STAT_MASK or mask_bits & 2)
    if ncb <= 8 and 8 % ncb == 0 and bits_ok and operands in PERSISTENT_SETS:
        return 2
    return 1 if nb == 2 else 0


def _refused(form):
    p = dict.fromkeys(PLAN_KEYS, 0)
    p["form"] = form
    return p


def plan(form, n, h, w, cin, cout, operands=0, mask_bits=0, affine=False, ncus=256):
    """The launch ``adyolo_conv3x3_fwd`` (direct, stem) / ``adyolo_wino_fwd`` (wino2) / ``adyolo_wino4_fwd`` (wino4) makes; kernel
    0: refused (direct / stem: or the entry point takes the other of its two kernels).  Keys: PLAN_KEYS, form, and for the
    persistent kernel ``body``."""
    assert form in FORMS
    p = _refused(form)
    affine = bool(affine)
    if mask_bits & ~3 or (mask_bits and (h * w * (cout // 4)) % 64):
        return p
    if (operands & ADDEND_MASK and not operands & ADDEND) or (operands & (STAT_AUX | STAT_MASK) and not operands & STATS):
        return p
    if form in ("direct", "stem"):
        if cout % 32 or (cin != 8 and cin % 32):
            return p
        wide = w >= 32
        stem = cin == 8 and cout == 32 and wide and not affine and not operands & (ADDEND | STAT_AUX | STAT_MASK)
        if stem != (form == "stem"):
            return p
        bn = 64 if cin != 8 and cout % 64 == 0 else 32
        tw = 32 if wide else 16
        th = 8 if stem else 256 // tw
        p.update(kernel=2 if stem else 1, ph=th, pw=tw, patches_h=cdiv(h, th), patches_w=cdiv(w, tw), nb=bn // 32, ncb=cout // bn,
                 grid_y=1 if stem else cout // bn, aff=int(affine and not stem), kc=8 if cin == 8 else 32, bn=bn, tw=tw)
        p["nsp"] = p["grid_x"] = n * p["patches_h"] * p["patches_w"]
        return p
    if cin % 32 or cout % 32 or cin > WMAXC:
        return p
    halo = 2 if form == "wino4" else 0
    if (h + halo) * w * cin * 4 >= 2 ** 31 or h * w * cout * 4 >= 2 ** 31 or h * w >= 2 ** 23:
        return p
    nb = 2 if cout % 64 == 0 else 1
    ncb = cout // (32 * nb)
    dealt = ncb <= 8 and 8 % ncb == 0
    if form == "wino2":
        p.update(kernel=3, ph=8, pw=16, patches_h=cdiv(h, 8), patches_w=cdiv(w, 16), nb=nb, ncb=ncb, grid_y=1, aff=int(affine),
                 one=int(cin == 32))
        p["nsp"] = n * p["patches_h"] * p["patches_w"]
        p["xcd_div"] = 8 // ncb if dealt else 0
        p["grid_x"] = cdiv(p["nsp"], p["xcd_div"]) * 8 if dealt else p["nsp"] * ncb
        return p
    kind = w4_form(cout, operands, mask_bits)
    if not kind:
        return p
    narrow = w <= 8 and not operands and not affine and nb == 2 and dealt
    tc = (1 if w <= 4 else 2) if narrow else (8 if w >= 32 else 4)
    tr = 32 // tc
    p.update(kernel=3 + kind, ph=4 * tr, pw=4 * tc, patches_h=cdiv(h, 4 * tr), patches_w=cdiv(w, 4 * tc), nb=nb, ncb=ncb, grid_y=1,
             tc=tc, aff=int(affine), narrow=int(narrow))
    p["nsp"] = n * p["patches_h"] * p["patches_w"]
    p["xcd_div"] = 8 // ncb if dealt else 0
    p["grid_x"] = cdiv(p["nsp"], p["xcd_div"]) * 8 if dealt else p["nsp"] * ncb
    if kind == 1:
        return p
    p["slots"] = min(cdiv(p["nsp"], p["xcd_div"]), ncus // 8)
    p["grid_x"] = p["slots"] * 8
    # the instantiation: wino4p_variant
    e3 = operands in (15, 27, 31)
    need = (1 if operands & ADDEND_MASK else 0) | (2 if operands & STAT_MASK else 0)
    mkshare = e3 and w % 4 == 0 and not affine and mask_bits & need == need
    if narrow:
        p.update(aff=0, nb=2, body="narrow%d" % tc)
    elif mkshare and nb == 2 and tc == 8 and cout == 64:
        p.update(aff=0, mkm=2, body="mkm2")
    elif mkshare and nb == 1 and tc == 8 and cout == 32 and cin == 32:
        p.update(aff=0, full=1, mkm=1, body="full_mkm1")
    elif nb == 1 and cin == 32 and e3 and not affine:
        p.update(aff=0, full=1, body="full")
    elif nb == 1 and cin == 32 and operands in (0, 1, 2, 9):
        p.update(bres=1, body="bres")
    else:
        p["body"] = "ring%d" % nb
    return p


def plan_out24(p):
    """What ``adyolo_conv_fwd_plan`` reports for the launch of ``p``."""
    return [p[k] for k in PLAN_KEYS] + [0, 0]


def walks(p):
    """Persistent kernel: for every workgroup (in blockIdx order: xcd = b & 7, slot = b >> 3) the patches it takes, in order."""
    out = []
    step = p["slots"] * p["xcd_div"]
    for b in range(p["grid_x"]):
        xcd, slot = b & 7, b >> 3
        out.append(list(range(slot * p["xcd_div"] + xcd // p["ncb"], p["nsp"], step)))
    return out


def patch_box(p, h, w, sp):
    """Patch sp -> (sample, first row, first column, rows in the image, columns in the image, ragged)."""
    pw_ = sp % p["patches_w"]
    ph_ = (sp // p["patches_w"]) % p["patches_h"]
    s = sp // (p["patches_w"] * p["patches_h"])
    r0, c0 = ph_ * p["ph"], pw_ * p["pw"]
    nr, nc = min(p["ph"], h - r0), min(p["pw"], w - c0)
    return s, r0, c0, nr, nc, nr < p["ph"] or nc < p["pw"]


# --------------------------------------------------------------------------------------------------------------- branches
PERSISTENT_BODIES = ("ring2", "ring1", "bres", "full", "full_mkm1", "mkm2", "narrow1", "narrow2")
_WALK = {"walk1", "walk2", "walk3plus", "uneven_deal", "workgroups_return", "next_same_row", "next_in_next_row", "next_in_next_sample",
         "full_to_ragged", "ragged_to_full", "last_patch_ragged", "multi_patch_fwd_pack", "multi_patch_dgrad_pack"}
# What a body cannot do at 256 CUs under MAX_ELEMENTS (the step between two patches of a walk is 32 * xcd_div = 256 / ncb patches):
#   TC = 1, 2 (narrow): one patch column, so no next patch in the same row; plain launches without an affine only;
#   TC = 2 with a next patch in the next row of the SAME sample needs > 256 / ncb patch rows of 64 x (5..8) pixels:
#       at ncb = 8 (Cout = 512) 2049 x 5 x 512 = 5.2 M elements;
#   MKM 2 (Cout = 64, W >= 32) the same: 257 patch rows are 4097 x 32 x 64 = 8.4 M elements;
#   TC = 1, 2: a walk that changes between full and ragged patches needs an odd number of patches per sample (the step is even), so
#       three (full, full, ragged) of 128 x 4 or 64 x 8 pixels: 257 patches of them at Cout = 64 are 88 samples x 257 x 4 x 64 = 5.8 M
#       elements, and the product (256 / ncb) patches x 64 ncb channels is the same for every ncb;
#   MKM 1 / 2 are TC = 8 only and take no affine; FULL takes none either.
BODY_BRANCHES = {
    "ring2": _WALK | {"tc4", "tc8", "aff", "no_aff", "npairs2", "npairs4", "cin512", "ncb1", "ncb2", "ncb4", "ncb8", "cin_gt_cout",
                      "cin_lt_cout"},
    "ring1": _WALK | {"tc4", "tc8", "aff", "no_aff", "npairs4", "cin512", "ncb1", "cin_gt_cout"},
    "bres": _WALK | {"tc4", "tc8", "aff", "no_aff", "ncb1"},
    "full": _WALK | {"tc4", "tc8", "ncb1"},
    "full_mkm1": _WALK | {"tc8", "ncb1"},
    "mkm2": (_WALK - {"next_in_next_row"}) | {"tc8", "ncb1", "cin_gt_cout", "cin_lt_cout"},
    "narrow1": (_WALK - {"next_same_row", "full_to_ragged", "ragged_to_full"}) | {"ncb1", "ncb8"},
    "narrow2": (_WALK - {"next_same_row", "next_in_next_row", "full_to_ragged", "ragged_to_full"}) | {"ncb1", "ncb8"},
}
ALL_BRANCHES = {
    "direct": {"tw16", "tw32", "bn32", "bn64", "kc8", "ragged_rows", "ragged_columns", "map_smaller_than_tile", "cin32", "cin_ge_64",
               "aff", "no_aff", "bias", "relu", "dgrad_pack", "float_masks", "bits_masks"} | {"set%d" % s for s in (0, 1, 9, 15, 27, 31)},
    "stem": {"w32", "w_gt_32_ragged", "h_lt_8", "ragged_rows", "bias_relu", "no_bias_no_relu", "stats"},
    "wino2": {"nt1", "nt2", "one", "not_one", "ncb1", "ncb2", "ncb4", "ncb8", "ncb3_or_6", "workgroups_return", "ragged_rows",
              "ragged_columns", "aff", "no_aff", "dgrad_pack", "float_masks", "bits_masks"} | {"set%d" % s for s in (0, 1, 9, 15, 27, 31)},
    "wino4": {"onepatch:" + b for b in ("tc4", "tc8", "aff", "no_aff", "ncb1", "ncb2", "ncb4", "ncb8", "ncb3_or_6", "workgroups_return",
                                        "bias", "float_masks", "ragged_rows", "ragged_columns")}
    | {"%s:%s" % (body, b) for body, bs in BODY_BRANCHES.items() for b in bs}
    | {"multi_patch_set%d" % s for s in PERSISTENT_SETS},
}


def branches(p, case):
    """The named branches the launch of ``case`` with plan ``p`` exercises."""
    f, h, w, cin, cout, epi = case["form"], case["h"], case["w"], case["cin"], case["cout"], case["epi"]
    out = set()
    ragged_rows, ragged_cols = h % p["ph"] != 0, w % p["pw"] != 0
    returns = p["xcd_div"] > 0 and p["nsp"] % p["xcd_div"] != 0
    if f == "direct":
        out |= {"tw%d" % p["tw"], "bn%d" % p["bn"], "cin32" if cin == 32 else "cin_ge_64" if cin >= 64 else "kc8"}
        out.add("aff" if case["affine"] else "no_aff")
        if epi in (0, 1, 9, 15, 27, 31):
            out.add("set%d" % epi)
    elif f == "stem":
        out.add("w32" if w == 32 else "w_gt_32_ragged" if w % 32 else "w_multiple_of_32")
        if h < 8:
            out.add("h_lt_8")
        out.add("bias_relu" if case["bias"] and case["relu"] else "no_bias_no_relu" if not case["bias"] and not case["relu"] else "mixed")
        if epi & STATS:
            out.add("stats")
        out -= {"w_multiple_of_32", "mixed"}
    elif f == "wino2":
        out |= {"nt%d" % p["nb"], "one" if p["one"] else "not_one", "aff" if case["affine"] else "no_aff"}
        out.add("ncb%d" % p["ncb"] if p["xcd_div"] else "ncb3_or_6")
        if returns:
            out.add("workgroups_return")
        if epi in (0, 1, 9, 15, 27, 31):
            out.add("set%d" % epi)
    if f in ("direct", "wino2"):
        if case["bias"]:
            out.add("bias")
        if case["relu"]:
            out.add("relu")
        if case["dgrad"]:
            out.add("dgrad_pack")
        if case["maskform"]:
            out.add(case["maskform"] + "_masks")
        out -= {"bias", "relu"} if f == "wino2" else set()
    if f != "wino4":
        if ragged_rows:
            out.add("ragged_rows")
        if ragged_cols:
            out.add("ragged_columns")
        if f == "direct" and h < p["ph"] and w < p["pw"]:
            out.add("map_smaller_than_tile")
        if f == "stem":
            out.discard("ragged_columns")
        return out
    if p["kernel"] == 4:
        b = {"tc%d" % p["tc"], "aff" if case["affine"] else "no_aff", "ncb%d" % p["ncb"] if p["xcd_div"] else "ncb3_or_6"}
        if returns:
            b.add("workgroups_return")
        if case["bias"]:
            b.add("bias")
        if case["maskform"] == "float":
            b.add("float_masks")
        if ragged_rows:
            b.add("ragged_rows")
        if ragged_cols:
            b.add("ragged_columns")
        return {"onepatch:" + x for x in b}
    body = p["body"]
    b = {"ncb%d" % p["ncb"]}
    if not body.startswith("narrow"):
        b.add("tc%d" % p["tc"])
    if body in ("ring2", "ring1", "bres"):
        b.add("aff" if case["affine"] else "no_aff")
    if body in ("ring2", "ring1"):
        if cin == 32:
            b.add("npairs2")
        if cin == 64:
            b.add("npairs4")
        if cin == 512:
            b.add("cin512")
    if cin > cout:
        b.add("cin_gt_cout")
    if cin < cout:
        b.add("cin_lt_cout")
    ws_ = walks(p)
    lens = [len(x) for x in ws_]
    for ln in set(lens):
        b.add("workgroups_return" if ln == 0 else "walk1" if ln == 1 else "walk2" if ln == 2 else "walk3plus")
    if len({ln for ln in lens if ln}) > 1:
        b.add("uneven_deal")
    multi = False
    for wk in ws_:
        boxes = [patch_box(p, h, w, sp) for sp in wk]
        if len(wk) > 1:
            multi = True
            if boxes[-1][5]:
                b.add("last_patch_ragged")
        for a, c in zip(boxes, boxes[1:]):
            b.add("next_in_next_sample" if a[0] != c[0] else "next_same_row" if a[1] == c[1] else "next_in_next_row")
            if a[5] != c[5]:
                b.add("ragged_to_full" if a[5] else "full_to_ragged")
    if multi:
        b.add("multi_patch_dgrad_pack" if case["dgrad"] else "multi_patch_fwd_pack")
    out = {"%s:%s" % (body, x) for x in b if x in BODY_BRANCHES[body]}
    if multi:
        out.add("multi_patch_set%d" % epi)
    return out


# ------------------------------------------------------------------------------------------------------------------ cases
def make_case(form, n, h, w, cin, cout, epi=0, maskform=None, affine=False, bias=False, relu=False, dgrad=False):
    """epi: the ADYOLO_W4_* bits without the bias; maskform: "bits" / "float" where epi has a mask."""
    assert bool(epi & (ADDEND_MASK | STAT_MASK)) == (maskform is not None), "maskform goes with the mask bits of epi"
    name = "%s_%dx%dx%d_c%d_%d_e%d%s%s%s%s%s" % (form, n, h, w, cin, cout, epi, "_" + maskform if maskform else "", "_aff" if affine else "",
                                                 "_bias" if bias else "", "_relu" if relu else "", "_dgrad" if dgrad else "")
    return {"form": form, "n": n, "h": h, "w": w, "cin": cin, "cout": cout, "epi": epi, "maskform": maskform, "affine": bool(affine),
            "bias": bool(bias), "relu": bool(relu), "dgrad": bool(dgrad), "name": name,
            "seed": 7000 + 131 * n + 17 * h + 7 * w + cin + 3 * cout + 11 * epi + FORM_ID[form]}


def case_operands(case):
    return case["epi"] | (BIAS if case["bias"] else 0)


def case_mask_bits(case):
    if case["maskform"] != "bits":
        return 0
    return (1 if case["epi"] & ADDEND_MASK else 0) | (2 if case["epi"] & STAT_MASK else 0)


def case_plan(case, ncus=256):
    return plan(case["form"], case["n"], case["h"], case["w"], case["cin"], case["cout"], case_operands(case), case_mask_bits(case),
                case["affine"], ncus)


def case_branches(case, ncus=256):
    return branches(case_plan(case, ncus), case)


def _older_geometries():
    """Shapes of test_conv3x3_forward, test_conv3x3_dgrad_wgrad, the narrow-map test (tests/test_gpu_kernels.py) and EPI_SMALL of
    tests/test_gpu_block_stage.py, through the kernels that take them there."""
    c, out = make_case, []
    for i, s in enumerate([(2, 13, 16, 32, 32), (1, 5, 5, 32, 64), (2, 37, 40, 64, 64), (3, 20, 32, 64, 96), (2, 9, 64, 32, 128),
                           (1, 33, 16, 64, 256), (2, 70, 48, 32, 32)]):
        epi = (1, 9, 15, 27, 31)[i % 5]
        bits_ok = (s[1] * s[2] * (s[4] // 4)) % 64 == 0
        mf = None if not epi & 20 else "bits" if bits_ok else "float"
        for form in ("direct", "wino2", "wino4"):
            cs = c(form, *s, epi=epi, maskform=mf, affine=epi == 1)
            if case_plan(cs)["kernel"]:
                out.append(cs)
    for s in [(2, 16, 64, 32, 32), (2, 13, 32, 32, 64), (1, 18, 16, 64, 128), (1, 9, 16, 256, 256), (2, 21, 19, 96, 32)]:
        out.append(c("direct", *s, dgrad=True))
        out.append(c("wino2", *s, dgrad=True))
        if case_plan(c("wino4", *s, dgrad=True))["kernel"]:
            out.append(c("wino4", *s, dgrad=True))
    for s in [(2, 70, 4, 64, 64), (3, 133, 8, 64, 128), (2, 260, 3, 64, 64), (2, 100, 7, 128, 128)]:
        out.append(c("wino4", *s))
    for s in [(2, 20, 64), (3, 11, 37), (1, 5, 64)]:
        out.append(c("stem", s[0], s[1], s[2], 8, 32, epi=1, bias=True, relu=True))
    return out


def _edge_cases():
    """Found with ``plan`` and ``walks``: the branches the older geometries do not reach.  Per sample the cheapest maps are the
    ragged ones (a partial patch counts in full): 33 x 65 is 3 x 3 patches of 16 x 32, 2 x 65 one row of three."""
    c = make_case
    return [
        # ---- direct
        c("direct", 2, 12, 20, 8, 32, epi=1, affine=True),                    # KC = 8 beside the stem kernel: W < 32, affine
        c("direct", 2, 9, 40, 8, 32, epi=3, bias=True, relu=True),            # KC = 8, TW = 32, with an addend
        c("direct", 1, 5, 9, 32, 32, bias=True, relu=True),                   # a map smaller than a tile
        c("direct", 2, 19, 45, 64, 96, epi=27, maskform="float", relu=True),  # BN = 32, ragged both ways
        c("direct", 2, 8, 32, 32, 64, epi=31, maskform="bits"),
        # ---- stem
        c("stem", 2, 8, 32, 8, 32),                                           # W = 32, no bias, no ReLU, no statistics
        c("stem", 3, 5, 70, 8, 32, epi=1, bias=True, relu=True),              # H < 8, ragged W > 32
        c("stem", 2, 19, 45, 8, 32, epi=1),                                   # ragged rows
        # ---- F(2x2)
        c("wino2", 3, 9, 20, 64, 128, epi=1, affine=True),                    # ncb = 2, 12 patches
        c("wino2", 1, 20, 40, 32, 256, epi=0),                                # ncb = 4: 9 patches, workgroups return
        c("wino2", 1, 11, 17, 64, 512, epi=9),                                # ncb = 8
        c("wino2", 3, 9, 17, 32, 192, epi=0, dgrad=True),                     # ncb = 3: no XCD dealing
        c("wino2", 1, 12, 24, 32, 32, epi=0),                                 # NT = 1, ONE; 4 patches on 8 workgroups
        c("wino2", 2, 16, 32, 64, 64, epi=31, maskform="bits"),
        c("wino2", 2, 9, 17, 64, 32, epi=27, maskform="float"),
        # ---- F(4x4), one patch per workgroup: what the persistent form refuses
        c("wino4", 2, 21, 40, 64, 64, epi=1, bias=True, relu=True),           # a bias
        c("wino4", 1, 37, 20, 32, 128, epi=31, maskform="float", affine=True),   # masks as floats, TC = 4, ncb = 2
        c("wino4", 1, 17, 33, 64, 256, epi=3),                                # operand set 3: not built; ncb = 4, workgroups return
        c("wino4", 1, 9, 16, 32, 512, epi=5 | 2, maskform="float"),           # ncb = 8
        c("wino4", 1, 20, 16, 64, 192, epi=0),                                # ncb = 3: no XCD dealing, no persistent form
        # ---- F(4x4), persistent: B ring, NB = 2
        c("wino4", 29, 33, 65, 64, 64, epi=1, affine=True),                   # 261 patches: one slot takes two
        c("wino4", 65, 33, 17, 32, 64, epi=0),                                # TC = 4, npairs = 2: the turn falls on pair 0
        c("wino4", 9, 37, 24, 32, 512, epi=9),                                # ncb = 8: 36 patches on 32 slots
        c("wino4", 171, 2, 65, 32, 64, epi=2),                                # 513 patches: a walk of three
        c("wino4", 33, 2, 17, 64, 512, epi=1, affine=True),                   # ncb = 8, 66 patches: walks of three and two
        c("wino4", 33, 2, 17, 512, 512, epi=0, dgrad=True),                   # Cin = 512 (the longest pair loop), a data-gradient pack
        c("wino4", 2, 17, 33, 128, 64, epi=0),                                # Cin > Cout
        c("wino4", 9, 33, 33, 64, 256, epi=15, maskform="bits", dgrad=True),  # ncb = 4 (H W Cout / 4 % 64 == 0)
        c("wino4", 1, 1, 1025, 32, 512, epi=0),                               # 33 patches in one row: the next patch in the same row
        c("wino4", 1, 1025, 3, 64, 512, epi=1),                               # TC = 4, 33 patch rows: the next patch one row down
        c("wino4", 30, 33, 64, 64, 64, epi=27, maskform="float"),             # float masks refuse the persistent form: one-patch
        c("wino4", 33, 32, 33, 64, 64, epi=27, maskform="bits", dgrad=True),  # B ring with mask bits (W % 4 != 0: no MKM); 132 patches
        c("wino4", 44, 33, 33, 64, 64, epi=9),                                # 264 patches: ragged -> full and full -> ragged
        c("wino4", 44, 36, 34, 64, 64, epi=31, maskform="bits"),              # both masks as bits on the B ring (W % 4 != 0: no MKM)
        # ---- persistent, NB = 1 with Cin > 32 (B ring), 32 -> 32 resident U (BRES), whole lines (FULL)
        c("wino4", 29, 33, 65, 64, 32, epi=1, affine=True),
        c("wino4", 129, 1, 33, 512, 32, epi=9, dgrad=True),                   # Cin = 512: 258 patches of one row
        c("wino4", 65, 33, 17, 64, 32, epi=0),
        c("wino4", 171, 4, 66, 64, 32, epi=31, maskform="bits", dgrad=True),
        c("wino4", 1, 1, 8193, 64, 32, epi=0),
        c("wino4", 1, 8193, 3, 64, 32, epi=2),
        c("wino4", 44, 33, 33, 64, 32, epi=1, affine=True),
        c("wino4", 1, 5, 5, 64, 32, epi=0, affine=True),
        c("wino4", 29, 33, 65, 32, 32, epi=1, affine=True),                   # BRES
        c("wino4", 65, 33, 17, 32, 32, epi=9, dgrad=True),
        c("wino4", 171, 2, 65, 32, 32, epi=2),
        c("wino4", 1, 1, 8193, 32, 32, epi=0),
        c("wino4", 1, 8193, 3, 32, 32, epi=1),
        c("wino4", 44, 33, 33, 32, 32, epi=0, affine=True, dgrad=True),
        c("wino4", 1, 5, 5, 32, 32, epi=0),
        c("wino4", 29, 36, 66, 32, 32, epi=15, maskform="bits"),              # FULL (W % 4 != 0: no MKM)
        c("wino4", 65, 36, 18, 32, 32, epi=27, maskform="bits", dgrad=True),
        c("wino4", 171, 4, 66, 32, 32, epi=31, maskform="bits"),
        c("wino4", 1, 8, 8193, 32, 32, epi=15, maskform="bits"),
        c("wino4", 1, 8200, 3, 32, 32, epi=27, maskform="bits"),
        c("wino4", 44, 36, 34, 32, 32, epi=31, maskform="bits", dgrad=True),
        c("wino4", 1, 8, 34, 32, 32, epi=15, maskform="bits"),                # two patches on eight workgroups
        c("wino4", 1, 5, 5, 32, 32, epi=15, maskform="float", affine=True),   # 32 -> 32 with float masks: refused (asserted by the GPU module)
        # ---- persistent, shared mask words: FULL + MKM 1 (32 -> 32), MKM 2 (Cout = 64)
        c("wino4", 29, 33, 72, 32, 32, epi=31, maskform="bits"),
        c("wino4", 171, 2, 72, 32, 32, epi=15, maskform="bits", dgrad=True),
        c("wino4", 1, 1, 8200, 32, 32, epi=27, maskform="bits"),
        c("wino4", 1, 4104, 32, 32, 32, epi=31, maskform="bits"),
        c("wino4", 44, 36, 36, 32, 32, epi=27, maskform="bits", dgrad=True),
        c("wino4", 1, 8, 40, 32, 32, epi=15, maskform="bits"),
        c("wino4", 29, 33, 68, 64, 64, epi=31, maskform="bits"),
        c("wino4", 171, 2, 68, 32, 64, epi=15, maskform="bits", dgrad=True),
        c("wino4", 1, 1, 8196, 128, 64, epi=27, maskform="bits"),
        c("wino4", 44, 36, 36, 64, 64, epi=27, maskform="bits", dgrad=True),
        c("wino4", 1, 8, 36, 64, 64, epi=15, maskform="bits"),
        # ---- persistent, narrow patches (plain launches, W <= 8)
        c("wino4", 129, 129, 3, 64, 64),                                      # TC = 1: 258 patches
        c("wino4", 65, 2, 3, 64, 512, dgrad=True),                            # ncb = 8: 65 patches, a walk of three
        c("wino4", 1, 4097, 1, 64, 512),                                      # 33 patch rows of one sample
        c("wino4", 1, 5, 2, 64, 64),
        c("wino4", 129, 65, 5, 64, 64),                                       # TC = 2: 258 patches
        c("wino4", 65, 2, 8, 64, 512, dgrad=True),
        c("wino4", 1, 5, 6, 64, 64),
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
REFUSED_CASES = ("wino4_1x5x5_c32_32_e15_float_aff",)       # in the list on purpose: a 32-channel block with float masks


def cases(form=None):
    return [c for c in CASES if (form is None or c["form"] == form) and c["name"] not in REFUSED_CASES]


def case_elements(cs):
    return cs["n"] * cs["h"] * cs["w"] * max(cs["cin"], cs["cout"])


def coverage(ncus=256):
    """Asserts that CASES reach every named branch of every form on a device with ``ncus`` CUs, that every case is taken by the
    kernel family it names and is small.  -> {form: {branch: [case names]}}"""
    table = {}
    for f in FORMS:
        got = {}
        for cs in cases(f):
            p = case_plan(cs, ncus)
            assert p["kernel"], "%s is refused" % cs["name"]
            assert case_elements(cs) <= MAX_ELEMENTS, cs["name"]
            for b in branches(p, cs):
                got.setdefault(b, []).append(cs["name"])
        missing = ALL_BRANCHES[f] - set(got)
        extra = set(got) - ALL_BRANCHES[f]
        assert not missing and not extra, "%s: missing %s, unknown %s" % (f, sorted(missing), sorted(extra))
        table[f] = got
    for name in REFUSED_CASES:
        cs = next(c for c in CASES if c["name"] == name)
        assert not case_plan(cs, ncus)["kernel"], name
    return table


# ----------------------------------------------------------------------------------------------------------------- inputs
def spike_positions(case, p):
    """[(sample, row, column)] of the large isolated values: the image corners, the last row and column, either side of the
    first and last three patch boundaries in both directions, the first and last row of every sample, and the first and last
    in-image pixel of the first and last patch of every multi-patch walk and of its k > 0 patches (at most 64 walks)."""
    n, h, w = case["n"], case["h"], case["w"]
    rows = {0, h - 1}
    cols = {0, w - 1}
    for size, step, acc in ((h, p["ph"], rows), (w, p["pw"], cols)):
        bnd = list(range(step, size, step))
        for b in (bnd if len(bnd) <= 6 else bnd[:3] + bnd[-3:]):
            acc |= {b - 1, b}
    pos = {(s, r, c) for s in {0, n - 1} for r in rows for c in cols}
    for s in range(n):
        pos |= {(s, 0, 0), (s, 0, w - 1), (s, h - 1, 0), (s, h - 1, w - 1), (s, 0, (w - 1) // 2), (s, h - 1, (w - 1) // 2)}
    if p["kernel"] == 5:
        multi = [wk for wk in walks(p) if len(wk) > 1]
        for wk in multi[:32] + multi[-32:]:
            for sp in wk:
                s, r0, c0, nr, nc, _ = patch_box(p, h, w, sp)
                pos |= {(s, r0, c0), (s, r0 + nr - 1, c0 + nc - 1)}
    return sorted(pos)


def build(case):
    """-> dict of float32 / bool arrays: x, wt (the layer's filter: [Cout][Cin][3][3], or [Cin][Cout][3][3] for a data-gradient
    pack), scale, shift, bias, addend, amask, smask, aux, mean, invstd, spikes."""
    rng = np.random.default_rng(case["seed"])
    n, h, w, cin, cout = (case[k] for k in ("n", "h", "w", "cin", "cout"))
    p = case_plan(case)
    cin_real = 7 if cin == 8 else cin
    x = (rng.standard_normal((n, h, w, cin), dtype=F32) * F32(0.7) + F32(0.3))
    x[..., cin_real:] = 0
    shape = (cin, cout, 3, 3) if case["dgrad"] else (cout, cin_real, 3, 3)
    wt = (rng.standard_normal(shape) / np.sqrt(9.0 * cin_real)).astype(F32)
    t = {"x": x, "wt": wt, "scale": (rng.random(cin) + 0.5).astype(F32), "shift": (rng.standard_normal(cin) * 0.3).astype(F32),
         "bias": (rng.standard_normal(cout) * 0.1).astype(F32)}
    epi = case["epi"]
    if epi & ADDEND:
        t["addend"] = rng.standard_normal((n, h, w, cout), dtype=F32)
        t["amask"] = rng.random((n, h, w, cout), dtype=F32) < 0.5
    if epi & STAT_MASK:
        t["smask"] = rng.random((n, h, w, cout), dtype=F32) < 0.5
    if epi & STAT_AUX:
        t["aux"] = np.maximum(rng.standard_normal((n, h, w, cout), dtype=F32) * F32(2) + F32(0.5), 0)
    spikes = spike_positions(case, p)
    for k, (s, r, c) in enumerate(spikes):
        sign = F32(1.0 if k % 3 else -1.0)
        ck = (7 * k + 3) % cout
        x[s, r, c, ck % cin_real] = F32(700.0) * sign
        if "addend" in t:
            t["addend"][s, r, c, ck] = F32(-1000.0) * sign
            t["amask"][s, r, c, ck] = k % 2 == 0
        if "smask" in t:
            t["smask"][s, r, c, ck] = k % 4 < 2
        if "aux" in t:
            t["aux"][s, r, c, (ck + 1) % cout] = F32(2000.0)
    if "aux" in t:
        a = t["aux"].astype(np.float64).reshape(-1, cout)
        t["mean"] = a.mean(0).astype(F32)
        t["invstd"] = (1.0 / np.sqrt(a.var(0) + 1e-5)).astype(F32)
    t["spikes"] = spikes
    return t


def float_mask(mask, seed):
    """A bool mask as the float tensor the kernels compare with 0: > 0 where on; -1 or (half of them) exactly 0 where off."""
    rng = np.random.default_rng(seed)
    f = np.where(mask, F32(1), F32(-1)).astype(F32)
    f[(~mask) & (rng.random(mask.shape, dtype=F32) < 0.5)] = 0
    return f


# -------------------------------------------------------------------------------------------------------------- reference
def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def equivalent_filter(case, inp, dtype=torch.float64):
    """g [Cout][Cin][3][3] with y = conv2d(x', g): the layer's filter, or its flipped transpose for a data-gradient pack (Cin = 8: the
    eighth input channel has no filter)."""
    g = torch.from_numpy(inp["wt"]).to(dtype)
    if case["dgrad"]:
        return g.flip(2, 3).transpose(0, 1).contiguous()
    if g.shape[1] < case["cin"]:
        g = F.pad(g, (0, 0, 0, 0, 0, case["cin"] - g.shape[1]))
    return g


def input_nchw(case, inp, dtype=torch.float64, absolute=False):
    """x' [N][Cin][H][W] (no padding), in ``dtype``; absolute: |x| |scale| + |shift|."""
    x = torch.from_numpy(inp["x"]).to(dtype)
    if absolute:
        x = x.abs()
    if case["affine"]:
        sc, sh = torch.from_numpy(inp["scale"]).to(dtype), torch.from_numpy(inp["shift"]).to(dtype)
        x = x * sc.abs() + sh.abs() if absolute else x * sc + sh
    return x.permute(0, 3, 1, 2)


def conv64(case, inp):
    """The bare convolution in float64, [N][H][W][Cout]: F.conv2d of x' with zero padding; for a data-gradient pack the autograd
    gradient of the layer's convolution with respect to its input."""
    xa = input_nchw(case, inp).contiguous()
    if case["dgrad"]:
        n, h, w, cout = case["n"], case["h"], case["w"], case["cout"]
        y = torch.nn.grad.conv2d_input((n, cout, h, w), torch.from_numpy(inp["wt"]).double(), xa, padding=1)
    else:
        y = F.conv2d(xa, equivalent_filter(case, inp), None, padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


def finish(case, inp, conv, dtype=torch.float64):
    """conv [N][H][W][Cout] -> y: + bias, + addend * mask, ReLU, in ``dtype``."""
    y = conv.to(dtype)
    if case["bias"]:
        y = y + torch.from_numpy(inp["bias"]).to(dtype)
    if case["epi"] & ADDEND:
        a = torch.from_numpy(inp["addend"]).to(dtype)
        if case["epi"] & ADDEND_MASK:
            a = a * torch.from_numpy(inp["amask"]).to(dtype)
        y = y + a
    return y.relu() if case["relu"] else y


def reference(case, inp):
    return finish(case, inp, conv64(case, inp)).numpy()


WINO = {"wino2": (2, BT2, A2M.T.copy(), G2), "wino4": (4, BT4, A4M.T.copy(), G4)}      # m, B^T [p][p], A^T [m][p], G [p][3]


def winograd_conv(x, g, m, bt, at, gm, dtype=torch.float64, filter_in_double=True, chunk=2 ** 19):
    """Y = A^T [ sum_cin (G g G^T) (.) (B^T d B) ] A per m x m output tile with the given matrices, arithmetic in ``dtype``
    (filter_in_double: the filter transform in float64, rounded to ``dtype`` once).  x [N][Cin][H][W] unpadded, g [Cout][Cin][3][3]
    -> [N][H][W][Cout].  Samples are processed in chunks of about ``chunk`` input elements."""
    n, cin, h, w = x.shape
    cout, p = g.shape[0], m + 2
    th, tw = cdiv(h, m), cdiv(w, m)
    bt_, at_ = torch.as_tensor(bt).to(dtype), torch.as_tensor(at).to(dtype)
    gdt = torch.float64 if filter_in_double else dtype
    u = torch.einsum("ai,ocij,bj->abco", torch.as_tensor(gm).to(gdt), g.to(gdt), torch.as_tensor(gm).to(gdt)).to(dtype)
    out = torch.empty(n, h, w, cout, dtype=dtype)
    per = max(1, chunk // max(1, cin * h * w))
    for s0 in range(0, n, per):
        xs = F.pad(x[s0:s0 + per].to(dtype), (1, tw * m - w + 1, 1, th * m - h + 1))
        d = xs.unfold(2, p, m).unfold(3, p, m)                                # [n][Cin][th][tw][p][p]
        v = torch.einsum("ai,nchwij,bj->abnhwc", bt_, d, bt_).reshape(p, p, -1, cin)
        mm = torch.matmul(v, u)                                                # [p][p][tiles][Cout]
        y = torch.einsum("ia,abto,jb->toij", at_, mm, at_)                     # [tiles][Cout][m][m]
        y = y.reshape(-1, th, tw, cout, m, m).permute(0, 1, 4, 2, 5, 3).reshape(-1, th * m, tw * m, cout)
        out[s0:s0 + per] = y[:, :h, :w]
    return out


def magnitude(case, inp):
    """S of the bound, float64 [N][H][W][Cout]."""
    xa = input_nchw(case, inp, absolute=True).contiguous()
    g = equivalent_filter(case, inp).abs()
    if case["form"] in ("direct", "stem"):
        s = F.conv2d(xa, g, None, padding=1).permute(0, 2, 3, 1)
    else:
        m, bt, at, gm = WINO[case["form"]]
        s = winograd_conv(xa, g, m, np.abs(bt), np.abs(at), np.abs(gm))
    s = s.contiguous()
    if case["bias"]:
        s = s + _t64(inp["bias"]).abs()
    if case["epi"] & ADDEND:
        a = _t64(inp["addend"]).abs()
        s = s + (a * _t64(inp["amask"]) if case["epi"] & ADDEND_MASK else a)
    return s.numpy()


def roundings(case):
    """c of the bound: see the module's docstring."""
    f = case["form"]
    cin = case["cin"]
    if f in ("direct", "stem"):
        c = 9 * cin + 1
    elif f == "wino2":
        c = cin + 1 + 2 + 4 + 4
    else:
        c = cin + 1 + 4 + 1 + 6
    c += (1 if case["bias"] else 0) + (1 if case["epi"] & ADDEND else 0)
    return c + (2 if case["affine"] else 0)


@functools.lru_cache(maxsize=4)
def prepared(name):
    """(case, inputs, reference y, bound) of a case of CASES by name (treat as read-only)."""
    case = next(c for c in _cases() if c["name"] == name)
    inp = build(case)
    return case, inp, reference(case, inp), roundings(case) * U * magnitude(case, inp)


# ------------------------------------------------------------------------------------------------------------------ check
def y_floats(case):
    return case["n"] * case["h"] * case["w"] * case["cout"]


def stats_floats(case, p=None):
    p = p or case_plan(case)
    return 2 * p["nsp"] * case["cout"] if case["epi"] & STATS else 0


def new_buffer(nfloats):
    """GUARD sentinels, ``nfloats`` of NaN (the kernel must write every one), GUARD sentinels."""
    buf = np.full(2 * GUARD + nfloats, SENT, dtype=F32)
    buf[GUARD:GUARD + nfloats] = np.nan
    return buf


def _window(what, name, buf, nf):
    out = np.asarray(buf, dtype=F32).reshape(-1)
    assert out.size == 2 * GUARD + nf, "%s: %s buffer of %d floats" % (name, what, out.size)
    guard = np.concatenate([out[:GUARD], out[GUARD + nf:]])
    changed = guard.view(np.int32) != SENT.view(np.int32)
    assert not changed.any(), "%s: %d guard words beside %s changed" % (name, int(changed.sum()), what)
    got = out[GUARD:GUARD + nf].astype(np.float64)
    bad = ~np.isfinite(got)
    assert not bad.any(), "%s: %d of %d elements of %s are not finite (first at %d)" % (name, int(bad.sum()), nf, what, int(np.argmax(bad)))
    return got


def patch_sums(case, inp, p, y):
    """y: the tensor the launch wrote (float64 [N][H][W][Cout]) -> (sums [2][patches][Cout], bounds [2][patches][Cout]): the float64
    sums over each patch's in-image pixels of t = y * stat_mask and of t * t (t * xhat(aux) with stat_aux), and
    ``fp32_sum_bound`` with T = the pixels of a patch."""
    n, h, w, cout = case["n"], case["h"], case["w"], case["cout"]
    t0 = torch.from_numpy(np.ascontiguousarray(y)).double().reshape(n, h, w, cout)
    if case["epi"] & STAT_MASK:
        t0 = t0 * torch.from_numpy(inp["smask"]).double()
    if case["epi"] & STAT_AUX:
        t1 = t0 * onet.xhat_nhwc(_t64(inp["aux"]), _t64(inp["mean"]), _t64(inp["invstd"]))
    else:
        t1 = t0 * t0
    ph, pw, nh, nw = p["ph"], p["pw"], p["patches_h"], p["patches_w"]

    def per_patch(t):
        t = F.pad(t, (0, 0, 0, nw * pw - w, 0, nh * ph - h))
        return t.reshape(n, nh, ph, nw, pw, cout).sum(dim=(2, 4)).reshape(n * nh * nw, cout)
    sums = torch.stack([per_patch(t0), per_patch(t1)])
    bnds = torch.stack([onet.fp32_sum_bound(per_patch(t0.abs()), ph * pw), onet.fp32_sum_bound(per_patch(t1.abs()), ph * pw)])
    return sums, bnds


LAST = {}                 # figures of the last ``check``: stats_ratio, the worst err / bound of the per-patch sums


def check(case, inp, ref, bnd, ybuf, statsbuf=None, quiet=True):
    """ybuf / statsbuf: the whole output buffers after the call.  Guard words bitwise unchanged, no NaN in y or stats, every
    element of y within its bound, every patch's sums those of that patch of the y written.  -> worst err / bound of y"""
    name = case["name"]
    LAST.clear()
    got = _window("y", name, ybuf, y_floats(case)).reshape(ref.shape)
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bnd, 1e-300)).max())
    over = err > bnd
    assert not over.any(), "%s: %d of %d elements of y over the bound, worst err / bound %.3f (err %.3e) at %s" % (
        name, int(over.sum()), over.size, ratio, float(err.max()), np.unravel_index(int(np.argmax(err / np.maximum(bnd, 1e-300))), err.shape))
    if case["epi"] & STATS:
        p = case_plan(case)
        assert statsbuf is not None, "%s: no statistics buffer" % name
        st = _window("stats", name, statsbuf, stats_floats(case, p)).reshape(2, p["nsp"], case["cout"])
        sums, bnds = patch_sums(case, inp, p, got)
        for which in (0, 1):
            if quiet:
                e = np.abs(st[which] - sums[which].numpy())
                bad = e > bnds[which].numpy()
                pos = bnds[which].numpy() > 0
                LAST["stats_ratio"] = max(LAST.get("stats_ratio", 0.0), float((e[pos] / bnds[which].numpy()[pos]).max()) if pos.any() else 0.0)
                assert not bad.any(), "%s: sum %d of %d (patch, channel) entries over the bound, first patch %d" % (
                    name, which, int(bad.sum()), int(np.argmax(bad.any(axis=1))))
            else:
                sum_check("%s per-patch sum %d" % (name, which), torch.from_numpy(st[which]), sums[which], bnds[which])
    return ratio


# -------------------------------------------------------------------------------------------------------------- emulation
def emulate_conv(case, inp, algorithm=None):
    """float32 model of the bare convolution by "direct", "wino2" or "wino4" (default: the case's own): float32 affine,
    transforms, products and sums.  -> float32 torch [N][H][W][Cout]"""
    algorithm = algorithm or {"stem": "direct"}.get(case["form"], case["form"])
    xa = input_nchw(case, inp, dtype=torch.float32).contiguous()
    g = equivalent_filter(case, inp, dtype=torch.float32)
    if algorithm == "direct":
        return F.conv2d(xa, g, None, padding=1).permute(0, 2, 3, 1).contiguous()
    m, bt, at, gm = WINO[algorithm]
    return winograd_conv(xa, g, m, bt, at, gm, dtype=torch.float32, filter_in_double=algorithm == "wino4")


def emulated_outputs(case, inp, conv32):
    """(ybuf, statsbuf) a float32 implementation leaves: y = finish(conv32) in float32, per-patch sums of it in float32."""
    y = finish(case, inp, conv32, dtype=torch.float32).numpy()
    ybuf = new_buffer(y_floats(case))
    ybuf[GUARD:-GUARD] = y.reshape(-1)
    sbuf = None
    if case["epi"] & STATS:
        p = case_plan(case)
        sums, _ = patch_sums(case, inp, p, y.astype(np.float64))
        sbuf = new_buffer(stats_floats(case, p))
        sbuf[GUARD:-GUARD] = sums.numpy().astype(F32).reshape(-1)
    return ybuf, sbuf


# -------------------------------------------------------------------------------------------------------------- mutations
MUTATIONS = ("halo_row_dropped_at_patch_boundary", "halo_row_from_neighbouring_sample", "halo_column_wrapped_to_neighbouring_row",
             "shift_on_padding", "pair0_from_previous_patch", "b_fragments_of_last_group_after_patch_change", "addend_mask_shifted",
             "stats_of_second_patch_in_first_slot")


def _row_conv(xrow, g_ky):
    """One input row [N][Cin][W] through the taps g_ky [Cout][Cin][3] -> its contribution [N][W][Cout] to one output row."""
    return F.conv1d(xrow, g_ky, None, padding=1).permute(0, 2, 1)


def _second_patch(case, p):
    """(first, second) patch of the first multi-patch walk of a persistent launch, or None."""
    if p["kernel"] != 5:
        return None
    for wk in walks(p):
        if len(wk) > 1:
            return wk[0], wk[1]
    return None


def _patch_input(case, p, xa, sp):
    """The (ph + 2) x (pw + 2) halo'd input of patch sp from xa [N][Cin][H][W], zero outside the image: [1][Cin][ph+2][pw+2]."""
    h, w = case["h"], case["w"]
    s, r0, c0, _, _, _ = patch_box(p, h, w, sp)
    xp = F.pad(xa[s:s + 1], (1, p["pw"] + 1, 1, p["ph"] + 1))
    return xp[:, :, r0:r0 + p["ph"] + 2, c0:c0 + p["pw"] + 2]


def mutate(case, inp, conv32, what):
    """(ybuf, statsbuf) of the emulation with the named fault planted; None where the fault does not apply to the case."""
    assert what in MUTATIONS
    p = case_plan(case)
    n, h, w, cin = case["n"], case["h"], case["w"], case["cin"]
    xa = input_nchw(case, inp, dtype=torch.float32).contiguous()
    g = equivalent_filter(case, inp, dtype=torch.float32)
    conv = conv32.clone()
    if what == "halo_row_dropped_at_patch_boundary":
        if p["patches_h"] < 2:
            return None
        r = p["ph"] * (p["patches_h"] - 1)                     # the first row of the last patch row loses its upper halo row
        conv[:, r] -= _row_conv(xa[:, :, r - 1, :], g[:, :, 0, :])
    elif what == "halo_row_from_neighbouring_sample":
        conv[:, 0] += _row_conv(xa[:, :, h - 1, :].roll(1, 0), g[:, :, 0, :])
    elif what == "halo_column_wrapped_to_neighbouring_row":
        # column -1 of row r reads the last pixel of row r - 1 (a map of one row has no such row in its sample)
        if h < 2:
            return None
        col = F.pad(xa[:, :, :-1, w - 1], (1, 0))                                          # [N][Cin][H]: what column -1 of row r holds
        conv[:, :, 0] += F.conv1d(col, g[:, :, :, 0].contiguous(), None, padding=1).permute(0, 2, 1)
    elif what == "shift_on_padding":
        if not case["affine"]:
            return None
        border = torch.ones(1, cin, h + 2, w + 2)
        border[:, :, 1:-1, 1:-1] = 0
        border = border * torch.from_numpy(inp["shift"])[None, :, None, None]
        conv += F.conv2d(border, g, None).permute(0, 2, 3, 1)
    elif what in ("pair0_from_previous_patch", "b_fragments_of_last_group_after_patch_change"):
        pair = _second_patch(case, p)
        if pair is None:
            return None
        s, r0, c0, nr, nc, _ = patch_box(p, h, w, pair[1])
        mine = _patch_input(case, p, xa, pair[1])
        if what == "pair0_from_previous_patch":
            delta = F.conv2d(_patch_input(case, p, xa, pair[0])[:, :16] - mine[:, :16], g[:, :16], None)
        else:
            delta = F.conv2d(mine[:, :8], g[:, cin - 8:] - g[:, :8], None)
        conv[s, r0:r0 + nr, c0:c0 + nc] += delta[0, :, :nr, :nc].permute(1, 2, 0)
    elif what == "addend_mask_shifted":
        if not case["epi"] & ADDEND_MASK:
            return None
        other = dict(inp)
        other["amask"] = np.roll(inp["amask"].reshape(-1, case["cout"]), 1, axis=0).reshape(inp["amask"].shape)
        ybuf, sbuf = emulated_outputs(case, other, conv)
        return ybuf, sbuf
    elif what == "stats_of_second_patch_in_first_slot":
        pair = _second_patch(case, p)
        if pair is None or not case["epi"] & STATS:
            return None
        ybuf, sbuf = emulated_outputs(case, inp, conv)
        st = sbuf[GUARD:-GUARD].reshape(2, p["nsp"], case["cout"])
        st[:, pair[0]] = st[:, pair[1]]                        # the second patch's own slot keeps what the first launch of the
        return ybuf, sbuf                                      # buffer left there: here the right sums, so only the VALUES can tell
    return emulated_outputs(case, inp, conv)
