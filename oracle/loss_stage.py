"""Oracle (test infrastructure): cases, input builders and float64 / float32 references of the loss-stage tests
(tests/test_loss_stage_cpu.py pins them on the CPU, tests/test_gpu_loss_stage.py compares csrc/loss.hip and csrc/losses.hip with
them).  Everything is seeded; the kernels see the float32 inputs built here, the float64 reference starts from the same numbers.

AD-YOLO cases (``ADYOLO_CASES``) name a geometry, a batch and a seed; ``adyolo_inputs`` builds the logits and the target rows,
``adyolo_reference`` evaluates oracle/adyolo_loss.py in float64 and in float32 with autograd and marks the fragile anchors.
``constructed_inputs`` is one hand-built frame whose discrete decisions are known in advance (tie, elevation clamp, azimuth
wrap, shared anchor).  The class-wise builders give outputs and targets of the SEDDOA / ACCDOA / ADPIT losses and of the head
activation."""
import functools
import math

import torch

from . import adyolo_loss as oloss
from . import other_losses as ool

# ------------------------------------------------------------------------------------------------------------ AD-YOLO
DEFAULT = dict(grid_size=(45.0, 45.0), a=5, g_overlap=0.5, thr=(45.0, 25.0, 10.0), gains=(5.0, 1.0, 5.0, 3.0), m=None,
               v_scale=1.0, identical_ok=False)
# NA = B T G A anchors of C + 3 floats; the main kernel works on tiles of 256 anchors and has a PAD form for even C + 3
ADYOLO_CASES = {
    "8x4_a5_c12": dict(b=2, t=7, c=12, seed=11),                   # NA 2240: 8 full tiles and one of 192; non-PAD
    "8x4_a5_c13_pad": dict(b=3, t=5, c=13, seed=12),               # NA 2400; PAD
    "3x3_a3_c12": dict(b=1, t=5, c=12, a=3, grid_size=(120.0, 60.0), seed=5, v_scale=0.3),   # NA 135, 2025 floats: % 4 == 1
    "3x3_a3_c11_pad": dict(b=1, t=5, c=11, a=3, grid_size=(120.0, 60.0), seed=6, v_scale=0.3),   # 1890 floats: % 4 == 2, PAD
    "8x4_a8_c32": dict(b=2, t=3, c=32, a=8, seed=26),              # every lane of the octet, class bit 31; NA 1536
    "4x2_a1_c1_pad": dict(b=2, t=3, c=1, a=1, grid_size=(90.0, 90.0), seed=15),   # NA 48
    "m1": dict(b=2, t=7, c=12, seed=11, m=1),                      # one assign workgroup, one row
    "m32": dict(b=2, t=7, c=12, seed=11, m=32),                    # one assign workgroup, full
    "m33": dict(b=2, t=7, c=12, seed=11, m=33),                    # two assign workgroups
    "non_default": dict(b=2, t=7, c=12, seed=21, g_overlap=0.25, thr=(60.0, 30.0, 5.0), gains=(2.0, 1.5, 4.0, 0.5)),
}
FRAGILE_CAP = 5e-3                 # of a case's anchors (the cap of test_adyolo_loss_at_bench_shape)
NO_EXCLUSIONS_BELOW = 1000         # anchors: smaller cases must have no fragile anchor at all
# Inputs keep every compared pair this far from D = 0 and D = 180 (asserted on the float64 D by tests/test_loss_stage_cpu.py).  The
# reference takes D = acos(c) of a float32 c that any evaluation rounds by about 2^-24 at least once: D moves by 2^-24 / sin D
# radians, 2e-4 degree at D = 1, whichever way that one rounding falls.  Closer in, the error of a float32 evaluation is that single
# draw, and the float32 oracle's own draw (err_ref) says nothing about another evaluation's.  DESIGN.md (K8 / K10) has the history.
MIN_PAIR_DEG = 1.0
GROUPS = ("objectness of negatives", "objectness of positives", "class columns of positives", "angle columns")


def adyolo_case(name):
    cs = dict(DEFAULT)
    cs.update(ADYOLO_CASES[name])
    cs["grid"] = (int(math.ceil(360.0 / cs["grid_size"][0])), int(math.ceil(180.0 / cs["grid_size"][1])))
    cs["gains_dict"] = dict(zip(("angular_gain", "object_gain", "nonobj_gain", "class_gain"), cs["gains"]))
    return cs


def adyolo_inputs(name):
    """-> case dict, logit (B,T,G A (C+3)) float32, target (M,7) float32."""
    if name == "constructed":
        return constructed_inputs()[:3]
    cs = adyolo_case(name)
    g = torch.Generator().manual_seed(cs["seed"])
    n_cell = cs["grid"][0] * cs["grid"][1]
    logit = torch.randn(cs["b"], cs["t"], n_cell * cs["a"], cs["c"] + 3, generator=g) * 1.5
    logit[..., -1] *= cs["v_scale"]
    target = oloss.build_target(cs["b"], cs["t"], cs["c"], cs["grid_size"], cs["g_overlap"], seed=cs["seed"])
    if cs["m"] is not None:
        target = target[:cs["m"]].contiguous()
    return cs, logit.reshape(cs["b"], cs["t"], -1).contiguous(), target


def constructed_inputs():
    """One frame (B 1, T 2, grid 8x4, A 5, C 12: 320 anchors) whose decisions are known in advance; frame 1 holds two plain rows.
    -> case dict, logit, target, where: {"tie": (cell, lower twin, upper twin, class), "clamp": (cell, anchor),
    "wrap": (cell, anchor), "shared": (cell, anchor, classes, target rows)} with cell = gi * 4 + gj of frame 0.

    * tie    cell (4, 2), centre (22.5, 22.5): anchors 1 and 3 carry bit-identical (u, v) logits -0.5 -> (1.7, 1.7), 51.7 degrees
             from the target (40, 40); the others sit at (-20.9, -20.9), 83 degrees away.  Every anchor is beyond 45 degrees, so
             the arg-min alone makes a positive, and of the twins the lower index wins (loss.py:226, torch.argmin).
    * clamp  cell (2, 3), centre (-67.5, 67.5): anchor 0 has v logit 1.5 -> raw elevation 108.2, clamped to 90; it is 20 degrees
             from the target (-60, 70) whatever its azimuth.
    * wrap   cell (7, 1), centre (157.5, -22.5): anchor 4 has u logit 1.0 -> raw azimuth 191.8 -> -168.2, 10.5 degrees from the
             target (-179, -15), which the label encoder places in this cell as the wrap-around neighbour of cell 0.
    * shared cell (0, 0), centre (-157.5, -67.5): anchor 2 at (-153.0, -50.4) is 5 to 8 degrees from three targets of classes
             2, 5, 9; anchor 0 wraps the other way (-198.2 -> 161.8) and clamps at -90."""
    cs = dict(DEFAULT)
    cs.update(b=1, t=2, c=12, seed=21, grid=(8, 4), identical_ok=True)           # (the twins of the tie)
    cs["gains_dict"] = dict(zip(("angular_gain", "object_gain", "nonobj_gain", "class_gain"), cs["gains"]))
    g = torch.Generator().manual_seed(cs["seed"])
    logit = torch.randn(1, 2, 32, 5, 15, generator=g) * 0.5
    uv = logit[0, 0, :, :, 13:]                                                # (32 cells, 5 anchors, 2), a view
    tie, clamp, wrap, shared = 4 * 4 + 2, 2 * 4 + 3, 7 * 4 + 1, 0
    uv[tie] = -2.0
    uv[tie, 1] = -0.5
    uv[tie, 3] = -0.5
    uv[clamp] = torch.tensor([0.0, -1.5])
    uv[clamp, 0] = torch.tensor([0.3, 1.5])
    uv[wrap] = torch.tensor([-1.0, 0.0])
    uv[wrap, 4] = torch.tensor([1.0, 0.2])
    uv[shared] = torch.tensor([[-1.5, -1.0], [-0.8, -0.2], [0.1, 0.4], [0.9, 0.1], [0.5, 0.9]])
    target = torch.tensor([[0, 0, 4, 2, 3, 40.0, 40.0],
                           [0, 0, 2, 3, 7, -60.0, 70.0],
                           [0, 0, 7, 1, 0, -179.0, -15.0],
                           [0, 0, 0, 0, 2, -145.0, -50.0],
                           [0, 0, 0, 0, 5, -152.0, -57.0],
                           [0, 0, 0, 0, 9, -163.0, -47.0],
                           [0, 1, 3, 1, 11, -30.0, -20.0],
                           [0, 1, 5, 2, 4, 60.0, 10.0]], dtype=torch.float32)
    where = {"tie": (tie, 1, 3, 3), "clamp": (clamp, 0), "wrap": (wrap, 4), "shared": (shared, 2, (2, 5, 9), (3, 4, 5))}
    return cs, logit.reshape(1, 2, -1).contiguous(), target, where


def invalid_rows(cs):
    """Rows the kernel must ignore, each with one field just out of range: b = B, t = -1, gi = Gaz, cl = C."""
    b, gaz, c = float(cs["b"]), float(cs["grid"][0]), float(cs["c"])
    return torch.tensor([[b, 0, 1, 1, 0, 10.0, 10.0], [0, -1, 1, 1, 0, 10.0, 10.0], [0, 0, gaz, 1, 0, 10.0, 10.0],
                         [0, 0, 1, 1, c, 10.0, 10.0]], dtype=torch.float32)


def _adyolo_eval(cs, logit, target):
    lo = logit.clone().requires_grad_(True)
    loss, aux = oloss.adyolo_loss(lo, target, cs["c"], cs["grid_size"], cs["a"], cs["g_overlap"], cs["thr"], cs["gains_dict"],
                                  return_aux=True)
    loss.backward()
    return loss.detach(), lo.grad, aux


def adyolo_reference_of(cs, logit, target):
    """float64 and float32 evaluations of the oracle on the float32 inputs.  -> dict: loss64 / loss32 (1,), g64 / g32 (NA, C+3),
    d64 / d32 (M,A), anchor_ids (M,A), pos (NA,) positive at any threshold in float64, fragile (NA,), counts, coverage."""
    loss64, g64, aux64 = _adyolo_eval(cs, logit.double(), target)
    loss32, g32, aux32 = _adyolo_eval(cs, logit, target)
    assert loss32.dtype == torch.float32 and g32.dtype == torch.float32 and aux32["D"].dtype == torch.float32
    assert loss64.dtype == torch.float64 and g64.dtype == torch.float64 and aux64["D"].dtype == torch.float64
    ch = cs["c"] + 3
    na = logit.numel() // ch
    ids = aux64["anchor_ids"]
    pos = torch.zeros(na, dtype=torch.bool)
    pos[ids[aux64["masks"].any(dim=0)]] = True
    fragile, counts = oloss.fragile_anchors(aux64["D"], ids, na, cs["thr"], cs["identical_ok"])
    _, raw = oloss.decode_raw(logit.double(), cs["c"], cs["grid_size"], cs["a"], cs["g_overlap"])
    raw = raw.reshape(-1, cs["a"], 2)[aux64["cell"]]                          # (M,A,2) of the (target, anchor) pairs
    m0 = aux64["masks"][0]
    tc = target[:, 4].long()
    cls_sets = torch.zeros(na, cs["c"], dtype=torch.bool)
    cls_sets[ids[m0], tc[:, None].expand_as(m0)[m0]] = True
    coverage = {"wrapped pairs": int((((raw[..., 0] >= 180.0) | (raw[..., 0] < -180.0)) & m0).sum()),
                "clamped pairs": int(((raw[..., 1].abs() > 90.0) & m0).sum()),
                "anchors shared by 3 classes": int((cls_sets.sum(dim=1) >= 3).sum()),
                "last class positive": int(cls_sets[:, cs["c"] - 1].sum()),
                "positives": int(pos.sum()), "rows": int(target.shape[0])}
    return {"loss64": loss64, "loss32": loss32, "g64": g64.reshape(na, ch), "g32": g32.reshape(na, ch), "d64": aux64["D"],
            "d32": aux32["D"], "pos": pos, "fragile": fragile, "counts": counts, "coverage": coverage, "na": na,
            "anchor_ids": ids}


@functools.lru_cache(maxsize=None)
def adyolo_reference(name):
    """``adyolo_reference_of`` of a named case (or "constructed"), computed once per process."""
    cs, logit, target = adyolo_inputs(name)
    return adyolo_reference_of(cs, logit, target)


def adyolo_groups(ref, grad, nb_classes):
    """grad (NA, C+3) -> {group: its entries}; with grad=None the ``keep`` masks (not fragile) of the same shapes."""
    pos, c = ref["pos"], nb_classes
    if grad is None:
        ok = ~ref["fragile"]
        return {GROUPS[0]: ok[~pos], GROUPS[1]: ok[pos], GROUPS[2]: ok[pos][:, None].expand(-1, c),
                GROUPS[3]: ok[:, None].expand(-1, 2)}
    grad = grad.detach().cpu().reshape(ref["na"], c + 3)
    return {GROUPS[0]: grad[~pos, 0], GROUPS[1]: grad[pos, 0], GROUPS[2]: grad[pos, 1:c + 1], GROUPS[3]: grad[:, c + 1:]}


# --------------------------------------------------------------------------------------------------------- class-wise
# rows x C.  5462 x 12 x 4 = 262 176 elements: the grid-stride loop of seddoa_loss_kernel (1024 x 256 lanes) holds 32 in its second
# round; 21846 x 12 = 262 152 ADPIT items: 8 in the second round; 21846 x 48 = 1 048 608 activations: 32 past the 4096 x 256 grid.
SEDDOA_CASES = [(16, 12), (1, 12), (7, 13), (5462, 12)]
ADPIT_CASES = [(16, 12), (7, 13), (21846, 12)]
ACT_CASES = [(15, 48, 12), (15, 36, 0), (21846, 48, 12)]
ADPIT_FRAGILE_CAP = 1e-4


def _unit_xyz(g, *shape):
    v = torch.randn(*shape, 3, generator=g)
    return v / v.norm(dim=-1, keepdim=True)


def seddoa_inputs(rows, c, seed=31):
    """out (rows, 4C) [sed | x | y | z] and target of the SEDDOA losses; sat (rows, C) int marks the SED outputs set to exactly
    0.0 / 1.0: 1 = output equals the target (loss 0 through the -100 clamp of the log, gradient 0), 2 = output opposite to the
    target (loss 100, gradient -+1 / 1e-12 through the clamp of the denominator).  Every case holds all four combinations."""
    g = torch.Generator().manual_seed(seed + rows)
    sed = torch.sigmoid(torch.randn(rows, c, generator=g) * 2.0)
    doa = torch.tanh(torch.randn(rows, 3 * c, generator=g))
    act = (torch.rand(rows, c, generator=g) < 0.3).float()
    sat = torch.zeros(rows, c, dtype=torch.int64)
    for k in range(0, rows, 5):                                       # rows 0, 5, 10, ...: columns 0..3
        sed[k, 0], act[k, 0], sat[k, 0] = 0.0, 0.0, 1
        sed[k, 1], act[k, 1], sat[k, 1] = 1.0, 1.0, 1
        sed[k, 2], act[k, 2], sat[k, 2] = 0.0, 1.0, 2
        sed[k, 3], act[k, 3], sat[k, 3] = 1.0, 0.0, 2
    xyz = _unit_xyz(g, rows, c) * act[..., None]                      # (rows, C, 3)
    tgt = torch.cat([act, xyz[..., 0], xyz[..., 1], xyz[..., 2]], dim=1)
    return torch.cat([sed, doa], dim=1).contiguous(), tgt.contiguous(), sat


def accdoa_inputs(rows, c, seed=37):
    out, tgt, _ = seddoa_inputs(rows, c, seed)
    return out[:, c:].contiguous(), tgt[:, c:].contiguous()


def adpit_inputs(rows, c, seed=41):
    """out (rows, 9C) and target (rows, 6, 4, C): per (row, class) no event (40 %), one (A0, 30 %), two of the class (B0 B1,
    20 %) or three (C0 C1 C2, 10 %).  -> out, target, kind (rows, C) in 0..3."""
    g = torch.Generator().manual_seed(seed + rows)
    out = torch.tanh(torch.randn(rows, 9 * c, generator=g))
    r = torch.rand(rows, c, generator=g)
    kind = (r >= 0.4).long() + (r >= 0.7).long() + (r >= 0.9).long()
    xyz = _unit_xyz(g, rows, 6, c)                                    # (rows, 6, C, 3)
    slot_kind = torch.tensor([1, 2, 2, 3, 3, 3])
    act = (kind[:, None, :] == slot_kind[None, :, None]).float()     # (rows, 6, C)
    tgt = torch.cat([act[:, :, None, :], (xyz * act[..., None]).permute(0, 1, 3, 2)], dim=2)   # (rows, 6, 4, C)
    return out.contiguous(), tgt.contiguous(), kind


def act_inputs(rows, cols, seed=43):
    g = torch.Generator().manual_seed(seed + rows + cols)
    return torch.randn(rows, cols, generator=g) * 2.0, torch.randn(rows, cols, generator=g)


def seddoa_reference(out, tgt, c, kind):
    """kind: "seddoa", "masked" or "accdoa".  -> {dtype: (loss, dout)} from oracle/other_losses.py with autograd."""
    res = {}
    for dt in (torch.float64, torch.float32):
        o = out.detach().to(dt).clone().requires_grad_(True)
        t = tgt.to(dt)
        loss = ool.accdoa_loss(o[None], t[None]) if kind == "accdoa" else ool.seddoa_loss(o[None], t[None], c, kind == "masked")
        loss.backward()
        assert loss.dtype == dt
        res[dt] = (loss.detach(), o.grad)
    return res


def adpit_reference(out, tgt, c):
    """-> {dtype: (loss, dout)}, fragile (rows, C) judged on the float64 candidate losses."""
    res = {}
    for dt in (torch.float64, torch.float32):
        o = out.detach().to(dt).clone().requires_grad_(True)
        loss = ool.adpit_loss(o[None], tgt.to(dt)[None], c)
        loss.backward()
        assert loss.dtype == dt
        res[dt] = (loss.detach(), o.grad)
    with torch.no_grad():
        losses, cands = ool.adpit_candidates(out.double()[None], tgt.double()[None], c)
        fragile = ool.adpit_fragile_items(losses, cands)[0]
    return res, fragile


def act_reference(x, probe, n_sig):
    """-> {dtype: (y, dx)} of sum(head_activation(x) * probe)."""
    res = {}
    for dt in (torch.float64, torch.float32):
        xx = x.detach().to(dt).clone().requires_grad_(True)
        y = ool.head_activation(xx, n_sig)
        (y * probe.to(dt)).sum().backward()
        res[dt] = (y.detach(), xx.grad)
    return res
