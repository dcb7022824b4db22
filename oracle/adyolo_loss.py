"""Oracle (test infrastructure): AD-YOLO angular-distance responsibility-assignment loss,
PyTorch-CPU with autograd (the gradient oracle is ``torch.autograd`` of this), in the dtype of the logits: float32 restates the
reference, float64 is the reference of the kernel tests (tests/test_gpu_loss_stage.py).

Restates ``/root/reference/src/models/loss.py:156-251`` (``ADYOLOloss``):
  * ``__init__`` :157-180   grid [8,4], grid_offset (i*45-180+22.5, j*45-90+22.5), gains, train_unify
  * decode     :193-213   sigmoid on [obj, cls x C], tanh on [u, v]; UV = tanh*(0.5+g_overlap)*grid+offset;
                           V clamp [-90, 90]; U >= 180 -> -360; U < -180 -> +360
  * distance   :182-187   great-circle distance in degrees, acos argument clipped to +-(1 - 1e-7)
  * assignment :222-229   per threshold: D < thr  OR  arg-min anchor of the target's cell
  * BCE terms  :231-239   class BCE over positive anchors, objectness BCE over positives / negatives
                           (``nn.BCELoss``: log clamped at -100)
  * total      :241-251   i == 0 adds angular_gain * mean(D[mask] / 180) over (target, anchor) pairs;
                           every i adds (object*pos + nonobj*neg + class*cls) / len(train_unify)
Pinned by ``tests/golden/adyolo_loss.npz`` (loss value and dlogits of the real reference for three cases; the distance
matrix D and the masks are not stored -- they are pinned indirectly through the loss and its gradient).
"""
import math
import torch

DEFAULT_GAINS = {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0}


def grid_geometry(grid_size=(45.0, 45.0), dtype=torch.float32):
    n_az = int(math.ceil(360.0 / grid_size[0]))
    n_el = int(math.ceil(180.0 / grid_size[1]))
    gs = torch.tensor([float(grid_size[0]), float(grid_size[1])], dtype=dtype)
    ii, jj = torch.meshgrid(torch.arange(n_az), torch.arange(n_el), indexing="ij")
    offset = torch.stack([ii, jj], dim=-1).to(dtype) * gs - torch.tensor([180.0, 90.0], dtype=dtype) + gs * 0.5
    return n_az, n_el, gs, offset


def decode_raw(logit, nb_classes, grid_size=(45.0, 45.0), nb_anchors=5, g_overlap=0.5):
    """prob (B,T,Gi,Gj,A,C+1) and the (u, v) of loss.py:203 BEFORE the elevation clamp and the azimuth wrap, in the dtype of logit."""
    b, t, _ = logit.shape
    n_az, n_el, gs, offset = grid_geometry(grid_size, logit.dtype)
    out = logit.reshape(b, t, n_az, n_el, nb_anchors, nb_classes + 3)
    prob = torch.sigmoid(out[..., :nb_classes + 1])
    uv = torch.tanh(out[..., nb_classes + 1:]) * (0.5 + g_overlap) * gs + offset[None, None, :, :, None, :]
    return prob, uv


def decode(logit, nb_classes, grid_size=(45.0, 45.0), nb_anchors=5, g_overlap=0.5):
    """loss.py:193-213 -> prob (B,T,Gi,Gj,A,C+1), uv (B,T,Gi,Gj,A,2) in degrees."""
    prob, uv = decode_raw(logit, nb_classes, grid_size, nb_anchors, g_overlap)
    u = uv[..., 0]
    v = torch.clamp(uv[..., 1], -90.0, 90.0)
    u = torch.where(u >= 180.0, u - 360.0, u)
    u = torch.where(u < -180.0, u + 360.0, u)
    return prob, torch.stack([u, v], dim=-1)


def angular_distance_deg(uv_a, uv_b):
    """loss.py:182-187."""
    a, b = torch.deg2rad(uv_a), torch.deg2rad(uv_b)
    c = torch.sin(a[..., 1]) * torch.sin(b[..., 1]) + \
        torch.cos(a[..., 1]) * torch.cos(b[..., 1]) * torch.cos(torch.abs(a[..., 0] - b[..., 0]))
    return torch.rad2deg(torch.acos(torch.clip(c, -1 + 1e-7, 1 - 1e-7)))


def _bce_mean(p, y):
    """nn.BCELoss(reduction='mean') (loss.py:180): forward logs clamped at -100; backward is
    (p - y) / max(p (1 - p), 1e-12), which stays finite when the sigmoid saturates to exactly 0 or 1."""
    return torch.nn.functional.binary_cross_entropy(p, y, reduction="mean")


def adyolo_loss(logit, target, nb_classes, grid_size=(45.0, 45.0), nb_anchors=5, g_overlap=0.5,
                train_unify=(45.0, 25.0, 10.0), gains=None, return_aux=False):
    """logit (B,T,G*A*(C+3)); target (M,7) [b, frame, Gi, Gj, cls, U, V] -> loss tensor of shape (1,).
    Every tensor follows the dtype of logit: a float64 call is float64 end to end (the target's U, V are widened exactly), a
    float32 call is the float32 evaluation pinned by the golden."""
    gains = gains or DEFAULT_GAINS
    dt = logit.dtype
    prob, uv = decode(logit, nb_classes, grid_size, nb_anchors, g_overlap)
    b, t, n_az, n_el, a, _ = prob.shape
    m = target.shape[0]
    tb, tt, gi, gj, tc = (target[:, k].long() for k in range(5))
    cell = ((tb * t + tt) * n_az + gi) * n_el + gj                        # (M,)
    uv_cell = uv.reshape(-1, a, 2)[cell]                                   # (M,A,2)
    dist = angular_distance_deg(uv_cell, target[:, None, 5:7].to(dt).expand(m, a, 2))   # (M,A)
    nearest = dist.argmin(dim=1)
    flat_obj = prob[..., 0].reshape(-1)                                    # (B*T*G*A,)
    flat_cls = prob[..., 1:].reshape(-1, nb_classes)
    anchor_ids = cell[:, None] * a + torch.arange(a)[None, :]              # (M,A)

    total = torch.zeros(1, dtype=dt)
    masks = []
    for i, thr in enumerate(train_unify):
        mask = dist < thr
        mask[torch.arange(m), nearest] = True
        masks.append(mask)
        pos = torch.zeros(flat_obj.shape[0], dtype=torch.bool)
        pos[anchor_ids[mask]] = True
        cls_t = torch.zeros(flat_obj.shape[0], nb_classes, dtype=dt)
        cls_t[anchor_ids[mask], tc[:, None].expand(m, a)[mask]] = 1.0
        cls_term = _bce_mean(flat_cls[pos], cls_t[pos])
        pos_term = _bce_mean(flat_obj[pos], torch.ones(int(pos.sum()), dtype=dt))
        neg_term = _bce_mean(flat_obj[~pos], torch.zeros(int((~pos).sum()), dtype=dt))
        if i == 0:
            total = total + (dist[mask] / 180.0).mean() * gains["angular_gain"]
        total = total + (pos_term * gains["object_gain"] + neg_term * gains["nonobj_gain"]
                         + cls_term * gains["class_gain"]) / len(train_unify)
    if return_aux:
        return total, {"D": dist.detach(), "masks": torch.stack(masks, 0), "uv": uv.detach(),
                       "prob": prob.detach(), "cell": cell,
                       "anchor_ids": anchor_ids}
    return total


def build_target(b, t, nb_classes, grid_size=(45.0, 45.0), g_overlap=0.5, seed=0, p_events=(0.4, 0.3, 0.2, 0.1),
                 p_cluster=0.25, el_max=60.0):
    """Seeded target rows (M,7) float32 [b, t, gi, gj, cls, U, V] for any grid, without a label encoder.  Every (sample, frame)
    draws 0..3 events (p_events), class ~ U{0..C-1}, U ~ U[-180, 180), V ~ U[-el_max, el_max]; with probability p_cluster an
    event brings two companions of the next two classes within 3 degrees of it (rows of different classes that claim the same
    anchors).  An event goes in its own cell and, when it lies within g_overlap cells of an azimuth edge, in that azimuth
    neighbour as well, wrap-around included (as the overlapping grid of datasets.py:219-238 assigns it)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    n_az, n_el = int(math.ceil(360.0 / grid_size[0])), int(math.ceil(180.0 / grid_size[1]))
    rows = []
    for bi in range(b):
        for ti in range(t):
            events = []
            for _ in range(int(rng.choice(len(p_events), p=p_events))):
                cl, u, v = int(rng.integers(0, nb_classes)), float(rng.uniform(-180.0, 180.0)), float(rng.uniform(-el_max, el_max))
                events.append((cl, u, v))
                if nb_classes >= 3 and rng.random() < p_cluster:
                    for k in (1, 2):
                        du, dv = rng.uniform(-3.0, 3.0, size=2)
                        events.append(((cl + k) % nb_classes, float(np.clip(u + du, -180.0, 179.99)),
                                       float(np.clip(v + dv, -el_max, el_max))))
            for cl, u, v in events:
                fi = (u + 180.0) / grid_size[0]
                gi, gj = min(int(fi), n_az - 1), min(int((v + 90.0) / grid_size[1]), n_el - 1)
                rows.append((bi, ti, gi, gj, cl, u, v))
                frac = fi - gi
                if n_az > 1 and frac < g_overlap:
                    rows.append((bi, ti, (gi - 1) % n_az, gj, cl, u, v))
                elif n_az > 1 and frac >= 1.0 - g_overlap:
                    rows.append((bi, ti, (gi + 1) % n_az, gj, cl, u, v))
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 7)


def fragile_anchors(dist64, anchor_ids, n_anchors, train_unify=(45.0, 25.0, 10.0), identical_ok=False):
    """Anchors whose discrete decisions float32 round-off can turn, judged on the float64 distances (M,A) (the rule of
    tests/test_gpu_parity_scale.py::test_adyolo_loss_at_bench_shape): D within 1e-3 degree of a threshold (``D < thr`` goes either
    way), the two nearest anchors of a row within 1e-3 degree (another anchor is forced positive; all the row's anchors are
    marked), D within 0.5 degree of 0 or 180 (the acos argument is clipped at +-(1 - 1e-7) and 1 - |cos D| < 4e-5 carries
    round-off of its own order).  identical_ok: a row whose two nearest distances are EQUAL is no tie -- for inputs built with
    bit-identical twin anchors, which every evaluation decides by the index, not by rounding.  -> (bool (n_anchors,), {"threshold", "tie", "singular": pairs or rows})."""
    d = dist64.double()
    near_thr = torch.zeros_like(d, dtype=torch.bool)
    for thr in train_unify:
        near_thr |= (d - float(thr)).abs() < 1e-3
    if d.shape[1] > 1:
        srt, _ = d.sort(dim=1)
        gap = srt[:, 1] - srt[:, 0]
        tie = ((gap < 1e-3) & ~((gap == 0) & bool(identical_ok)))[:, None].expand_as(d)
    else:
        tie = torch.zeros_like(near_thr)
    singular = (d < 0.5) | (d > 179.5)
    fragile = torch.zeros(n_anchors, dtype=torch.bool)
    fragile[anchor_ids[near_thr | tie | singular]] = True
    return fragile, {"threshold": int(near_thr.sum()), "tie": int(tie[:, 0].sum()), "singular": int(singular.sum())}
