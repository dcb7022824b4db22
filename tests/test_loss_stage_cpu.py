"""CPU tests of the references behind tests/test_gpu_loss_stage.py (oracle/adyolo_loss.py, oracle/other_losses.py,
oracle/loss_stage.py): the float64 path of the AD-YOLO oracle against its float32 path and the goldens, the caps on the
fragile anchors / ADPIT items of every case the GPU module runs (asserted here, on the float64 reference alone, not on the
GPU), and that every case contains what it is there for."""
import os

import numpy as np
import pytest
import torch

from oracle import adyolo_loss as oloss
from oracle import loss_stage as ls
from oracle import other_losses as ool

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL_ADYOLO = list(ls.ADYOLO_CASES) + ["constructed"]


# ------------------------------------------------------------------------------------------------- oracle agreement
@pytest.mark.parametrize("tag,nb_classes", [("c12", 12), ("c13", 13), ("sat", 12)])
def test_adyolo_oracle_float64_and_float32_reproduce_the_golden(tag, nb_classes):
    """The float32 call stays float32 (loss, gradient, D, every auxiliary tensor) and reproduces adyolo_loss.npz as
    tests/test_oracle_golden.py asks; the float64 call stays float64 and agrees with it to float32 accuracy: the loss to
    16 * 2^-24, D to 2e-5 of its absmax and the gradient to 1e-5 of its absmax away from the fragile anchors (whose decisions
    round-off turns, ``oloss.fragile_anchors``).  The ``sat`` golden is the exception by design: its logits of +-40 .. +-120
    saturate the FLOAT32 sigmoid to exactly 0 and 1 (the -100 clamp of nn.BCELoss, loss 94.6); in float64 the sigmoid does not
    saturate there, so only type, shape and finiteness are asserted for it."""
    g = np.load(os.path.join(G, "adyolo_loss.npz"))
    target = torch.from_numpy(g[tag + "_target"])
    res = {}
    for dt in (torch.float32, torch.float64):
        lo = torch.from_numpy(g[tag + "_logit"]).to(dt).requires_grad_(True)
        loss, aux = oloss.adyolo_loss(lo, target, nb_classes, return_aux=True)
        loss.backward()
        assert loss.dtype == dt and lo.grad.dtype == dt and loss.shape == (1,)
        assert aux["D"].dtype == dt and aux["uv"].dtype == dt and aux["prob"].dtype == dt
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(lo.grad).all())
        res[dt] = (loss.detach().double(), lo.grad.double().reshape(-1, nb_classes + 3), aux)
    (l32, g32, a32), (l64, g64, a64) = res[torch.float32], res[torch.float64]
    np.testing.assert_allclose(l32.numpy(), g[tag + "_loss"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(g32.numpy().reshape(g[tag + "_dlogit"].shape), g[tag + "_dlogit"], rtol=1e-5, atol=1e-8)
    _, gs, off = oloss.grid_geometry((45.0, 45.0))[1:]
    assert gs.dtype == torch.float32 and off.dtype == torch.float32
    assert oloss.grid_geometry((45.0, 45.0), torch.float64)[3].dtype == torch.float64
    if tag == "sat":
        return
    gold = torch.from_numpy(g[tag + "_dlogit"]).double().reshape(-1, nb_classes + 3)
    fragile, counts = oloss.fragile_anchors(a64["D"], a64["anchor_ids"], g64.shape[0])
    keep, pairs = ~fragile, ~fragile[a64["anchor_ids"]]
    print("%s: fragile %d of %d anchors %s" % (tag, int(fragile.sum()), g64.shape[0], counts))
    assert abs(float(l32 - l64)) <= 16 * 2.0 ** -24 * abs(float(l64))
    assert abs(float(l64) - float(g[tag + "_loss"].reshape(-1)[0])) <= 16 * 2.0 ** -24 * abs(float(l64))
    assert float((a32["D"].double() - a64["D"]).abs()[pairs].max()) <= 2e-5 * float(a64["D"].abs().max())
    assert float((g32 - g64).abs()[keep].max()) <= 1e-5 * float(g64.abs().max())
    assert float((gold - g64).abs()[keep].max()) <= 1e-5 * float(g64.abs().max())


def test_other_losses_float64_and_float32_reproduce_the_golden():
    g = np.load(os.path.join(G, "other_losses.npz"))
    cases = [("seddoa", "sed_target", lambda o, t: ool.seddoa_loss(o, t, 12, False)),
             ("masked", "sed_target", lambda o, t: ool.seddoa_loss(o, t, 12, True)),
             ("accdoa", "accdoa_target", ool.accdoa_loss),
             ("adpit", "adpit_target", lambda o, t: ool.adpit_loss(o, t, 12))]
    for tag, tkey, fn in cases:
        for dt in (torch.float32, torch.float64):
            o = torch.from_numpy(g[tag + "_out"]).to(dt).requires_grad_(True)
            loss = fn(o, torch.from_numpy(g[tkey]).to(dt))
            loss.backward()
            assert loss.dtype == dt and o.grad.dtype == dt
            np.testing.assert_allclose(loss.detach().numpy(), g[tag + "_loss"], rtol=1e-5, atol=1e-6, err_msg=tag)
            np.testing.assert_allclose(o.grad.numpy(), g[tag + "_dout"], rtol=1e-4, atol=1e-7, err_msg=tag)


def test_adpit_candidates_are_the_reference_minimum():
    """The 13 candidate losses reduce to adpit_loss; a candidate's loss is the mean squared distance to its target vector."""
    out, tgt, _ = ls.adpit_inputs(7, 13)
    losses, cands = ool.adpit_candidates(out.double()[None], tgt.double()[None], 13)
    assert losses.shape == (13, 1, 7, 13) and cands.shape == (13, 1, 7, 9, 13)
    assert torch.equal(losses.min(dim=0).values.mean(), ool.adpit_loss(out.double()[None], tgt.double()[None], 13))
    o = out.double().reshape(1, 7, 9, 13)
    assert torch.equal(losses[5], ((o - cands[5]) ** 2).mean(dim=2))


# ----------------------------------------------------------------------------------------------------- target builder
@pytest.mark.parametrize("name", list(ls.ADYOLO_CASES))
def test_target_builder_rows_are_valid_and_cover_the_neighbours(name):
    cs, logit, target = ls.adyolo_inputs(name)
    n_az, n_el = cs["grid"]
    assert logit.shape == (cs["b"], cs["t"], n_az * n_el * cs["a"] * (cs["c"] + 3)) and logit.dtype == torch.float32
    assert target.dtype == torch.float32 and target.shape[1] == 7 and target.shape[0] > 0
    b, t, gi, gj, cl, u, v = target.unbind(1)
    for col, hi in ((b, cs["b"]), (t, cs["t"]), (gi, n_az), (gj, n_el), (cl, cs["c"])):
        assert bool(((col >= 0) & (col < hi) & (col == col.round())).all())
    assert bool(((u >= -180) & (u < 180) & (v >= -90) & (v <= 90)).all())
    own = ((u.double() + 180.0) / cs["grid_size"][0]).floor().clamp(max=n_az - 1)
    assert bool((((gi - own) % n_az == 0) | ((gi - own) % n_az == 1) | ((gi - own) % n_az == n_az - 1)).all())
    assert bool((gj == ((v.double() + 90.0) / cs["grid_size"][1]).floor().clamp(max=n_el - 1)).all())
    if cs["m"] is None:
        assert int(((gi - own).abs() == n_az - 1).sum()) > 0, "no wrap-around neighbour row"
    assert torch.equal(target, ls.adyolo_inputs(name)[2])              # seeded


# ------------------------------------------------------------------------------------------------------------- caps
@pytest.mark.parametrize("name", ALL_ADYOLO)
def test_fragile_anchors_stay_under_the_caps(name):
    ref = ls.adyolo_reference(name)
    n = int(ref["fragile"].sum())
    print("%-16s %d anchors, fragile %d (%.3f %%): %s" % (name, ref["na"], n, 100.0 * n / ref["na"], ref["counts"]))
    assert n <= ls.FRAGILE_CAP * ref["na"]
    if ref["na"] < ls.NO_EXCLUSIONS_BELOW:
        assert n == 0
    d = ref["d64"][~ref["fragile"][ref["anchor_ids"]]]                 # (fragile pairs are left out of the value checks anyway)
    print("%-16s D of the compared pairs: %.3f .. %.3f degrees" % (name, float(d.min()), float(d.max())))
    assert float(d.min()) >= ls.MIN_PAIR_DEG and float(d.max()) <= 180.0 - ls.MIN_PAIR_DEG


def test_fragile_rule_marks_what_it_names():
    """Thresholds, ties and the two singular ends on a hand-made D; equal twins count as a tie unless identical_ok."""
    d = torch.tensor([[44.9995, 80.0, 90.0], [30.0, 30.0005, 90.0], [0.4, 90.0, 100.0], [50.0, 120.0, 179.6], [50.0, 50.0, 70.0],
                      [20.0, 60.0, 70.0]], dtype=torch.float64)
    ids = torch.arange(18).reshape(6, 3)
    fr, counts = oloss.fragile_anchors(d, ids, 18)
    assert counts == {"threshold": 1, "tie": 2, "singular": 2}
    assert fr.tolist() == [True, False, False, True, True, True, True, False, False, False, False, True, True, True, True,
                           False, False, False]
    fr2, counts2 = oloss.fragile_anchors(d, ids, 18, identical_ok=True)
    assert counts2["tie"] == 1 and not bool(fr2[12:15].any())


@pytest.mark.parametrize("rows,c", ls.ADPIT_CASES)
def test_fragile_adpit_items_stay_under_the_cap(rows, c):
    out, tgt, kind = ls.adpit_inputs(rows, c)
    _, fragile = ls.adpit_reference(out, tgt, c)
    n = int(fragile.sum())
    print("adpit %d x %d: fragile %d of %d items; none / A / B / C: %s" % (rows, c, n, fragile.numel(),
                                                                          [int((kind == k).sum()) for k in range(4)]))
    assert n <= ls.ADPIT_FRAGILE_CAP * fragile.numel()
    assert all(int((kind == k).sum()) > 0 for k in range(4))
    act = tgt[:, :, 0, :]
    assert bool((act.sum(dim=1) == torch.tensor([0.0, 1.0, 2.0, 3.0])[kind]).all())


def test_fragile_adpit_rule_on_a_made_tie():
    """Two tracks of class B mirrored about the output make the B permutations tie: fragile.  A lone event (all candidates share
    one target vector) and an empty item are not."""
    tgt = torch.zeros(1, 1, 6, 4, 3, dtype=torch.float64)
    tgt[0, 0, 1, :, 0] = torch.tensor([1.0, 1.0, 0.0, 0.0])
    tgt[0, 0, 2, :, 0] = torch.tensor([1.0, -1.0, 0.0, 0.0])
    tgt[0, 0, 0, :, 1] = torch.tensor([1.0, 0.0, 1.0, 0.0])
    out = torch.zeros(1, 1, 27, dtype=torch.float64)
    losses, cands = ool.adpit_candidates(out, tgt, 3)
    assert ool.adpit_fragile_items(losses, cands)[0, 0].tolist() == [True, False, False]


# --------------------------------------------------------------------------------------------------------- coverage
def test_adyolo_cases_contain_what_they_are_there_for():
    need = {"8x4_a5_c12": ("wrapped pairs", "clamped pairs", "anchors shared by 3 classes", "last class positive"),
            "8x4_a5_c13_pad": ("wrapped pairs", "clamped pairs", "anchors shared by 3 classes", "last class positive"),
            "3x3_a3_c12": ("wrapped pairs", "anchors shared by 3 classes"), "3x3_a3_c11_pad": ("wrapped pairs",),
            "8x4_a8_c32": ("wrapped pairs", "clamped pairs", "anchors shared by 3 classes", "last class positive"),
            "4x2_a1_c1_pad": ("wrapped pairs", "clamped pairs", "last class positive"),
            "m1": (), "m32": ("clamped pairs",), "m33": ("clamped pairs",),
            "non_default": ("wrapped pairs", "clamped pairs", "anchors shared by 3 classes"),
            "constructed": ("wrapped pairs", "clamped pairs", "anchors shared by 3 classes")}
    assert set(need) == set(ALL_ADYOLO)
    for name, keys in need.items():
        cs, logit, target = ls.adyolo_inputs(name)
        cov = ls.adyolo_reference(name)["coverage"]
        print("%-16s %s" % (name, cov))
        for k in keys:
            assert cov[k] > 0, (name, k)
        assert 0 < cov["positives"] < logit.numel() // (cs["c"] + 3)
        if cs["m"] is not None:
            assert target.shape[0] == cs["m"]
    # the tile arithmetic the shapes were chosen for (csrc/loss.hip: tiles of 256 anchors, float4 body + scalar tail)
    na = {n: ls.adyolo_reference(n)["na"] for n in ALL_ADYOLO}
    assert na["8x4_a5_c12"] == 2240 and na["3x3_a3_c12"] == 135 and na["8x4_a8_c32"] == 1536 and na["4x2_a1_c1_pad"] == 48
    assert (135 * 15) % 4 == 1 and (135 * 14) % 4 == 2


def test_constructed_frame_decides_as_designed():
    """In float64: the twins are bit-equal and nearest, beyond every threshold, and the lower one alone is positive; the clamped
    anchor has raw elevation > 90, the wrapped one raw azimuth >= 180; anchor 2 of cell 0 is positive for classes 2, 5, 9."""
    cs, logit, target, where = ls.constructed_inputs()
    ref = ls.adyolo_reference("constructed")
    d = ref["d64"]
    cell, lo, hi, _ = where["tie"]
    assert d[0, lo] == d[0, hi] and int(d[0].argmin()) == lo and float(d[0].min()) > max(cs["thr"])
    assert ref["d32"][0, lo] == ref["d32"][0, hi] and int(ref["d32"][0].argmin()) == lo
    a0 = cell * 5
    assert ref["pos"][a0:a0 + 5].tolist() == [k == lo for k in range(5)]
    _, raw = oloss.decode_raw(logit.double(), 12)
    raw = raw.reshape(2, 32, 5, 2)[0]
    cell, a = where["clamp"]
    assert float(raw[cell, a, 1]) > 90.0 and bool(ref["pos"][cell * 5 + a])
    assert float(ref["g64"][cell * 5 + a, 14]) == 0.0 and float(ref["g64"][cell * 5 + a, 13]) != 0.0
    cell, a = where["wrap"]
    assert float(raw[cell, a, 0]) >= 180.0 and bool(ref["pos"][cell * 5 + a]) and float(ref["g64"][cell * 5 + a, 13]) > 0.0
    cell, a, classes, rows = where["shared"]
    assert all(float(d[r, a]) < min(cs["thr"]) for r in rows)
    assert tuple(int(target[r, 4]) for r in rows) == classes


@pytest.mark.parametrize("rows,c", ls.SEDDOA_CASES)
def test_seddoa_inputs_hold_exact_zeros_and_ones_against_both_targets(rows, c):
    out, tgt, sat = ls.seddoa_inputs(rows, c)
    sed, act = out[:, :c], tgt[:, :c]
    for o, t, mark in ((0.0, 0.0, 1), (1.0, 1.0, 1), (0.0, 1.0, 2), (1.0, 0.0, 2)):
        hit = (sed == o) & (act == t)
        assert int(hit.sum()) > 0 and bool((sat[hit] == mark).all())
    assert bool((((sed == 0.0) | (sed == 1.0)) == (sat > 0)).all())
    assert out.shape == (rows, 4 * c) and tgt.shape == (rows, 4 * c)
    # the float64 reference is finite there and clamps like nn.BCELoss: an opposite pair costs 100, its gradient is -+1 / (float32(1e-12) n)
    ref = ls.seddoa_reference(out, tgt, c, "seddoa")[torch.float64]
    assert bool(torch.isfinite(ref[0]).all()) and bool(torch.isfinite(ref[1]).all())
    g = ref[1][:, :c]
    assert bool((g[sat == 1] == 0).all())
    np.testing.assert_allclose(g[sat == 2].abs().numpy(), 1.0 / float(np.float32(1e-12)) / (rows * c), rtol=1e-12)


def test_grid_stride_sizes():
    """The large cases pass the grids of csrc/losses.hip (1024 x 256 lanes; 4096 x 256 for the activation) by 32, 8 and 32."""
    assert 5462 * 48 - 1024 * 256 == 32 and 21846 * 12 - 1024 * 256 == 8 and 21846 * 48 - 4096 * 256 == 32
    assert (5462, 12) in ls.SEDDOA_CASES and (21846, 12) in ls.ADPIT_CASES and (21846, 48, 12) in ls.ACT_CASES
