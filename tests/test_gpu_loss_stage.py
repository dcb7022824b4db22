"""GPU tests of the loss stage (run with ``-m gpu`` on an MI355X): the AD-YOLO assign / main / final kernels and the two-phase
entry of csrc/loss.hip (K8) and the head activation, SEDDOA / masked SEDDOA / ACCDOA and ADPIT kernels of csrc/losses.hip (K10),
each against the PyTorch-CPU oracle evaluated in float64 on the float32 numbers the kernel sees (oracle/adyolo_loss.py,
oracle/other_losses.py; inputs, cases and references: oracle/loss_stage.py, pinned on the CPU by tests/test_loss_stage_cpu.py).

Bars, none taken from what a kernel returns (oracle/checks.py):

* value: err = max |q - q64| / max |q64| <= max(4 err_ref, 16 * 2^-24), err_ref the same error of the float32 CPU oracle on the
  same inputs.  Gradients are compared GROUP BY GROUP, each against the float64 absmax of its own group: the AD-YOLO gradient as
  objectness of negatives / objectness of positives / class columns of positives / angle columns (the global absmax belongs to
  the angle columns and hides the other three), the SEDDOA gradient as BCE columns / saturated BCE entries / MSE columns
  (w_mse = 1000 makes the global absmax the MSE columns');
* exact: gradients that are zeros, decisions built into the inputs, runs that promise the same bits.

Anchors whose discrete decisions float32 round-off turns (``oracle.adyolo_loss.fragile_anchors``) and ADPIT items whose arg-min
it turns (``oracle.other_losses.adpit_fragile_items``) are judged on the float64 reference and left out of the value checks; the
CPU module caps their number per case.  Every check prints its figures; the ones of an MI355X run stand next to the asserts and
in DESIGN.md (K8 / K10)."""
import pytest
import torch

from oracle import loss_stage as ls
from oracle.checks import Collect, value_check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def dev(t):
    return t.to("cuda:0").contiguous()


# ============================================================================================================ AD-YOLO
def run_adyolo(ops, cs, logit, target, **kw):
    loss, dlogit, dist = ops.adyolo_loss(dev(logit), dev(target), cs["c"], cs["grid"], cs["a"], cs["thr"], cs["gains"],
                                         cs["grid_size"], cs["g_overlap"], want_dist=True, **kw)
    torch.cuda.synchronize()
    return loss.cpu(), None if dlogit is None else dlogit.cpu(), dist.cpu()


def check_adyolo(col, tag, cs, ref, loss, dlogit, dist):
    """loss, dist and the four gradient groups by value; class and angle gradients of negative anchors exactly 0."""
    col(value_check, tag + " loss", loss, ref["loss64"], ref["loss32"])
    if dist is not None:
        col(value_check, tag + " dist", dist, ref["d64"], ref["d32"], keep=~ref["fragile"][ref["anchor_ids"]])
    got, g64, g32 = (ls.adyolo_groups(ref, g, cs["c"]) for g in (dlogit, ref["g64"], ref["g32"]))
    keep = ls.adyolo_groups(ref, None, cs["c"])
    for name in ls.GROUPS:
        col(value_check, "%s dlogit, %s" % (tag, name), got[name], g64[name], g32[name], keep=keep[name])
    neg = ~ref["pos"] & ~ref["fragile"]
    rest = dlogit.reshape(ref["na"], cs["c"] + 3)[neg, 1:]

    def negatives_are_zero():
        assert bool((rest == 0).all()), "%s: %d class / angle gradients of negative anchors are not 0" % (tag, int((rest != 0).sum()))
    col(negatives_are_zero)


@pytest.mark.parametrize("name", list(ls.ADYOLO_CASES))
def test_adyolo_loss_dist_and_gradient_groups(ops, name):
    # MI355X, worst over the cases (err_gpu, err_ref, bar): loss 7.5e-8, 2.8e-8, 9.5e-7; dist 7.2e-7, 4.5e-7, 1.8e-6; objectness of
    # negatives 1.6e-7, 2.3e-7, 9.5e-7; of positives 1.7e-7, 9.5e-8, 9.5e-7; class columns 1.8e-7, 2.1e-7, 9.5e-7; angle columns
    # 6.3e-6, 2.6e-6, 1.0e-5 (non_default: err_gpu / bar 0.61, the module's worst)
    cs, logit, target = ls.adyolo_inputs(name)
    ref = ls.adyolo_reference(name)
    print("%s: %d anchors, %d rows, %d fragile %s" % (name, ref["na"], target.shape[0], int(ref["fragile"].sum()), ref["counts"]))
    loss, dlogit, dist = run_adyolo(ops, cs, logit, target)
    col = Collect()
    check_adyolo(col, name, cs, ref, loss, dlogit, dist)
    col.finish()


def test_adyolo_grad_scale_and_need_grad(ops):
    """grad_scale = 0.125 (a power of two) scales every gradient entry exactly; need_grad=False returns the same loss bits."""
    cs, logit, target = ls.adyolo_inputs("8x4_a5_c12")
    loss, dlogit, _ = run_adyolo(ops, cs, logit, target)
    loss_s, dlogit_s, _ = run_adyolo(ops, cs, logit, target, grad_scale=0.125)
    loss_n, dlogit_n, _ = run_adyolo(ops, cs, logit, target, need_grad=False)
    assert dlogit_n is None
    assert torch.equal(loss_s, loss) and torch.equal(loss_n, loss)
    assert torch.equal(dlogit_s, 0.125 * dlogit)
    assert int((dlogit != 0).sum()) > ls.adyolo_reference("8x4_a5_c12")["na"]


def test_adyolo_loss_class_backward_with_2025_logits(ops):
    """``models.loss.ADYOLOloss`` at the 3x3 geometry (2025 logits, no multiple of 4), scaled by an incoming gradient of 0.5:
    the bits of 0.5 dlogit (``ops.scale_dev`` refused sizes that are no multiple of 4)."""
    from adyolo_amd.models.loss import ADYOLOloss
    cs, logit, target = ls.adyolo_inputs("3x3_a3_c12")
    prm = {"args": {"device": "cuda:0"}, "data_config": {"nb_classes": cs["c"]},
           "train_config": {"grid_size": list(cs["grid_size"]), "nb_anchors": cs["a"], "train_unify": list(cs["thr"]),
                            "g_overlap": cs["g_overlap"], "loss_gains": cs["gains_dict"]}}
    lo = dev(logit).requires_grad_(True)
    loss_c = ADYOLOloss(prm)(lo, target)
    (loss_c * 0.5).backward()
    loss, dlogit, _ = run_adyolo(ops, cs, logit, target)
    assert logit.numel() == 2025 and torch.equal(loss_c.detach().cpu(), loss)
    assert torch.equal(lo.grad.cpu(), 0.5 * dlogit)


def test_adyolo_constructed_decisions(ops):
    """Tie, elevation clamp, azimuth wrap and shared anchor of ``oracle.loss_stage.constructed_inputs``: by value like every
    case, and exactly."""
    cs, logit, target, where = ls.constructed_inputs()
    ref = ls.adyolo_reference("constructed")
    loss, dlogit, dist = run_adyolo(ops, cs, logit, target)
    col = Collect()
    check_adyolo(col, "constructed", cs, ref, loss, dlogit, dist)          # MI355X: angle columns 1.8e-6 (bar 4.5e-6)
    g = dlogit.reshape(2, 32, 5, 15)[0]                                     # frame 0: [cell][anchor][obj, cls x 12, u, v]

    def tie():
        cell, lo, hi, cl = where["tie"]
        assert dist[0, lo] == dist[0, hi], "the twins' distances differ"
        assert float(g[cell, lo, 0]) < 0, "the lower twin is not positive"
        assert all(float(g[cell, a, 0]) > 0 for a in range(5) if a != lo), "another anchor of the tie cell is positive"
        assert bool((g[cell, lo, 1:13] != 0).all()) and float(g[cell, lo, 1 + cl]) < 0
        assert bool((g[cell, lo, 1:13][torch.arange(12) != cl] > 0).all())
        for a in range(5):
            if a != lo:
                assert bool((g[cell, a, 1:] == 0).all()), "anchor %d of the tie cell has class / angle gradients" % a

    def clamp():
        cell, a = where["clamp"]
        assert float(g[cell, a, 0]) < 0 and float(g[cell, a, 14]) == 0.0 and float(g[cell, a, 13]) != 0.0

    def wrap():
        cell, a = where["wrap"]
        assert float(g[cell, a, 0]) < 0 and float(g[cell, a, 13]) > 0.0

    def shared():
        cell, a, classes, rows = where["shared"]
        assert float(g[cell, a, 0]) < 0
        sign = g[cell, a, 1:13] < 0
        assert sorted(torch.nonzero(sign).flatten().tolist()) == list(classes)
        perm = torch.tensor([5, 7, 3, 0, 4, 6, 2, 1])
        loss_p, dlogit_p, dist_p = run_adyolo(ops, cs, logit, target[perm].contiguous())
        assert torch.equal(dlogit_p, dlogit), "dlogit depends on the order of the target rows"
        assert torch.equal(dist_p, dist[perm])
        value_check("constructed, permuted rows: loss", loss_p, ref["loss64"], ref["loss32"])
    for check in (tie, clamp, wrap, shared):
        col(check)
    col.finish()


def test_adyolo_invalid_rows_are_ignored(ops):
    """Rows with b = B, t = -1, gi = Gaz or cl = C among valid ones: dlogit keeps its bits, the loss stays within its bar."""
    cs, logit, target = ls.adyolo_inputs("constructed")
    ref = ls.adyolo_reference("constructed")
    bad = ls.invalid_rows(cs)
    mixed = torch.cat([target[:3], bad[:2], target[3:], bad[2:]], dim=0).contiguous()
    loss, dlogit, dist = run_adyolo(ops, cs, logit, target)
    loss_m, dlogit_m, dist_m = run_adyolo(ops, cs, logit, mixed)
    assert torch.equal(dlogit_m, dlogit)
    assert torch.equal(torch.cat([dist_m[:3], dist_m[5:10]]), dist)
    value_check("invalid rows: loss", loss_m, ref["loss64"], ref["loss32"])


class _TwoRanks:
    """Stands in for ``ops.EXACT`` (a process group of two ranks) on one device: the first pass records a rank's four header
    counts, the second replaces them by the counts of the whole batch, as the all-reduce between the phases would."""
    on, world = True, 2

    def __init__(self, counts=None):
        self.counts, self.seen = counts, None

    def all_reduce(self, t):
        if t.dtype == torch.int32:
            assert t.numel() == 4
            self.seen = t.clone()
            if self.counts is not None:
                t.copy_(self.counts)
        return t


def test_adyolo_two_phases_add_up_to_the_one_call_loss(ops, monkeypatch):
    """phases 1, then 2 with na_total of the whole batch, on the two halves of a batch (``ops.adyolo_loss`` under EXACT, the
    collectives replaced by ``_TwoRanks``): the shares add up to the one-call loss, the concatenated dlogit has its bits."""
    name = "8x4_a5_c12"
    cs, logit, target = ls.adyolo_inputs(name)
    ref = ls.adyolo_reference(name)
    loss, dlogit, _ = run_adyolo(ops, cs, logit, target)
    halves = []
    for r in range(2):
        rows = target[target[:, 0] == r].clone()
        rows[:, 0] = 0
        assert rows.shape[0] > 0
        halves.append((logit[r:r + 1].contiguous(), rows.contiguous()))
    counts = []
    for lg, tg in halves:                                                  # pass 1: every rank's own counts
        rank = _TwoRanks()
        monkeypatch.setattr(ops, "EXACT", rank)
        run_adyolo(ops, cs, lg, tg)
        counts.append(rank.seen)
    total = counts[0] + counts[1]
    print("header counts of the halves %s + %s = %s" % (counts[0].tolist(), counts[1].tolist(), total.tolist()))
    assert int(total[0]) == ref["coverage"]["positives"]                  # threshold 0 is the widest: positive at any threshold
    shares, grads = [], []
    for lg, tg in halves:                                                  # pass 2: the counts of the whole batch
        monkeypatch.setattr(ops, "EXACT", _TwoRanks(total))
        ls_, dl_, _ = run_adyolo(ops, cs, lg, tg)
        shares.append(ls_)
        grads.append(dl_)
    monkeypatch.undo()
    assert torch.equal(torch.cat(grads, dim=0), dlogit)
    value_check("two phases: sum of the shares", shares[0].double() + shares[1].double(), ref["loss64"], ref["loss32"])   # MI355X: 2.7e-8 (bar 9.5e-7)


# ========================================================================================================= class-wise
def seddoa_groups(g, c, sat):
    g = g.detach().cpu().reshape(sat.shape[0], -1)
    return {"BCE columns": g[:, :c][sat == 0], "BCE columns, outputs of exactly 0 / 1": g[:, :c][sat > 0], "MSE columns": g[:, c:]}


@pytest.mark.parametrize("kind", ["seddoa", "masked", "accdoa"])
@pytest.mark.parametrize("rows,c", ls.SEDDOA_CASES)
def test_seddoa_and_accdoa_loss_and_gradient_groups(ops, rows, c, kind):
    # MI355X, worst over the cases (err_gpu, err_ref; bar 9.5e-7): loss 4.8e-8, 4.8e-8; BCE columns 1.0e-7, 4.0e-8; outputs of
    # exactly 0 / 1 4.6e-8, 1.9e-8; MSE columns 1.2e-7, 1.6e-7
    from adyolo_amd.models.loss import ACCDOAloss, SEDDOAloss
    if kind == "accdoa":
        out, tgt = ls.accdoa_inputs(rows, c)
        args, crit, nsed, sat = (0, 0, 0.0, 1.0), ACCDOAloss(c), 0, torch.zeros(rows, 0, dtype=torch.int64)
    else:
        out, tgt, sat = ls.seddoa_inputs(rows, c)
        args, crit, nsed = (c, int(kind == "masked"), 1.0, 1000.0), SEDDOAloss(c, masked_mse=kind == "masked"), c
    ref = ls.seddoa_reference(out, tgt, c, kind)
    (l64, g64), (l32, g32) = ref[torch.float64], ref[torch.float32]
    loss, dout = ops.seddoa_loss(dev(out), dev(tgt), *args)
    loss_n, dout_n = ops.seddoa_loss(dev(out), dev(tgt), *args, need_grad=False)
    o = dev(out[None]).requires_grad_(True)
    loss_c = crit(o, tgt[None])
    loss_c.backward()
    torch.cuda.synchronize()
    assert dout_n is None and torch.equal(loss_n, loss)
    col = Collect()
    tag = "%s %d x %d" % (kind, rows, c)
    for via, lv, gv in (("ops", loss, dout), ("class", loss_c, o.grad)):
        col(value_check, "%s (%s) loss" % (tag, via), lv.reshape(()), l64, l32)
        got, r64, r32 = (seddoa_groups(g, nsed, sat) for g in (gv, g64, g32))
        for name in got:
            if got[name].numel():
                col(value_check, "%s (%s) dout, %s" % (tag, via, name), got[name], r64[name], r32[name])
        if nsed:                                        # output equal to its target of 0 or 1: the gradient is 0, not merely small

            def matched_are_zero(gv=gv, via=via):
                z = gv.detach().cpu().reshape(rows, -1)[:, :c][sat == 1]
                assert z.numel() > 0 and bool((z == 0).all()), "%s (%s): gradient of an output equal to its 0 / 1 target is not 0" % (tag, via)
            col(matched_are_zero)
    col.finish()


@pytest.mark.parametrize("rows,c", ls.ADPIT_CASES)
def test_adpit_loss_and_gradient(ops, rows, c):
    # MI355X, worst over the cases (err_gpu, err_ref; bar 9.5e-7): loss 4.7e-8, 6.1e-8; dout 1.1e-7, 1.1e-7 (7 x 13)
    from adyolo_amd.models.loss import ADPITloss
    out, tgt, _ = ls.adpit_inputs(rows, c)
    ref, fragile = ls.adpit_reference(out, tgt, c)
    (l64, g64), (l32, g32) = ref[torch.float64], ref[torch.float32]
    keep = (~fragile)[:, None, :].expand(rows, 9, c).reshape(rows, 9 * c)
    print("adpit %d x %d: %d fragile items of %d" % (rows, c, int(fragile.sum()), fragile.numel()))
    loss, dout = ops.adpit_loss(dev(out), dev(tgt), c)
    loss_n, dout_n = ops.adpit_loss(dev(out), dev(tgt), c, need_grad=False)
    o = dev(out[None]).requires_grad_(True)
    loss_c = ADPITloss(c)(o, tgt[None])
    loss_c.backward()
    torch.cuda.synchronize()
    assert dout_n is None and torch.equal(loss_n, loss)
    col = Collect()
    for via, lv, gv in (("ops", loss, dout), ("class", loss_c, o.grad)):
        col(value_check, "adpit %d x %d (%s) loss" % (rows, c, via), lv.reshape(()), l64, l32)
        col(value_check, "adpit %d x %d (%s) dout" % (rows, c, via), gv.reshape(rows, 9 * c), g64, g32, keep=keep)
    col.finish()


@pytest.mark.parametrize("rows,cols,n_sig", ls.ACT_CASES)
def test_head_activation_forward_and_backward(ops, rows, cols, n_sig):
    # MI355X, worst over the cases (err_gpu = err_ref but for tanh y 7.9e-8 against 3.1e-8): y 8.8e-8 / 7.9e-8 (sigmoid / tanh
    # columns), dx 2.5e-7 / 7.6e-8; bars 9.5e-7, 1.0e-6 for the sigmoid dx
    from adyolo_amd import functional as Fn
    x, probe = ls.act_inputs(rows, cols)
    ref = ls.act_reference(x, probe, n_sig)
    (y64, dx64), (y32, dx32) = ref[torch.float64], ref[torch.float32]
    xg = dev(x).requires_grad_(True)
    y = Fn.ActFn.apply(xg, n_sig)
    (y * dev(probe)).sum().backward()
    torch.cuda.synchronize()
    col = Collect()
    tag = "act %d x %d, n_sig %d" % (rows, cols, n_sig)
    for name, sl in (("sigmoid columns", slice(0, n_sig)), ("tanh columns", slice(n_sig, cols))):
        if sl.stop > sl.start:
            col(value_check, "%s y, %s" % (tag, name), y[:, sl], y64[:, sl], y32[:, sl])
            col(value_check, "%s dx, %s" % (tag, name), xg.grad[:, sl], dx64[:, sl], dx32[:, sl])
    col.finish()
