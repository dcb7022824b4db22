"""GPU: parameter groups of the fused optimizers (csrc/optim.hip, the ``*_groups`` entry points).

The oracle for bits is the existing ungrouped scheduled entry point, never the new code: a group's elements, gathered into a
contiguous buffer and stepped by ``adam_step_sched_dev`` / ``sgd_step_sched_dev`` with the same counter, a table whose base is
the group's rate and the group's decay, must come out bit-equal to what the grouped launch left in place.  With clipping
the norm and the coefficient of the grouped call are first required to be ``grad_norm_dev``'s on the whole buffer (bits), and
the oracle runs unclipped with ``grad_scale`` = the float32 product 0.25 * coef, which is the ``gs`` the grouped kernel forms.
Against torch.optim the bounds are those of test_gpu_optimizers (1e-6 absolute on N(0,1) parameters and on the moments, 1e-5
on the momentum buffer)."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


CONSTANT = {"name": "constant"}
COSINE = {"name": "cosine", "T_max": 5, "eta_min": 1e-5, "warmup_steps": 2, "warmup_start_factor": 0.25}
EMA_DECAY = 0.9


def _table(cfg, base, ema):
    from adyolo_amd import lr_schedule
    return lr_schedule.table(lr_schedule.normalise(cfg), base, ema_decay=EMA_DECAY if ema else None)


def _dev64(x):
    return torch.tensor(x, dtype=torch.float64).to(DEV)


def _f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ layouts
def _runs(n, lengths, groups, start=0, base=None):
    m = torch.zeros(n, dtype=torch.uint8) if base is None else base
    i, k = start, 0
    while i < n:
        ln = lengths[k % len(lengths)]
        m[i:i + ln] = groups[k % len(groups)]
        i += ln
        k += 1
    return m


def _layout(name):
    """-> (n, map on the CPU, number of groups)"""
    if name == "tail_only":                       # n = 3: no float4 access at all, two groups
        return 3, torch.tensor([0, 1, 0], dtype=torch.uint8), 2
    if name == "change_in_tail":                  # n = 4099: the 3-element tail holds groups 0 | 1 | 1, a 2+2 split before it
        m = torch.zeros(4099, dtype=torch.uint8)
        m[2050:3000] = 1
        m[4097:] = 1
        return 4099, m, 2
    if name == "every_offset":                    # n = 10004: changes at offsets 1, 2, 3, 0 mod 4; four groups in one vector; a
        m = torch.zeros(10004, dtype=torch.uint8)  # group of one element; a group made of many separate runs
        m[101:202] = 1                            # starts 1 + 3, ends 2 + 2
        m[202:303] = 2                            # ends 3 + 1
        m[303:400] = 3                            # ends on a vector boundary
        m[1000:1004] = torch.tensor([0, 1, 2, 3], dtype=torch.uint8)
        m[5001] = 4                               # a single element
        m = _runs(9000, [7, 13, 4, 1, 30], [5, 0], start=6000, base=m)      # group 5: ~ 270 separate runs
        return 10004, m, 6
    if name == "sixteen":                         # 16 groups in runs of odd lengths
        m = _runs(10004, [37, 5, 111, 2, 64, 9], list(range(16)))
        assert len(set(m.tolist())) == 16
        return 10004, m, 16
    if name == "grid_stride":                     # more than 2048 x 256 float4: the loop runs twice for some lanes
        n = 2200003
        assert n // 4 > 2048 * 256
        return n, _runs(n, [100003, 7, 65537, 1, 299999], [0, 1, 2]), 3
    raise KeyError(name)


LAYOUTS = ["tail_only", "change_in_tail", "every_offset", "sixteen", "grid_stride"]
KINDS = ["adam", "adamw", "sgd_momentum", "sgd_nesterov"]
_DATA = {}


def _data(name, steps=3):
    """parameters, pre-multiplied gradients and an EMA start, made once per layout and never written"""
    if name not in _DATA:
        n, m, ng = _layout(name)
        g = torch.Generator().manual_seed(1234 + n % 1000)
        p0 = torch.randn(n, generator=g)
        grads = [(torch.randn(n, generator=g) * 4.0).to(DEV) for _ in range(steps)]
        idx = [torch.nonzero(m == k).flatten().to(DEV) for k in range(ng)]
        assert all(len(i) > 0 for i in idx)
        _DATA[name] = (n, m.to(DEV), ng, p0.to(DEV), grads, idx)
    return _DATA[name]


def _group_values(kind, ng):
    base = 0.01 if kind.startswith("sgd") else 1e-3
    rates = [base * (1.0 + 0.37 * k) for k in range(ng)]
    wds = [0.01 * ((k + 1) % 3) for k in range(ng)]          # 0.01, 0.02, 0, ...: both sides of the wd != 0 test
    return rates, wds


class _State:
    """the buffers of one optimizer run over n elements"""

    def __init__(self, ops, kind, p, ema):
        self.kind, self.p = kind, p.clone()
        self.sgd = kind.startswith("sgd")
        self.bufs = [torch.full_like(p, 123.0)] if self.sgd else [torch.zeros_like(p), torch.zeros_like(p)]
        self.ema = torch.full_like(p, -7.0) if ema else None          # (the first update does not read it)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device=DEV)
        self.out = torch.zeros(ops.SCHED_OUT_FLOATS, device=DEV)

    def tensors(self):
        return [("p", self.p)] + [("state%d" % i, b) for i, b in enumerate(self.bufs)] + ([("ema", self.ema)] if self.ema is not None else [])

    def sched_step(self, ops, grad, table, wd, grad_scale, partials=None, max_norm=None):
        """the ungrouped scheduled entry point"""
        kw = dict(grad_scale=grad_scale, partials=partials, max_norm=max_norm)
        if self.sgd:
            ops.sgd_step_sched_dev(self.p, grad, self.bufs[0], self.step_dev, self.st, table, self.out, self.ema, weight_decay=wd,
                                   momentum=0.9, nesterov=self.kind == "sgd_nesterov", **kw)
        else:
            ops.adam_step_sched_dev(self.p, grad, self.bufs[0], self.bufs[1], self.step_dev, self.st, table, self.out, self.ema,
                                    weight_decay=wd, decoupled=self.kind == "adamw", **kw)

    def groups_step(self, ops, grad, table, gdev, gout, gmap, grad_scale, partials=None, max_norm=None):
        kw = dict(grad_scale=grad_scale, partials=partials, max_norm=max_norm)
        if self.sgd:
            ops.sgd_step_groups_dev(self.p, grad, self.bufs[0], self.step_dev, self.st, table, self.out, gdev, gout, gmap,
                                    self.ema, momentum=0.9, nesterov=self.kind == "sgd_nesterov", **kw)
        else:
            ops.adam_step_groups_dev(self.p, grad, self.bufs[0], self.bufs[1], self.step_dev, self.st, table, self.out, gdev,
                                     gout, gmap, self.ema, decoupled=self.kind == "adamw", **kw)


def _groups_dev(rates, wds):
    return _dev64([[r, _f32(w)] for r, w in zip(rates, wds)])


def _run_grouped(ops, kind, name, ema, clip, cfg, rates, wds):
    """3 grouped steps -> the state and, per step, (st[2], st[3]) as the grouped call left them"""
    n, gmap, ng, p0, grads, _ = _data(name)
    s = _State(ops, kind, p0, ema)
    table = _dev64(_table(cfg, rates[0], ema))
    gdev, gout = _groups_dev(rates, wds), torch.zeros(ng, ops.GROUP_OUT_FLOATS, device=DEV)
    parts = torch.zeros(ops.GRAD_SUMSQ_MAX_PARTS, dtype=torch.float64, device=DEV) if clip else None
    seen = []
    for gr in grads:
        s.groups_step(ops, gr, table, gdev, gout, gmap, 0.25, parts, clip)
        seen.append(s.st[2:4].clone())
    return s, seen, gout


def _clip_for(name):
    """a max_norm that binds on every step: a tenth of the smallest gradient norm"""
    grads = _data(name)[4]
    return 0.1 * min(float(g.double().norm()) * 0.25 for g in grads)


# ------------------------------------------------------------------------------------------------ 1. per group, bit for bit
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", LAYOUTS)
def test_every_group_gets_the_bits_of_the_ungrouped_step(ops, name, kind):
    n, gmap, ng, p0, grads, idx = _data(name)
    rates, wds = _group_values(kind, ng)
    for ema in (False, True):
        for clip in (None, _clip_for(name)):
            for cfg in (CONSTANT, COSINE):
                what = (name, kind, ema, clip is not None, cfg["name"])
                s, seen, gout = _run_grouped(ops, kind, name, ema, clip, cfg, rates, wds)
                scales = [0.25] * len(grads)
                if clip is not None:                  # the norm is global: grad_norm_dev on the WHOLE buffer, as bits
                    st2 = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device=DEV)
                    parts = torch.zeros(ops.GRAD_SUMSQ_MAX_PARTS, dtype=torch.float64, device=DEV)
                    for k, gr in enumerate(grads):
                        ops.grad_norm_dev(gr, parts, st2, clip, grad_scale=0.25)
                        assert torch.equal(st2[2:4], seen[k]), (what, k, st2[2:4].tolist(), seen[k].tolist())
                        coef = float(seen[k][1])
                        assert 0.0 < coef < 1.0, (what, k, coef)
                        scales[k] = float(np.float32(0.25) * np.float32(coef))
                else:
                    assert all(float(x[1]) == 1.0 for x in seen), what
                assert int(s.step_dev) == len(grads)
                got = dict(s.tensors())
                for g in range(ng):
                    o = _State(ops, kind, p0[idx[g]], ema)
                    table = _dev64(_table(cfg, rates[g], ema))
                    for k, gr in enumerate(grads):
                        o.sched_step(ops, gr[idx[g]].contiguous(), table, wds[g], scales[k])
                    assert _f32(float(gout[g, 0])) == float(o.out[0]) and float(gout[g, 3]) == _f32(wds[g]), (what, g)
                    for label, want in o.tensors():
                        have = got[label][idx[g]]
                        assert torch.equal(have, want), (what, g, label, int((have != want).sum()), len(want))
                assert bool(torch.isfinite(s.p).all()) and not torch.equal(s.p, p0)


# ------------------------------------------------------------------------------------------------ 2. equal groups are no groups
@gpu
@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd_momentum"])
@pytest.mark.parametrize("name", ["change_in_tail", "sixteen"])
def test_equal_groups_are_no_groups(ops, name, kind):
    """every group at the same rate and decay, EMA and a binding clip: the bits of the ungrouped scheduled call on the whole
    buffer, scratch and ``sched_out`` included"""
    n, gmap, ng, p0, grads, _ = _data(name)
    rate, wd, clip = (0.01 if kind.startswith("sgd") else 1e-3), 0.01, _clip_for(name)
    for cfg in (CONSTANT, COSINE):
        s, seen, gout = _run_grouped(ops, kind, name, True, clip, cfg, [rate] * ng, [wd] * ng)
        o = _State(ops, kind, p0, True)
        table = _dev64(_table(cfg, rate, True))
        parts = torch.zeros(ops.GRAD_SUMSQ_MAX_PARTS, dtype=torch.float64, device=DEV)
        for k, gr in enumerate(grads):
            o.sched_step(ops, gr, table, wd, 0.25, parts, clip)
            assert torch.equal(o.st[2:4], seen[k]) and float(seen[k][1]) < 1.0
        for (label, have), (_, want) in zip(s.tensors() + [("st", s.st), ("out", s.out)], o.tensors() + [("st", o.st), ("out", o.out)]):
            assert torch.equal(have, want), (name, kind, cfg["name"], label, int((have != want).sum()))
        assert torch.equal(gout[:, 0], o.out[0:1].expand(ng))


# ------------------------------------------------------------------------------------------------ 3. against torch
@gpu
@pytest.mark.parametrize("kind", ["adamw", "sgd_momentum"])
def test_grouped_step_matches_torch(ops, kind):
    """7 steps against torch.optim.AdamW / SGD(momentum 0.9) with two groups (decay 0.01 / 0, rates 1e-3 / 1e-4) on the CPU;
    n = 4099 with the group change inside a vector and inside the tail"""
    n, m, ng = _layout("change_in_tail")
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=g)
    idx = [torch.nonzero(m == k).flatten() for k in range(2)]
    refs = [p0[i].clone().requires_grad_(True) for i in idx]
    rates, wds = [1e-3, 1e-4], [0.01, 0.0]
    tg = [{"params": [r], "lr": lr, "weight_decay": wd} for r, lr, wd in zip(refs, rates, wds)]
    opt = torch.optim.AdamW(tg) if kind == "adamw" else torch.optim.SGD(tg, lr=1.0, momentum=0.9)
    s = _State(ops, kind, p0.to(DEV), False)
    table, gdev = _dev64(_table(CONSTANT, rates[0], False)), _groups_dev(rates, wds)
    gout, gmap = torch.zeros(2, ops.GROUP_OUT_FLOATS, device=DEV), m.to(DEV)
    for _ in range(7):
        grad = torch.randn(n, generator=g)
        for r, i in zip(refs, idx):
            r.grad = grad[i].clone()
        opt.step()
        s.groups_step(ops, (grad * 4.0).to(DEV), table, gdev, gout, gmap, 0.25)
    for k, (r, i) in enumerate(zip(refs, idx)):
        err = float((s.p.cpu()[i] - r.detach()).abs().max())
        print("%s group %d: max |p - torch| = %.3e" % (kind, k, err))
        assert err <= 1e-6, (kind, k, err)
        state = opt.state[r]
        if kind == "adamw":
            assert float((s.bufs[0].cpu()[i] - state["exp_avg"]).abs().max()) <= 1e-6
            assert float((s.bufs[1].cpu()[i] - state["exp_avg_sq"]).abs().max()) <= 1e-6
        else:
            assert float((s.bufs[0].cpu()[i] - state["momentum_buffer"]).abs().max()) <= 1e-5
    assert float((s.p.cpu() - p0).abs().max()) > 1e-4


# ------------------------------------------------------------------------------------------------ optimizer-level helpers
class _Bag(torch.nn.Module):
    def __init__(self, seed=9):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.body = torch.nn.Parameter(torch.randn(37, 111, generator=g))         # 4107: no float4 boundary anywhere
        self.scale = torch.nn.Parameter(torch.randn(5, generator=g))
        self.head = torch.nn.Parameter(torch.randn(3, 7, generator=g))
        self.bias = torch.nn.Parameter(torch.randn(1, generator=g))


def _bag_flat(seed=9):
    from adyolo_amd.dist import FlatParameters
    net = _Bag(seed).to(DEV)
    return net, FlatParameters(net)


def _set_grads(net, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    grads = [torch.randn(p.shape, generator=g) for p in net.parameters()]
    for p, gr in zip(net.parameters(), grads):
        p.grad.copy_((gr * scale).to(DEV))
    return grads


def _member_index(flat, group):
    """the flat-buffer indices of a resolved group's elements"""
    where = {id(p): k for k, p in enumerate(flat.params)}
    out = []
    for i in group["params"]:
        off, n = flat.offsets[where[id(flat.module_params[i])]]
        out.append(torch.arange(off, off + n))
    return torch.cat(out).to(DEV)


# ------------------------------------------------------------------------------------------------ 4. a rate-0 group
@gpu
@pytest.mark.parametrize("cfg", [CONSTANT, COSINE], ids=["constant", "cosine"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_a_rate_zero_group_stands_still_until_released(ops, wd, cfg):
    from adyolo_amd.train import FusedAdamW
    net, flat = _bag_flat()
    groups = [{"name": "frozen", "lr": 0.0, "weight_decay": wd, "params": [0, 1]},
              {"name": "head", "lr": 2e-3, "weight_decay": 0.01, "params": [2, 3]}]
    opt = FusedAdamW(flat, lr_schedule=cfg, param_groups=groups)
    idx = [_member_index(flat, g) for g in opt.groups]
    p0 = flat.flat.clone()
    oracle = _State(ops, "adamw", p0[idx[1]], False)
    table = _dev64(_table(cfg, 2e-3, False))
    for k in range(3):
        _set_grads(net, 40 + k)
        oracle.sched_step(ops, flat.flat_grad[idx[1]].contiguous(), table, 0.01, 1.0)
        opt.step()
        assert opt.current_lrs.tolist() == [0.0, opt.lr_at(k + 1, group="head")]
    assert torch.equal(flat.flat[idx[0]], p0[idx[0]])                          # bit-unchanged ...
    assert float(opt.exp_avg[idx[0]].abs().min()) > 0.0 and float(opt.exp_avg_sq[idx[0]].abs().min()) > 0.0   # ... moments moved
    assert torch.equal(flat.flat[idx[1]], oracle.p) and torch.equal(opt.exp_avg[idx[1]], oracle.bufs[0])
    assert not torch.equal(flat.flat[idx[1]], p0[idx[1]])
    # released: the next step moves it exactly as the ungrouped step with that base does, from the moments it has gathered
    opt.set_lr(1e-3, group="frozen")
    rel = _State(ops, "adamw", flat.flat[idx[0]], False)
    rel.bufs = [opt.exp_avg[idx[0]].clone(), opt.exp_avg_sq[idx[0]].clone()]
    rel.step_dev.fill_(3)
    _set_grads(net, 43)
    rel.sched_step(ops, flat.flat_grad[idx[0]].contiguous(), _dev64(_table(cfg, 1e-3, False)), wd, 1.0)
    opt.step()
    assert torch.equal(flat.flat[idx[0]], rel.p) and not torch.equal(rel.p, p0[idx[0]])
    assert torch.equal(opt.exp_avg[idx[0]], rel.bufs[0]) and torch.equal(opt.exp_avg_sq[idx[0]], rel.bufs[1])
    assert float(opt.current_lrs[0]) == opt.lr_at(4, group="frozen") > 0.0


# ------------------------------------------------------------------------------------------------ 5. device rates
RATE_COMMON = {"every": 2, "warmup_steps": 3, "warmup_start_factor": 0.25}
RATE_KINDS = {"constant": {}, "step": {"gamma": 0.7, "step_size": 2}, "multistep": {"gamma": 0.3, "milestones": [2, 5]},
              "exponential": {"gamma": 0.93}, "cosine": {"T_max": 5, "eta_min": 1e-5}}


@gpu
@pytest.mark.parametrize("optim", ["adam", "sgd"])
@pytest.mark.parametrize("kind", sorted(RATE_KINDS))
def test_device_rates_follow_lr_at(ops, kind, optim):
    """``current_lrs`` after each of 12 steps (warm-up 3, ``every`` 2) equals ``lr_at(t, g)`` for every group, a rate-0 group
    among them; ``current_lr`` is group 0's"""
    from adyolo_amd.train import FusedAdam, FusedSGD
    net, flat = _bag_flat()
    groups = [{"name": "a", "lr": 0.03, "weight_decay": 0.0, "params": [0]}, {"name": "b", "lr": 2e-3, "weight_decay": 0.1, "params": [1, 3]},
              {"name": "still", "lr": 0.0, "weight_decay": 0.0, "params": [2]}]
    cfg = dict(RATE_KINDS[kind], name=kind, **RATE_COMMON)
    opt = (FusedAdam if optim == "adam" else FusedSGD)(flat, lr_schedule=cfg, param_groups=groups)
    for t in range(1, 13):
        opt.step()
        got, want = opt.current_lrs.tolist(), [opt.lr_at(t, group=g) for g in range(3)]
        print("%s %s t=%d: device %r host %r" % (kind, optim, t, got, want))
        assert got == want, (kind, optim, t, got, want)
        assert float(opt.current_lr) == got[0] and got[2] == 0.0 and got[0] > 0.0 and got[1] > 0.0


# ------------------------------------------------------------------------------------------------ 6. whole step
def _params(**train_config):
    tc = {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
          "conf_thresh": 0.5, "clss_thresh": 0.5, "unify_thresh": 15.0, "nms": "conn-merge",
          "loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
          "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0}
    tc.update(train_config)
    return {"args": {"device": "cuda:0", "encoder": "se-resnet34", "loss": "adyolo"},
            "data_config": {"nb_classes": 12}, "train_config": tc}


def _trainer(graph, t=80, **train_config):
    from adyolo_amd.wrapper import WrapperModel, WrapperCriterion
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.train import TrainStep
    torch.manual_seed(100)
    prm = _params(**train_config)
    model = WrapperModel((1, 7, t, 64), (), prm).to("cuda:0")
    return TrainStep(model, WrapperCriterion(prm), FeatureExtractor(None, "cuda:0"), prm, graph=graph)


NO_DECAY = {"optim": "AdamW", "weight_decay": 0.01, "clip_grad_norm": 3.0,
            "param_groups": [{"name": "no_decay", "ndim_max": 1, "weight_decay": 0.0}]}


@gpu
def test_graphed_grouped_step_is_bit_identical_to_eager(ops):
    """2 clips x 2 s, AdamW with the no-decay grouping + clip_grad_norm: 6 steps eager against hipGraph replay are bit-equal
    in loss, parameters, moments, ``grad_norm`` and the groups' rates; a ``set_lr(group=)`` between replays changes the next
    step and records nothing"""
    from adyolo_amd.datasets import synthetic_audio, synthetic_targets
    audios = [synthetic_audio(2, 24000 * 2, seed=70 + i).to("cuda:0") for i in range(3)]
    targets = [synthetic_targets(2, 20, 12, seed=80 + i) for i in range(6)]
    te, tg = _trainer(False, **NO_DECAY), _trainer(True, **NO_DECAY)
    oe, og = te.optimizer, tg.optimizer
    assert tg.graphs is not None and te.graphs is None and oe.kind == "adamw"
    assert [g["name"] for g in og.groups] == ["default", "no_decay"] and [g["weight_decay"] for g in og.groups] == [0.01, 0.0]
    assert sum(tg.flat.module_params[i].numel() for i in og.groups[1]["params"]) == int((og.group_map == 1).sum())
    rates = []
    for i in range(6):
        a = te.step(audios[i % 3], targets[i])
        b = tg.step(audios[i % 3], targets[i])
        assert torch.equal(a, b), "loss of step %d: eager %r graph %r" % (i + 1, float(a), float(b))
        for name, x, y in (("p", te.flat.flat, tg.flat.flat), ("m", oe.exp_avg, og.exp_avg), ("v", oe.exp_avg_sq, og.exp_avg_sq),
                           ("lrs", oe.current_lrs, og.current_lrs), ("norm", oe.grad_norm, og.grad_norm)):
            assert torch.equal(x, y), (i + 1, name)
        rates.append(og.current_lrs.tolist())
        if i == 3:
            entries = len(tg.graphs.entries)
            oe.set_lr(5e-4, group="no_decay")
            og.set_lr(5e-4, group="no_decay")
    assert tg.graphs.captures == 1 and tg.graphs.replays == 5 and tg.graphs.eager_steps == 1
    assert len(tg.graphs.entries) == entries == 1
    assert rates[:4] == [[_f32(1e-3)] * 2] * 4 and rates[4:] == [[_f32(1e-3), _f32(5e-4)]] * 2
    assert bool(torch.isfinite(tg.flat.flat).all()) and float(og.grad_norm) > 0.0
    assert oe.step_count == og.step_count == 6 and int(og.step_dev) == 6


# ------------------------------------------------------------------------------------------------ 7. resume
@gpu
def test_resume_from_a_grouped_torch_checkpoint(ops):
    from adyolo_amd import checkpoint as ck
    from adyolo_amd import param_groups
    from adyolo_amd.train import FusedAdamW
    net, flat = _bag_flat(seed=21)
    groups = param_groups.resolve([{"name": "no_decay", "ndim_max": 1, "weight_decay": 0.0, "lr": 1e-4}], flat, 1e-3, 0.01)
    twin = [torch.nn.Parameter(p.detach().cpu().clone()) for p in net.parameters()]

    def torch_groups(ps):
        return [{"params": [ps[i] for i in g["params"]], "lr": g["lr"], "weight_decay": g["weight_decay"]} for g in groups]

    topt = torch.optim.AdamW(torch_groups(twin))
    for k in range(2):                                                   # the run that wrote the checkpoint: torch alone
        for p, gr in zip(twin, _set_grads(net, 60 + k)):
            p.grad = gr.clone()
        topt.step()
    saved = topt.state_dict()
    with torch.no_grad():
        for p, q in zip(net.parameters(), twin):
            p.copy_(q.to(DEV))
    opt = FusedAdamW(flat, lr=5e-2, weight_decay=0.3, param_groups=[dict(g, lr=0.5) for g in groups])
    ck.load_optimizer_state_dict(opt, net, saved)
    assert opt.step_count == 2 and [(g["lr"], g["weight_decay"]) for g in opt.groups] == [(1e-3, 0.01), (1e-4, 0.0)]
    for k in range(2):                                                   # two more steps on both sides
        for p, gr in zip(twin, _set_grads(net, 62 + k)):
            p.grad = gr.clone()
        topt.step()
        opt.step()
    for i, (p, q) in enumerate(zip(net.parameters(), twin)):
        err = float((p.detach().cpu() - q.detach()).abs().max())
        print("parameter %d: max |fused - torch| = %.3e" % (i, err))
        assert err <= 1e-6, (i, err)
    out = ck.optimizer_state_dict(opt, net)
    fresh = torch.optim.AdamW(torch_groups([torch.nn.Parameter(q.detach().clone()) for q in twin]))
    fresh.load_state_dict(out)
    back, want = fresh.state_dict(), topt.state_dict()
    assert [g["params"] for g in back["param_groups"]] == [g["params"] for g in want["param_groups"]]
    assert [(g["lr"], g["weight_decay"]) for g in back["param_groups"]] == [(1e-3, 0.01), (1e-4, 0.0)]
    for i in want["state"]:
        assert int(back["state"][i]["step"]) == 4
        assert float((back["state"][i]["exp_avg"] - want["state"][i]["exp_avg"]).abs().max()) <= 1e-6
        assert float((back["state"][i]["exp_avg_sq"] - want["state"][i]["exp_avg_sq"]).abs().max()) <= 1e-6
