"""GPU: gradient accumulation in the fused optimizers (csrc/optim.hip, ``adyolo_*_step_accum_dev``;
``train_config['accum_steps']``).  K calls are one optimizer step: K - 1 hold calls that move the accumulator and the
accumulation record and nothing else, and a last call that is today's step of the same form on the accumulator under
``float32(float64(grad_scale) / K)``.  Every comparison is bitwise (``torch.equal`` on the raw buffers) except the one against
torch.optim, which keeps the bounds of test_gpu_optimizers' tests of the same rules and sizes (1e-6 on parameters and Adam's
moments, 1e-5 on the momentum buffer).

The sum of squares of a cycle's last call is FUSED into the accumulation pass; ``test_fused_sum_of_squares...`` pins it to the
bits ``adyolo_grad_norm_dev`` gives on the finished accumulator."""
import copy

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"

N_TAIL, N_MID, N_BIG = 3, 1027, 1048576 + 1024 + 2       # tail only | one workgroup's vectors + 3 | past the sum-of-squares grid cap
SIZES = (N_TAIL, N_MID, N_BIG)
RULES = ("adam", "adamw", "sgd", "sgdm")
FORMS = ("plain", "sched", "sched_ema", "groups", "groups_ema")
LR = 0.01
NAN, INF = float("nan"), float("inf")
CLIPS = {"noclip": None, "clip": 1.0, "loose": 1e4}       # off | binds on every gradient used here | never binds


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


_CLEAN = {}


def _clean(n, seed):
    """N(0, 1) gradients, made once per (n, seed) and never written"""
    if (n, seed) not in _CLEAN:
        _CLEAN[n, seed] = torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return _CLEAN[n, seed]


def _scale_eff(grad_scale, k):
    """float32(float64(float32(grad_scale)) / k), as a Python float"""
    return float(np.float32(np.float64(np.float32(grad_scale)) / k))


class Rig:
    """The buffers of one optimizer at the level of ``ops``: rule x form x clipping [x guard] over n elements, stepped
    through the accumulating entry point (``micro``) or through today's entry point of the same form (``today``)."""

    def __init__(self, ops, rule, form, clip, n, guarded=False, k=3, seed=0):
        from adyolo_amd import lr_schedule
        self.ops, self.rule, self.form, self.n, self.guarded, self.k = ops, rule, form, n, guarded, k
        self.max_norm = CLIPS[clip] if isinstance(clip, str) else (1.0 if clip else None)
        self.adam = rule in ("adam", "adamw")
        self.wd = 0.0 if rule == "sgd" else 0.01
        self.p = torch.randn(n, generator=torch.Generator().manual_seed(1000 + seed)).to(DEV)
        self.state = [torch.zeros_like(self.p) for _ in range(2 if self.adam else 1 if rule == "sgdm" else 0)]
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device=DEV)
        self.partials = torch.zeros(ops.GRAD_SUMSQ_MAX_PARTS, dtype=torch.float64, device=DEV)
        self.guard = torch.zeros(ops.OPTIM_GUARD_WORDS, dtype=torch.int64, device=DEV)
        self.accum = torch.full((n,), NAN, device=DEV)     # (a cycle's first call must overwrite, not read, it)
        self.acc = torch.zeros(ops.OPTIM_ACCUM_WORDS, dtype=torch.int64, device=DEV)
        self.sched_dev = self.sched_out = self.ema = self.groups_dev = self.groups_out = self.gmap = None
        if form != "plain":
            ema = form.endswith("_ema")
            cfg = lr_schedule.normalise({"name": "cosine", "T_max": 20, "warmup_steps": 3})
            tb = lr_schedule.table(cfg, LR, ema_decay=0.9 if ema else None, ema_warmup=ema)
            self.sched_dev = torch.tensor(tb, dtype=torch.float64).to(DEV)
            self.sched_out = torch.zeros(ops.SCHED_OUT_FLOATS, device=DEV)
            self.ema = torch.zeros_like(self.p) if ema else None
        if form.startswith("groups"):
            wd32 = float(torch.tensor(self.wd, dtype=torch.float32))
            self.groups_dev = torch.tensor([[LR, wd32], [LR / 2, 0.0]], dtype=torch.float64).to(DEV)
            self.groups_out = torch.zeros(2, ops.GROUP_OUT_FLOATS, device=DEV)
            self.gmap = (torch.arange(n) % 7 < 3).to(torch.uint8).to(DEV)         # both groups inside single vectors

    def fork(self):
        twin = copy.copy(self)
        for k, v in vars(self).items():
            if torch.is_tensor(v):
                setattr(twin, k, v.clone())
        twin.state = [s.clone() for s in self.state]
        return twin

    def buffers(self):
        """everything a hold call must leave alone (``st`` whole: norm and coefficient included)"""
        out = {"p": self.p, "step_dev": self.step_dev, "st": self.st}
        out.update({"state%d" % k: s for k, s in enumerate(self.state)})
        for k in ("ema", "sched_out", "groups_out"):
            if getattr(self, k) is not None:
                out[k] = getattr(self, k)
        if self.guarded:
            out["guard"] = self.guard
        return out

    def snapshot(self):
        return {k: v.clone() for k, v in self.buffers().items()}

    def _parts(self):
        return self.partials if (self.max_norm is not None or self.guarded) else None

    def micro(self, grad, grad_scale=1.0, k=None):
        """one call of the accumulating entry point"""
        ops = self.ops
        kw = dict(accum=self.accum, accum_dev=self.acc, accum_steps=self.k if k is None else k,
                  guard=self.guard if self.guarded else None, partials=self._parts(), lr=LR, weight_decay=self.wd,
                  grad_scale=grad_scale, max_norm=self.max_norm, sched_dev=self.sched_dev, sched_out=self.sched_out,
                  ema=self.ema, groups_dev=self.groups_dev, groups_out=self.groups_out, group_map=self.gmap)
        if self.adam:
            m, v = self.state
            return ops.adam_step_accum_dev(self.p, grad, m, v, self.step_dev, self.st, decoupled=self.rule == "adamw", **kw)
        buf = self.state[0] if self.state else None
        ops.sgd_step_accum_dev(self.p, grad, buf, self.step_dev, self.st, momentum=0.9 if buf is not None else 0.0,
                               dampening=0.1 if buf is not None else 0.0, **kw)

    def today(self, grad, grad_scale=1.0):
        """one step through the entry point that exists without accumulation: the guarded one, or the form's own"""
        ops, mn, parts = self.ops, self.max_norm, self._parts()
        sched = (self.sched_dev, self.sched_out)
        groups = (self.groups_dev, self.groups_out, self.gmap)
        if self.adam:
            dec = self.rule == "adamw"
            m, v = self.state
            if self.guarded:
                ops.adam_step_guard_dev(self.p, grad, m, v, self.step_dev, self.st, self.guard, parts, lr=LR,
                                        weight_decay=self.wd, grad_scale=grad_scale, max_norm=mn, decoupled=dec,
                                        sched_dev=self.sched_dev, sched_out=self.sched_out, ema=self.ema,
                                        groups_dev=self.groups_dev, groups_out=self.groups_out, group_map=self.gmap)
            elif self.groups_dev is not None:
                ops.adam_step_groups_dev(self.p, grad, m, v, self.step_dev, self.st, *sched, *groups, self.ema,
                                         grad_scale=grad_scale, partials=parts, max_norm=mn, decoupled=dec)
            elif self.sched_dev is not None:
                ops.adam_step_sched_dev(self.p, grad, m, v, self.step_dev, self.st, *sched, self.ema, weight_decay=self.wd,
                                        grad_scale=grad_scale, partials=parts, max_norm=mn, decoupled=dec)
            else:
                ops.adam_step_dev(self.p, grad, m, v, self.step_dev, self.st, lr=LR, weight_decay=self.wd,
                                  grad_scale=grad_scale, partials=parts, max_norm=mn, decoupled=dec)
            return
        buf = self.state[0] if self.state else None
        kw = dict(momentum=0.9 if buf is not None else 0.0, dampening=0.1 if buf is not None else 0.0, grad_scale=grad_scale,
                  max_norm=mn)
        if self.guarded:
            ops.sgd_step_guard_dev(self.p, grad, buf, self.step_dev, self.st, self.guard, parts, lr=LR, weight_decay=self.wd,
                                   sched_dev=self.sched_dev, sched_out=self.sched_out, ema=self.ema,
                                   groups_dev=self.groups_dev, groups_out=self.groups_out, group_map=self.gmap, **kw)
        elif self.groups_dev is not None:
            ops.sgd_step_groups_dev(self.p, grad, buf, self.step_dev, self.st, *sched, *groups, self.ema, partials=parts, **kw)
        elif self.sched_dev is not None:
            ops.sgd_step_sched_dev(self.p, grad, buf, self.step_dev, self.st, *sched, self.ema, weight_decay=self.wd,
                                   partials=parts, **kw)
        else:
            ops.sgd_step_dev(self.p, grad, buf, self.step_dev, self.st, lr=LR, weight_decay=self.wd, partials=parts, **kw)


def _assert_equal(got, want, what=""):
    for k, v in got.items():
        assert torch.equal(v, want[k]) or (k == "st" and _same_bits(v, want[k])), (what, k, v.tolist()[:8], want[k].tolist()[:8])


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _one_cycle_in(ops, rule, form, clip, n, guarded, k=3):
    """a rig after one full clean cycle (state, counter, schedule and EMA are past their first step)"""
    rig = Rig(ops, rule, form, clip, n, guarded, k)
    for j in range(k):
        rig.micro(_clean(n, 10 + j), 0.5)
    torch.cuda.synchronize()
    assert rig.acc.tolist() == [0, k, 1, 0] and int(rig.step_dev) == 1 and bool(torch.isfinite(rig.p).all())
    return rig


MATRIX = [(r, f, c) for r in RULES for f in FORMS for c in ("noclip", "clip")]
MATRIX_IDS = ["%s-%s-%s" % m for m in MATRIX]


# ------------------------------------------------------------------------------------------------ 1. the accumulator
@gpu
@pytest.mark.parametrize("n", SIZES)
def test_accumulator_holds_the_left_to_right_fp32_sum(ops, n):
    """K = 3 on an accumulator full of NaN: after calls 1, 2, 3 it is g0, g0 + g1, (g0 + g1) + g2 as torch adds them in fp32
    -- the first call overwrote the NaN, the second and third did not overwrite the sum.  The record reads {next index,
    calls, cycles, held}; a second cycle starts over from its own first gradient."""
    rig = Rig(ops, "sgd", "plain", "noclip", n)
    g = [_clean(n, 40 + j) for j in range(4)]
    want = [g[0], g[0] + g[1], (g[0] + g[1]) + g[2]]
    records = [[1, 1, 0, 1], [2, 2, 0, 1], [0, 3, 1, 0]]
    assert bool(torch.isnan(rig.accum).all())
    for j in range(3):
        rig.micro(g[j])
        torch.cuda.synchronize()
        assert torch.equal(rig.accum, want[j]), (j, int((rig.accum != want[j]).sum()))
        assert rig.acc.tolist() == records[j]
    assert not torch.equal(want[2], g[0] + (g[1] + g[2])) or n == N_TAIL          # (the order is visible in the bits)
    rig.micro(g[3])
    torch.cuda.synchronize()
    assert torch.equal(rig.accum, g[3]) and rig.acc.tolist() == [1, 4, 1, 1]


# ------------------------------------------------------------------------------------------------ 2. hold calls
@gpu
@pytest.mark.parametrize("guarded", [False, True], ids=["unguarded", "guarded"])
@pytest.mark.parametrize("rule,form,clip", MATRIX, ids=MATRIX_IDS)
def test_hold_calls_change_nothing_but_accumulator_and_record(ops, rule, form, clip, guarded):
    """One clean cycle in, then the two hold calls of a K = 3 cycle, the second on a gradient with a NaN in it: parameters,
    state, EMA, ``step_dev``, ``st`` (all four floats), ``sched_out``, ``groups_out`` and the guard record keep their bits."""
    rig = _one_cycle_in(ops, rule, form, clip, N_MID, guarded)
    before = rig.snapshot()
    bad = _clean(N_MID, 21).clone()
    bad[1026] = NAN
    for j, grad in enumerate((_clean(N_MID, 20), bad)):
        rig.micro(grad, 0.5)
        torch.cuda.synchronize()
        _assert_equal(rig.buffers(), before, "hold call %d" % j)
        assert rig.acc.tolist() == [j + 1, 4 + j, 1, 1]
    assert torch.equal(rig.accum[:1026], (_clean(N_MID, 20) + bad)[:1026]) and bool(torch.isnan(rig.accum[1026]))


# ------------------------------------------------------------------------------------------------ 3. the last call
def _last_call_case(ops, rule, form, clip, guarded):
    rig = _one_cycle_in(ops, rule, form, clip, N_MID, guarded)
    g = [_clean(N_MID, 30 + j) for j in range(3)]
    rig.micro(g[0], 0.5)
    rig.micro(g[1], 0.5)
    twin = rig.fork()
    summed = (g[0] + g[1]) + g[2]
    rig.micro(g[2], 0.5)
    twin.today(summed, _scale_eff(0.5, 3))
    torch.cuda.synchronize()
    assert torch.equal(rig.accum, summed)
    _assert_equal(rig.buffers(), twin.buffers(), "last call")
    assert int(rig.step_dev) == 2 and rig.acc.tolist() == [0, 6, 2, 0] and bool(torch.isfinite(rig.p).all())
    return rig, twin


@gpu
@pytest.mark.parametrize("guarded", [False, True], ids=["unguarded", "guarded"])
@pytest.mark.parametrize("rule,form,clip", MATRIX, ids=MATRIX_IDS)
def test_last_call_is_todays_step_on_the_accumulator(ops, rule, form, clip, guarded):
    """The third call of a K = 3 cycle against a twin forked before it and stepped through today's entry point of the same
    form (guarded: the guarded one) with ``grad = (g0 + g1) + g2`` and ``grad_scale = float32(float64(0.5) / 3)``: every
    buffer is bit-equal, ``st[2]`` (norm) and ``st[3]`` (coefficient) included; where clipping is on, it binds."""
    rig, twin = _last_call_case(ops, rule, form, clip, guarded)
    if clip == "clip":
        assert 0.0 < float(rig.st[3]) < 1.0 and float(rig.st[2]) > 1.0
    else:
        assert float(rig.st[3]) == 1.0
    if guarded:
        assert rig.guard.tolist() == [2, 0, 0, 0]


@gpu
@pytest.mark.parametrize("guarded", [False, True], ids=["unguarded", "guarded"])
@pytest.mark.parametrize("rule,form", [("adamw", "groups_ema"), ("adam", "plain"), ("sgdm", "sched_ema"), ("sgd", "groups")])
def test_last_call_with_a_clip_that_does_not_bind(ops, rule, form, guarded):
    """the same with max_norm 1e4: the norm is computed and written, the coefficient is exactly 1"""
    rig, twin = _last_call_case(ops, rule, form, "loose", guarded)
    assert float(rig.st[3]) == 1.0 and 1.0 < float(rig.st[2]) < 1e4


@gpu
@pytest.mark.parametrize("rule,form", [(r, f) for r in RULES for f in FORMS], ids=["%s-%s" % (r, f) for r in RULES for f in FORMS])
def test_one_micro_step_per_cycle_gives_todays_bits(ops, rule, form):
    """K = 1 through the new entry points, three steps, clipped and guarded or neither: every call is a last call and equals
    today's step of the form on the same gradient under the same ``grad_scale``."""
    for clip, guarded in (("clip", True), ("noclip", False)):
        rig = Rig(ops, rule, form, clip, N_MID, guarded, k=1)
        twin = rig.fork()
        for j in range(3):
            rig.micro(_clean(N_MID, 50 + j), 0.5)
            twin.today(_clean(N_MID, 50 + j), 0.5)
        torch.cuda.synchronize()
        _assert_equal(rig.buffers(), twin.buffers(), "K = 1, %s" % clip)
        assert int(rig.step_dev) == 3 and rig.acc.tolist() == [0, 3, 3, 0] and torch.equal(rig.accum, _clean(N_MID, 52))


# ------------------------------------------------------------------------------------------------ 5. the fused sum of squares
@gpu
@pytest.mark.parametrize("n", SIZES)
def test_fused_sum_of_squares_equals_grad_norm_dev_on_the_accumulator(ops, n):
    """After a K = 3 cycle's last call the partials, the fp32 norm and the coefficient are the bits ``adyolo_grad_norm_dev``
    gives on the finished accumulator under the same scale: same grid, same per-lane walk, same reduction order."""
    rig = Rig(ops, "adam", "plain", "clip", n)
    rig.partials.fill_(-1.0)
    for j in range(3):
        rig.micro(_clean(n, 60 + j), 0.5)
        if j < 2:
            torch.cuda.synchronize()
            assert bool((rig.partials == -1.0).all())                             # hold calls sum nothing
    parts = ops.grad_sumsq_parts(n)
    want_p, want_st = torch.full_like(rig.partials, -1.0), torch.zeros_like(rig.st)
    ops.grad_norm_dev(rig.accum, want_p, want_st, 1.0, _scale_eff(0.5, 3))
    torch.cuda.synchronize()
    assert torch.equal(rig.partials[:parts], want_p[:parts]) and bool((rig.partials[parts:] == -1.0).all())
    assert torch.equal(rig.st[2:4], want_st[2:4]) and float(rig.st[2]) > 0.0
    ref = float(((rig.accum.double() * _scale_eff(0.5, 3)) ** 2).sum().sqrt())
    assert abs(float(rig.st[2]) - ref) <= 1e-5 * ref                              # (and it is the norm)


# ------------------------------------------------------------------------------------------------ 6. trajectories
class _Net(torch.nn.Sequential):
    def __init__(self, seed=7):
        torch.manual_seed(seed)
        super().__init__(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5))       # 703 + 19 + 95 + 5 = 822 (padded to 824)


CASE_A = {"optim": "Adam", "lr": 1e-3, "weight_decay": 0.01, "clip_grad_norm": 1.0, "ema_decay": 0.9, "ema_warmup": True,
          "lr_schedule": {"name": "cosine", "T_max": 10, "warmup_steps": 3},
          "param_groups": [{"name": "no_decay", "ndim_max": 1, "weight_decay": 0.0}]}
CASE_B = {"optim": "SGD", "lr": 0.05, "momentum": 0.9, "dampening": 0.5}


def _optimizer(train_config, seed=7, **more):
    from adyolo_amd.dist import FlatParameters
    from adyolo_amd.train import get_optimizers
    net = _Net(seed).to(DEV)
    flat = FlatParameters(net)
    return net, get_optimizers({"train_config": dict(train_config, **more)}, flat)


def _grad_lists(net, count, seed):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(p.shape, generator=g).to(DEV) for p in net.parameters()] for _ in range(count)]


def _drive(net, opt, grads, grad_scale=1.0):
    for grs in grads:
        opt.zero_grad()
        for p, gr in zip(net.parameters(), grs):
            p.grad.copy_(gr)
        opt.step(grad_scale)


def _opt_buffers(opt):
    own = {"momentum_buffer": opt.momentum_buffer} if opt.kind == "sgd" else {"exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}
    own.update(p=opt.flat.flat, step_dev=opt.step_dev, st=opt.st_dev)
    for k in ("ema", "current_lr", "current_lrs"):
        if getattr(opt, k) is not None:
            own[k] = getattr(opt, k)
    return own


@gpu
@pytest.mark.parametrize("case", ["adam_groups_cosine_ema", "sgd_momentum"])
def test_three_cycles_of_two_equal_three_steps_on_the_summed_gradients(ops, case):
    """Through ``get_optimizers``: six micro-steps at ``accum_steps: 2`` end where three steps of the optimizer built without
    the key end on the pre-summed gradients under ``grad_scale`` 1/2 -- parameters, state, EMA, rates, counter, ``st``.  The
    device counter is 3 and ``current_lr`` the third step's rate: the schedule's clock saw cycles."""
    tc = CASE_A if case.startswith("adam") else CASE_B
    net_a, acc = _optimizer(tc, accum_steps=2)
    net_p, plain = _optimizer(tc)
    assert acc.accum_dev is not None and plain.accum_dev is None
    micro = _grad_lists(net_a, 6, 51)
    summed = [[a + b for a, b in zip(micro[2 * c], micro[2 * c + 1])] for c in range(3)]
    _drive(net_a, acc, micro)
    _drive(net_p, plain, summed, grad_scale=0.5)
    torch.cuda.synchronize()
    _assert_equal(_opt_buffers(acc), _opt_buffers(plain), case)
    assert int(acc.step_dev) == 3 and acc.step_count == 3 and acc.micro_index == 0 and acc.accum_dev.tolist() == [0, 6, 3, 0]
    if case.startswith("adam"):
        assert float(acc.current_lr) == acc.lr_at(3) != acc.lr_at(6)
        assert acc.ema_updates == 3 and acc.sched_step == 3 and not torch.equal(acc.ema, acc.flat.flat)
        assert float(acc.grad_norm) > 0.0 and float(acc.st_dev[3]) < 1.0
    assert bool(torch.isfinite(acc.flat.flat).all())


# ------------------------------------------------------------------------------------------------ 7. with the guard
GUARD_CONFIGS = {"adam_groups_ema_clip": ("adam", "groups_ema", "clip"), "sgdm_plain_noclip": ("sgdm", "plain", "noclip")}
POISONS = [(m, v) for m in (0, 1, 2) for v in (NAN, INF, -INF)]


def _poisoned_cycle(n, micro, value, where):
    grads = [_clean(n, 70 + j) for j in range(3)]
    grads[micro] = grads[micro].clone()
    grads[micro][where] = value
    return grads


@gpu
@pytest.mark.parametrize("config", sorted(GUARD_CONFIGS))
@pytest.mark.parametrize("micro,value", POISONS, ids=["micro%d-%s" % p for p in POISONS])
def test_one_poisoned_micro_gradient_skips_the_cycle(ops, config, micro, value):
    """K = 3, one NaN / +inf / -inf element (vector body or tail, going round) in the gradient of micro-step 0, 1 or 2: the
    cycle is one skipped attempt -- nothing but the accumulator, the two records and ``st[2]`` moves -- and the clean cycle
    after it gives the bits of a run in which the poisoned cycle was never drawn."""
    rig = _one_cycle_in(ops, *GUARD_CONFIGS[config], N_MID, True)
    never = rig.fork()
    before = rig.snapshot()
    where = (0, 1023, 1026)[(micro + POISONS.index((micro, value))) % 3]
    for grad in _poisoned_cycle(N_MID, micro, value, where):
        rig.micro(grad, 0.5)
    torch.cuda.synchronize()
    assert rig.guard.tolist() == [2, 1, 1, 1] and rig.acc.tolist() == [0, 6, 2, 0]
    assert not bool(torch.isfinite(rig.st[2])) and not bool(torch.isfinite(rig.accum).all())
    for k, v in rig.buffers().items():
        if k == "st":
            assert _same_bits(v[[0, 1, 3]], before[k][[0, 1, 3]]), (k, v.tolist(), before[k].tolist())
        elif k != "guard":
            assert torch.equal(v, before[k]), (k, int((v != before[k]).sum()))
    for j in range(3):
        rig.micro(_clean(N_MID, 80 + j), 0.5)
        never.micro(_clean(N_MID, 80 + j), 0.5)
    torch.cuda.synchronize()
    got, want = rig.buffers(), never.buffers()
    assert got.pop("guard").tolist() == [3, 1, 0, 0] and want.pop("guard").tolist() == [2, 0, 0, 0]
    _assert_equal(got, want, "the clean cycle after the skipped one")
    assert torch.equal(rig.accum, never.accum) and int(rig.step_dev) == 2 and bool(torch.isfinite(rig.p).all())


@gpu
@pytest.mark.parametrize("config", sorted(GUARD_CONFIGS))
@pytest.mark.parametrize("calls", [1, 2])
def test_a_poisoned_partial_cycle_dropped_by_a_reset_leaks_nothing(ops, config, calls):
    """One or two calls of a cycle, the first on a NaN gradient, then index 0 written to the record (what
    ``reset_accumulation`` does): the next three calls are a whole clean cycle, applied, with the bits of a run that never
    saw the partial one -- the NaN in the accumulator was overwritten, not read."""
    rig = _one_cycle_in(ops, *GUARD_CONFIGS[config], N_MID, True)
    never = rig.fork()
    for grad in _poisoned_cycle(N_MID, 0, NAN, 5)[:calls]:
        rig.micro(grad, 0.5)
    rig.acc[0:1].zero_()
    for j in range(3):
        rig.micro(_clean(N_MID, 80 + j), 0.5)
        never.micro(_clean(N_MID, 80 + j), 0.5)
    torch.cuda.synchronize()
    _assert_equal(rig.buffers(), never.buffers(), "after the reset")
    assert rig.guard.tolist() == [2, 0, 0, 0] and rig.acc.tolist() == [0, 6 + calls, 2, 0]
    assert torch.equal(rig.accum, never.accum) and bool(torch.isfinite(rig.accum).all())


@gpu
def test_reset_accumulation_of_the_optimizer_on_the_device(ops):
    """the same through the class: a NaN micro-step, ``reset_accumulation()``, a clean cycle -- applied, nothing skipped"""
    net, opt = _optimizer(CASE_A, accum_steps=2, skip_nonfinite=True)
    net_n, never = _optimizer(CASE_A, accum_steps=2, skip_nonfinite=True)
    clean = _grad_lists(net, 2, 52)
    bad = [t.clone() for t in clean[0]]
    bad[1].view(-1)[-1] = NAN
    _drive(net, opt, [bad])
    assert opt.micro_index == 1
    opt.reset_accumulation()
    assert opt.micro_index == 0
    _drive(net, opt, clean)
    _drive(net_n, never, clean)
    torch.cuda.synchronize()
    _assert_equal(_opt_buffers(opt), _opt_buffers(never), "class-level reset")
    assert opt.reconcile() == {"attempts": 1, "skipped": 0, "last_skipped": False, "run": 0} and opt.step_count == 1
    assert opt.accum_dev.tolist() == [0, 3, 1, 0]


# ------------------------------------------------------------------------------------------------ 8. replay
@gpu
def test_one_recording_made_at_micro_index_one_serves_every_micro_step(ops):
    """The accumulating step (AdamW, groups + EMA, clipping, guarded, K = 3) recorded in ONE hipGraph at micro index 1 -- after
    one eager call -- on a static gradient buffer, and replayed for the other eight calls of three cycles with the buffer
    rewritten between replays (the second cycle poisoned): after every call all buffers equal the eager run's."""
    n = N_MID
    Rig(ops, "adamw", "groups_ema", "clip", n, True).micro(_clean(n, 90))          # (first call: nothing left to load under capture)
    eager = Rig(ops, "adamw", "groups_ema", "clip", n, True)
    replayed = eager.fork()
    grads = [_clean(n, 90 + j) for j in range(9)]
    grads[4] = grads[4].clone()
    grads[4][n - 1] = INF
    static = torch.zeros(n, device=DEV)
    eager.micro(grads[0])
    replayed.micro(grads[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed.micro(static)
    torch.cuda.synchronize()
    assert replayed.acc.tolist() == [1, 1, 0, 1] and int(replayed.step_dev) == 0   # recording ran nothing
    for j in range(1, 9):
        static.copy_(grads[j])
        graph.replay()
        eager.micro(grads[j])
        torch.cuda.synchronize()
        _assert_equal(replayed.buffers(), eager.buffers(), "call %d" % j)
        assert replayed.acc.tolist() == eager.acc.tolist() == [(j + 1) % 3, j + 1, (j + 1) // 3, int((j + 1) % 3 != 0)]
        assert _same_bits(replayed.accum, eager.accum)
    assert replayed.guard.tolist() == eager.guard.tolist() == [3, 1, 0, 0]
    assert int(replayed.step_dev) == 2 and bool(torch.isfinite(replayed.p).all())


# ------------------------------------------------------------------------------------------------ 9. against torch
def _max_err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _torch_cycle(ref, opt, micro):
    """what a torch loop does: ``(loss / 4).backward()`` four times -- p.grad accumulates g / 4 left to right -- then a step"""
    ref.grad = None
    for gr in micro:
        ref.grad = gr / 4.0 if ref.grad is None else ref.grad + gr / 4.0
    opt.step()


@gpu
@pytest.mark.parametrize("n", [3, 4099, 10004])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_accumulating_adamw_matches_torch(ops, n, wd):
    """K = 4 against torch.optim.AdamW on ``p.grad`` accumulated from ``loss / 4`` over four micro-gradients, seven cycles; the
    bounds are test_adamw_device_step_matches_torch's.  (4 is a power of two: torch's pre-scaled and this build's post-scaled
    sums are the same fp32 values.)"""
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=g)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=wd)
    pg = p0.to(DEV)
    m, v, accum = torch.zeros_like(pg), torch.zeros_like(pg), torch.full_like(pg, NAN)
    step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device=DEV)
    acc = torch.zeros(ops.OPTIM_ACCUM_WORDS, dtype=torch.int64, device=DEV)
    for _ in range(7):
        micro = [torch.randn(n, generator=g) for _ in range(4)]
        _torch_cycle(ref, opt, micro)
        for gr in micro:
            ops.adam_step_accum_dev(pg, gr.to(DEV), m, v, step_dev, st, accum, acc, 4, lr=1e-3, weight_decay=wd, decoupled=True)
    torch.cuda.synchronize()
    assert int(step_dev) == 7 and acc.tolist() == [0, 28, 7, 0] and float(st[3]) == 1.0
    err = _max_err(pg, ref)
    print("accumulating adamw n=%d wd=%g: max |p - torch| = %.3e" % (n, wd, err))
    assert err <= 1e-6, err
    sd = opt.state_dict()["state"][0]
    assert _max_err(m, sd["exp_avg"]) <= 1e-6 and _max_err(v, sd["exp_avg_sq"]) <= 1e-6


SGD_FORMS = {"plain": {}, "wd": {"weight_decay": 0.01}, "momentum": {"momentum": 0.9},
             "nesterov": {"momentum": 0.9, "nesterov": True}, "dampening": {"momentum": 0.9, "dampening": 0.1}}


@gpu
@pytest.mark.parametrize("n", [3, 4099, 10004])
@pytest.mark.parametrize("form", sorted(SGD_FORMS))
def test_accumulating_sgd_matches_torch(ops, n, form):
    """K = 4 against torch.optim.SGD in the five forms of test_sgd_device_step_matches_torch, with its bounds"""
    kw = SGD_FORMS[form]
    g = torch.Generator().manual_seed(4)
    p0 = torch.randn(n, generator=g)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([ref], lr=0.01, **kw)
    pg = p0.to(DEV)
    buf = torch.full_like(pg, 123.0) if kw.get("momentum") else None      # garbage: the first step must overwrite, not read, it
    accum = torch.full_like(pg, NAN)
    step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device=DEV)
    acc = torch.zeros(ops.OPTIM_ACCUM_WORDS, dtype=torch.int64, device=DEV)
    for _ in range(7):
        micro = [torch.randn(n, generator=g) for _ in range(4)]
        _torch_cycle(ref, opt, micro)
        for gr in micro:
            ops.sgd_step_accum_dev(pg, gr.to(DEV), buf, step_dev, st, accum, acc, 4, lr=0.01, **kw)
    torch.cuda.synchronize()
    assert int(step_dev) == 7 and acc.tolist() == [0, 28, 7, 0]
    err = _max_err(pg, ref)
    print("accumulating sgd %s n=%d: max |p - torch| = %.3e" % (form, n, err))
    assert err <= 1e-6, err
    if buf is not None:
        berr = _max_err(buf, opt.state_dict()["state"][0]["momentum_buffer"])
        assert berr <= 1e-5, berr


# ------------------------------------------------------------------------------------------------ 10. the trainer
def _params(nb_classes=12, loss="adyolo", **train_config):
    tc = {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
          "conf_thresh": 0.5, "clss_thresh": 0.5, "unify_thresh": 15.0, "nms": "conn-merge",
          "loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
          "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0}
    tc.update(train_config)
    return {"args": {"device": DEV, "encoder": "se-resnet34", "loss": loss},
            "data_config": {"nb_classes": nb_classes}, "train_config": tc}


def _trainer(graph, t=80, **train_config):
    from adyolo_amd.wrapper import WrapperModel, WrapperCriterion
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.train import TrainStep
    torch.manual_seed(100)
    prm = _params(**train_config)
    model = WrapperModel((1, 7, t, 64), (), prm).to(DEV)
    return TrainStep(model, WrapperCriterion(prm), FeatureExtractor(None, DEV), prm, graph=graph)


TRAINER_CONFIG = {"optim": "AdamW", "weight_decay": 0.01, "clip_grad_norm": 3.0, "skip_nonfinite": True, "accum_steps": 2}


def _running_mean(trainer):
    return next(b for name, b in trainer.model.named_buffers() if name.endswith("running_mean"))


@gpu
def test_train_step_accumulates_eager_and_replayed_alike(ops, tmp_path):
    """``TrainStep`` with ``accum_steps: 2`` (AdamW, clipping, guarded), 2 clips x 2 s, eager against hipGraph over six calls:
    losses and parameters bit-identical; parameters unchanged after calls 1, 3 and 5 and changed after 2, 4 and 6; BatchNorm
    running statistics move on EVERY call; three steps counted, one recording.  Then a checkpoint written at the cycle
    boundary and loaded into the graph trainer after it ran three calls ahead (into the middle of a cycle): the next four
    calls equal the eager trainer's bit for bit."""
    from adyolo_amd import checkpoint
    from adyolo_amd.datasets import synthetic_audio, synthetic_targets
    audios = [synthetic_audio(2, 24000 * 2, seed=70 + i).to(DEV) for i in range(3)]
    targets = [synthetic_targets(2, 20, 12, seed=80 + i) for i in range(13)]
    te, tg = _trainer(False, **TRAINER_CONFIG), _trainer(True, **TRAINER_CONFIG)
    assert tg.graphs is not None and te.graphs is None and te.optimizer.accum_steps == 2
    for i in range(6):
        p_before, bn_before = te.flat.flat.clone(), _running_mean(te).clone()
        a, b = te.step(audios[i % 3], targets[i]), tg.step(audios[i % 3], targets[i])
        assert torch.equal(a, b), "loss of call %d: eager %r graph %r" % (i, float(a), float(b))
        assert torch.equal(te.flat.flat, p_before) == (i % 2 == 0), "parameters after call %d" % (i + 1)
        assert not torch.equal(_running_mean(te), bn_before), "running statistics after call %d" % (i + 1)
        assert torch.equal(te.flat.flat, tg.flat.flat) and torch.equal(_running_mean(te), _running_mean(tg))
        assert te.optimizer.micro_index == tg.optimizer.micro_index == (i + 1) % 2
    assert tg.graphs.captures == 1 and tg.graphs.replays == 5 and tg.graphs.eager_steps == 1
    for opt in (te.optimizer, tg.optimizer):
        assert opt.step_count == 3 and int(opt.step_dev) == 3 and opt.accum_dev.tolist() == [0, 6, 3, 0]
        assert opt.reconcile() == {"attempts": 3, "skipped": 0, "last_skipped": False, "run": 0}
    assert torch.equal(te.optimizer.exp_avg, tg.optimizer.exp_avg) and torch.equal(te.optimizer.accum, tg.optimizer.accum)
    assert bool(torch.isfinite(te.flat.flat).all())
    path = str(tmp_path / "model_ckpt.h5")
    checkpoint.save_checkpoint(path, te.model, te.optimizer, 1, 0.5, {}, [], DEV)
    for i in range(6, 9):                                                         # the graph trainer runs ahead, into a cycle ...
        tg.step(audios[i % 3], targets[i])
    assert tg.optimizer.micro_index == 1
    with pytest.raises(ValueError, match="accumulation cycle"):
        tg.optimizer.state_dict()
    checkpoint.load_checkpoint(path, tg.model, tg.optimizer, device=DEV)          # ... and is rolled back to the boundary
    assert tg.optimizer.micro_index == 0 and tg.optimizer.step_count == 3
    for i in range(9, 13):
        a, b = te.step(audios[i % 3], targets[i]), tg.step(audios[i % 3], targets[i])
        assert torch.equal(a, b), i
    torch.cuda.synchronize()
    assert tg.graphs.captures == 1 and te.optimizer.step_count == tg.optimizer.step_count == 5
    assert torch.equal(te.flat.flat, tg.flat.flat) and torch.equal(te.optimizer.exp_avg_sq, tg.optimizer.exp_avg_sq)


# ------------------------------------------------------------------------------------------------ 11. refusals
def _raw_args(ops, rule, n=8, accum="ok", record="ok", k=3):
    """the C argument list of adyolo_{adam,sgd}_step_accum_dev (plain form, unguarded, no clipping); tensors kept alive"""
    f32 = lambda: torch.zeros(n + 4, device=DEV)                                  # noqa: E731
    keep = {"p": f32(), "g": f32(), "m": f32(), "v": f32(), "accum": f32(),
            "step": torch.zeros(1, dtype=torch.int64, device=DEV), "st": torch.zeros(4, device=DEV),
            "rec": torch.zeros(2 * ops.OPTIM_ACCUM_WORDS + 2, dtype=torch.int32, device=DEV)}
    P, null = ops._p, ops._p(None)
    accum_p = {"ok": P(keep["accum"]), "null": null, "misaligned": P(keep["accum"][1:])}[accum]
    rec_p = {"ok": P(keep["rec"]), "null": null, "misaligned": P(keep["rec"][1:])}[record]
    form = [null, null, null, null, null, 0, null, null, accum_p, rec_p, k, ops._stream()]
    if rule == "adam":
        head = [P(keep["p"]), P(keep["g"]), P(keep["m"]), P(keep["v"]), n, LR, 0.9, 0.999, 1e-8, 0.0, 0]
    else:
        head = [P(keep["p"]), P(keep["g"]), null, n, LR, 0.0, 0.0, 0.0, 0]
    return keep, head + [P(keep["step"]), P(keep["st"]), null, 0.0, 1.0] + form


REFUSALS = {"null_accumulator": dict(accum="null"), "misaligned_accumulator": dict(accum="misaligned"),
            "null_record": dict(record="null"), "misaligned_record": dict(record="misaligned"),
            "accum_steps_0": dict(k=0), "accum_steps_negative": dict(k=-1)}


@gpu
@pytest.mark.parametrize("rule", ["adam", "sgd"])
@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_entry_points_refuse_bad_accumulation_arguments(ops, rule, case):
    """at the C ABI: the call fails with an error before any launch, and touches nothing"""
    from adyolo_amd import _lib
    name = "adyolo_%s_step_accum_dev" % rule
    keep, args = _raw_args(ops, rule, **REFUSALS[case])
    with pytest.raises(_lib.AdyoloHipError, match="accum"):
        _lib.call(name, *args)
    torch.cuda.synchronize()
    assert all(not bool(t.any()) for t in keep.values())
    keep, args = _raw_args(ops, rule)                                             # and the list itself is a good one
    _lib.call(name, *args)
    torch.cuda.synchronize()
    assert keep["rec"].view(torch.int64)[:4].tolist() == [1, 1, 0, 1] and int(keep["step"]) == 0


@gpu
def test_wrappers_and_optimizer_refuse_too(ops):
    from adyolo_amd import _lib
    rig = Rig(ops, "sgd", "plain", "noclip", N_MID)
    g = _clean(N_MID, 1)
    for bad in (dict(accum=None), dict(accum=torch.zeros(N_MID + 1, device=DEV)[1:]), dict(accum=torch.zeros(8, device=DEV)),
                dict(accum_dev=None), dict(accum_dev=torch.zeros(4, dtype=torch.int32, device=DEV)), dict(accum_steps=0),
                dict(accum_steps=2.5)):
        kw = dict(accum=rig.accum, accum_dev=rig.acc, accum_steps=3)
        kw.update(bad)
        with pytest.raises(_lib.AdyoloHipError):
            ops.sgd_step_accum_dev(rig.p, g, None, rig.step_dev, rig.st, lr=LR, **kw)
    with pytest.raises(_lib.AdyoloHipError, match="partials"):                   # a guard needs the partials
        ops.sgd_step_accum_dev(rig.p, g, None, rig.step_dev, rig.st, rig.accum, rig.acc, 3, guard=rig.guard, lr=LR)
    torch.cuda.synchronize()
    assert rig.acc.tolist() == [0, 0, 0, 0] and bool(torch.isnan(rig.accum).all())
    net, opt = _optimizer(CASE_B, accum_steps=2)
    _drive(net, opt, _grad_lists(net, 1, 3))
    with pytest.raises(ValueError, match="middle of an accumulation cycle"):
        opt.state_dict()
    _drive(net, opt, _grad_lists(net, 1, 4))
    assert opt.state_dict()["param_groups"][0]["momentum"] == 0.9
