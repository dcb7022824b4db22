"""GPU: the non-finite guard of the fused optimizers (csrc/optim.hip, ``adyolo_*_step_guard_dev``;
``train_config['skip_nonfinite']``).  A step whose gradient is not finite does nothing at all, a step whose gradient is finite
is the unguarded step, and a run with skipped attempts is the run without them.  Every comparison is bitwise
(``torch.equal`` on the raw buffers).

One reading of the specification is fixed here.  A guarded step always sums the squares and always writes ``st[2]`` (the
norm; ``grad_norm`` exists with or without clipping), while the unguarded UNCLIPPED step never touches ``st[2]``.  So where
clipping is off, "the bits of the unguarded entry point in every buffer, ``st`` included" is asserted for ``st[0]``, ``st[1]``
and ``st[3]``, and ``st[2]`` against the norm ``ops.grad_norm_dev`` gives for the same gradient; with clipping on all four
floats are compared.

The two poison cases without special values use min(4, n) elements of 3e38: at n = 3 three elements still give a float64
sum of 2.7e77, whose root 5.2e38 is beyond fp32's 3.4e38."""
import copy

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"

N_TAIL, N_MID, N_BIG = 3, 1027, 1048576 + 1024 + 2       # tail only | one workgroup's vectors + 3 | past the sum-of-squares grid cap
RULES = ("adam", "adamw", "sgd", "sgdm")
FORMS = ("plain", "sched", "sched_ema", "groups", "groups_ema")
LR, MAX_NORM = 0.01, 1.0
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _clean(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(DEV)


class Rig:
    """The buffers of one optimizer at the level of ``ops``: rule x form x clipping over n elements, stepped through the
    guarded entry point or through the unguarded one of the same form."""

    def __init__(self, ops, rule, form, clip, n, seed=0):
        from adyolo_amd import lr_schedule
        self.ops, self.rule, self.form, self.clip, self.n = ops, rule, form, clip, n
        self.adam = rule in ("adam", "adamw")
        self.wd = 0.0 if rule == "sgd" else 0.01
        self.p = _clean(n, 1000 + seed)
        self.state = [torch.zeros_like(self.p) for _ in range(2 if self.adam else 1 if rule == "sgdm" else 0)]
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device=DEV)
        self.partials = torch.zeros(ops.GRAD_SUMSQ_MAX_PARTS, dtype=torch.float64, device=DEV)
        self.guard = torch.zeros(ops.OPTIM_GUARD_WORDS, dtype=torch.int64, device=DEV)
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
        out = {"p": self.p, "step_dev": self.step_dev, "st01": self.st[0:2], "st3": self.st[3:4]}
        out.update({"state%d" % k: s for k, s in enumerate(self.state)})
        for k in ("ema", "sched_out", "groups_out"):
            if getattr(self, k) is not None:
                out[k] = getattr(self, k)
        return out

    def snapshot(self):
        return {k: v.clone() for k, v in self.buffers().items()}

    def step(self, grad, guarded, grad_scale=1.0):
        ops, mn = self.ops, MAX_NORM if self.clip else None
        parts = self.partials if (self.clip or guarded) else None
        sched = (self.sched_dev, self.sched_out)
        groups = (self.groups_dev, self.groups_out, self.gmap)
        if self.adam:
            dec = self.rule == "adamw"
            m, v = self.state
            if guarded:
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
        if guarded:
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


def _two_steps_in(ops, rule, form, clip, n):
    rig = Rig(ops, rule, form, clip, n)
    for k in range(2):
        rig.step(_clean(n, 10 + k), True)
    torch.cuda.synchronize()
    assert rig.guard.tolist() == [2, 0, 0, 0] and int(rig.step_dev) == 2 and bool(torch.isfinite(rig.p).all())
    return rig


def _assert_skipped(rig, bad, grad_scale=1.0):
    """one guarded attempt on ``bad`` from the rig's state: nothing but st[2] and the record moves"""
    before, rec = rig.snapshot(), rig.guard.tolist()
    rig.step(bad, True, grad_scale)
    torch.cuda.synchronize()
    for k, v in rig.buffers().items():
        assert torch.equal(v, before[k]), (k, int((v != before[k]).sum()))
    assert rig.guard.tolist() == [rec[0] + 1, rec[1] + 1, 1, rec[3] + 1], (rig.guard.tolist(), rec)
    assert not bool(torch.isfinite(rig.st[2])), float(rig.st[2])


MATRIX = [(r, f, c) for r in RULES for f in FORMS for c in (False, True)]
POISONS = [(v, i) for v in (NAN, INF, -INF) for i in (0, 1023, 1026)]           # n = 1027: first, last vector element, last tail element


# ------------------------------------------------------------------------------------------------ 1. a skipped step
@gpu
@pytest.mark.parametrize("rule,form,clip", MATRIX, ids=["%s-%s-%s" % (r, f, "clip" if c else "noclip") for r, f, c in MATRIX])
def test_skipped_step_leaves_every_byte_unchanged(ops, rule, form, clip):
    """Every rule x form x clipping state, two clean guarded steps in, then a guarded step on a gradient with one poisoned
    element (the 9 value x position pairs of n = 1027 go round the 40 cases): parameters, moments / momentum buffer, EMA,
    ``step_dev``, ``st[0..1]``, ``st[3]``, ``sched_out`` and ``groups_out`` keep their bits, the record reads one more attempt,
    one more skip, flag 1, run + 1, and ``st[2]`` is not finite.  A second poisoned attempt extends the run to 2."""
    rig = _two_steps_in(ops, rule, form, clip, N_MID)
    value, index = POISONS[MATRIX.index((rule, form, clip)) % len(POISONS)]
    bad = _clean(N_MID, 20)
    bad[index] = value
    _assert_skipped(rig, bad)
    _assert_skipped(rig, bad)
    assert rig.guard.tolist() == [4, 2, 1, 2]


def _positions(n):
    n4 = (n >> 2) * 4
    pos = {"first": 0, "last_tail": n - 1}
    if n4:
        pos["last_vector"] = n4 - 1
    if n > 1048576:
        pos["past_grid_cap"] = 1048576 + 7
    return pos


POISON_CASES = [(n, where, v) for n in (N_TAIL, N_MID, N_BIG) for where in _positions(n) for v in (NAN, INF, -INF)]
CONFIGS = {"adam_groups_ema_clip": ("adam", "groups_ema", True), "sgdm_plain_noclip": ("sgdm", "plain", False)}


@gpu
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("n,where,value", POISON_CASES, ids=["%d-%s-%s" % c for c in POISON_CASES])
def test_one_poisoned_element_anywhere_skips_the_step(ops, config, n, where, value):
    """NaN, +inf or -inf at index 0, in the last vector element, in the last tail element and, at the large n, at an index the
    sum-of-squares grid reaches only on its second trip."""
    rig = _two_steps_in(ops, *CONFIGS[config], n)
    bad = _clean(n, 21)
    bad[_positions(n)[where]] = value
    _assert_skipped(rig, bad)


@gpu
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("n", [N_TAIL, N_MID, N_BIG])
@pytest.mark.parametrize("case", ["product_overflows", "norm_overflows"])
def test_overflow_without_special_values_skips_the_step(ops, config, n, case):
    """A finite gradient of 3e38 under grad_scale 2 (the product is inf), and min(4, n) elements of 3e38 under grad_scale 1
    (every element and the float64 sum are finite, the fp32 norm is not)."""
    rig = _two_steps_in(ops, *CONFIGS[config], n)
    bad = _clean(n, 22)
    if case == "product_overflows":
        bad[n - 1] = 3e38
        assert bool(torch.isfinite(bad).all())
        _assert_skipped(rig, bad, grad_scale=2.0)
    else:
        bad[:min(4, n)] = 3e38
        total = float(bad.double().pow(2).sum())
        assert bool(torch.isfinite(bad).all()) and total < 1.8e308 and total ** 0.5 > 3.5e38
        _assert_skipped(rig, bad)


# ------------------------------------------------------------------------------------------------ 2. a finite gradient
@gpu
@pytest.mark.parametrize("rule,form,clip", MATRIX, ids=["%s-%s-%s" % (r, f, "clip" if c else "noclip") for r, f, c in MATRIX])
def test_guard_changes_nothing_on_a_finite_gradient(ops, rule, form, clip):
    """From the same state two steps in: the unguarded entry point of the form on a finite gradient, and the guarded one on the
    same gradient AFTER a skipped attempt (so that flag and run have something to reset).  Every buffer, ``st`` and
    ``sched_out`` included, is bit-equal (``st[2]`` without clipping: see the module's docstring); the record reads flag 0,
    run 0."""
    rig = _two_steps_in(ops, rule, form, clip, N_MID)
    plain = rig.fork()
    grad = _clean(N_MID, 30)
    bad = grad.clone()
    bad[5] = NAN
    rig.step(bad, True, 0.5)
    rig.step(grad, True, 0.5)
    plain.step(grad, False, 0.5)
    norm = ops.grad_norm_dev(grad, torch.zeros_like(rig.partials), torch.zeros_like(rig.st), MAX_NORM, 0.5)[2:3].clone()
    torch.cuda.synchronize()
    want = plain.buffers()
    for k, v in rig.buffers().items():
        assert torch.equal(v, want[k]), (k, int((v != want[k]).sum()))
    assert int(rig.step_dev) == 3 and bool(torch.isfinite(rig.p).all())
    assert torch.equal(rig.st[2:3], norm) and float(norm) > 0.0
    if clip:
        assert torch.equal(rig.st, plain.st) and float(rig.st[3]) < 1.0          # the clip binds
    else:
        assert float(rig.st[3]) == 1.0
    assert rig.guard.tolist() == [4, 1, 0, 0]


# ------------------------------------------------------------------------------------------------ 3. trajectories
class _Net(torch.nn.Sequential):
    def __init__(self, seed=7):
        torch.manual_seed(seed)
        super().__init__(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5))       # 703 + 19 + 95 + 5 = 822 (padded to 824)


CASE_A = {"optim": "Adam", "lr": 1e-3, "weight_decay": 0.01, "clip_grad_norm": 1.0, "ema_decay": 0.9, "ema_warmup": True,
          "lr_schedule": {"name": "cosine", "T_max": 10, "warmup_steps": 3},
          "param_groups": [{"name": "no_decay", "ndim_max": 1, "weight_decay": 0.0}]}
CASE_B = {"optim": "SGD", "lr": 0.05, "momentum": 0.9, "dampening": 0.5}


def _optimizer(train_config, guarded, seed=7):
    from adyolo_amd.dist import FlatParameters
    from adyolo_amd.train import get_optimizers
    net = _Net(seed).to(DEV)
    flat = FlatParameters(net)
    tc = dict(train_config, skip_nonfinite=True) if guarded else dict(train_config)
    opt = get_optimizers({"train_config": tc}, flat)
    assert (opt.guard_dev is not None) == guarded
    return net, opt


def _grad_lists(net, count, seed):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(p.shape, generator=g).to(DEV) for p in net.parameters()] for _ in range(count)]


def _poisoned(grads, which, value):
    out = [t.clone() for t in grads]
    out[which].view(-1)[-1] = value
    return out


def _drive(net, opt, grads):
    for grs in grads:
        opt.zero_grad()
        for p, gr in zip(net.parameters(), grs):
            p.grad.copy_(gr)
        opt.step()


def _opt_buffers(opt):
    own = {"momentum_buffer": opt.momentum_buffer} if opt.kind == "sgd" else {"exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}
    own.update(p=opt.flat.flat, step_dev=opt.step_dev)
    for k in ("ema", "current_lr", "current_lrs"):
        if getattr(opt, k) is not None:
            own[k] = getattr(opt, k)
    return own


def _seven_attempts(net, clean):
    """attempt 1 (the very first) and attempt 4 poisoned, the five clean gradients in order around them"""
    return [_poisoned(clean[0], 0, NAN), clean[0], clean[1], _poisoned(clean[4], 3, -INF), clean[2], clean[3], clean[4]]


def _run_case(train_config):
    net_g, guarded = _optimizer(train_config, True)
    net_c, straight = _optimizer(train_config, False)
    clean = _grad_lists(net_g, 5, 51)
    _drive(net_g, guarded, _seven_attempts(net_g, clean))
    _drive(net_c, straight, clean)
    torch.cuda.synchronize()
    return guarded, straight


def _assert_same_trajectory(guarded, straight):
    want = _opt_buffers(straight)
    for k, v in _opt_buffers(guarded).items():
        assert torch.equal(v, want[k]), (k, int((v != want[k]).sum()))
    assert int(guarded.step_dev) == 5 and guarded.step_count == 7               # the mirror counts attempts until told
    assert guarded.reconcile() == {"attempts": 7, "skipped": 2, "last_skipped": False, "run": 0}
    assert guarded.step_count == 5 and guarded._dev_step_value == 5
    assert guarded.reconcile()["skipped"] == 2 and guarded.step_count == 5       # once only
    assert bool(torch.isfinite(guarded.flat.flat).all())


@gpu
def test_trajectory_with_skips_equals_trajectory_without_adam(ops):
    """Case A: Adam, two parameter groups, cosine with a 3-step warm-up, EMA with warm-up, clipping on.  Seven attempts with
    the first and the fourth poisoned end where the five clean steps of the UNGUARDED optimizer end: parameters, moments, EMA,
    ``current_lr(s)``, ``step_dev``.  (A bias correction or the EMA's first-copy flag that ticked on a skip would show.)"""
    guarded, straight = _run_case(CASE_A)
    assert guarded.groups is not None and len(guarded.groups) == 2 and guarded.ema is not None
    _assert_same_trajectory(guarded, straight)
    assert guarded.lr_at(guarded.step_count) == float(guarded.current_lr)
    assert guarded.ema_updates == 5 and guarded.sched_step == 5
    assert not torch.equal(guarded.ema, guarded.flat.flat)


@gpu
def test_trajectory_with_skips_equals_trajectory_without_sgd(ops):
    """Case B: SGD, momentum 0.9, dampening 0.5.  The skipped first attempt must leave the next one the first: it initialises
    the momentum buffer with the gradient, undampened."""
    guarded, straight = _run_case(CASE_B)
    _assert_same_trajectory(guarded, straight)
    assert guarded.ema_updates == 0 and guarded.lr_at(guarded.step_count) == float(torch.tensor(0.05, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ 4. replay
@gpu
def test_replayed_guarded_step_follows_the_buffers_content(ops):
    """One guarded step (AdamW, groups + EMA, clipping) recorded in a hipGraph on a static gradient buffer and replayed over
    a clean, a poisoned and a clean gradient copied into it: the buffers equal the eager guarded sequence's, the record reads
    3 attempts and 1 skip."""
    n = N_MID
    Rig(ops, "adamw", "groups_ema", True, n).step(_clean(n, 60), True)           # (first call: nothing left to load under capture)
    eager = Rig(ops, "adamw", "groups_ema", True, n)
    replayed = eager.fork()
    static = torch.zeros(n, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed.step(static, True)
    torch.cuda.synchronize()
    assert replayed.guard.tolist() == [0, 0, 0, 0] and int(replayed.step_dev) == 0          # recording ran nothing
    grads = [_clean(n, 61), _clean(n, 62), _clean(n, 63)]
    grads[1][n - 1] = INF
    for k, gr in enumerate(grads):
        static.copy_(gr)
        graph.replay()
        eager.step(gr, True)
        torch.cuda.synchronize()
        want = eager.buffers()
        for name, v in replayed.buffers().items():
            assert torch.equal(v, want[name]), (k, name)
        assert torch.equal(replayed.st[2:3], eager.st[2:3]) or k == 1
    assert replayed.guard.tolist() == eager.guard.tolist() == [3, 1, 0, 0]
    assert int(replayed.step_dev) == 2 and bool(torch.isfinite(replayed.p).all())


# ------------------------------------------------------------------------------------------------ 5. checkpoint
@gpu
def test_state_dict_counts_applied_steps_and_loads_into_torch(ops):
    """``state_dict()`` after case A (not reconciled by the caller): ``step`` == 5 for every parameter, and torch.optim.Adam
    with the same grouping takes it."""
    net, opt = _optimizer(CASE_A, True)
    _drive(net, opt, _seven_attempts(net, _grad_lists(net, 5, 51)))
    assert opt.step_count == 7
    sd = opt.state_dict()
    assert opt.step_count == 5
    params = list(net.parameters())
    assert len(sd["state"]) == len(params) and all(float(s["step"]) == 5.0 for s in sd["state"].values())
    twin = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    ref = torch.optim.Adam([{"params": [twin[i] for i in g["params"]]} for g in opt.groups])
    ref.load_state_dict(sd)
    assert all(float(s["step"]) == 5.0 for s in ref.state_dict()["state"].values())
    assert [g["weight_decay"] for g in ref.param_groups] == [0.01, 0.0]
    assert opt.guard_state_dict() == {"attempts": 7, "skipped": 2}
    assert opt.sched_state_dict()["step"] == 5 and opt.sched_state_dict()["ema_updates"] == 5


@gpu
def test_resume_between_skips_continues_bit_for_bit(ops, tmp_path):
    """Eight attempts, the 1st, 4th and 5th poisoned; a checkpoint file after the 4th (the last attempt before it a skip, the
    first after it too), loaded into a fresh model and optimizer: the end state equals the uninterrupted run's bit for bit,
    the counts carry over.  The same file loads into an unguarded optimizer."""
    from adyolo_amd import checkpoint as ck
    net_a, straight = _optimizer(CASE_A, True)
    clean = _grad_lists(net_a, 5, 71)
    attempts = [_poisoned(clean[0], 1, INF), clean[0], clean[1], _poisoned(clean[1], 2, NAN), _poisoned(clean[2], 0, -INF),
                clean[2], clean[3], clean[4]]
    _drive(net_a, straight, attempts)
    net_b, first = _optimizer(CASE_A, True)
    _drive(net_b, first, attempts[:4])
    path = str(tmp_path / "model_ckpt.h5")
    ck.save_checkpoint(path, net_b, first, 1, 0.5, {}, [], DEV)
    saved = torch.load(path, map_location="cpu", weights_only=False)
    assert saved["guard_state_dict"] == {"attempts": 4, "skipped": 2} and saved["sched_state_dict"]["step"] == 2
    assert all(float(s["step"]) == 2.0 for s in saved["optim_state_dict"]["state"].values())
    net_c, second = _optimizer(CASE_A, True, seed=99)
    ck.load_checkpoint(path, net_c, second, device=DEV, restore_rng=False)
    assert second.step_count == 2 and second.guard_dev.tolist() == [4, 2, 0, 0]
    _drive(net_c, second, attempts[4:])
    torch.cuda.synchronize()
    want = _opt_buffers(straight)
    for k, v in _opt_buffers(second).items():
        assert torch.equal(v, want[k]), (k, int((v != want[k]).sum()))
    assert second.reconcile() == straight.reconcile() == {"attempts": 8, "skipped": 3, "last_skipped": False, "run": 0}
    assert second.step_count == straight.step_count == 5 and second.sched_step == 5 and second.ema_updates == 5
    net_d, unguarded = _optimizer(CASE_A, False, seed=98)
    ck.load_checkpoint(path, net_d, unguarded, device=DEV, restore_rng=False)
    assert unguarded.step_count == 2 and unguarded.guard_dev is None and torch.equal(unguarded.exp_avg, first.exp_avg)
