"""GPU: the device-computed learning-rate schedules and the weight EMA of the fused optimizers (csrc/optim.hip, the ``*_sched``
entry points): bit identity of a constant schedule with the plain entry points, the rate against the host mirror, parameters
against torch.optim driven by ``lr_at``, the EMA against float64, ``set_lr`` / resume, hipGraph replay and ``ema_weights()``.

The float64 formulas compared against live in this file.  Bounds: the rate within one float32 ulp of the host mirror and
equal in at least 90 % of the steps (device and host ``pow`` / ``cos`` may differ in the last double bits); parameters within
the 1e-6 absolute of test_gpu_optimizers on N(0,1) data; the EMA within 2^-23 * max|p| / (1 - decay) of float64 (one rounding
per step, contracted by ``decay``); everything else bit for bit."""
import math

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _table(cfg, base, **kw):
    from adyolo_amd import lr_schedule
    return lr_schedule.table(lr_schedule.normalise(cfg), base, **kw)


def _dev_table(tb):
    return torch.tensor(tb, dtype=torch.float64).to("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. bit identity
IDENTITY_CASES = {"adam": {}, "adamw": {"weight_decay": 0.01}, "sgd": {},
                  "sgd_nesterov": {"momentum": 0.9, "nesterov": True}, "adam_clip": {}}
BIG = 2048 * 256 * 4 + 5              # one element group past OX_MAX_BLOCKS * OX_THREADS * 4: grid-stride loop and tail both run


def _identity_run(ops, case, n, p0, grads, sched):
    kw = dict(IDENTITY_CASES[case], grad_scale=0.25)
    pg = p0.to("cuda:0")
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device="cuda:0")
    if case == "adam_clip":
        kw.update(partials=torch.zeros(ops.GRAD_SUMSQ_MAX_PARTS, dtype=torch.float64, device="cuda:0"), max_norm=0.05)
    sgd = case.startswith("sgd")
    lr = 0.01 if sgd else 1e-3
    state = [torch.full_like(pg, 123.0)] if case == "sgd_nesterov" else [] if sgd else [torch.zeros_like(pg), torch.zeros_like(pg)]
    extra = ()
    if sched:
        extra = (_dev_table(_table({"name": "constant"}, lr)), torch.zeros(ops.SCHED_OUT_FLOATS, device="cuda:0"))
    coefs = []
    for gr in grads:
        gd = gr.to("cuda:0")
        if sgd:
            buf = state[0] if state else None
            if sched:
                ops.sgd_step_sched_dev(pg, gd, buf, step_dev, st, *extra, **kw)
            else:
                ops.sgd_step_dev(pg, gd, buf, step_dev, st, lr=lr, **kw)
        elif sched:
            ops.adam_step_sched_dev(pg, gd, state[0], state[1], step_dev, st, *extra, decoupled=case == "adamw", **kw)
        else:
            ops.adam_step_dev(pg, gd, state[0], state[1], step_dev, st, lr=lr, decoupled=case == "adamw", **kw)
        coefs.append(st[3:4].clone())
    torch.cuda.synchronize()
    assert int(step_dev) == len(grads)
    if sched:
        assert float(extra[1][0]) == float(np.float32(lr))
    return [pg] + state + [st.clone()], [float(c) for c in coefs]


@gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, BIG])
@pytest.mark.parametrize("case", sorted(IDENTITY_CASES))
def test_constant_schedule_is_bit_identical_to_the_plain_entry_points(ops, case, n):
    """``constant``, no warm-up, no EMA, through the scheduled entry points: 7 steps on random gradients leave the parameters,
    every state buffer and the scratch ``st`` bit-equal to the plain entry points' -- the rounding rule (the rate rounded to
    float32 once, then used exactly like the ``lr`` argument)."""
    g = torch.Generator().manual_seed(1000 + n % 1000)
    p0 = torch.randn(n, generator=g)
    draws = [torch.randn(n, generator=g) for _ in range(7)]
    grads = [(r + 0.5 * torch.sign(r)) * 4.0 for r in draws]                   # |g * grad_scale| >= 0.5 also for n = 1 ...
    assert all(float(gr.double().norm()) * 0.25 > 10 * 0.05 for gr in grads)    # ... so max_norm 0.05 binds on every step
    plain, c0 = _identity_run(ops, case, n, p0, grads, False)
    sched, c1 = _identity_run(ops, case, n, p0, grads, True)
    if case == "adam_clip":
        assert all(c < 1.0 for c in c0), c0
    else:
        assert all(c == 1.0 for c in c0), c0
    assert c0 == c1
    for k, (a, b) in enumerate(zip(plain, sched)):
        assert torch.equal(a, b), (case, n, k, int((a != b).sum()))
    assert bool(torch.isfinite(plain[0]).all()) and not torch.equal(plain[0].cpu(), p0)


# ------------------------------------------------------------------------------------------------ 2. the rate itself
RATE_BASE = 0.03
RATE_COMMON = {"every": 2, "warmup_steps": 3, "warmup_start_factor": 0.25}
RATE_KINDS = {"constant": {}, "step": {"gamma": 0.7, "step_size": 2}, "multistep": {"gamma": 0.3, "milestones": [2, 5]},
              "exponential": {"gamma": 0.93}, "cosine": {"T_max": 5, "eta_min": 1e-3}}
RATE_STEPS = 14                       # e = 0 .. 6: the end of warm-up (t = 4), a step boundary (e = 2), both milestones, T_max (e = 5, 6)


def _rate_other_order(kind, t):
    """lr(t) in float64 with the operations in another order and other primitives: powers by repeated multiplication, the
    cosine through the half angle, the warm-up factor applied last"""
    own = RATE_KINDS[kind]
    e = (t - 1) // 2
    if kind == "constant":
        main = RATE_BASE
    elif kind == "cosine":
        half = math.cos(math.pi * min(e, own["T_max"]) / (2 * own["T_max"]))
        main = own["eta_min"] + (RATE_BASE - own["eta_min"]) * half * half       # (1 + cos x) / 2 = cos^2 (x / 2)
    else:
        k = {"step": e // 2, "exponential": e}.get(kind)
        if kind == "multistep":
            k = sum(1 for m in own["milestones"] if m <= e)
        main = RATE_BASE
        for _ in range(k):
            main *= own["gamma"]
    w = RATE_COMMON["warmup_steps"]
    s = RATE_COMMON["warmup_start_factor"]
    return main * ((s * (w - min(t - 1, w)) + min(t - 1, w)) / w)


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


@pytest.mark.parametrize("kind", sorted(RATE_KINDS))
def test_host_mirror_agrees_with_another_operation_order(kind):
    """CPU: with the parameters chosen above the host mirror itself, rounded to float32, is within one ulp of a float64
    recomputation in a different operation order at every step and equal in at least 90 % of them -- so the same allowance on
    the device cannot hide a wrong formula behind a rounding that these parameters make unstable."""
    import adyolo_amd  # noqa: F401
    from adyolo_amd import lr_schedule
    tb = _table(dict(RATE_KINDS[kind], name=kind, **RATE_COMMON), RATE_BASE)
    exact = 0
    for t in range(1, RATE_STEPS + 1):
        got, want = lr_schedule.lr_at(tb, t), float(np.float32(_rate_other_order(kind, t)))
        assert _ulps(got, want) <= 1, (kind, t, got, want)
        assert abs(lr_schedule.lr_double(tb, t) - _rate_other_order(kind, t)) <= 1e-14 * RATE_BASE
        exact += got == want
    assert exact >= 0.9 * RATE_STEPS, (kind, exact)


@gpu
@pytest.mark.parametrize("optim", ["adam", "sgd"])
@pytest.mark.parametrize("kind", sorted(RATE_KINDS))
def test_device_rate_follows_the_host_mirror(ops, kind, optim):
    """``current_lr`` after each of 14 steps (warm-up 3, ``every`` 2) against ``lr_at(t)``: at most one float32 ulp apart,
    equal in at least 90 % of the steps.  AdamW's decay (sched_out[1]) is the float of 1 - lr * wd in double."""
    from adyolo_amd import lr_schedule
    tb = _table(dict(RATE_KINDS[kind], name=kind, **RATE_COMMON), RATE_BASE)
    sched_dev, out = _dev_table(tb), torch.zeros(ops.SCHED_OUT_FLOATS, device="cuda:0")
    n = 5
    p, gr = torch.ones(n, device="cuda:0"), torch.zeros(n, device="cuda:0")
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device="cuda:0")
    exact, seen = 0, []
    for t in range(1, RATE_STEPS + 1):
        if optim == "adam":
            ops.adam_step_sched_dev(p, gr, m, v, step_dev, st, sched_dev, out, weight_decay=0.125, decoupled=True)
        else:
            ops.sgd_step_sched_dev(p, gr, None, step_dev, st, sched_dev, out)
        got_all = out.cpu()
        got, want = float(got_all[0]), lr_schedule.lr_at(tb, t)
        seen.append(got)
        print("%s %s t=%d: device %.9e host %.9e (%d ulp)" % (kind, optim, t, got, want, _ulps(got, want)))
        assert _ulps(got, want) <= 1, (kind, t, got, want)
        exact += got == want
        if optim == "adam":
            assert float(got_all[1]) == float(np.float32(1.0 - float(np.float32(got)) * 0.125))
    assert exact >= 0.9 * RATE_STEPS, (kind, exact)
    assert _ulps(seen[0], RATE_BASE * 0.25) <= 1 and seen[1] > seen[0]                   # warm-up starts at s * base
    if kind != "constant":
        assert seen[-1] < seen[3]                                               # and the main schedule decays
    else:
        assert seen[3:] == [float(np.float32(RATE_BASE))] * (RATE_STEPS - 3)


# ------------------------------------------------------------------------------------------------ 3. parameters under a schedule
class _Bag(torch.nn.Module):
    def __init__(self, seed, n=4099):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(n, generator=g))                # 4099 + 6 = 4105 -> padded to 4108
        self.b = torch.nn.Parameter(torch.randn(2, 3, generator=g))


SCHED_STEP = {"name": "step", "every": 2, "warmup_steps": 3, "warmup_start_factor": 0.25, "gamma": 0.5, "step_size": 2}


def _fused(name, flat, **kw):
    from adyolo_amd.train import FusedAdam, FusedAdamW, FusedSGD
    if name == "Adam":
        return FusedAdam(flat, lr=1e-3, weight_decay=0.01, **kw)
    if name == "AdamW":
        return FusedAdamW(flat, lr=1e-3, weight_decay=0.01, **kw)
    return FusedSGD(flat, lr=0.05, momentum=0.9, weight_decay=0.01, **kw)


def _max_err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


@gpu
@pytest.mark.parametrize("name", ["Adam", "AdamW", "SGD"])
def test_scheduled_parameters_match_torch_driven_by_lr_at(ops, name):
    """10 steps under warm-up 3 + ``step`` against torch.optim on the CPU whose ``param_group['lr']`` is set to ``lr_at(t)``
    before every step; the 1e-6 absolute of the unscheduled comparison (test_gpu_optimizers)."""
    from adyolo_amd.dist import FlatParameters
    bag = _Bag(21)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in bag.parameters()]
    bag = bag.to("cuda:0")
    flat = FlatParameters(bag)
    fused = _fused(name, flat, lr_schedule=SCHED_STEP)
    ref = {"Adam": lambda: torch.optim.Adam(twin, lr=1e-3, weight_decay=0.01),
           "AdamW": lambda: torch.optim.AdamW(twin, lr=1e-3, weight_decay=0.01),
           "SGD": lambda: torch.optim.SGD(twin, lr=0.05, momentum=0.9, weight_decay=0.01)}[name]()
    g = torch.Generator().manual_seed(22)
    rates = []
    for t in range(1, 11):
        grads = [torch.randn(p.shape, generator=g) for p in twin]
        ref.param_groups[0]["lr"] = fused.lr_at(t)
        for p, gr in zip(twin, grads):
            p.grad = gr.clone()
        ref.step()
        fused.zero_grad()
        for p, gr in zip(bag.parameters(), grads):
            p.grad.copy_((gr * 4.0).to("cuda:0"))
        fused.step(grad_scale=0.25)
        rates.append(float(fused.current_lr))
        assert _ulps(rates[-1], fused.lr_at(t)) <= 1 and fused.sched_step == t
    assert len(set(rates)) == 4 and rates[9] < rates[4] < rates[3]             # the rate moved: warm-up (x 0.25, 0.5, 0.75, 1), two drops
    for p, q in zip(bag.parameters(), twin):
        err = _max_err(p, q)
        print("%s: max |p - torch| = %.3e" % (name, err))
        assert err <= 1e-6, err
    assert float(flat.flat[flat.numel:].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ 4. EMA
def _ema_run(ops, n, decay, warm, ema_on, steps=12, kind="adam"):
    g = torch.Generator().manual_seed(77 + n)
    p = torch.randn(n, generator=g).to("cuda:0")
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ema = torch.full_like(p, 55.0) if ema_on else None                         # garbage: the first update must not read it
    tb = _table({"name": "exponential", "gamma": 0.9}, 0.05, ema_decay=decay if ema_on else None, ema_warmup=warm and ema_on)
    sched_dev, out = _dev_table(tb), torch.zeros(ops.SCHED_OUT_FLOATS, device="cuda:0")
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device="cuda:0")
    ps, es, ws = [], [], []
    for _ in range(steps):
        gr = torch.randn(n, generator=g).to("cuda:0")
        if kind == "adam":
            ops.adam_step_sched_dev(p, gr, m, v, step_dev, st, sched_dev, out, ema)
        else:
            ops.sgd_step_sched_dev(p, gr, m, step_dev, st, sched_dev, out, ema, momentum=0.9)
        ps.append(p.cpu())
        ws.append(out.cpu())
        if ema_on:
            es.append(ema.cpu())
    return ps, es, ws, (p, m, v)


@gpu
@pytest.mark.parametrize("n", [5, 1027])
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("decay", [0.5, 0.9])
def test_ema_matches_float64_over_the_gpu_parameter_sequence(ops, decay, warm, n):
    """12 steps; the oracle is float64 over the parameters the GPU itself produced (read back after every step):
    ema_1 = p_1, ema_j = ema + (p_j - ema) * (1 - decay_eff), decay_eff = decay or min(decay, (1 + k) / (10 + k)) after k
    updates.  Bound: 2^-23 * max|p| / (1 - decay).  The first EMA is bit-equal to p; p, m, v are bit-equal to the run without
    EMA.  n = 5 and 1027 put 1 and 3 elements in the scalar tail."""
    ps, es, ws, state = _ema_run(ops, n, decay, warm, True)
    _, _, _, state_off = _ema_run(ops, n, decay, warm, False)
    for name, a, b in zip("pmv", state, state_off):
        assert torch.equal(a, b), name
    assert torch.equal(es[0], ps[0])
    oracle = ps[0].double()
    pmax = max(float(q.abs().max()) for q in ps)
    bound = 2.0 ** -23 * pmax / (1.0 - decay)
    worst = 0.0
    for k in range(1, len(ps)):
        keep = min(decay, (1.0 + k) / (10.0 + k)) if warm else decay
        oracle = oracle + (ps[k].double() - oracle) * (1.0 - keep)
        worst = max(worst, float((es[k].double() - oracle).abs().max()))
        assert float(ws[k][2]) == float(np.float32(1.0 - keep)) and float(ws[k][3]) == 0.0
    assert float(ws[0][3]) == 1.0
    print("ema decay=%g warm=%s n=%d: max |ema - float64| = %.3e (bound %.3e)" % (decay, warm, n, worst, bound))
    assert worst <= bound, (worst, bound)
    assert not torch.equal(es[-1], ps[-1])                                      # it lags behind the parameters


@gpu
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_ema_body_and_tail_round_alike(ops, kind):
    """n = 1027 puts elements 1024..1026 in the scalar tail, the same data extended to n = 1028 in a float4: the EMA of the
    first 1027 elements is equal bit for bit (both runs cut their parameters and gradients from the same draws of 1028)."""
    def run(n):
        g = torch.Generator().manual_seed(5)
        p = torch.randn(1028, generator=g)[:n].clone().to("cuda:0")
        m, v, ema = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
        tb = _table({"name": "constant"}, 0.05, ema_decay=0.9)
        sched_dev, out = _dev_table(tb), torch.zeros(ops.SCHED_OUT_FLOATS, device="cuda:0")
        step_dev = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device="cuda:0")
        for _ in range(4):
            gr = torch.randn(1028, generator=g)[:n].clone().to("cuda:0")
            if kind == "adam":
                ops.adam_step_sched_dev(p, gr, m, v, step_dev, st, sched_dev, out, ema)
            else:
                ops.sgd_step_sched_dev(p, gr, m, step_dev, st, sched_dev, out, ema, momentum=0.9)
        torch.cuda.synchronize()
        return p, ema
    (pt, et), (pb, eb) = run(1027), run(1028)
    assert torch.equal(pt, pb[:1027]) and torch.equal(et, eb[:1027])
    assert not torch.equal(et, pt) and float(et.abs().sum()) > 0.0


# ------------------------------------------------------------------------------------------------ 5. set_lr and resume
def _fresh(name, seed=31, **kw):
    from adyolo_amd.dist import FlatParameters
    bag = _Bag(seed).to("cuda:0")
    flat = FlatParameters(bag)
    return bag, flat, _fused(name, flat, **kw)


def _drive(bag, opt, grads):
    for grs in grads:
        opt.zero_grad()
        for p, gr in zip(bag.parameters(), grs):
            p.grad.copy_(gr)
        opt.step()


def _states(opt):
    own = [opt.momentum_buffer] if opt.kind == "sgd" else [opt.exp_avg, opt.exp_avg_sq]
    return [opt.flat.flat, opt.ema] + own


@gpu
@pytest.mark.parametrize("name", ["Adam", "SGD"])
def test_resume_continues_schedule_and_ema_bit_for_bit(ops, name):
    """3 steps, ``state_dict`` + ``sched_state_dict`` + EMA saved, a fresh optimizer, load, 3 steps == 6 straight steps, for Adam
    and for SGD with momentum (whose ``step_count`` restarts at 1 after the load: the table's offsets carry the clocks).  The
    padding of the flat buffers stays zero in p, state and EMA."""
    from adyolo_amd import checkpoint as ck
    kw = {"lr_schedule": SCHED_STEP, "ema_decay": 0.9, "ema_warmup": True}
    g = torch.Generator().manual_seed(41)
    grads = [[torch.randn(4099, generator=g).to("cuda:0"), torch.randn(2, 3, generator=g).to("cuda:0")] for _ in range(6)]
    bag_a, flat_a, straight = _fresh(name, **kw)
    _drive(bag_a, straight, grads)
    bag_b, flat_b, first = _fresh(name, **kw)
    _drive(bag_b, first, grads[:3])
    saved = (first.state_dict(), first.sched_state_dict(), ck.ema_state_dict(first, bag_b),
             {k: v.detach().cpu().clone() for k, v in bag_b.state_dict().items()})
    assert saved[1]["step"] == 3 and saved[1]["ema_updates"] == 3 and list(saved[2]) == list(saved[3])
    bag_c, flat_c, second = _fresh(name, seed=99, **kw)
    bag_c.load_state_dict(saved[3])
    second.load_state_dict(saved[0])
    second.load_sched_state_dict(saved[1])
    ck.load_ema_state_dict(second, bag_c, saved[2])
    assert second.step_count == (3 if name == "Adam" else 1) and second.sched_step == 3 and second.ema_updates == 3
    _drive(bag_c, second, grads[3:])
    torch.cuda.synchronize()
    assert second.sched_step == straight.sched_step == 6
    assert torch.equal(second.current_lr, straight.current_lr) and _ulps(float(second.current_lr), straight.lr_at(6)) <= 1
    for k, (a, b) in enumerate(zip(_states(straight), _states(second))):
        assert torch.equal(a, b), (name, k)
        assert float(a[flat_a.numel:].abs().sum()) == 0.0 and float(a.abs().sum()) > 0.0
    assert not torch.equal(straight.ema, straight.flat.flat)


@gpu
def test_set_lr_takes_effect_at_the_next_step(ops):
    """``set_lr`` between steps: ``current_lr`` of the next step is the new base times the same factors (4x the base is an
    exact factor in float32, and steps 5 and 6 share their unit: the device's own two rates differ by exactly 4)."""
    bag, flat, opt = _fresh("Adam", lr_schedule=SCHED_STEP)
    g = torch.Generator().manual_seed(43)
    grads = [[torch.randn(4099, generator=g).to("cuda:0"), torch.randn(2, 3, generator=g).to("cuda:0")] for _ in range(8)]
    _drive(bag, opt, grads[:5])
    last = float(opt.current_lr)
    assert _ulps(last, opt.lr_at(5)) <= 1
    before = [opt.lr_at(t) for t in (6, 7, 8)]
    opt.set_lr(4e-3)
    assert float(opt.current_lr) == last                                       # not yet: still the last step's rate
    for t in (6, 7, 8):
        _drive(bag, opt, grads[t - 1:t])
        assert opt.lr_at(t) == 4 * before[t - 6] and _ulps(float(opt.current_lr), opt.lr_at(t)) <= 1, t
        if t == 6:
            assert float(opt.current_lr) == 4 * last
    _, _, plain = _fresh("Adam")
    with pytest.raises(ValueError, match="lr_schedule: {name: constant}"):
        plain.set_lr(1e-4)


# ------------------------------------------------------------------------------------------------ 6. graph replay, ema_weights
def _params(**train_config):
    tc = {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
          "conf_thresh": 0.5, "clss_thresh": 0.5, "unify_thresh": 15.0, "nms": "conn-merge",
          "loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
          "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0}
    tc.update(train_config)
    return {"args": {"device": "cuda:0", "encoder": "se-resnet34", "loss": "adyolo"},
            "data_config": {"nb_classes": 12}, "train_config": tc}


FULL = {"optim": "AdamW", "weight_decay": 0.01, "clip_grad_norm": 3.0, "lr_schedule": SCHED_STEP, "ema_decay": 0.9}


def _trainer(graph, t=80, **train_config):
    from adyolo_amd.wrapper import WrapperModel, WrapperCriterion
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.train import TrainStep
    torch.manual_seed(100)
    prm = _params(**train_config)
    model = WrapperModel((1, 7, t, 64), (), prm).to("cuda:0")
    return TrainStep(model, WrapperCriterion(prm), FeatureExtractor(None, "cuda:0"), prm, graph=graph), prm


@gpu
def test_graphed_scheduled_step_is_bit_identical_to_eager(ops):
    """2 clips x 2 s (the shape of test_gpu_graph's step test), AdamW + clip + warm-up 3 + ``step`` (``every`` 2, step_size 2) +
    EMA, 8 steps: loss, parameters, moments, EMA and ``current_lr`` are bit-equal after EVERY step; a ``set_lr`` after step 5
    is followed by both paths and records nothing new."""
    from adyolo_amd.datasets import synthetic_audio, synthetic_targets
    audios = [synthetic_audio(2, 24000 * 2, seed=70 + i).to("cuda:0") for i in range(3)]
    targets = [synthetic_targets(2, 20, 12, seed=80 + i) for i in range(8)]
    (te, _), (tg, _) = _trainer(False, **FULL), _trainer(True, **FULL)
    assert tg.graphs is not None and te.graphs is None and te.optimizer.kind == "adamw" and te.optimizer.ema is not None
    rates = []
    for i in range(8):
        a = te.step(audios[i % 3], targets[i])
        b = tg.step(audios[i % 3], targets[i])
        assert torch.equal(a, b), "loss of step %d: eager %r graph %r" % (i + 1, float(a), float(b))
        oe, og = te.optimizer, tg.optimizer
        for name, x, y in (("p", te.flat.flat, tg.flat.flat), ("m", oe.exp_avg, og.exp_avg), ("v", oe.exp_avg_sq, og.exp_avg_sq),
                           ("ema", oe.ema, og.ema), ("lr", oe.current_lr, og.current_lr), ("norm", oe.grad_norm, og.grad_norm)):
            assert torch.equal(x, y), (i + 1, name)
        rates.append(float(og.current_lr))
        assert _ulps(rates[-1], oe.lr_at(i + 1)) <= 1, (i + 1, rates[-1], oe.lr_at(i + 1))
        if i == 4:
            te.optimizer.set_lr(2e-3)
            tg.optimizer.set_lr(2e-3)
    assert tg.graphs.captures == 1 and tg.graphs.replays == 7 and tg.graphs.eager_steps == 1
    assert rates[5] == 2 * rates[4]                                             # t = 5, 6 share e = 2: only the base moved
    assert rates[0] < rates[1] < rates[2] < rates[3] and rates[4] == rates[3] / 2 and rates[7] == rates[5]
    assert bool(torch.isfinite(te.flat.flat).all()) and not torch.equal(te.optimizer.ema, te.flat.flat)
    assert te.optimizer.step_count == tg.optimizer.step_count == 8 and int(tg.optimizer.step_dev) == 8


@gpu
def test_ema_weights_swaps_the_average_in_and_out(ops):
    """Inside ``ema_weights()`` an evaluation forward equals the forward of a second model loaded from ``ema_state_dict``; after
    the exit it equals the forward before the entry (both bit for bit: a missing ``params_changed()`` would serve stale packed
    weights)."""
    from adyolo_amd import checkpoint as ck
    from adyolo_amd.datasets import synthetic_audio, synthetic_targets
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.wrapper import WrapperModel
    tr, prm = _trainer(False, **FULL)
    audio = synthetic_audio(2, 24000 * 2, seed=5).to("cuda:0")
    clip = synthetic_audio(1, 24000 * 2, seed=6).to("cuda:0")
    for i in range(3):
        tr.step(audio, synthetic_targets(2, 20, 12, seed=5 + i))
    fx = FeatureExtractor(None, "cuda:0")

    def forward(model):
        model.eval()
        with torch.no_grad():
            return model(fx(clip, channels_last8=True), channels_last8=True).clone()

    live = tr.flat.flat.clone()
    before = forward(tr.model)
    torch.manual_seed(7)
    twin = WrapperModel((1, 7, 80, 64), (), prm).to("cuda:0")
    twin.load_state_dict(ck.ema_state_dict(tr.optimizer, tr.model))
    want = forward(twin)
    with tr.ema_weights():
        assert torch.equal(tr.flat.flat, tr.optimizer.ema) and not torch.equal(tr.flat.flat, live)
        inside = forward(tr.model)
    assert torch.equal(inside, want), float((inside - want).abs().max())
    assert not torch.equal(inside, before)
    assert torch.equal(tr.flat.flat, live)
    assert torch.equal(forward(tr.model), before)
    plain, _ = _trainer(False)
    with pytest.raises(ValueError):
        with plain.ema_weights():
            pass
