"""CPU: the host surface of the device-side learning-rate schedules and the weight EMA: ``get_optimizers`` dispatch, the
closed forms of ``lr_at`` against ``torch.optim.lr_scheduler``, and the checkpoint round trip of ``sched_state_dict`` /
``ema_state_dict``.  No HIP call is made: the state containers are filled by hand and live on the CPU (the pattern of
test_optimizers_cpu)."""
import math

import pytest
import torch

import adyolo_amd  # noqa: F401  (import shim at the repo root)


def _cpu_params(**train_config):
    tc = {"grid_size": [45, 45], "nb_anchors": 5, "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0}
    tc.update(train_config)
    return {"args": {"device": "cpu", "encoder": "se-resnet34", "loss": "adyolo"}, "data_config": {"nb_classes": 12},
            "train_config": tc}


def _small_net(seed=5):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.BatchNorm1d(3), torch.nn.Linear(3, 2))   # 15+3+3+3+6+2 = 32
    return net


def _small_flat(seed=5):
    from adyolo_amd.dist import FlatParameters
    net = _small_net(seed)
    return net, FlatParameters(net)


# ------------------------------------------------------------------------------------------------ dispatch
def test_get_optimizers_dispatch_with_and_without_the_keys():
    from adyolo_amd import ops
    from adyolo_amd.train import FusedAdam, FusedAdamW, FusedSGD, get_optimizers
    _, flat = _small_flat()
    for name in ("Adam", "AdamW", "SGD"):
        o = get_optimizers(_cpu_params(optim=name), flat)                    # without the keys: today's path, nothing new
        assert o.sched_dev is None and o.sched_out is None and o.ema is None and o.current_lr is None
        assert tuple(o.st_dev.shape) == (ops.OPTIM_SCRATCH_FLOATS,) == (4,)
        assert "sched_dev" not in vars(o) and "ema" not in vars(o)
        with pytest.raises(ValueError, match="lr_schedule: {name: constant}"):
            o.set_lr(1e-4)
        assert o.lr_at(1) == o.lr_at(50) == float(torch.tensor(1e-3, dtype=torch.float32))
    cfg = {"name": "step", "every": 2, "warmup_steps": 3, "warmup_start_factor": 0.25, "gamma": 0.5, "step_size": 2}
    for name, cls in (("Adam", FusedAdam), ("AdamW", FusedAdamW), ("SGD", FusedSGD)):
        o = get_optimizers(_cpu_params(optim=name, lr=2e-3, lr_schedule=cfg), flat)
        assert type(o) is cls and o.ema is None and o.lr == 2e-3
        assert o.sched_dev.dtype == torch.float64 and tuple(o.sched_dev.shape) == (ops.SCHED_TABLE_DOUBLES,)
        assert o.sched_out.dtype == torch.float32 and tuple(o.sched_out.shape) == (ops.SCHED_OUT_FLOATS,)
        assert tuple(o.current_lr.shape) == (1,) and o.current_lr.data_ptr() == o.sched_out.data_ptr()
        assert tuple(o.st_dev.shape) == (ops.OPTIM_SCRATCH_FLOATS,)
        tb = o.sched_dev.tolist()
        assert tb[ops.SCHED_KIND] == ops.SCHED_KINDS["step"] and tb[ops.SCHED_BASE] == 2e-3 and tb[ops.SCHED_EVERY] == 2
        assert (tb[ops.SCHED_WARMUP], tb[ops.SCHED_START], tb[ops.SCHED_GAMMA], tb[ops.SCHED_STEP_SIZE]) == (3, 0.25, 0.5, 2)
        assert tb[ops.SCHED_OFFSET] == 0 and o.sched_step == 0
        o.set_lr(5e-4)
        assert o.lr == 5e-4 and o.sched_dev.tolist()[ops.SCHED_BASE] == 5e-4
    o = get_optimizers(_cpu_params(ema_decay=0.99), flat)                     # EMA alone: a constant schedule carries it
    assert o.sched_config["name"] == "constant" and o.ema.shape == flat.flat.shape and o.ema_warmup is False
    assert float(o.ema.abs().sum()) == 0.0 and o.ema_updates == 0
    assert o.sched_dev.tolist()[ops.SCHED_EMA_DECAY] == 0.99 and o.sched_dev.tolist()[ops.SCHED_EMA_WARMUP] == 0
    o = get_optimizers(_cpu_params(optim="SGD", ema_decay=0.9, ema_warmup=True, lr_schedule={"name": "constant"}), flat)
    assert o.sched_dev.tolist()[ops.SCHED_EMA_WARMUP] == 1 and o.ema is not None
    from adyolo_amd import _lib
    lib = _lib.load()                                                         # the library's own sizes of the two buffers
    assert lib.adyolo_sched_table_doubles() == ops.SCHED_TABLE_DOUBLES and lib.adyolo_sched_out_floats() == ops.SCHED_OUT_FLOATS
    ms = {"name": "multistep", "milestones": [2, 5, 9], "gamma": 0.3}
    tb = get_optimizers(_cpu_params(lr_schedule=ms), flat).sched_dev.tolist()
    assert tb[ops.SCHED_N_MILESTONES] == 3 and tb[ops.SCHED_MILESTONE0:ops.SCHED_MILESTONE0 + 4] == [2, 5, 9, 0]


def test_bad_schedules_raise():
    from adyolo_amd.train import get_optimizers
    _, flat = _small_flat()
    for bad in ({"name": "onecycle"}, {"name": "cyclic"}, {}):
        with pytest.raises(NotImplementedError):                             # like an unknown ``optim``
            get_optimizers(_cpu_params(lr_schedule=bad), flat)
    with pytest.raises(NotImplementedError):
        get_optimizers(_cpu_params(optim="RMSprop", lr_schedule={"name": "constant"}), flat)
    bad_values = [{"name": "constant", "every": 0}, {"name": "constant", "every": 1.5}, {"name": "constant", "warmup_steps": -1},
                  {"name": "constant", "warmup_start_factor": 0.0}, {"name": "constant", "warmup_start_factor": 1.5},
                  {"name": "constant", "gamma": 0.5},                        # a key of another kind
                  {"name": "step", "gamma": 0.5}, {"name": "step", "step_size": 0}, {"name": "step", "step_size": 2, "gamma": 0.0},
                  {"name": "multistep"}, {"name": "multistep", "milestones": [5, 2]},
                  {"name": "multistep", "milestones": list(range(9))}, {"name": "exponential"},
                  {"name": "cosine"}, {"name": "cosine", "T_max": 0}, {"name": "cosine", "T_max": 5, "eta_min": -1.0}]
    for bad in bad_values:
        with pytest.raises(ValueError):
            get_optimizers(_cpu_params(lr_schedule=bad), flat)
    with pytest.raises(ValueError):
        get_optimizers(_cpu_params(lr=0.0, lr_schedule={"name": "cosine", "T_max": 5}), flat)       # base / base
    for decay in (1.0, -0.1):
        with pytest.raises(ValueError):
            get_optimizers(_cpu_params(ema_decay=decay), flat)
    with pytest.raises(ValueError):
        get_optimizers(_cpu_params(ema_warmup=True), flat)
    with pytest.raises(ValueError):                                            # as torch.optim.SGD, schedule or not
        get_optimizers(_cpu_params(optim="SGD", nesterov=True, lr_schedule={"name": "constant"}), flat)
    o = get_optimizers(_cpu_params(lr_schedule={"name": "cosine", "T_max": 5}), flat)
    with pytest.raises(ValueError):
        o.set_lr(-1.0)


# ------------------------------------------------------------------------------------------------ closed forms vs torch
BASE, UNITS, WARM_UNITS, START = 0.05, 60, 4, 0.25
KINDS = {"step": ({"gamma": 0.7, "step_size": 7}, lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=7, gamma=0.7)),
         "multistep": ({"gamma": 0.3, "milestones": [5, 11, 11, 40]},
                       lambda o: torch.optim.lr_scheduler.MultiStepLR(o, milestones=[5, 11, 11, 40], gamma=0.3)),
         "exponential": ({"gamma": 0.93}, lambda o: torch.optim.lr_scheduler.ExponentialLR(o, gamma=0.93)),
         "cosine": ({"T_max": 60, "eta_min": 1e-3},
                    lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=60, eta_min=1e-3)),
         # chained with LinearLR, torch's recursion lr' = eta_min + (lr - eta_min) * ratio is a product of factors only for
         # eta_min = 0 (otherwise the warm-up factor also scales the eta_min it subtracts, which no closed form follows)
         "cosine_warm": ({"T_max": 60, "eta_min": 0.0},
                         lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=60, eta_min=0.0))}
DRIFT = 4 * 7.2e-16


def _warm(t, every):
    w = WARM_UNITS * every
    return START + (1 - START) * min(t - 1, w) / w


def _torch_rates(make, warm):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE)
    scheds = [make(opt)]
    if warm:
        scheds.insert(0, torch.optim.lr_scheduler.LinearLR(opt, start_factor=START, total_iters=WARM_UNITS))
    sch = torch.optim.lr_scheduler.ChainedScheduler(scheds) if warm else scheds[0]
    rates = []
    for u in range(UNITS + 1):                                               # units 0 .. 60: 60 scheduler steps
        rates.append(opt.param_groups[0]["lr"])
        if u < UNITS:
            opt.step()
            sch.step()
    return rates


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("kind", ["cosine", "exponential", "multistep", "step"])
def test_closed_forms_match_torch_schedulers(kind, warm, every):
    """``lr_at``'s closed form, BEFORE its rounding to float32, against torch's scheduler stepped once per unit on a
    one-parameter CPU optimizer (StepLR, MultiStepLR, ExponentialLR, CosineAnnealingLR up to T_max = 60; each also chained with
    LinearLR), 60 units, ``every`` in {1, 3}.  torch's unit u is the rate of the steps t = u * every + 1 .. (u + 1) * every.
    Warm-up counts STEPS here, units in torch: at the first step of a unit the two agree when warmup_steps = total_iters *
    every (min(u * every, W) / W = min(u, iters) / iters), so the chained forms are compared there, and the other steps of
    the unit must carry the same main factor.

    Bound: torch's forms are recursive (lr *= factor per unit) and drift from the closed forms by rounding only.  Largest
    relative difference measured here over all 16 cases: 7.2e-16 (7.107e-16, cosine with warm-up; about 3 double ulps over 60
    units; exponential with warm-up 5.7e-16, the others below 5e-16); the assertion is that figure times 4.  The chained cosine
    runs with eta_min = 0 (see ``KINDS``), the plain one with eta_min = 1e-3."""
    from adyolo_amd import lr_schedule
    from adyolo_amd.train import FusedSGD
    _, flat = _small_flat()
    own, make = KINDS["cosine_warm" if kind == "cosine" and warm else kind]
    cfg = dict(own, name=kind, every=every)
    if warm:
        cfg.update(warmup_steps=WARM_UNITS * every, warmup_start_factor=START)
    opt = FusedSGD(flat, lr=BASE, lr_schedule=cfg)
    tb = opt.sched_dev.tolist()
    ref = _torch_rates(make, warm)
    worst = 0.0
    for u, want in enumerate(ref):
        t0 = u * every + 1
        got = lr_schedule.lr_double(tb, t0)
        worst = max(worst, abs(got - want) / want if want > 0.0 else abs(got))     # (cosine, eta_min 0, at T_max: both are 0)
        assert opt.lr_at(t0) == float(torch.tensor(got, dtype=torch.float64).float())      # the float32 the device hands on
        for t in range(t0 + 1, t0 + every):                                  # the unit's other steps: the same main factor
            other = lr_schedule.lr_double(tb, t)
            if warm:                                                         # (two divisions by warm(t): a few double ulps)
                assert abs(other / _warm(t, every) - got / _warm(t0, every)) <= 1e-15 * got / _warm(t0, every)
            else:
                assert other == got
    print("%s warm=%s every=%d: largest relative difference from torch %.3e" % (kind, warm, every, worst))
    assert worst <= DRIFT, worst


def test_cosine_holds_eta_min_after_t_max_and_step_one_is_the_base_rate():
    from adyolo_amd import lr_schedule
    from adyolo_amd.train import FusedAdam
    _, flat = _small_flat()
    opt = FusedAdam(flat, lr=BASE, lr_schedule={"name": "cosine", "T_max": 6, "eta_min": 1e-3, "every": 2})
    tb = opt.sched_dev.tolist()
    assert lr_schedule.lr_double(tb, 1) == BASE and lr_schedule.lr_double(tb, 2) == BASE
    for t in range(13, 40):                                                    # e >= T_max: held, not periodic
        assert abs(lr_schedule.lr_double(tb, t) - 1e-3) <= 1e-3 * 4e-16, t
        assert opt.lr_at(t) == float(torch.tensor(1e-3).float())
    assert lr_schedule.lr_double(tb, 12) > 1e-3 * 1.5
    for name, own in (("constant", {}), ("step", {"step_size": 3}), ("multistep", {"milestones": [1]}),
                      ("exponential", {"gamma": 0.9})):
        o = FusedAdam(flat, lr=BASE, lr_schedule=dict(own, name=name))
        assert lr_schedule.lr_double(o.sched_dev.tolist(), 1) == BASE
    o = FusedAdam(flat, lr=BASE, lr_schedule={"name": "constant", "warmup_steps": 4, "warmup_start_factor": 0.5})
    for t, want in zip((1, 2, 3, 4, 5, 6), (0.5, 0.625, 0.75, 0.875, 1, 1)):
        assert abs(lr_schedule.lr_double(o.sched_dev.tolist(), t) - BASE * want) <= 4e-16 * BASE


# ------------------------------------------------------------------------------------------------ checkpoints
def _fill(buf, flat, seed):
    g = torch.Generator().manual_seed(seed)
    buf[:flat.numel].copy_(torch.randn(flat.numel, generator=g))


SCHED = {"name": "multistep", "every": 2, "warmup_steps": 3, "warmup_start_factor": 0.5, "gamma": 0.5, "milestones": [1, 3]}


def test_files_gain_the_two_entries_only_when_the_features_are_on(tmp_path):
    from adyolo_amd import checkpoint as ck
    from adyolo_amd.dist import FlatParameters
    from adyolo_amd.train import FusedAdam, FusedSGD
    net = _small_net()
    flat = FlatParameters(net)
    plain = FusedAdam(flat)
    plain.step_count = 2
    ck.save_checkpoint(str(tmp_path / "a.h5"), net, plain, 1, 0.5, {}, [], "cpu")
    ck.save_best(str(tmp_path / "b.h5"), net, plain, 1, 0.5)
    a = torch.load(str(tmp_path / "a.h5"), weights_only=False)
    b = torch.load(str(tmp_path / "b.h5"), weights_only=False)
    assert list(a) == ["start_epoch_nb", "model_state_dict", "optim_state_dict", "confidence_thresh", "rng_state", "best_log",
                       "train_remaining_file"]
    assert list(b) == ["epoch_nb", "model_state_dict", "optim_state_dict", "confidence_thresh"]
    sched_only = FusedSGD(flat, lr_schedule=SCHED)
    ck.save_best(str(tmp_path / "c.h5"), net, sched_only, 1, 0.5)
    c = torch.load(str(tmp_path / "c.h5"), weights_only=False)
    assert list(c) == list(b) + ["sched_state_dict"]
    both = FusedAdam(flat, lr_schedule=SCHED, ema_decay=0.9)
    _fill(both.ema, flat, 3)
    both.step_count = 4
    ck.save_checkpoint(str(tmp_path / "d.h5"), net, both, 1, 0.5, {}, [], "cpu")
    ck.save_best(str(tmp_path / "e.h5"), net, both, 1, 0.5)
    d = torch.load(str(tmp_path / "d.h5"), weights_only=False)
    e = torch.load(str(tmp_path / "e.h5"), weights_only=False)
    assert list(d) == list(a) + ["sched_state_dict", "ema_state_dict"] and list(e) == list(b) + ["sched_state_dict", "ema_state_dict"]
    assert list(d["ema_state_dict"]) == list(d["model_state_dict"]) == list(net.state_dict())
    assert d["sched_state_dict"]["config"] == both.sched_config and d["sched_state_dict"]["step"] == 4
    assert d["sched_state_dict"]["base_lr"] == both.lr and d["sched_state_dict"]["ema_updates"] == 4
    names = {k for k, _ in net.named_parameters()}
    for k, v in d["ema_state_dict"].items():
        if k in names:                                                         # parameters: the EMA's
            p = dict(net.named_parameters())[k]
            i = [id(q) for q in flat.params].index(id(p))
            off, n = flat.offsets[i]
            assert torch.equal(v, both.ema[off:off + n].view(p.shape)) and not torch.equal(v, p.detach())
        else:                                                                  # buffers: the live model's
            assert torch.equal(v, net.state_dict()[k])
    twin = _small_net(seed=9)                                                 # the reference's way: load it as a model
    twin.load_state_dict(d["ema_state_dict"], strict=True)


@pytest.mark.parametrize("name", ["Adam", "AdamW", "SGD", "SGD_momentum"])
def test_save_then_load_restores_table_offset_and_ema(tmp_path, name):
    """Resume continues the schedule for all three optimizers: FusedSGD's ``step_count`` restarts (1 with momentum buffers,
    0 without), the schedule's clock and the EMA's update count do not -- the table's offsets carry the difference."""
    from adyolo_amd import checkpoint as ck
    from adyolo_amd import ops
    from adyolo_amd.dist import FlatParameters
    from adyolo_amd.train import get_optimizers
    net = _small_net()
    flat = FlatParameters(net)
    tc = {"optim": name.split("_")[0], "lr": 0.02, "lr_schedule": SCHED, "ema_decay": 0.9, "ema_warmup": True}
    if name == "SGD_momentum":
        tc["momentum"] = 0.9
    src = get_optimizers(_cpu_params(**tc), flat)
    _fill(src.ema, flat, 4)
    for buf in ([src.exp_avg, src.exp_avg_sq] if src.kind != "sgd" else [src.momentum_buffer] if tc.get("momentum") else []):
        _fill(buf, flat, 5)
    src.step_count = 7
    src.set_lr(0.005)                                                          # a plateau drop before the save
    path = str(tmp_path / "model_ckpt.h5")
    ck.save_checkpoint(path, net, src, 3, 0.5, {}, [], "cpu")
    net2 = _small_net(seed=6)
    flat2 = FlatParameters(net2)
    dst = get_optimizers(_cpu_params(**dict(tc, lr=0.02, lr_schedule={"name": "constant"})), flat2)
    ck.load_checkpoint(path, net2, dst, device="cpu", restore_rng=False)
    assert dst.step_count == {"Adam": 7, "AdamW": 7, "SGD": 0, "SGD_momentum": 1}[name]
    assert dst.sched_step == 7 and dst.ema_updates == 7 and dst.lr == 0.005 and dst.sched_config == src.sched_config
    want = src.sched_dev.tolist()
    got = dst.sched_dev.tolist()
    for i in range(ops.SCHED_TABLE_DOUBLES):
        if i not in (ops.SCHED_OFFSET, ops.SCHED_EMA_OFFSET):
            assert got[i] == want[i], i
    assert got[ops.SCHED_OFFSET] == got[ops.SCHED_EMA_OFFSET] == 7 - dst.step_count
    assert got[ops.SCHED_BASE] == 0.005
    assert torch.equal(dst.ema, src.ema) and float(dst.ema[flat2.numel:].abs().sum()) == 0.0
    assert [dst.lr_at(t) for t in range(1, 12)] == [src.lr_at(t) for t in range(1, 12)]
    dst.sync_device_step()
    assert int(dst.step_dev) + got[ops.SCHED_OFFSET] == 7                     # what the prep kernel adds up


def test_a_file_without_ema_starts_the_ema_from_the_loaded_parameters(tmp_path):
    from adyolo_amd import checkpoint as ck
    from adyolo_amd import ops
    from adyolo_amd.dist import FlatParameters
    from adyolo_amd.train import FusedAdam
    net = _small_net()
    flat = FlatParameters(net)
    old = FusedAdam(flat, lr=0.01)                                             # a run from before the features
    old.step_count = 5
    path = str(tmp_path / "model_ckpt.h5")
    ck.save_checkpoint(path, net, old, 3, 0.5, {}, [], "cpu")
    net2 = _small_net(seed=6)
    flat2 = FlatParameters(net2)
    new = FusedAdam(flat2, lr=0.5, lr_schedule={"name": "exponential", "gamma": 0.9}, ema_decay=0.99)
    ck.load_checkpoint(path, net2, new, device="cpu", restore_rng=False)
    assert torch.equal(flat2.flat, flat.flat) and torch.equal(new.ema, flat2.flat)
    assert new.ema_updates == 1 and new.step_count == 5 and new.sched_step == 5      # the schedule follows the optimizer's step
    assert new.lr == 0.01 and new.sched_dev.tolist()[ops.SCHED_BASE] == 0.01          # the file's rate is the base rate
    assert new.sched_config["name"] == "exponential"
    assert math.isclose(new.lr_at(6), 0.01 * 0.9 ** 5, rel_tol=1e-6)
