"""CPU: the optimizer surface of ``train.get_optimizers`` (reference src/train.py:29-37: 'Adam' | 'AdamW' | 'SGD') and the
checkpoint interchange of FusedAdamW / FusedSGD with torch.optim.AdamW / torch.optim.SGD.  No HIP call is made: the state
containers are filled by hand, the model lives on the CPU (the pattern of test_host_cpu's checkpoint test)."""
import pytest
import torch

import adyolo_amd  # noqa: F401  (import shim at the repo root)


def _cpu_params(**train_config):
    tc = {"grid_size": [45, 45], "nb_anchors": 5, "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0}
    tc.update(train_config)
    return {"args": {"device": "cpu", "encoder": "se-resnet34", "loss": "adyolo"}, "data_config": {"nb_classes": 12},
            "train_config": tc}


def _small_flat():
    from adyolo_amd.dist import FlatParameters
    torch.manual_seed(5)
    net = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))      # 15 + 3 + 6 + 2 = 26 -> padded to 28
    return net, FlatParameters(net)


def _model_and_twin(seed=3):
    from adyolo_amd.wrapper import WrapperModel
    torch.manual_seed(seed)
    model = WrapperModel((1, 7, 64, 64), (), _cpu_params())
    twin = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    return model, twin


def _two_cpu_steps(opt, twin):
    for _ in range(2):
        for p in twin:
            p.grad = torch.randn_like(p)
        opt.step()
    return opt.state_dict()


def _fill(buf, flat, seed):
    """distinct values in every element of a flat state buffer (padding stays zero)"""
    g = torch.Generator().manual_seed(seed)
    buf[:flat.numel].copy_(torch.randn(flat.numel, generator=g))


def _slice_of(flat, buf, p):
    k = [id(q) for q in flat.params].index(id(p))
    off, n = flat.offsets[k]
    return buf[off:off + n].view(p.shape)


def test_get_optimizers_dispatch():
    """'Adam' stays the same class with the same arguments; 'AdamW' / 'SGD' take lr / weight_decay as the reference passes
    them; the optional keys are honoured; anything else raises NotImplementedError."""
    from adyolo_amd import ops
    from adyolo_amd.train import FusedAdam, FusedAdamW, FusedSGD, get_optimizers
    _, flat = _small_flat()
    o = get_optimizers(_cpu_params(lr=2e-3, weight_decay=0.1), flat)
    assert type(o) is FusedAdam and o.max_norm is None and o.grad_norm is None
    assert (o.lr, o.betas, o.eps, o.weight_decay) == (2e-3, (0.9, 0.999), 1e-8, 0.1)
    assert tuple(o.st_dev.shape) == (ops.OPTIM_SCRATCH_FLOATS,) and o.step_count == 0 and o.kind == "adam"
    o = get_optimizers(_cpu_params(optim="AdamW", lr=3e-3, weight_decay=0.02), flat)
    assert type(o) is FusedAdamW and (o.lr, o.weight_decay, o.max_norm) == (3e-3, 0.02, None)
    assert get_optimizers({"train_config": {"optim": "AdamW"}}, flat).weight_decay == 1e-2            # torch.optim.AdamW's default
    o = get_optimizers(_cpu_params(optim="SGD", lr=0.05, weight_decay=1e-4), flat)
    assert type(o) is FusedSGD and (o.lr, o.weight_decay, o.momentum, o.dampening, o.nesterov) == (0.05, 1e-4, 0.0, 0.0, False)
    assert o.momentum_buffer is None and o.max_norm is None             # no momentum: nothing allocated
    o = get_optimizers(_cpu_params(optim="SGD", momentum=0.9, dampening=0.1, clip_grad_norm=3.0), flat)
    assert (o.momentum, o.dampening, o.nesterov, o.max_norm) == (0.9, 0.1, False, 3.0)
    assert o.momentum_buffer.shape == flat.flat.shape and tuple(o.grad_norm.shape) == (1,)
    o = get_optimizers(_cpu_params(optim="SGD", momentum=0.9, nesterov=True), flat)
    assert o.nesterov is True
    for name in ("Adam", "AdamW"):
        o = get_optimizers(_cpu_params(optim=name, clip_grad_norm=3), flat)
        assert o.max_norm == 3.0 and tuple(o.grad_norm.shape) == (1,) and o.grad_norm.dtype == torch.float32
        assert get_optimizers(_cpu_params(optim=name, clip_grad_norm=None), flat).max_norm is None
    with pytest.raises(NotImplementedError):
        get_optimizers(_cpu_params(optim="RMSprop"), flat)
    with pytest.raises(ValueError):
        get_optimizers(_cpu_params(optim="SGD", nesterov=True), flat)                                   # as torch.optim.SGD


def test_fused_classes_keep_the_contract_of_fused_adam():
    """What graph.StepGraphs and checkpoint use: flat, step_count (settable), _dev_step_value, step_dev, the methods."""
    from adyolo_amd.train import FusedAdam, FusedAdamW, FusedSGD
    _, flat = _small_flat()
    for o in (FusedAdam(flat, max_norm=1.0), FusedAdamW(flat), FusedSGD(flat, momentum=0.5), FusedSGD(flat)):
        assert o.flat is flat and o.step_count == 0 and o._dev_step_value == 0
        assert o.step_dev.dtype == torch.int64 and o.step_dev.numel() == 1
        o.step_count = 4
        assert o.step_count == 4 and o._dev_step_value == 0
        o.sync_device_step()
        assert int(o.step_dev) == 4 and o._dev_step_value == 4
        for name in ("replayed", "zero_grad", "step", "state_dict", "load_state_dict"):
            assert callable(getattr(o, name))


def test_adamw_state_round_trips_with_torch():
    from adyolo_amd import checkpoint as ck
    from adyolo_amd.dist import FlatParameters
    from adyolo_amd.train import FusedAdamW
    model, twin = _model_and_twin()
    flat = FlatParameters(model)
    # fused -> torch
    opt = FusedAdamW(flat, lr=2e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=0.03)
    _fill(opt.exp_avg, flat, 1)
    _fill(opt.exp_avg_sq, flat, 2)
    opt.exp_avg_sq.abs_()
    opt.step_count = 5
    sd = ck.optimizer_state_dict(opt, model)
    assert list(sd["param_groups"][0]) == ["lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable",
                                           "differentiable", "fused", "decoupled_weight_decay", "params"]
    assert sd["param_groups"][0]["decoupled_weight_decay"] is True
    tw = torch.optim.AdamW(twin)
    tw.load_state_dict(sd)
    got = tw.state_dict()
    assert got["param_groups"][0]["lr"] == 2e-3 and got["param_groups"][0]["weight_decay"] == 0.03
    for i, p in enumerate(model.parameters()):
        assert int(got["state"][i]["step"]) == 5
        assert torch.equal(got["state"][i]["exp_avg"], _slice_of(flat, opt.exp_avg, p))
        assert torch.equal(got["state"][i]["exp_avg_sq"], _slice_of(flat, opt.exp_avg_sq, p))
    # torch -> fused
    ref = _two_cpu_steps(torch.optim.AdamW(twin, lr=4e-3, betas=(0.85, 0.97), eps=1e-6, weight_decay=0.02), twin)
    opt2 = FusedAdamW(flat)
    ck.load_optimizer_state_dict(opt2, model, ref)
    assert (opt2.lr, opt2.betas, opt2.eps, opt2.weight_decay, opt2.step_count) == (4e-3, (0.85, 0.97), 1e-6, 0.02, 2)
    for i, p in enumerate(model.parameters()):
        assert torch.equal(_slice_of(flat, opt2.exp_avg, p), ref["state"][i]["exp_avg"])
        assert torch.equal(_slice_of(flat, opt2.exp_avg_sq, p), ref["state"][i]["exp_avg_sq"])
    assert float(opt2.exp_avg[flat.numel:].abs().sum()) == 0.0
    # the two layouts do not mix
    adam_sd = torch.optim.Adam(twin).state_dict()
    if adam_sd["param_groups"][0].get("decoupled_weight_decay") is False:
        with pytest.raises(ValueError):
            ck.load_optimizer_state_dict(opt2, model, adam_sd)
    with pytest.raises(ValueError):
        ck.load_optimizer_state_dict(opt2, model, torch.optim.SGD(twin, lr=0.1).state_dict())


def test_sgd_state_round_trips_with_torch():
    from adyolo_amd import checkpoint as ck
    from adyolo_amd.dist import FlatParameters
    from adyolo_amd.train import FusedSGD
    model, twin = _model_and_twin(seed=4)
    flat = FlatParameters(model)
    # fused -> torch
    opt = FusedSGD(flat, lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    assert ck.optimizer_state_dict(opt, model)["state"] == {}              # before the first step: no buffers, like torch
    _fill(opt.momentum_buffer, flat, 7)
    opt.step_count = 3
    sd = ck.optimizer_state_dict(opt, model)
    assert list(sd["param_groups"][0]) == ["lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize", "foreach",
                                           "differentiable", "fused", "params"]
    assert all(list(st) == ["momentum_buffer"] for st in sd["state"].values())
    tw = torch.optim.SGD(twin, lr=1.0)
    tw.load_state_dict(sd)
    got = tw.state_dict()
    g = got["param_groups"][0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"]) == (0.05, 0.9, 0.1, 1e-4, False)
    for i, p in enumerate(model.parameters()):
        assert torch.equal(got["state"][i]["momentum_buffer"], _slice_of(flat, opt.momentum_buffer, p))
    # torch -> fused: buffers present = the first step is behind us
    ref = _two_cpu_steps(torch.optim.SGD(twin, lr=0.02, momentum=0.8, weight_decay=1e-3), twin)
    opt2 = FusedSGD(flat, momentum=0.9)
    assert opt2.first_step
    ck.load_optimizer_state_dict(opt2, model, ref)
    assert (opt2.lr, opt2.momentum, opt2.dampening, opt2.weight_decay, opt2.nesterov) == (0.02, 0.8, 0, 1e-3, False)
    assert not opt2.first_step and opt2.step_count == 1
    opt2.sync_device_step()
    assert int(opt2.step_dev) == 1                                        # the device-side flag derives from this counter
    for i, p in enumerate(model.parameters()):
        assert torch.equal(_slice_of(flat, opt2.momentum_buffer, p), ref["state"][i]["momentum_buffer"])
    # a state without buffers (a momentum run saved before its first step): the first step is still to come
    fresh = torch.optim.SGD(twin, lr=0.02, momentum=0.8).state_dict()
    assert fresh["state"] == {}
    ck.load_optimizer_state_dict(opt2, model, fresh)
    assert opt2.first_step and opt2.step_count == 0 and float(opt2.momentum_buffer.abs().sum()) == 0.0
    opt2.sync_device_step()
    assert int(opt2.step_dev) == 0
    # without momentum: no per-parameter state in either direction, nothing allocated
    plain = FusedSGD(flat, lr=0.1, weight_decay=0.01)
    plain.step_count = 2
    sd0 = ck.optimizer_state_dict(plain, model)
    assert sd0["state"] == {} and plain.momentum_buffer is None
    tw0 = torch.optim.SGD(twin, lr=1.0)
    tw0.load_state_dict(sd0)
    ck.load_optimizer_state_dict(plain, model, _two_cpu_steps(torch.optim.SGD(twin, lr=0.3, weight_decay=0.02), twin))
    assert (plain.lr, plain.weight_decay, plain.momentum) == (0.3, 0.02, 0) and plain.momentum_buffer is None
    with pytest.raises(ValueError):                                        # the buffer exists, or not, since construction
        ck.load_optimizer_state_dict(plain, model, ref)
    with pytest.raises(ValueError):
        ck.load_optimizer_state_dict(plain, model, torch.optim.Adam(twin).state_dict())


def test_parameter_count_mismatch_raises():
    from adyolo_amd import checkpoint as ck
    from adyolo_amd.train import FusedAdamW, FusedSGD
    net, flat = _small_flat()
    twin = [torch.nn.Parameter(p.detach().clone()) for p in net.parameters()][:-1]
    with pytest.raises(ValueError):
        ck.load_optimizer_state_dict(FusedAdamW(flat), net, torch.optim.AdamW(twin).state_dict())
    with pytest.raises(ValueError):
        ck.load_optimizer_state_dict(FusedSGD(flat, momentum=0.9), net, torch.optim.SGD(twin, lr=0.1, momentum=0.9).state_dict())


def test_fused_adam_state_dict_is_unchanged():
    """What FusedAdam writes does not change by a key (torch.optim.Adam's group as this build has always written it)."""
    from adyolo_amd.train import FusedAdam
    net, flat = _small_flat()
    opt = FusedAdam(flat, max_norm=3.0)                                    # clip_grad_norm is configuration, not state
    opt.step_count = 1
    sd = opt.state_dict()
    assert list(sd["param_groups"][0]) == ["lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable",
                                           "differentiable", "fused", "params"]
    assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
