"""CPU: parameter groups of the fused optimizers -- selection from ``train_config['param_groups']``, the group map, the
untouched ungrouped path, the torch.optim state_dict layout with more than one group, and ``lr_at(t, group)``.  No HIP call
is made: the state containers are filled by hand, the models live on the CPU (the pattern of test_optimizers_cpu)."""
import pytest
import torch

import adyolo_amd  # noqa: F401  (import shim at the repo root)


def _cpu_params(**train_config):
    tc = {"grid_size": [45, 45], "nb_anchors": 5, "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0}
    tc.update(train_config)
    return {"args": {"device": "cpu", "encoder": "se-resnet34", "loss": "adyolo"}, "data_config": {"nb_classes": 12},
            "train_config": tc}


def _small_flat(reverse=True):
    from adyolo_amd.dist import FlatParameters
    torch.manual_seed(5)
    net = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))      # 15 + 3 + 6 + 2 = 26 -> padded to 28
    return net, FlatParameters(net, reverse=reverse)


@pytest.fixture(scope="module")
def real():
    from adyolo_amd.dist import FlatParameters
    from adyolo_amd.wrapper import WrapperModel
    torch.manual_seed(3)
    model = WrapperModel((1, 7, 64, 64), (), _cpu_params())
    return model, FlatParameters(model)


def _resolve(entries, flat, lr=1e-3, wd=0.01):
    from adyolo_amd import param_groups
    return param_groups.resolve(entries, flat, lr, wd)


# ------------------------------------------------------------------------------------------------ selection
def test_names_follow_module_params():
    net, flat = _small_flat()
    assert flat.names == ["0.weight", "0.bias", "1.weight", "1.bias"]
    assert all(p is q for p, q in zip(flat.module_params, net.parameters()))


def test_selection_on_the_small_net():
    _, flat = _small_flat()
    assert _resolve(None, flat) is None and _resolve([], flat) is None
    # match alone; defaults of lr / weight_decay / name; the default group comes first
    g = _resolve([{"match": ["1.*"], "lr": 1e-4}], flat)
    assert g == [{"name": "default", "lr": 1e-3, "weight_decay": 0.01, "params": [0, 1]},
                 {"name": 0, "lr": 1e-4, "weight_decay": 0.01, "params": [2, 3]}]
    # ndim_max alone
    g = _resolve([{"name": "no_decay", "ndim_max": 1, "weight_decay": 0.0}], flat)
    assert [(x["name"], x["params"], x["weight_decay"]) for x in g] == [("default", [0, 2], 0.01), ("no_decay", [1, 3], 0.0)]
    # both selectors: AND
    g = _resolve([{"name": "b1", "match": ["1.*"], "ndim_max": 1}], flat)
    assert [(x["name"], x["params"]) for x in g] == [("default", [0, 1, 2]), ("b1", [3])]
    # the first entry that selects a parameter takes it
    g = _resolve([{"name": "bias", "match": ["*.bias"]}, {"name": "head", "match": ["1.*"]}], flat)
    assert [(x["name"], x["params"]) for x in g] == [("default", [0]), ("bias", [1, 3]), ("head", [2])]
    # an empty default group is dropped
    g = _resolve([{"name": "a", "match": ["0.*"], "lr": 0.0}, {"name": "b", "match": ["*"]}], flat)
    assert [(x["name"], x["params"], x["lr"]) for x in g] == [("a", [0, 1], 0.0), ("b", [2, 3], 1e-3)]


def test_selection_errors_name_the_entry():
    _, flat = _small_flat()
    for entries, word in (([{"name": "typo", "match": ["encoder.*"]}], "typo"),                   # selects nothing
                          ([{"name": "x", "match": ["*"], "momentum": 0.9}], "momentum"),         # unknown key
                          ([{"name": "second", "match": ["*"]}, {"name": "shadowed", "match": ["1.*"]}], "shadowed"),
                          ([{"name": "neg", "match": ["*"], "lr": -1e-3}], "neg"),
                          ([{"name": "nan", "match": ["*"], "weight_decay": float("nan")}], "nan"),
                          ([{"name": "inf", "match": ["*"], "lr": float("inf")}], "inf"),
                          ([{"match": ["*"], "weight_decay": -0.1}], "0")):
        with pytest.raises(ValueError) as e:
            _resolve(entries, flat)
        assert word in str(e.value), (entries, str(e.value))
    with pytest.raises(ValueError) as e:
        _resolve([{"name": "g%d" % k, "match": ["*"]} for k in range(16)], flat)
    assert "16" in str(e.value) and "15" in str(e.value)


def test_selection_on_the_real_model(real):
    model, flat = real
    g = _resolve([{"name": "no_decay", "ndim_max": 1, "weight_decay": 0.0}], flat)
    want = [i for i, p in enumerate(model.parameters()) if p.ndim <= 1]
    assert [x["name"] for x in g] == ["default", "no_decay"] and g[1]["params"] == want and 0 < len(want) < len(flat.names)
    assert g[0]["params"] == [i for i, p in enumerate(model.parameters()) if p.ndim > 1]
    names = [n for n, _ in model.named_parameters()]
    g = _resolve([{"name": "enc_small", "match": ["encoder.*"], "ndim_max": 1, "lr": 1e-5},
                  {"name": "enc", "match": ["encoder.*"], "lr": 1e-4}], flat)
    assert [x["name"] for x in g] == ["default", "enc_small", "enc"]
    assert g[1]["params"] == [i for i, (n, p) in enumerate(model.named_parameters()) if n.startswith("encoder.") and p.ndim <= 1]
    assert g[2]["params"] == [i for i, (n, p) in enumerate(model.named_parameters()) if n.startswith("encoder.") and p.ndim > 1]
    assert g[0]["params"] == [i for i, n in enumerate(names) if not n.startswith("encoder.")] and g[0]["params"]


# ------------------------------------------------------------------------------------------------ the map
def _check_map(flat, groups):
    from adyolo_amd import param_groups
    m = param_groups.group_map(groups, flat)
    assert m.dtype == torch.uint8 and m.shape == flat.flat.shape and m.device == flat.flat.device
    where = {id(p): k for k, p in enumerate(flat.params)}
    seen = 0
    for k, g in enumerate(groups):
        for i in g["params"]:
            off, n = flat.offsets[where[id(flat.module_params[i])]]
            assert bool((m[off:off + n] == k).all()), (k, i)
            seen += n
    assert seen == flat.numel and bool((m[flat.numel:] == 0).all())
    return m


@pytest.mark.parametrize("reverse", [True, False])
def test_group_map_small(reverse):
    _, flat = _small_flat(reverse)
    assert flat.flat.numel() == 28 and flat.numel == 26
    groups = _resolve([{"name": "bias", "match": ["*.bias"]}, {"name": "head", "match": ["1.*"]}], flat)
    m = _check_map(flat, groups)
    # reverse: 1.bias (2) 1.weight (6) 0.bias (3) 0.weight (15) + 2 of padding
    want = [1] * 2 + [2] * 6 + [1] * 3 + [0] * 15 + [0] * 2 if reverse else [0] * 15 + [1] * 3 + [2] * 6 + [1] * 2 + [0] * 2
    assert m.tolist() == want


def test_group_map_real_model(real):
    _, flat = real
    groups = _resolve([{"name": "no_decay", "ndim_max": 1, "weight_decay": 0.0}], flat)
    m = _check_map(flat, groups)
    runs = 1 + int((m[1:] != m[:-1]).sum())
    assert runs > 100                      # the rule cuts the buffer into many alternating runs, few on a float4 boundary


# ------------------------------------------------------------------------------------------------ no key: nothing changes
def test_without_the_key_nothing_changes():
    from adyolo_amd.train import FusedAdam, FusedAdamW, FusedSGD, get_optimizers
    _, flat = _small_flat()
    for tc, cls in (({}, FusedAdam), ({"optim": "AdamW", "param_groups": []}, FusedAdamW),
                    ({"optim": "SGD", "param_groups": None}, FusedSGD)):
        o = get_optimizers(_cpu_params(**tc), flat)
        assert type(o) is cls and o.groups is None and o.group_map is None and o.groups_dev is None and o.groups_out is None
        assert o.current_lrs is None and o.sched_dev is None and o.sched_out is None          # the plain entry points
        with pytest.raises(ValueError):
            o.set_weight_decay(0.1)
    o = get_optimizers(_cpu_params(lr_schedule={"name": "constant"}), flat)
    assert o.groups is None and o.group_map is None and o.sched_dev is not None
    o.set_lr(2e-3)                                                                            # as before, no group needed
    assert o.lr == 2e-3 and "group_base_lrs" not in o.sched_state_dict()
    with pytest.raises(ValueError):
        o.set_lr(2e-3, group=0)


def test_get_optimizers_passes_the_key_through():
    from adyolo_amd import ops
    from adyolo_amd.train import FusedAdamW, FusedSGD, get_optimizers
    _, flat = _small_flat()
    pg = [{"name": "no_decay", "ndim_max": 1, "weight_decay": 0.0, "lr": 1e-4}]
    o = get_optimizers(_cpu_params(optim="AdamW", lr=2e-3, weight_decay=1e-2, param_groups=pg), flat)
    assert type(o) is FusedAdamW and o.sched_config["name"] == "constant"                    # a constant schedule, like the EMA
    assert o.groups == [{"name": "default", "lr": 2e-3, "weight_decay": 1e-2, "params": [0, 2]},
                        {"name": "no_decay", "lr": 1e-4, "weight_decay": 0.0, "params": [1, 3]}]
    assert (o.lr, o.weight_decay) == (2e-3, 1e-2)
    assert o.groups_dev.dtype == torch.float64 and tuple(o.groups_dev.shape) == (2, 2)
    assert o.groups_dev.tolist() == [[2e-3, float(torch.tensor(1e-2, dtype=torch.float32))], [1e-4, 0.0]]
    assert o.groups_out.dtype == torch.float32 and tuple(o.groups_out.shape) == (2, ops.GROUP_OUT_FLOATS)
    assert tuple(o.current_lrs.shape) == (2,) and o.group_map.dtype == torch.uint8
    # set_lr / set_weight_decay rewrite the table, by index or by name; without a group they are refused
    with pytest.raises(ValueError):
        o.set_lr(1e-3)
    with pytest.raises(ValueError):
        o.set_weight_decay(0.0)
    with pytest.raises(ValueError):
        o.set_lr(1e-3, group="nobody")
    with pytest.raises(ValueError):
        o.set_lr(-1.0, group=1)
    o.set_lr(5e-4, group="no_decay")
    o.set_weight_decay(0.5, group=0)
    assert o.groups_dev.tolist() == [[2e-3, 0.5], [5e-4, 0.0]] and o.weight_decay == 0.5 and o.groups[1]["lr"] == 5e-4
    assert o.sched_state_dict()["group_base_lrs"] == [2e-3, 5e-4]
    o = get_optimizers(_cpu_params(optim="SGD", momentum=0.9, param_groups=pg), flat)
    assert type(o) is FusedSGD and [g["weight_decay"] for g in o.groups] == [0.0, 0.0] and o.groups[1]["lr"] == 1e-4
    with pytest.raises(ValueError):
        get_optimizers(_cpu_params(param_groups=[{"name": "typo", "match": ["encoder.*"]}]), flat)


# ------------------------------------------------------------------------------------------------ state-dict layout
def _twin_groups(net, groups, **extra):
    twin = [torch.nn.Parameter(p.detach().clone()) for p in net.parameters()]
    return twin, [dict({"params": [twin[i] for i in g["params"]], "lr": g["lr"], "weight_decay": g["weight_decay"]}, **extra)
                  for g in groups]


def _two_cpu_steps(opt, twin):
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        for p in twin:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt.state_dict()


def _slice_of(flat, buf, p):
    k = [id(q) for q in flat.params].index(id(p))
    off, n = flat.offsets[k]
    return buf[off:off + n].view(p.shape)


PG = [{"name": "no_decay", "ndim_max": 1, "weight_decay": 0.0, "lr": 1e-4}]


def _same_state_dict(a, b, tensors):
    assert sorted(a["state"]) == sorted(b["state"]) and len(a["param_groups"]) == len(b["param_groups"])
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert sorted(ga) == sorted(gb), (list(ga), list(gb))
        for k in ga:
            assert ga[k] == gb[k] or (k == "betas" and tuple(ga[k]) == tuple(gb[k])), (k, ga[k], gb[k])
    for i in a["state"]:
        assert sorted(a["state"][i]) == sorted(b["state"][i]) == sorted(tensors)
        for k in tensors:
            assert torch.equal(torch.as_tensor(a["state"][i][k]), torch.as_tensor(b["state"][i][k])), (i, k)


@pytest.mark.parametrize("which", ["small", "real"])
def test_adamw_grouped_state_round_trips_with_torch(which, real):
    from adyolo_amd import checkpoint as ck
    from adyolo_amd.train import FusedAdamW
    net, flat = _small_flat() if which == "small" else real
    groups = _resolve(PG, flat, lr=1e-3, wd=0.01)
    twin, tg = _twin_groups(net, groups)
    ref = _two_cpu_steps(torch.optim.AdamW(tg, betas=(0.85, 0.97), eps=1e-6), twin)
    assert [g["params"] for g in ref["param_groups"]][0][:2] == [0, 1] and len(ref["param_groups"]) == 2
    # other group values on the optimizer than in the file: the file's are taken
    mine = [dict(g, lr=g["lr"] * 3, weight_decay=0.5) for g in groups]
    opt = FusedAdamW(flat, param_groups=mine)
    ck.load_optimizer_state_dict(opt, net, ref)
    assert (opt.betas, opt.eps, opt.step_count) == ((0.85, 0.97), 1e-6, 2)
    assert [(g["lr"], g["weight_decay"]) for g in opt.groups] == [(1e-3, 0.01), (1e-4, 0.0)] and (opt.lr, opt.weight_decay) == (1e-3, 0.01)
    assert opt.groups_dev.tolist() == [[1e-3, float(torch.tensor(0.01, dtype=torch.float32))], [1e-4, 0.0]]
    ids = [i for g in groups for i in g["params"]]                       # torch's numbering: position k holds parameter ids[k]
    params = list(net.parameters())
    for k, i in enumerate(ids):
        assert torch.equal(_slice_of(flat, opt.exp_avg, params[i]), ref["state"][k]["exp_avg"])
        assert torch.equal(_slice_of(flat, opt.exp_avg_sq, params[i]), ref["state"][k]["exp_avg_sq"])
    assert float(opt.exp_avg[flat.numel:].abs().sum()) == 0.0
    # written back: torch's own dictionary again, and torch loads it
    out = ck.optimizer_state_dict(opt, net)
    _same_state_dict(out, ref, ("step", "exp_avg", "exp_avg_sq"))
    twin2, tg2 = _twin_groups(net, groups)
    fresh = torch.optim.AdamW(tg2)
    fresh.load_state_dict(out)
    _same_state_dict(fresh.state_dict(), ref, ("step", "exp_avg", "exp_avg_sq"))
    # a one-group file (an ungrouped run) into the grouped optimizer: state by position, the optimizer's group values stay
    twin1 = [torch.nn.Parameter(p.detach().clone()) for p in net.parameters()]
    one = _two_cpu_steps(torch.optim.AdamW(twin1, lr=7e-3, weight_decay=0.3), twin1)
    opt2 = FusedAdamW(flat, param_groups=mine)
    ck.load_optimizer_state_dict(opt2, net, one)
    assert [(g["lr"], g["weight_decay"]) for g in opt2.groups] == [(1e-3 * 3, 0.5), (1e-4 * 3, 0.5)] and opt2.step_count == 2
    for i, p in enumerate(params):
        assert torch.equal(_slice_of(flat, opt2.exp_avg, p), one["state"][i]["exp_avg"])
        assert torch.equal(_slice_of(flat, opt2.exp_avg_sq, p), one["state"][i]["exp_avg_sq"])


def test_sgd_grouped_state_round_trips_with_torch():
    from adyolo_amd import checkpoint as ck
    from adyolo_amd.train import FusedSGD
    net, flat = _small_flat()
    groups = _resolve(PG, flat, lr=0.02, wd=1e-3)
    twin, tg = _twin_groups(net, groups)
    ref = _two_cpu_steps(torch.optim.SGD(tg, lr=1.0, momentum=0.9), twin)
    opt = FusedSGD(flat, momentum=0.5, param_groups=[dict(g, lr=0.5) for g in groups])
    ck.load_optimizer_state_dict(opt, net, ref)
    assert [(g["lr"], g["weight_decay"]) for g in opt.groups] == [(0.02, 1e-3), (1e-4, 0.0)]
    assert (opt.momentum, opt.dampening, opt.nesterov, opt.step_count) == (0.9, 0, False, 1) and not opt.first_step
    ids = [i for g in groups for i in g["params"]]
    params = list(net.parameters())
    for k, i in enumerate(ids):
        assert torch.equal(_slice_of(flat, opt.momentum_buffer, params[i]), ref["state"][k]["momentum_buffer"])
    out = ck.optimizer_state_dict(opt, net)
    _same_state_dict(out, ref, ("momentum_buffer",))
    twin2, tg2 = _twin_groups(net, groups)
    fresh = torch.optim.SGD(tg2, lr=1.0, momentum=0.9)
    fresh.load_state_dict(out)
    _same_state_dict(fresh.state_dict(), ref, ("momentum_buffer",))
    # one-group file: by position, group values kept
    twin1 = [torch.nn.Parameter(p.detach().clone()) for p in net.parameters()]
    one = _two_cpu_steps(torch.optim.SGD(twin1, lr=0.3, momentum=0.9, weight_decay=0.2), twin1)
    opt2 = FusedSGD(flat, momentum=0.9, param_groups=[dict(g, lr=0.5) for g in groups])
    ck.load_optimizer_state_dict(opt2, net, one)
    assert [(g["lr"], g["weight_decay"]) for g in opt2.groups] == [(0.5, 1e-3), (0.5, 0.0)]
    for i, p in enumerate(params):
        assert torch.equal(_slice_of(flat, opt2.momentum_buffer, p), one["state"][i]["momentum_buffer"])


def test_mismatched_groupings_raise():
    from adyolo_amd import checkpoint as ck
    from adyolo_amd.train import FusedAdamW, FusedSGD
    net, flat = _small_flat()
    groups = _resolve(PG, flat)                                          # sizes [2, 2]
    twin = [torch.nn.Parameter(p.detach().clone()) for p in net.parameters()]
    other = torch.optim.AdamW([{"params": twin[:1]}, {"params": twin[1:], "weight_decay": 0.0}]).state_dict()       # [1, 3]
    with pytest.raises(ValueError) as e:
        ck.load_optimizer_state_dict(FusedAdamW(flat, param_groups=groups), net, other)
    assert "[1, 3]" in str(e.value) and "[2, 2]" in str(e.value)
    with pytest.raises(ValueError) as e:                                 # a grouped file into an ungrouped optimizer
        ck.load_optimizer_state_dict(FusedAdamW(flat), net, other)
    assert "[1, 3]" in str(e.value) and "[4]" in str(e.value)
    three = torch.optim.SGD([{"params": twin[:1]}, {"params": twin[1:2]}, {"params": twin[2:]}], lr=0.1, momentum=0.9).state_dict()
    with pytest.raises(ValueError):
        ck.load_optimizer_state_dict(FusedSGD(flat, momentum=0.9, param_groups=groups), net, three)
    with pytest.raises(ValueError):                                      # per-group betas are not expressible
        ck.load_optimizer_state_dict(FusedAdamW(flat, param_groups=groups), net, torch.optim.AdamW(
            [{"params": twin[:2]}, {"params": twin[2:], "betas": (0.5, 0.9)}]).state_dict())
    with pytest.raises(ValueError):                                      # the existing refusals stay
        ck.load_optimizer_state_dict(FusedAdamW(flat, param_groups=groups), net, torch.optim.SGD(
            [{"params": twin[:2]}, {"params": twin[2:]}], lr=0.1).state_dict())
    with pytest.raises(NotImplementedError):
        ck.load_optimizer_state_dict(FusedAdamW(flat, param_groups=groups), net, torch.optim.AdamW(
            [{"params": twin[:2]}, {"params": twin[2:]}], amsgrad=True).state_dict())


# ------------------------------------------------------------------------------------------------ lr_at(t, group)
KINDS = {"constant": {}, "step": {"gamma": 0.7, "step_size": 2}, "multistep": {"gamma": 0.3, "milestones": [2, 5]},
         "exponential": {"gamma": 0.93}, "cosine": {"T_max": 5, "eta_min": 1e-5}}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_lr_at_per_group(kind):
    from adyolo_amd import lr_schedule
    from adyolo_amd.train import FusedAdam
    _, flat = _small_flat()
    cfg = dict(KINDS[kind], name=kind, every=2, warmup_steps=3, warmup_start_factor=0.25)
    groups = [{"name": "a", "lr": 0.03, "weight_decay": 0.0, "params": [0]}, {"name": "b", "lr": 2e-3, "weight_decay": 0.1, "params": [1, 2]},
              {"name": "frozen", "lr": 0.0, "weight_decay": 0.0, "params": [3]}]
    opt = FusedAdam(flat, lr_schedule=cfg, param_groups=groups)
    tables = [lr_schedule.table(lr_schedule.normalise(cfg), g["lr"]) for g in groups[:2]]
    for t in range(1, 15):
        assert opt.lr_at(t) == opt.lr_at(t, group=0) == opt.lr_at(t, group="a") == lr_schedule.lr_at(tables[0], t)
        assert opt.lr_at(t, group=1) == opt.lr_at(t, group="b") == lr_schedule.lr_at(tables[1], t)
        assert opt.lr_at(t, group="frozen") == 0.0
    assert opt.lr_at(14, group=1) < opt.lr_at(4, group=1) or kind == "constant"
    opt.set_lr(1e-3, group="frozen")                                     # released
    tb = lr_schedule.table(lr_schedule.normalise(cfg), 1e-3)
    assert [opt.lr_at(t, group=2) for t in range(1, 15)] == [lr_schedule.lr_at(tb, t) for t in range(1, 15)]
    assert opt.groups_dev.tolist()[2] == [1e-3, 0.0]
    with pytest.raises(ValueError):
        opt.lr_at(1, group=3)
