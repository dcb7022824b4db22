"""GPU: AdamW, SGD and gradient-norm clipping on the flat parameter buffer (csrc/optim.hip) against torch.optim /
torch.nn.utils.clip_grad_norm_ on the CPU; the whole train step with them, eager vs hipGraph replay (bit for bit); checkpoint
interchange with torch.optim.AdamW / torch.optim.SGD; two data-parallel ranks deriving the same clip coefficient.

Bounds: 1e-6 absolute on N(0,1) parameters (the bound of the project's two Adam tests); 1e-6 relative on the norm (float64
accumulation of fp32 squares is exact far below the 6e-8 rounding of the fp32 result)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _params(nb_classes=12, loss="adyolo", **train_config):
    tc = {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
          "conf_thresh": 0.5, "clss_thresh": 0.5, "unify_thresh": 15.0, "nms": "conn-merge",
          "loss_gains": {"angular_gain": 5.0, "object_gain": 1.0, "nonobj_gain": 5.0, "class_gain": 3.0},
          "optim": "Adam", "lr": 1e-3, "weight_decay": 0.0}
    tc.update(train_config)
    return {"args": {"device": "cuda:0", "encoder": "se-resnet34", "loss": loss},
            "data_config": {"nb_classes": nb_classes}, "train_config": tc}


def _trainer(graph, t=80, **train_config):
    from adyolo_amd.wrapper import WrapperModel, WrapperCriterion
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.train import TrainStep
    torch.manual_seed(100)
    prm = _params(**train_config)
    model = WrapperModel((1, 7, t, 64), (), prm).to("cuda:0")
    return TrainStep(model, WrapperCriterion(prm), FeatureExtractor(None, "cuda:0"), prm, graph=graph)


def _max_err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


# ------------------------------------------------------------------------------------------------ 3. kernels vs torch.optim
@pytest.mark.parametrize("n", [3, 4099, 10004])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_device_step_matches_torch(ops, n, wd):
    """adyolo_adam_step_dev (decoupled) against torch.optim.AdamW: 7 steps, gradients pre-multiplied by 4 with grad_scale 0.25;
    n = 4099 has a 3-element tail behind the 16-byte accesses, n = 3 is tail only (one workgroup, no float4 access)."""
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=g)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=wd)
    pg = p0.to("cuda:0")
    m, v = torch.zeros_like(pg), torch.zeros_like(pg)
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device="cuda:0")
    for _ in range(7):
        grad = torch.randn(n, generator=g)
        ref.grad = grad.clone()
        opt.step()
        ops.adamw_step_dev(pg, (grad * 4.0).to("cuda:0"), m, v, step_dev, st, lr=1e-3, weight_decay=wd, grad_scale=0.25)
    torch.cuda.synchronize()
    assert int(step_dev) == 7
    assert float(st[3]) == 1.0                                  # no clipping: the coefficient the update multiplies in is 1
    err = _max_err(pg, ref)
    print("adamw n=%d wd=%g: max |p - torch| = %.3e" % (n, wd, err))
    assert err <= 1e-6, err
    sd = opt.state_dict()["state"][0]
    assert _max_err(m, sd["exp_avg"]) <= 1e-6 and _max_err(v, sd["exp_avg_sq"]) <= 1e-6


SGD_FORMS = {"plain": {}, "wd": {"weight_decay": 0.01}, "momentum": {"momentum": 0.9},
             "nesterov": {"momentum": 0.9, "nesterov": True}, "dampening": {"momentum": 0.9, "dampening": 0.1}}


@pytest.mark.parametrize("n", [3, 4099, 10004])
@pytest.mark.parametrize("form", sorted(SGD_FORMS))
def test_sgd_device_step_matches_torch(ops, n, form):
    """adyolo_sgd_step_dev against torch.optim.SGD in five forms; the first step initialises the momentum buffer with the
    gradient (no dampening), as torch does; without momentum no buffer exists."""
    kw = SGD_FORMS[form]
    g = torch.Generator().manual_seed(4)
    p0 = torch.randn(n, generator=g)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([ref], lr=0.01, **kw)
    pg = p0.to("cuda:0")
    buf = torch.full_like(pg, 123.0) if kw.get("momentum") else None      # garbage: the first step must overwrite, not read, it
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device="cuda:0")
    for _ in range(7):
        grad = torch.randn(n, generator=g)
        ref.grad = grad.clone()
        opt.step()
        ops.sgd_step_dev(pg, (grad * 4.0).to("cuda:0"), buf, step_dev, st, lr=0.01, grad_scale=0.25, **kw)
    torch.cuda.synchronize()
    assert int(step_dev) == 7
    err = _max_err(pg, ref)
    print("sgd %s n=%d: max |p - torch| = %.3e" % (form, n, err))
    assert err <= 1e-6, err
    if buf is not None:
        berr = _max_err(buf, opt.state_dict()["state"][0]["momentum_buffer"])
        assert berr <= 1e-5, berr                               # (buffer values reach ~10: 1e-6 relative)


# ------------------------------------------------------------------------------------------------ 3b. pinned rounding
def _run_optimizer(ops, kind, p0, grads, n, clip=False):
    """3 steps of one optimizer on the first n elements of the given data; returns (p, state..., st) on the device"""
    pg = p0[:n].to("cuda:0")
    state = [torch.zeros_like(pg) for _ in range(1 if kind == "sgd" else 2)]
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device="cuda:0")
    kw = {"grad_scale": 0.25}
    if clip:
        kw.update(partials=torch.zeros(ops.GRAD_SUMSQ_MAX_PARTS, dtype=torch.float64, device="cuda:0"), max_norm=1e30)
    for gr in grads:
        gd = gr[:n].to("cuda:0")
        if kind == "sgd":
            ops.sgd_step_dev(pg, gd, state[0], step_dev, st, lr=0.01, weight_decay=0.01, momentum=0.9, **kw)
        else:
            ops.adam_step_dev(pg, gd, state[0], state[1], step_dev, st, lr=1e-3, weight_decay=0.01,
                              decoupled=kind == "adamw", **kw)
    torch.cuda.synchronize()
    assert int(step_dev) == len(grads)
    return [pg] + state + [st]


def _rounding_data(seed, n):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) * 4.0 for _ in range(3)]


@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
def test_body_and_tail_round_alike(ops, kind):
    """n = 4099 puts elements 4096..4098 in the scalar tail; the same data extended by one element to n = 4100 puts them in a
    float4.  Parameters and state of the first 4099 elements are equal bit for bit: the rounding is the source's, not the
    vectoriser's."""
    p0, grads = _rounding_data(31, 4100)
    tail = _run_optimizer(ops, kind, p0, grads, 4099)
    body = _run_optimizer(ops, kind, p0, grads, 4100)
    for name, a, b in zip(("p", "state0", "state1"), tail[:-1], body[:-1]):
        diff = (a != b[:4099]).nonzero().flatten().tolist()
        print("%s %s: elements that differ between tail and body: %r" % (kind, name, diff))
        assert torch.equal(a, b[:4099]), (kind, name, diff)
        assert float(a.abs().sum()) > 0.0


def test_a_clip_that_does_not_bind_changes_nothing(ops):
    """adam_step_dev with partials and max_norm = 1e30 (coefficient exactly 1.0) against adam_step_dev without: p, m, v equal
    bit for bit after 3 steps on n = 4099."""
    p0, grads = _rounding_data(32, 4099)
    plain = _run_optimizer(ops, "adam", p0, grads, 4099)
    clipped = _run_optimizer(ops, "adam", p0, grads, 4099, clip=True)
    assert float(clipped[-1][3]) == 1.0 and float(plain[-1][3]) == 1.0
    assert float(clipped[-1][2]) > 0.0                           # the norm was taken
    for name, a, b in zip("pmv", plain[:-1], clipped[:-1]):
        assert torch.equal(a, b), name


def test_misaligned_buffers_are_refused(ops):
    from adyolo_amd import _lib
    base = torch.zeros(4100, device="cuda:0")
    p, gr = torch.zeros(4096, device="cuda:0"), torch.zeros(4096, device="cuda:0")
    view = base[1:4097]                                         # 4 bytes past a 16-byte boundary
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device="cuda:0")
    with pytest.raises(_lib.AdyoloHipError):
        ops.sgd_step_dev(view, gr, None, step_dev, st)
    with pytest.raises(_lib.AdyoloHipError):
        ops.adamw_step_dev(p, view, torch.zeros_like(p), torch.zeros_like(p), step_dev, st)
    with pytest.raises(_lib.AdyoloHipError):
        ops.grad_sumsq(view, torch.zeros(ops.GRAD_SUMSQ_MAX_PARTS, dtype=torch.float64, device="cuda:0"))
    torch.cuda.synchronize()
    assert int(step_dev) == 0                                   # refused before anything was launched


# ------------------------------------------------------------------------------------------------ 4. norm
def _norm_case(ops, g_cpu, scale, max_norm=3.0):
    gd = g_cpu.to("cuda:0")
    parts = torch.zeros(ops.GRAD_SUMSQ_MAX_PARTS, dtype=torch.float64, device="cuda:0")
    st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device="cuda:0")
    ops.grad_norm_dev(gd, parts, st, max_norm, grad_scale=scale)
    torch.cuda.synchronize()
    first = (parts.clone(), st.clone())
    ops.grad_norm_dev(gd, parts, st, max_norm, grad_scale=scale)
    torch.cuda.synchronize()
    assert torch.equal(first[0], parts) and torch.equal(first[1], st), "two calls on the same buffer differ"
    ref = float(np.sqrt(np.sum((g_cpu.double().numpy() * scale) ** 2)))
    got = float(st[2])
    rel = abs(got - ref) / ref
    print("norm n=%d scale=%g: got %.9e, float64 %.9e, rel %.3e" % (g_cpu.numel(), scale, got, ref, rel))
    assert np.isfinite(got) and rel <= 1e-6, (got, ref, rel)
    coef = np.float32(max_norm) / (np.float32(got) + np.float32(1e-6))
    want = float(min(np.float32(1.0), coef))
    assert abs(float(st[3]) - want) <= 2e-7 * want, (float(st[3]), want)       # one fp32 division: within an ulp
    return got


@pytest.mark.parametrize("n", [4, 4099])
def test_grad_norm_matches_float64(ops, n):
    g = torch.Generator().manual_seed(n)
    _norm_case(ops, torch.randn(n, generator=g), 1.0)
    _norm_case(ops, torch.randn(n, generator=g) * 3.0, 0.25)


def test_grad_norm_at_the_real_model_size(ops):
    from adyolo_amd.dist import FlatParameters
    from adyolo_amd.wrapper import WrapperModel
    torch.manual_seed(100)
    flat = FlatParameters(WrapperModel((1, 7, 80, 64), (), _params()).to("cuda:0"))
    n = flat.flat_grad.numel()
    assert n % 4 == 0 and n >= flat.numel > 6_000_000
    assert ops.grad_sumsq_parts(n) == ops.GRAD_SUMSQ_MAX_PARTS
    g = torch.Generator().manual_seed(9)
    grad = torch.randn(n, generator=g) * 0.01
    grad[flat.numel:] = 0.0                                     # the padding of the flat buffer is zero
    _norm_case(ops, grad, 0.5)


def test_grad_norm_survives_squares_beyond_fp32(ops):
    """a few elements of 1e25: their squares overflow fp32, the float64 sum does not, and the norm (1.7e25) is an fp32 number"""
    g = torch.Generator().manual_seed(12)
    grad = torch.randn(4099, generator=g)
    grad[[5, 1000, 4098]] = 1e25
    got = _norm_case(ops, grad, 1.0)
    assert 1.7e25 < got < 1.8e25


# ------------------------------------------------------------------------------------------------ 5. clipping
class _Bag(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(4099, generator=g))          # 4099 + 6 = 4105 -> padded to 4108
        self.b = torch.nn.Parameter(torch.randn(2, 3, generator=g))


CLIP_SCALES = [1.0, 0.02, 0.5, 0.01, 2.0, 0.03]                 # ||N(0,1) x 4105|| ~ 64: three steps clip at max_norm 3, three do not


@pytest.mark.parametrize("name", ["Adam", "AdamW", "SGD"])
def test_clipped_step_matches_clip_grad_norm_and_torch(ops, name):
    from adyolo_amd.dist import FlatParameters
    from adyolo_amd.train import FusedAdam, FusedAdamW, FusedSGD
    bag = _Bag(21)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in bag.parameters()]
    bag = bag.to("cuda:0")
    flat = FlatParameters(bag)
    if name == "Adam":
        fused, ref = FusedAdam(flat, lr=1e-3, weight_decay=0.01, max_norm=3), torch.optim.Adam(twin, lr=1e-3, weight_decay=0.01)
    elif name == "AdamW":
        fused, ref = FusedAdamW(flat, lr=1e-3, weight_decay=0.01, max_norm=3), torch.optim.AdamW(twin, lr=1e-3, weight_decay=0.01)
    else:
        fused = FusedSGD(flat, lr=0.05, momentum=0.9, weight_decay=0.01, max_norm=3)
        ref = torch.optim.SGD(twin, lr=0.05, momentum=0.9, weight_decay=0.01)
    g = torch.Generator().manual_seed(22)
    clipped = []
    for k, s in enumerate(CLIP_SCALES):
        grads = [torch.randn(p.shape, generator=g) * s for p in twin]
        for p, gr in zip(twin, grads):
            p.grad = gr.clone()
        total = torch.nn.utils.clip_grad_norm_(twin, 3)
        clipped.append(float(total) > 3.0)
        ref.step()
        fused.zero_grad()
        for p, gr in zip(bag.parameters(), grads):
            p.grad.copy_((gr * 4.0).to("cuda:0"))
        fused.step(grad_scale=0.25)
        assert fused.grad_norm.is_cuda and tuple(fused.grad_norm.shape) == (1,)
        got = float(fused.grad_norm)
        rel = abs(got - float(total)) / float(total)
        print("%s step %d: norm %.7e torch %.7e rel %.2e clipped %s" % (name, k, got, float(total), rel, clipped[-1]))
        assert rel <= 1e-6, (k, got, float(total))
    assert sum(clipped) == 3 and len(clipped) == 6, clipped
    torch.cuda.synchronize()
    assert fused.step_count == 6 and int(fused.step_dev) == 6
    for p, q in zip(bag.parameters(), twin):
        err = _max_err(p, q)
        print("%s: max |p - torch| = %.3e" % (name, err))
        assert err <= 1e-6, err
    assert float(flat.flat[flat.numel:].abs().sum()) == 0.0     # the padding stayed zero


# ------------------------------------------------------------------------------------------------ 6. guard (passes on the parent too)
def test_adam_without_clip_key_is_the_adam_step_dev_path(ops):
    """'Adam' without ``clip_grad_norm``: six TrainStep steps, eager vs graph, parameters equal bit for bit, and the second
    moment equals a trainer whose optimizer step is ``ops.adam_step_dev`` called by hand."""
    from adyolo_amd.datasets import synthetic_audio, synthetic_targets
    from adyolo_amd.train import FusedAdam
    audios = [synthetic_audio(2, 24000 * 2, seed=70 + i).to("cuda:0") for i in range(3)]
    targets = [synthetic_targets(2, 20, 12, seed=80 + i) for i in range(6)]
    te, tg, th = _trainer(False), _trainer(True), _trainer(False)
    assert type(te.optimizer) is FusedAdam and getattr(te.optimizer, "max_norm", None) is None
    m, v = torch.zeros_like(th.flat.flat), torch.zeros_like(th.flat.flat)
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    bc = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device="cuda:0")

    def by_hand(grad_scale=1.0):
        ops.adam_step_dev(th.flat.flat, th.flat.flat_grad, m, v, step_dev, bc, 1e-3, (0.9, 0.999), 1e-8, 0.0, grad_scale)
        ops.params_changed()
    th.optimizer.step = by_hand
    for i in range(6):
        a = te.step(audios[i % 3], targets[i])
        b = tg.step(audios[i % 3], targets[i])
        c = th.step(audios[i % 3], targets[i])
        assert torch.equal(a, b) and torch.equal(a, c), i
    torch.cuda.synchronize()
    assert tg.graphs.captures == 1 and tg.graphs.replays == 5
    assert torch.equal(te.flat.flat, tg.flat.flat) and torch.equal(te.flat.flat, th.flat.flat)
    assert torch.equal(te.optimizer.exp_avg_sq, v) and torch.equal(tg.optimizer.exp_avg_sq, v)
    assert torch.equal(te.optimizer.exp_avg, m) and int(step_dev) == int(te.optimizer.step_dev) == 6


# ------------------------------------------------------------------------------------------------ 7. whole step, eager vs hipGraph
STEP_CONFIGS = {"adamw": {"optim": "AdamW", "weight_decay": 0.01},
                "sgd_momentum": {"optim": "SGD", "momentum": 0.9},
                "adam_clip": {"optim": "Adam", "clip_grad_norm": 3.0}}


def _state_tensors(opt):
    if opt.kind == "sgd":
        return [] if opt.momentum_buffer is None else [opt.momentum_buffer]
    return [opt.exp_avg, opt.exp_avg_sq]


@pytest.mark.parametrize("config", sorted(STEP_CONFIGS))
def test_graphed_train_step_is_bit_identical_to_eager(ops, config):
    """2 clips x 2 s, dropout on, target lists of different lengths, six steps: the recorded step (prep kernel, device step
    counter / first-step flag, norm partials, coefficient) replays to the same bits as the eager launches."""
    from adyolo_amd.datasets import synthetic_audio, synthetic_targets
    from adyolo_amd.train import FusedAdam, FusedAdamW, FusedSGD
    audios = [synthetic_audio(2, 24000 * 2, seed=70 + i).to("cuda:0") for i in range(3)]
    targets = [synthetic_targets(2, 20, 12, seed=80 + i) for i in range(6)]
    targets[3] = targets[3][: targets[3].shape[0] // 2].contiguous()
    assert len({t.shape[0] for t in targets}) > 1
    te, tg = _trainer(False, **STEP_CONFIGS[config]), _trainer(True, **STEP_CONFIGS[config])
    assert type(te.optimizer) is {"adamw": FusedAdamW, "sgd_momentum": FusedSGD, "adam_clip": FusedAdam}[config]
    assert tg.graphs is not None and te.graphs is None
    le, lg, ne, ng = [], [], [], []
    for i in range(6):
        le.append(te.step(audios[i % 3], targets[i]).clone())
        lg.append(tg.step(audios[i % 3], targets[i]).clone())
        if te.optimizer.grad_norm is not None:
            ne.append(te.optimizer.grad_norm.clone())
            ng.append(tg.optimizer.grad_norm.clone())
    torch.cuda.synchronize()
    assert tg.graphs.captures == 1 and tg.graphs.replays == 5 and tg.graphs.eager_steps == 1
    for i, (a, b) in enumerate(zip(le, lg)):
        assert torch.equal(a, b), "loss of step %d: eager %r graph %r" % (i, float(a), float(b))
    assert torch.equal(te.flat.flat, tg.flat.flat), "parameters after 6 steps"
    assert bool(torch.isfinite(te.flat.flat).all())
    for a, b in zip(_state_tensors(te.optimizer), _state_tensors(tg.optimizer)):
        assert torch.equal(a, b) and float(a.abs().sum()) > 0.0
    if config == "adam_clip":
        assert len(ne) == 6
        for i, (a, b) in enumerate(zip(ne, ng)):
            assert torch.equal(a, b) and float(a) > 0.0, "grad_norm of step %d: eager %r graph %r" % (i, float(a), float(b))
        print("grad norms:", [float(a) for a in ne])
    else:
        assert te.optimizer.grad_norm is None and tg.optimizer.grad_norm is None
    assert te.optimizer.step_count == tg.optimizer.step_count == 6
    assert int(tg.optimizer.step_dev) == 6 and int(te.optimizer.step_dev) == 6


# ------------------------------------------------------------------------------------------------ 8. checkpoints
@pytest.mark.parametrize("name", ["AdamW", "SGD"])
def test_resume_from_a_torch_checkpoint_continues_identically(ops, tmp_path, name):
    """A reference-side run (torch.optim.AdamW / torch.optim.SGD(momentum=0.9) on the CPU) checkpointed after 2 steps and
    resumed on the fused class takes the same third step."""
    from adyolo_amd import checkpoint as ck
    from adyolo_amd.dist import FlatParameters
    from adyolo_amd.train import FusedAdamW, FusedSGD
    from adyolo_amd.wrapper import WrapperModel
    torch.manual_seed(11)
    model = WrapperModel((1, 7, 64, 64), (), _params()).to("cuda:0")
    twin = [torch.nn.Parameter(p.detach().cpu().clone()) for p in model.parameters()]
    if name == "AdamW":
        ref = torch.optim.AdamW(twin, lr=1e-3, weight_decay=0.02)
    else:
        ref = torch.optim.SGD(twin, lr=0.01, momentum=0.9, dampening=0.1, weight_decay=1e-3)
    grads = [[torch.randn_like(p) for p in twin] for _ in range(3)]
    for s in range(2):
        for p, g_ in zip(twin, grads[s]):
            p.grad = g_.clone()
        ref.step()
    path = os.path.join(tmp_path, "model_ckpt.h5")
    msd = model.state_dict()
    for k, p in zip([k for k, _ in model.named_parameters()], twin):
        msd[k] = p.detach().clone()
    torch.save({"start_epoch_nb": 2, "model_state_dict": {k: v.cpu() for k, v in msd.items()},
                "optim_state_dict": ref.state_dict(), "confidence_thresh": 0.5, "rng_state": None, "best_log": {},
                "train_remaining_file": []}, path)
    flat = FlatParameters(model)
    opt = FusedAdamW(flat) if name == "AdamW" else FusedSGD(flat, momentum=0.5)
    ck.load_checkpoint(path, model, opt, device="cuda:0")
    if name == "AdamW":
        assert opt.step_count == 2 and opt.weight_decay == 0.02
    else:
        assert not opt.first_step and (opt.momentum, opt.dampening, opt.weight_decay) == (0.9, 0.1, 1e-3)
    for p, g_ in zip(model.parameters(), grads[2]):
        p.grad.copy_(g_.to("cuda:0"))
    opt.step()
    for p, g_ in zip(twin, grads[2]):
        p.grad = g_.clone()
    ref.step()
    torch.cuda.synchronize()
    worst = 0.0
    for (k, p), q in zip(model.named_parameters(), twin):
        err = _max_err(p, q)
        worst = max(worst, err)
        assert err <= 1e-6, "parameter %s after the resumed step: %.3e" % (k, err)
    print("%s: max |p - torch| after the resumed step = %.3e" % (name, worst))
    # and back: torch accepts what the fused optimizer writes after that step, state equal to its own
    back = ck.optimizer_state_dict(opt, model)
    key = "exp_avg" if name == "AdamW" else "momentum_buffer"
    mine = ref.state_dict()
    for i in mine["state"]:
        assert _max_err(back["state"][i][key], mine["state"][i][key]) <= 1e-5
    type(ref)(twin, lr=1.0).load_state_dict(back)


@pytest.mark.parametrize("config", ["adamw", "sgd_momentum"])
def test_graphed_step_survives_a_checkpoint_round_trip(ops, tmp_path, config):
    """Optimizer state restored from a checkpoint INTO a trainer that already holds a recorded graph: the device-side counter
    (and with it SGD's first-step flag) is re-synchronised from the host mirror and the next steps equal the eager run."""
    from adyolo_amd import checkpoint
    from adyolo_amd.datasets import synthetic_audio, synthetic_targets
    audio = synthetic_audio(2, 24000 * 2, seed=91).to("cuda:0")
    targets = [synthetic_targets(2, 20, 12, seed=92 + i) for i in range(6)]
    te, tg = _trainer(False, **STEP_CONFIGS[config]), _trainer(True, **STEP_CONFIGS[config])
    for i in range(3):
        te.step(audio, targets[i])
        tg.step(audio, targets[i])
    path = str(tmp_path / "model_ckpt.h5")
    checkpoint.save_checkpoint(path, te.model, te.optimizer, 1, 0.5, {}, [], "cuda:0")
    for i in range(3, 5):                                                     # the graph trainer runs ahead ...
        tg.step(audio, targets[i])
    checkpoint.load_checkpoint(path, tg.model, tg.optimizer, device="cuda:0")      # ... and is rolled back to step 3
    if config == "adamw":
        assert tg.optimizer.step_count == 3
    else:
        assert not tg.optimizer.first_step
    for i in range(3, 6):
        a, b = te.step(audio, targets[i]), tg.step(audio, targets[i])
        assert torch.equal(a, b), i
    assert tg.graphs.captures == 1
    assert torch.equal(te.flat.flat, tg.flat.flat)
    for a, b in zip(_state_tensors(te.optimizer), _state_tensors(tg.optimizer)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 9. two ranks
_CLIP2_CHILD = r"""
import hashlib, json, os, sys
sys.path.insert(0, os.environ["ADYOLO_REPO"])
import numpy as np
import torch
import torch.distributed as dist
import adyolo_amd
import bench
from adyolo_amd import dist as adist
from adyolo_amd.wrapper import WrapperModel, WrapperCriterion
from adyolo_amd.features import FeatureExtractor
from adyolo_amd.datasets import synthetic_audio, synthetic_targets
from adyolo_amd.train import TrainStep

b, n = 2, 24000 * 4                                     # clips per rank
MAX_NORM = float(os.environ["ADYOLO_CLIP2_MAX_NORM"])


def digest(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


rank, world, _ = adist.init_from_env("gloo")            # RCCL refuses two ranks on one device; gloo stages through the host
try:
    probe = torch.ones(4, device="cuda:0")
    dist.all_reduce(probe)
    assert float(probe[0]) == world
except Exception as exc:                                # a gloo build without device-tensor support
    print(json.dumps({"skip": repr(exc)[:300]}))
    sys.exit(0)
torch.manual_seed(100)
prm = bench.params("cuda:0")
prm["train_config"]["optim"] = "Adam"
prm["train_config"]["clip_grad_norm"] = MAX_NORM
model = WrapperModel((1, 7, n // 600, 64), (), prm).to("cuda:0")
model.encoder.lstm.dropout = 0.0
tr = TrainStep(model, WrapperCriterion(prm), FeatureExtractor(None, "cuda:0"), prm)
audio = synthetic_audio(b, n, seed=30 + rank).to("cuda:0")
target = synthetic_targets(b, n // 2400, 12, seed=40 + rank).to("cuda:0")
seen = []
opt_step = tr.optimizer.step


def spy(grad_scale=1.0):                                # the reduced gradients as the optimizer sees them, and their scale
    if not seen:
        g64 = tr.flat.flat_grad.detach().cpu().double().numpy() * grad_scale
        seen.append((float(np.sqrt(np.sum(g64 * g64))), grad_scale))
    opt_step(grad_scale=grad_scale)


tr.optimizer.step = spy
norms, bits, params = [], [], []
for _ in range(3):
    tr.step(audio, target)
    gn = tr.optimizer.grad_norm.detach().cpu()
    norms.append(float(gn))
    bits.append(int(gn.view(torch.int32)))
    params.append(digest(tr.flat.flat))
torch.cuda.synchronize()
print(json.dumps({"rank": rank, "world": world, "active": tr.reducer.active, "norms": norms, "bits": bits, "params": params,
                  "ref_norm0": seen[0][0], "grad_scale": seen[0][1], "optimizer": type(tr.optimizer).__name__,
                  "max_norm": tr.optimizer.max_norm}))
dist.barrier()
dist.destroy_process_group()
"""


def test_two_ranks_derive_the_same_clip_coefficient(ops):
    """Two real ranks (fresh processes, both on this GPU, gloo) run 3 clipped Adam steps on different half batches: the norm
    is taken of the reduced, averaged gradient every rank holds, summed in a fixed order -- both ranks report bit-identical
    ``grad_norm`` values and parameters after every step, with no collective beyond the gradient all-reduce; the first norm
    equals the float64 norm of the averaged gradient."""
    import json
    import socket
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    max_norm = 0.05
    base = dict(os.environ, ADYOLO_REPO=repo, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0",
                ADYOLO_CLIP2_MAX_NORM=repr(max_norm))
    base.pop("ADYOLO_FORCE_DP_HOOKS", None)
    base.pop("ADYOLO_DP_EXACT", None)
    procs = [subprocess.Popen([sys.executable, "-c", _CLIP2_CHILD], env=dict(base, WORLD_SIZE="2", RANK=str(r), LOCAL_RANK="0"),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, e[-3000:]
        outs.append(json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1]))
    if any("skip" in o for o in outs):
        pytest.skip("gloo cannot reduce device tensors in this build: %r" % outs)
    outs.sort(key=lambda o: o["rank"])
    print(outs)
    for o in outs:
        assert o["world"] == 2 and o["active"] and o["optimizer"] == "FusedAdam" and o["max_norm"] == max_norm
        assert o["grad_scale"] == 0.5                                         # the averaged gradient
        assert all(np.isfinite(v) and v > max_norm for v in o["norms"]), o["norms"]     # every step clipped
    assert outs[0]["bits"] == outs[1]["bits"], "grad_norm differs between the ranks"
    assert outs[0]["params"] == outs[1]["params"], "ranks diverged"
    assert len(set(outs[0]["params"])) == 3
    for o in outs:
        rel = abs(o["norms"][0] - o["ref_norm0"]) / o["ref_norm0"]
        assert rel <= 1e-6, (o["norms"][0], o["ref_norm0"], rel)
