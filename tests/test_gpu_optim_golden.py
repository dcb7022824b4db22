"""GPU: the fused optimizers' result bits, pinned to recorded sha256 digests (tests/golden/optim_digests.json).

The other optimizer tests compare the forms with each other (bit for bit) and with torch.optim (within a tolerance).  A slip
that moves every form alike in the last bit -- a lost contraction pragma, a reassociated ``grad_scale * clip_coef`` -- passes
all of them.  This file does not: one case per instantiation of the update kernels (Adam coupled / decoupled and SGD with /
without momentum, each plain, scheduled, scheduled + EMA, grouped, grouped + EMA: twenty), plus a binding clip per rule,
nesterov, dampening != 0 and a weight decay != 0 for coupled Adam and for ungrouped SGD (plain and scheduled); three steps
each (SGD's first-step buffer initialisation, the EMA's first-update copy and its first real update); after every step the
parameters, every state buffer, the EMA, ``st``, ``sched_out`` and ``groups_out`` go into one sha256.

Inputs are a closed-form integer hash (index * an odd constant + seed mod 2^32, the top 24 bits mapped to [-1, 1) exactly),
not an RNG stream.  Gradients are pushed away from zero so that ``max_norm`` 0.05 binds.  Scheduled forms run cosine with
warm-up; grouped forms three groups, one at rate 0, with boundaries at every offset mod 4, one float4 that holds three groups
and a tail that changes group: the one-group path, the per-element path and the tail's byte-wise lookup all run.

The fixture.  This file uses only the public ``ops`` names of the commit before the update kernels were merged into one per
rule, so it runs unchanged there: the fixture was recorded on that commit plus this one file, in one GPU run, with
``python tests/test_gpu_optim_golden.py --record``, and committed before the kernels were touched.  To re-record after a
toolchain change (a new compiler may round ``pow`` / ``cos`` in the prep kernel or ``sqrtf`` / the division differently): take
a commit at which the cross-form tests (test_gpu_optimizers, test_gpu_lr_schedule, test_gpu_param_groups) pass on the old and
on the new toolchain, record on the new one, and state the toolchain change in the commit that replaces the fixture.  Never
re-record to make a change of the kernels pass.

The set of keys in the fixture must equal the set of cases generated here: a missing or an extra key fails."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_digests.json")
STEPS = 3
GRAD_SCALE = 0.25
MAX_NORM = 0.05
EMA_DECAY = 0.9
BIG = 2048 * 256 * 4 + 5              # past OX_MAX_BLOCKS * OX_THREADS * 4: the grid-stride loop and the tail both run


# ------------------------------------------------------------------------------------------------ inputs
def _hash_pm1(n, seed):
    """float32 in [-1, 1): the top 24 bits of (i * 2654435761 + seed) mod 2^32, minus 2^23, over 2^23 (every step exact)"""
    u = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed)) & np.uint64(0xFFFFFFFF)
    return ((u >> np.uint64(8)).astype(np.int64) - (1 << 23)).astype(np.float32) / np.float32(1 << 23)


def _inputs(n):
    p0 = _hash_pm1(n, 0x9E3779B9)
    grads = []
    for k in range(STEPS):
        r = _hash_pm1(n, 0x7F4A7C15 + 0x01000193 * k)
        g = (r + np.where(r >= 0, np.float32(0.5), np.float32(-0.5))) * np.float32(4.0)       # |g * GRAD_SCALE| >= 0.5
        assert float(np.abs(g).min()) * GRAD_SCALE > 10 * MAX_NORM
        grads.append(torch.from_numpy(g).to(DEV))
    return torch.from_numpy(p0).to(DEV), grads


def _group_map(n):
    """three groups.  n = 5: one float4 with groups 0 | 1 | 2 | 2 and a tail element of group 1.  Else long runs (the one-group
    path), changes at offsets 1, 2, 3 and 0 mod 4, a float4 with three groups, and a tail that changes group."""
    if n == 5:
        return np.array([0, 1, 2, 2, 1], dtype=np.uint8)
    m = np.zeros(n, dtype=np.uint8)
    i, k, lengths = 0, 0, [100003, 7, 65537, 1, 299999]
    while i < n:
        m[i:i + lengths[k % 5]] = k % 3
        i += lengths[k % 5]
        k += 1
    m[101:202] = 1                    # starts at offset 1, ends at offset 2
    m[202:303] = 2                    # ends at offset 3
    m[303:400] = 1                    # ends on a float4 boundary
    m[500:504] = [0, 1, 2, 2]
    m[n - (n & 3):] = [2, 0, 1][:n & 3]
    return m


def _sched_table(ops, base, ema):
    """cosine, T_max 5, eta_min 1e-5, 2 warm-up steps from 0.25: the rate differs on each of the three steps"""
    tb = [0.0] * ops.SCHED_TABLE_DOUBLES
    tb[ops.SCHED_KIND] = float(ops.SCHED_KINDS["cosine"])
    tb[ops.SCHED_BASE] = base
    tb[ops.SCHED_EVERY] = 1.0
    tb[ops.SCHED_WARMUP] = 2.0
    tb[ops.SCHED_START] = 0.25
    tb[ops.SCHED_GAMMA] = 1.0
    tb[ops.SCHED_STEP_SIZE] = 1.0
    tb[ops.SCHED_T_MAX] = 5.0
    tb[ops.SCHED_ETA_MIN] = 1e-5
    tb[ops.SCHED_EMA_DECAY] = EMA_DECAY if ema else 0.0
    return torch.tensor(tb, dtype=torch.float64).to(DEV)


# ------------------------------------------------------------------------------------------------ cases
FORMS = ["plain", "sched", "sched_ema", "groups", "groups_ema"]
RULES = {"adam": dict(rule="adam", decoupled=False, weight_decay=0.0),
         "adamw": dict(rule="adam", decoupled=True, weight_decay=0.01),
         "sgd": dict(rule="sgd", momentum=0.0, weight_decay=0.0),
         "sgd_mom": dict(rule="sgd", momentum=0.9, weight_decay=0.0)}
CASES = {"%s_%s" % (r, f): dict(RULES[r], form=f) for r in RULES for f in FORMS}          # the twenty instantiations
CASES.update({
    "adam_plain_clip": dict(RULES["adam"], form="plain", clip=True),
    "sgd_mom_groups_clip": dict(RULES["sgd_mom"], form="groups", clip=True),
    "sgd_mom_sched_nesterov": dict(RULES["sgd_mom"], form="sched", nesterov=True),
    "sgd_mom_plain_dampening": dict(RULES["sgd_mom"], form="plain", dampening=0.1),
    "adam_plain_coupled_wd": dict(RULES["adam"], form="plain", weight_decay=0.01),
    "sgd_mom_plain_wd": dict(RULES["sgd_mom"], form="plain", weight_decay=0.01),          # SGD's decay outside the grouped forms
    "sgd_sched_wd": dict(RULES["sgd"], form="sched", weight_decay=0.01),
})
SIZES = {name: [5, 1027] for name in CASES}
SIZES["adamw_groups_ema"].append(BIG)
SIZES["sgd_mom_plain"].append(BIG)
KEYS = ["%s/n%d" % (name, n) for name in CASES for n in SIZES[name]]


def _digest(tensors):
    h = hashlib.sha256()
    for name, t in tensors:
        h.update(name.encode())
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def run_case(ops, key):
    """-> the STEPS digests of one case"""
    name, n = key.split("/n")
    case, n = CASES[name], int(n)
    form = case["form"]
    sgd, ema_on, grouped = case["rule"] == "sgd", form.endswith("_ema"), form.startswith("groups")
    base = 0.01 if sgd else 1e-3
    p, grads = _inputs(n)
    step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device=DEV)
    out = [("p", p), ("st", st)]
    if sgd:
        buf = torch.full_like(p, 123.0) if case["momentum"] != 0.0 else None                # (the first step does not read it)
        state = (buf,)
        out += [("buf", buf)] if buf is not None else []
        kw = dict(momentum=case["momentum"], dampening=case.get("dampening", 0.0), nesterov=case.get("nesterov", False))
    else:
        state = (torch.zeros_like(p), torch.zeros_like(p))
        out += [("exp_avg", state[0]), ("exp_avg_sq", state[1])]
        kw = dict(decoupled=case["decoupled"])
    kw["grad_scale"] = GRAD_SCALE
    if case.get("clip"):
        kw.update(partials=torch.zeros(ops.GRAD_SUMSQ_MAX_PARTS, dtype=torch.float64, device=DEV), max_norm=MAX_NORM)
    if form == "plain":
        fn = ops.sgd_step_dev if sgd else ops.adam_step_dev
        args = (step_dev, st)
        kw.update(lr=base, weight_decay=case["weight_decay"])
    else:
        sched_out = torch.zeros(ops.SCHED_OUT_FLOATS, device=DEV)
        ema = torch.full_like(p, -7.0) if ema_on else None                                  # (the first update does not read it)
        out += [("sched_out", sched_out)] + ([("ema", ema)] if ema_on else [])
        args = (step_dev, st, _sched_table(ops, base, ema_on), sched_out)
        if grouped:
            fn = ops.sgd_step_groups_dev if sgd else ops.adam_step_groups_dev
            groups_dev = torch.tensor([[base, 0.01], [base * 1.37, 0.0], [0.0, 0.02]], dtype=torch.float64).to(DEV)
            groups_out = torch.zeros(3, ops.GROUP_OUT_FLOATS, device=DEV)
            out += [("groups_out", groups_out)]
            args += (groups_dev, groups_out, torch.from_numpy(_group_map(n)).to(DEV), ema)
        else:
            fn = ops.sgd_step_sched_dev if sgd else ops.adam_step_sched_dev
            args += (ema,)
            kw.update(weight_decay=case["weight_decay"])
    digests = []
    for g in grads:
        fn(p, g, *state, *args, **kw)
        digests.append(_digest(out))
    assert int(step_dev) == STEPS
    if case.get("clip"):
        assert 0.0 < float(st[3]) < 1.0, "the clip did not bind"
    assert bool(torch.isfinite(p).all())
    return digests


# ------------------------------------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)["digests"]


def test_the_fixture_holds_exactly_the_generated_cases(recorded):
    assert len(CASES) == 27 and len(KEYS) == 56
    assert sorted(recorded) == sorted(KEYS), sorted(set(recorded) ^ set(KEYS))
    assert all(len(v) == STEPS and all(len(d) == 64 for d in v) for v in recorded.values())


@gpu
@pytest.mark.parametrize("key", KEYS)
def test_bits_are_the_recorded_ones(ops, recorded, key):
    assert key in recorded, "no recorded digest for %s" % key
    got = run_case(ops, key)
    assert got == recorded[key], (key, [a == b for a, b in zip(got, recorded[key])])


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_optim_golden.py --record")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    assert torch.cuda.is_available(), "recording needs the GPU"
    doc = {"what": "sha256 per step of the fused optimizers' buffers: tests/test_gpu_optim_golden.py",
           "digests": {key: run_case(_ops, key) for key in KEYS}}
    again = {key: run_case(_ops, key) for key in KEYS}
    assert again == doc["digests"], "two runs disagree: the digests are not deterministic"
    with open(FIXTURE, "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("recorded %d cases in %s" % (len(KEYS), FIXTURE))
