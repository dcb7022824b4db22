"""Optimizers and gradient clipping in the train step: what each choice costs (device events around synchronised work, warmed
up, repeated).

  step      one hipGraph-replayed TrainStep at 16 x 20 s (the reference's batch_size / chunk) and at 64 x 60 s (the bench shape)
            with 'Adam' (ops.adam_step_dev, the baseline), 'AdamW', 'SGD' (plain, as the reference calls it), 'Adam' with
            clip_grad_norm 3, 'Adam' under a device-side lr_schedule (ops.adam_step_sched_dev) and the same with ema_decay;
            'AdamW' under the schedule without and with the no-decay parameter grouping (ops.adam_step_groups_dev); 'Adam'
            behind the non-finite guard (skip_nonfinite, ops.adam_step_guard_dev) without and with clip_grad_norm 3; 'Adam'
            and the guarded clipped 'Adam' with accum_steps 4 (ops.adam_step_accum_dev: the mean over a cycle's four replays,
            three hold calls and one step)
  kernels   the optimizer launches alone on buffers of the real model's flat size (6.68 M floats): adam_step_dev (baseline),
            adamw_step_dev, sgd_step_dev without / with momentum, adam_step_dev with clipping, grad_norm_dev (sum of squares +
            prep); the scheduled forms adam / adamw / sgd_step_sched_dev (cosine with warm-up: the prep kernel's most expensive
            table) and the scheduled forms with the EMA in the update launch (two more streams); the grouped forms
            adam / adamw (+ EMA) / sgd_step_groups_dev with the real model's ``ndim_max: 1`` group map (150 runs), each beside
            its ungrouped scheduled counterpart; the guarded steps adam / adamw grouped + EMA / sgd_step_guard_dev without
            and with clipping, each beside the unguarded step of the same form without and with clipping (a guarded
            unclipped step should cost what the clipped one costs, a guarded clipped step the same again); the accumulating
            steps adam / adamw grouped + EMA (guarded, clipped) / sgd_step_accum_dev as a hold call (the accumulation pass, a
            one-workgroup prep and an update launch that returns at once; 12 bytes per element, 8 on a cycle's first call)
            and as a cycle's last call (the pass with the sum of squares fused in, then the step) -- the record is put at the
            wanted micro index by a 32-byte device copy in front of each call, timed alone as accum_record_preset

At 16 x 20 s the trainers live side by side and alternate inside each repeat; at 64 x 60 s they are built one after the
other (activations of one recorded step at a time).  The median of the repeats is reported (ms per call).

  python tools/optim_bench.py [--reps 7] [--iters 10] [--only step16] [--only step64] [--only kernels] [--json out.json]
"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

VARIANTS = {"adam": {"optim": "Adam"},
            "adamw": {"optim": "AdamW", "weight_decay": 0.01},
            "sgd": {"optim": "SGD"},
            "adam_clip3": {"optim": "Adam", "clip_grad_norm": 3.0},
            "adam_sched": {"optim": "Adam", "lr_schedule": {"name": "cosine", "T_max": 1000, "warmup_steps": 100}},
            "adam_sched_ema": {"optim": "Adam", "lr_schedule": {"name": "cosine", "T_max": 1000, "warmup_steps": 100},
                               "ema_decay": 0.999},
            "adamw_sched": {"optim": "AdamW", "weight_decay": 0.01,
                            "lr_schedule": {"name": "cosine", "T_max": 1000, "warmup_steps": 100}},
            "adamw_sched_groups": {"optim": "AdamW", "weight_decay": 0.01,
                                   "lr_schedule": {"name": "cosine", "T_max": 1000, "warmup_steps": 100},
                                   "param_groups": [{"name": "no_decay", "ndim_max": 1, "weight_decay": 0.0}]},
            "adam_guard": {"optim": "Adam", "skip_nonfinite": True},
            "adam_clip3_guard": {"optim": "Adam", "clip_grad_norm": 3.0, "skip_nonfinite": True},
            "adam_accum4": {"optim": "Adam", "accum_steps": 4},
            "adam_clip3_guard_accum4": {"optim": "Adam", "clip_grad_norm": 3.0, "skip_nonfinite": True, "accum_steps": 4}}


def timed(fns, reps, iters):
    """fns: {name: callable}; per repeat every variant runs ``iters`` times between two events, variants alternating ->
    {name: median ms per call}, {name: all repeats}."""
    out = {k: [] for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / iters)
    return {k: round(statistics.median(v), 4) for k, v in out.items()}, {k: [round(x, 4) for x in v] for k, v in out.items()}


def make_trainer(b, n, variant):
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.train import TrainStep
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    from __graft_entry__ import _params
    prm = _params()
    prm["train_config"].update(VARIANTS[variant])
    torch.manual_seed(0)
    model = WrapperModel((1, 7, n // 600, 64), (), prm).to("cuda:0")
    return TrainStep(model, WrapperCriterion(prm), FeatureExtractor(None, "cuda:0"), prm, graph=True)


def warm(tr, audio, target):
    for _ in range(4):                         # eager warm-up, capture, replays (accumulating: one whole cycle of 4)
        tr.step(audio, target)
    torch.cuda.synchronize()
    assert tr.graphs is not None and tr.graphs.captures == 1 and tr.graphs.replays >= 2, "the step was not recorded"


def bench_step(b, seconds, reps, iters, together):
    from adyolo_amd.datasets import synthetic_audio, synthetic_targets
    n = 24000 * seconds
    audio = synthetic_audio(b, n, seed=2).to("cuda:0")
    target = synthetic_targets(b, n // 2400, 12, seed=3)
    if together:
        trs = {v: make_trainer(b, n, v) for v in VARIANTS}
        for tr in trs.values():
            warm(tr, audio, target)
        return timed({v: (lambda tr=tr: tr.step(audio, target)) for v, tr in trs.items()}, reps, iters)
    med, runs = {}, {}
    for v in VARIANTS:
        tr = make_trainer(b, n, v)
        warm(tr, audio, target)
        m, r = timed({v: lambda: tr.step(audio, target)}, reps, iters)
        med.update(m)
        runs.update(r)
        del tr
        gc.collect()
        torch.cuda.empty_cache()
    return med, runs


def real_group_map():
    """the group map of the real model (se-resnet34 + BiGRU + the AD-YOLO head) under the no-decay rule ``ndim_max: 1``,
    built on the CPU: -> (uint8 map of the padded flat buffer on the GPU, number of runs)"""
    from adyolo_amd import param_groups
    from adyolo_amd.dist import FlatParameters
    from adyolo_amd.wrapper import WrapperModel
    from __graft_entry__ import _params
    flat = FlatParameters(WrapperModel((1, 7, 64, 64), (), _params("cpu")))
    groups = param_groups.resolve([{"name": "no_decay", "ndim_max": 1, "weight_decay": 0.0}], flat, 1e-3, 1e-2)
    m = param_groups.group_map(groups, flat)
    return m.to("cuda:0"), 1 + int((m[1:] != m[:-1]).sum())


def bench_kernels(reps, iters):
    from adyolo_amd import ops
    n = 6682096                                 # the flat buffer of se-resnet34 + the AD-YOLO head (6 682 093 padded to 4)
    g = torch.Generator().manual_seed(1)
    p = torch.randn(n, generator=g).to("cuda:0")
    grad = (torch.randn(n, generator=g) * 1e-2).to("cuda:0")
    m, v, buf = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    st = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, device="cuda:0")
    parts = torch.zeros(ops.GRAD_SUMSQ_MAX_PARTS, dtype=torch.float64, device="cuda:0")
    from adyolo_amd import lr_schedule
    cosine = lr_schedule.normalise({"name": "cosine", "T_max": 1000, "warmup_steps": 100})
    sched = torch.tensor(lr_schedule.table(cosine, 1e-3), dtype=torch.float64).to("cuda:0")
    sched_ema = torch.tensor(lr_schedule.table(cosine, 1e-3, ema_decay=0.999), dtype=torch.float64).to("cuda:0")
    out, ema = torch.zeros(ops.SCHED_OUT_FLOATS, device="cuda:0"), torch.zeros_like(p)
    gmap, runs = real_group_map()
    assert gmap.numel() == n, (gmap.numel(), n)
    print("group map: %d runs, %d elements in group 1" % (runs, int((gmap == 1).sum())))
    gdev = torch.tensor([[1e-3, 0.0], [1e-3, 0.0]], dtype=torch.float64).to("cuda:0")
    gdev_w = torch.tensor([[1e-3, float(torch.tensor(1e-2, dtype=torch.float32))], [1e-3, 0.0]], dtype=torch.float64).to("cuda:0")
    gout = torch.zeros(2, ops.GROUP_OUT_FLOATS, device="cuda:0")
    guard = torch.zeros(ops.OPTIM_GUARD_WORDS, dtype=torch.int64, device="cuda:0")
    form = dict(sched_dev=sched_ema, sched_out=out, ema=ema, groups_dev=gdev_w, groups_out=gout, group_map=gmap)
    # the accumulating steps: K = 4; the record is copied into place before each call: index 0 (a cycle's first call, which
    # overwrites), 1 (a hold call that adds) or 3 (the cycle's last call)
    accum = torch.zeros_like(p)
    acc = torch.zeros(ops.OPTIM_ACCUM_WORDS, dtype=torch.int64, device="cuda:0")
    at = {k: torch.tensor([k, 0, 0, 0], dtype=torch.int64, device="cuda:0") for k in (0, 1, 3)}

    def micro(index, fn, *args, **kw):
        def call():
            acc.copy_(at[index])
            fn(*args, accum, acc, 4, **kw)
        return call

    adam_args, sgd_args = (ops.adam_step_accum_dev, p, grad, m, v, step_dev, st), (ops.sgd_step_accum_dev, p, grad, None, step_dev, st)
    full = dict(guard=guard, partials=parts, max_norm=3.0, decoupled=True, **form)
    fns = {
        "accum_record_preset": lambda: acc.copy_(at[1]),
        "adam_step_accum_dev_first": micro(0, *adam_args),
        "adam_step_accum_dev_hold": micro(1, *adam_args),
        "adam_step_accum_dev_last": micro(3, *adam_args),
        "adam_step_accum_dev_clip_last": micro(3, *adam_args, partials=parts, max_norm=3.0),
        "adamw_step_accum_dev_guard_groups_ema_clip_hold": micro(1, *adam_args, **full),
        "adamw_step_accum_dev_guard_groups_ema_clip_last": micro(3, *adam_args, **full),
        "sgd_step_accum_dev_first": micro(0, *sgd_args),
        "sgd_step_accum_dev_hold": micro(1, *sgd_args),
        "sgd_step_accum_dev_last": micro(3, *sgd_args),
        "adam_step_guard_dev": lambda: ops.adam_step_guard_dev(p, grad, m, v, step_dev, st, guard, parts),
        "adam_step_guard_dev_clip": lambda: ops.adam_step_guard_dev(p, grad, m, v, step_dev, st, guard, parts, max_norm=3.0),
        "adamw_step_groups_dev_ema_clip": lambda: ops.adam_step_groups_dev(p, grad, m, v, step_dev, st, sched_ema, out, gdev_w,
                                                                           gout, gmap, ema, decoupled=True, partials=parts,
                                                                           max_norm=3.0),
        "adamw_step_guard_dev_groups_ema": lambda: ops.adam_step_guard_dev(p, grad, m, v, step_dev, st, guard, parts,
                                                                           decoupled=True, **form),
        "adamw_step_guard_dev_groups_ema_clip": lambda: ops.adam_step_guard_dev(p, grad, m, v, step_dev, st, guard, parts,
                                                                                max_norm=3.0, decoupled=True, **form),
        "sgd_step_dev_clip": lambda: ops.sgd_step_dev(p, grad, None, step_dev, st, partials=parts, max_norm=3.0),
        "sgd_step_guard_dev": lambda: ops.sgd_step_guard_dev(p, grad, None, step_dev, st, guard, parts),
        "sgd_step_guard_dev_clip": lambda: ops.sgd_step_guard_dev(p, grad, None, step_dev, st, guard, parts, max_norm=3.0),
        "adam_step_groups_dev": lambda: ops.adam_step_groups_dev(p, grad, m, v, step_dev, st, sched, out, gdev, gout, gmap),
        "adamw_step_groups_dev": lambda: ops.adam_step_groups_dev(p, grad, m, v, step_dev, st, sched, out, gdev_w, gout, gmap,
                                                                  decoupled=True),
        "adamw_step_sched_dev_ema": lambda: ops.adam_step_sched_dev(p, grad, m, v, step_dev, st, sched_ema, out, ema,
                                                                    weight_decay=1e-2, decoupled=True),
        "adamw_step_groups_dev_ema": lambda: ops.adam_step_groups_dev(p, grad, m, v, step_dev, st, sched_ema, out, gdev_w, gout,
                                                                      gmap, ema, decoupled=True),
        "sgd_step_groups_dev": lambda: ops.sgd_step_groups_dev(p, grad, None, step_dev, st, sched, out, gdev, gout, gmap),
        "adam_step_dev": lambda: ops.adam_step_dev(p, grad, m, v, step_dev, st),
        "adamw_step_dev": lambda: ops.adamw_step_dev(p, grad, m, v, step_dev, st),
        "sgd_step_dev": lambda: ops.sgd_step_dev(p, grad, None, step_dev, st),
        "sgd_step_dev_momentum": lambda: ops.sgd_step_dev(p, grad, buf, step_dev, st, momentum=0.9),
        "adam_step_dev_clip": lambda: ops.adam_step_dev(p, grad, m, v, step_dev, st, partials=parts, max_norm=3.0),
        "grad_norm_dev": lambda: ops.grad_norm_dev(grad, parts, st, 3.0),
        "adam_step_sched_dev": lambda: ops.adam_step_sched_dev(p, grad, m, v, step_dev, st, sched, out),
        "adamw_step_sched_dev": lambda: ops.adam_step_sched_dev(p, grad, m, v, step_dev, st, sched, out, weight_decay=1e-2,
                                                                decoupled=True),
        "sgd_step_sched_dev": lambda: ops.sgd_step_sched_dev(p, grad, None, step_dev, st, sched, out),
        "adam_step_sched_dev_ema": lambda: ops.adam_step_sched_dev(p, grad, m, v, step_dev, st, sched_ema, out, ema),
        "sgd_step_sched_dev_momentum_ema": lambda: ops.sgd_step_sched_dev(p, grad, buf, step_dev, st, sched_ema, out, ema,
                                                                          momentum=0.9),
    }
    for f in fns.values():
        for _ in range(3):
            f()
    return timed(fns, reps, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", choices=["step16", "step64", "kernels"], action="append")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "optim_bench needs the GPU"
    import adyolo_amd  # noqa: F401
    only = a.only or ["step16", "step64", "kernels"]
    res = {}
    if "kernels" in only:
        res["kernels_6p68M_ms"], res["kernels_runs"] = bench_kernels(a.reps, max(20, a.iters * 5))
    if "step16" in only:
        res["graph_step_16x20s_ms"], res["graph_step_16x20s_runs"] = bench_step(16, 20, a.reps, a.iters, together=True)
    if "step64" in only:
        res["graph_step_64x60s_ms"], res["graph_step_64x60s_runs"] = bench_step(64, 60, max(3, a.reps // 2), max(2, a.iters // 3),
                                                                              together=False)
    for k in ("kernels_6p68M_ms", "graph_step_16x20s_ms", "graph_step_64x60s_ms"):
        if k in res:
            print(k, res[k])
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
