"""SpecAug in the raw-audio train step: what the masks cost (device events around synchronised work, warmed up, repeated).

  features      FeatureExtractor at 64 x 60 s (T = 2400, the bench shape) without and with spec_ranges
  step          one hipGraph-replayed TrainStep at 16 x 20 s (the reference's batch_size / chunk, where --augment is used)
                without and with spec_ranges (a different table every step)
  mask_ranges   adyolo_mask_ranges on (64, 2400, 64, 8) in each library given by --mask-lib (e.g. a build of the parent commit
                and this one; default: the package's library), plus adyolo_mask_groups with the two FOA groups

Tables are the worst case of the reference's configuration (hyp_augmentation.yaml: mask params 40): every sample and group
masked with 40 frames and 40 bins.  Variants alternate inside each repeat; the median of the repeats is reported (ms per call).

  python tools/specaug_bench.py [--reps 7] [--iters 20] [--mask-lib A.so --mask-lib B.so] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def worst_tables(b, t, groups=2, width=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    t0 = torch.randint(0, t - width, (b, groups), generator=g)
    f0 = torch.randint(0, 64 - width, (b, groups), generator=g)
    return torch.stack([t0, t0 + width, f0, f0 + width], -1).to(torch.int32)


def timed(fns, reps, iters):
    """fns: {name: callable}; per repeat every variant runs ``iters`` times between two events, variants alternating ->
    {name: median ms per call}."""
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


def bench_features(reps, iters):
    from adyolo_amd.datasets import synthetic_audio
    from adyolo_amd.features import FeatureExtractor
    b, n = 64, 24000 * 60
    audio = synthetic_audio(b, n, seed=1).to("cuda:0")
    fx = FeatureExtractor(None, "cuda:0")
    r = worst_tables(b, n // 600).to("cuda:0")
    fns = {"plain": lambda: fx(audio), "masked": lambda: fx(audio, spec_ranges=r)}
    for f in fns.values():
        for _ in range(3):
            f()
    return timed(fns, reps, iters)


def bench_step(reps, iters):
    from adyolo_amd.datasets import synthetic_audio, synthetic_targets
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.train import TrainStep
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    from __graft_entry__ import _params
    b, n = 16, 24000 * 20
    t = n // 600
    prm = _params()
    torch.manual_seed(0)
    model = WrapperModel((1, 7, t, 64), (), prm).to("cuda:0")
    tr = TrainStep(model, WrapperCriterion(prm), FeatureExtractor(None, "cuda:0"), prm, graph=True)
    audio = synthetic_audio(b, n, seed=2).to("cuda:0")
    target = synthetic_targets(b, t // 4, 12, seed=3)
    tables = [worst_tables(b, t, seed=s) for s in range(8)]
    k = [0]

    def masked():
        k[0] += 1
        return tr.step(audio, target, spec_ranges=tables[k[0] % len(tables)])

    fns = {"plain": lambda: tr.step(audio, target), "masked": masked}
    for f in fns.values():
        for _ in range(4):                     # eager warm-up, capture, replays
            f()
    torch.cuda.synchronize()
    assert tr.graphs is not None and tr.graphs.captures == 2, "expected one graph per variant"
    return timed(fns, reps, iters)


def bench_mask_ranges(libs, reps, iters):
    b, t, f, c = 64, 2400, 64, 8
    feat = torch.randn(b, t, f, c, device="cuda:0")
    r1 = worst_tables(b, t, groups=1).to("cuda:0")
    r2 = worst_tables(b, t, groups=2).to("cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fp, p1, p2 = ctypes.c_void_p(feat.data_ptr()), ctypes.c_void_p(r1.data_ptr()), ctypes.c_void_p(r2.data_ptr())
    fns = {}
    for i, path in enumerate(libs):
        lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        fn = lib.adyolo_mask_ranges
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
        fns["mask_ranges[%d]" % i] = (lambda fn=fn: fn(fp, p1, b, t, f, c, stream))
        if hasattr(lib, "adyolo_mask_groups"):
            fg = lib.adyolo_mask_groups
            fg.restype = ctypes.c_int
            fg.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
            quads = (ctypes.c_int32 * 4)(0, 1, 1, 2)
            fns["mask_groups_foa[%d]" % i] = (lambda fg=fg, q=quads: fg(fp, p2, b, 2, t, f, c, ctypes.cast(q, ctypes.c_void_p), stream))
    for name, fn in fns.items():
        for _ in range(3):
            rc = fn()
            assert rc == 0, (name, rc)
    return timed(fns, reps, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mask-lib", action="append", default=[])
    ap.add_argument("--only", choices=["features", "step", "mask_ranges"], action="append")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "specaug_bench needs the GPU"
    import adyolo_amd  # noqa: F401
    from adyolo_amd import _lib
    libs = a.mask_lib or [_lib.LIB_PATH]
    only = a.only or ["features", "step", "mask_ranges"]
    res = {"libs": libs}
    if "features" in only:
        res["features_64x60s_ms"], res["features_runs"] = bench_features(a.reps, a.iters)
    if "step" in only:
        res["graph_step_16x20s_ms"], res["graph_step_runs"] = bench_step(a.reps, max(1, a.iters // 2))
    if "mask_ranges" in only:
        res["mask_64x60s_ms"], res["mask_runs"] = bench_mask_ranges(libs, a.reps, a.iters)
    for k in ("features_64x60s_ms", "graph_step_16x20s_ms", "mask_64x60s_ms"):
        if k in res:
            print(k, res[k])
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
