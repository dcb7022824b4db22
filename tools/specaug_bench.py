"""SpecAug in the raw-audio train step: what the masks cost (device events around synchronised work, warmed up, repeated).

  features      FeatureExtractor at 64 x 60 s (T = 2400, the bench shape) without and with spec_ranges
  step          one hipGraph-replayed TrainStep at 16 x 20 s (the reference's batch_size / chunk, where --augment is used)
                without and with spec_ranges (a different table every step)
  mask_ranges   adyolo_mask_ranges on (64, 2400, 64, 8) in each library given by --mask-lib (e.g. a build of the parent commit
                and this one; default: the package's library), plus adyolo_mask_groups with the two FOA groups

  feat_augment  (--shift and / or --cutout) adyolo_feat_augment on the FOA features (64, 2400, 64, 8) and the MIC features
                (64, 800, 64, 32) next to adyolo_mask_groups on the same tensor: "stripes" = the worst-case SpecAug rows alone (no
                sample shifted), "shift" = every sample shifted and nothing masked, "all" = every sample shifted under the
                worst-case stripes and a 40 x 20 rectangle, "empty" = an all-zero table (the launch alone).  Each with its byte
                model (read + write of the moving quads' unmasked elements, write of every masked element) as achieved GB/s.
                The step then gets a third variant with the (B, 4, 4) tables.

Tables are the worst case of the reference's configuration (hyp_augmentation.yaml: mask params 40): every sample and group
masked with 40 frames and 40 bins.  Variants alternate inside each repeat; the median of the repeats is reported (ms per call).

  python tools/specaug_bench.py [--reps 7] [--iters 20] [--shift] [--cutout] [--mask-lib A.so --mask-lib B.so] [--json out.json]
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


def aug_tables(b, t, shift, cutout, stripes=True, seed=0, max_bins=5):
    """(b, 4, 4) int32: the worst-case SpecAug rows (or zeros), a 40-frame x 20-bin rectangle for every sample (``cutout``) and a
    shift of 1..max_bins bins either way for every sample (``shift``)."""
    g = torch.Generator().manual_seed(1000 + seed)
    tab = torch.zeros(b, 4, 4, dtype=torch.int32)
    if stripes:
        tab[:, :2] = worst_tables(b, t, seed=seed)
    if cutout:
        t0 = torch.randint(0, t - 40, (b,), generator=g)
        f0 = torch.randint(0, 64 - 20, (b,), generator=g)
        tab[:, 2] = torch.stack([t0, t0 + 40, f0, f0 + 20], -1).to(torch.int32)
    if shift:
        size = torch.randint(1, max_bins + 1, (b,), generator=g)
        tab[:, 3, 0] = (size * (2 * torch.randint(0, 2, (b,), generator=g) - 1)).to(torch.int32)
    return tab


def model_bytes(tab, t, c4, groups, shift_groups):
    """HBM bytes the table asks for: every masked element written (16 B per quad), every unmasked element of a moving quad read
    and written."""
    total = 0
    for row in tab.tolist():
        cut = torch.zeros(t, 64, dtype=torch.bool)
        cut[row[2][0]:row[2][1], row[2][2]:row[2][3]] = True
        in_group = [False] * c4
        for (q0, q1), (t0, t1, f0, f1), moves in zip(groups, row[:2], shift_groups):
            m = cut.clone()
            m[t0:t1] = True
            m[:, f0:f1] = True
            masked = int(m.sum())
            moving = moves and row[3][0] != 0
            total += (q1 - q0) * 16 * (masked + (2 * (t * 64 - masked) if moving else 0))
            for q in range(q0, q1):
                in_group[q] = True
        total += in_group.count(False) * 16 * int(cut.sum())
    return total


def bench_feat_augment(reps, iters, shift, cutout):
    from adyolo_amd import ops
    out = {}
    for name, (b, t, c, groups, moves) in {"foa_64x60s": (64, 2400, 8, ((0, 1), (1, 2)), (True, True)),
                                           "mic_64x20s": (64, 800, 32, ((0, 1), (1, 3)), (True, False))}.items():
        feat = torch.randn(b, t, 64, c, device="cuda:0")
        cases = {"empty": aug_tables(b, t, False, False, stripes=False),
                 "stripes": aug_tables(b, t, False, False)}
        if shift:
            cases["shift"] = aug_tables(b, t, True, False, stripes=False)
        if cutout:
            cases["cutout"] = aug_tables(b, t, False, True, stripes=False)
        cases["all"] = aug_tables(b, t, shift, cutout)
        dev = {k: v.to("cuda:0") for k, v in cases.items()}
        spec = dev["stripes"][:, :2].contiguous()
        fns = {"mask_groups": lambda: ops.mask_groups_(feat, spec, groups)}
        for k in cases:
            fns["feat_augment[%s]" % k] = (lambda k=k: ops.feat_augment_(feat, dev[k], groups, moves))
        for f in fns.values():
            for _ in range(3):
                f()
        med, runs = timed(fns, reps, iters)
        nbytes = {"mask_groups": model_bytes(cases["stripes"], t, c // 4, groups, (False, False))}
        nbytes.update({"feat_augment[%s]" % k: model_bytes(v, t, c // 4, groups, moves) for k, v in cases.items()})
        out[name] = {k: {"ms": med[k], "runs_ms": runs[k], "model_MB": round(nbytes[k] / 1e6, 1),
                         "model_GBps": round(nbytes[k] / 1e6 / med[k], 1) if nbytes[k] else None} for k in fns}
        del feat
    return out


def bench_step(reps, iters, shift=False, cutout=False):
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
    if shift or cutout:
        tables4 = [aug_tables(b, t, shift, cutout, seed=s) for s in range(8)]

        def augmented():
            k[0] += 1
            return tr.step(audio, target, spec_ranges=tables4[k[0] % len(tables4)])
        fns["augmented"] = augmented
    for f in fns.values():
        for _ in range(4):                     # eager warm-up, capture, replays
            f()
    torch.cuda.synchronize()
    assert tr.graphs is not None and tr.graphs.captures == len(fns), "expected one graph per variant"
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
    ap.add_argument("--only", choices=["features", "step", "mask_ranges", "feat_augment"], action="append")
    ap.add_argument("--shift", action="store_true", help="the frequency-shift rows: feat_augment, and a third variant of the step")
    ap.add_argument("--cutout", action="store_true", help="the cutout rows: feat_augment, and a third variant of the step")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "specaug_bench needs the GPU"
    import adyolo_amd  # noqa: F401
    from adyolo_amd import _lib
    libs = a.mask_lib or [_lib.LIB_PATH]
    only = a.only or (["features", "step", "mask_ranges"] + (["feat_augment"] if a.shift or a.cutout else []))
    res = {"libs": libs}
    if "features" in only:
        res["features_64x60s_ms"], res["features_runs"] = bench_features(a.reps, a.iters)
    if "step" in only:
        res["graph_step_16x20s_ms"], res["graph_step_runs"] = bench_step(a.reps, max(1, a.iters // 2), a.shift, a.cutout)
    if "mask_ranges" in only:
        res["mask_64x60s_ms"], res["mask_runs"] = bench_mask_ranges(libs, a.reps, a.iters)
    if "feat_augment" in only:
        assert a.shift or a.cutout, "feat_augment needs --shift and / or --cutout"
        res["feat_augment"] = bench_feat_augment(a.reps, a.iters, a.shift, a.cutout)
        for name, rows in res["feat_augment"].items():
            for k, v in rows.items():
                print(name, k, v["ms"], "ms", v["model_MB"], "MB", v["model_GBps"], "GB/s")
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
