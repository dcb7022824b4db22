"""Golden vectors of the class-wise evaluation path (``--loss seddoa | masked-seddoa | accdoa | adpit``) from the REAL
reference (build container only; the reference's ``LabelPostProcessor`` imports there under make_golden.py's shims).

Run:  python tests/golden/make_golden_classwise.py        (needs /root/reference; never runs on the GPU box)

Writes
  * ``postprocess_classwise.npz``: planted outputs of the seddoa / accdoa / adpit heads (C = 12 and 13, 16 frames) and the
    rows ``[frame, class, x, y, z]`` of the reference's ``LabelPostProcessor.postprocess`` for conf thresholds 0.1 .. 0.9 (and
    1.0 for accdoa / adpit, where the reference's double threshold test keeps only unified rows) and, for adpit, unify
    thresholds 15 / 30 / 45.  Every activity is at least 1e-4 away from every tested threshold and every pair distance at
    least 0.1 degree away from 15 / 30 / 45, so that the fp32 decode of the code under test decides the same way.
  * ``seld_chain_adpit.npz``: the whole reference chain with ``loss='adpit'``, built like ``gen_seld_chain``.
Only data is stored, nothing of the reference's source.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                  # noqa: E402  (puts the repository root and the reference on sys.path)

CONF = np.arange(0.1, 1.0, 0.1)
HIGH = 1.0                                # a threshold >= 1 (accdoa / adpit)
UNIFY = (15.0, 30.0, 45.0)
T = 16


def _params(loss, nb_classes):
    prm = mg.make_params(nb_classes)
    prm["args"]["loss"] = loss
    return prm


def _act(x, y, z):
    x, y, z = (np.asarray(v, dtype=np.float32) for v in (x, y, z))
    return np.sqrt(x ** 2 + y ** 2 + z ** 2)


def _dist64(a, b):
    a = a / np.linalg.norm(a)
    b = b / np.linalg.norm(b)
    return float(np.degrees(np.arccos(np.clip(np.dot(a, b), -1.0, 1.0))))


def _safe_act(v, thresholds):
    return bool(np.all(np.abs(float(v) - np.asarray(thresholds)) >= 1e-4))


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _rotate_towards(a, angle_deg, rng):
    """a unit vector at exactly ``angle_deg`` from unit vector ``a`` (random azimuth around it)."""
    p = rng.normal(size=3)
    p -= np.dot(p, a) * a
    p /= np.linalg.norm(p)
    t = np.radians(angle_deg)
    return np.cos(t) * a + np.sin(t) * p


def planted_seddoa(rng, c):
    out = np.zeros((1, T, 4 * c), dtype=np.float32)
    for f in range(T):
        for k in range(c):
            while True:
                a = np.float32(rng.uniform(0.0, 1.0))
                if _safe_act(a, CONF):
                    break
            out[0, f, k] = a
            out[0, f, c + k::c][:3] = rng.uniform(-1.0, 1.0, size=3).astype(np.float32)
    return out


def _track(rng, direction, thresholds):
    """xyz (float32) of norm drawn so that the float32 activity is clear of every threshold."""
    while True:
        r = rng.choice([rng.uniform(0.0, 0.09), rng.uniform(0.1, 1.4)])
        v = (direction * r).astype(np.float32)
        if _safe_act(_act(*v), thresholds):
            return v


def planted_accdoa(rng, c):
    out = np.zeros((1, T, 3 * c), dtype=np.float32)
    for f in range(T):
        for k in range(c):
            v = _track(rng, _unit(rng), list(CONF) + [HIGH])
            out[0, f, k], out[0, f, c + k], out[0, f, 2 * c + k] = v
    return out


# adpit cases per (frame, class): directions of the three tracks and which of them are active
CASES = ("inactive", "random", "pair01", "pair12", "pair20", "two_pairs", "all_three", "pair_25deg", "pair_40deg")


def _adpit_dirs(rng, case):
    a = _unit(rng)
    far = lambda: _unit(rng)                                                           # noqa: E731
    if case in ("inactive", "random"):
        return [a, far(), far()]
    if case == "pair01":
        return [a, _rotate_towards(a, rng.uniform(1.0, 12.0), rng), far()]
    if case == "pair12":
        return [far(), a, _rotate_towards(a, rng.uniform(1.0, 12.0), rng)]
    if case == "pair20":
        return [_rotate_towards(a, rng.uniform(1.0, 12.0), rng), far(), a]
    if case == "two_pairs":                        # 0-1 and 1-2 close, 2-0 about twice as far (beyond 15 deg)
        b = _rotate_towards(a, 10.0, rng)
        return [a, b, b + (b - a)]
    if case == "all_three":
        return [a, _rotate_towards(a, rng.uniform(1.0, 5.0), rng), _rotate_towards(a, rng.uniform(1.0, 5.0), rng)]
    if case == "pair_25deg":                       # unified at 30 and 45, not at 15
        return [a, _rotate_towards(a, 25.0, rng), far()]
    if case == "pair_40deg":                       # unified at 45 only
        return [far(), a, _rotate_towards(a, 40.0, rng)]
    raise ValueError(case)


def planted_adpit(rng, c):
    out = np.zeros((1, T, 9 * c), dtype=np.float32)
    cases = np.empty((T, c), dtype=object)
    thr = list(CONF) + [HIGH]
    for f in range(T):
        for k in range(c):
            case = CASES[(f * c + k) % len(CASES)] if rng.random() < 0.8 else "random"
            while True:
                dirs = [d / np.linalg.norm(d) for d in _adpit_dirs(rng, case)]
                if case == "inactive":
                    vs = [(d * rng.uniform(0.0, 0.09)).astype(np.float32) for d in dirs]
                else:
                    vs = [_track(rng, d, thr) for d in dirs]
                    if rng.random() < 0.7:         # mostly clearly active tracks, so that the pair cases are reached
                        vs = [(d * rng.uniform(0.95, 1.35)).astype(np.float32) for d in dirs]
                acts = [_act(*v) for v in vs]
                if not all(_safe_act(a, thr) for a in acts):
                    continue
                ds = [_dist64(vs[0], vs[1]), _dist64(vs[1], vs[2]), _dist64(vs[2], vs[0])]
                if all(abs(d - u) >= 0.1 for d in ds for u in UNIFY):
                    break
            for t, v in enumerate(vs):
                for ax in range(3):
                    out[0, f, (3 * t + ax) * c + k] = v[ax]
            cases[f, k] = case
    return out, cases


def _coverage(out, c):
    """the unify situations reached by a planted adpit output (own float64 arithmetic, a check of the plant only)."""
    v = out[0].reshape(T, 3, 3, c).transpose(0, 3, 1, 2).astype(np.float64)      # [T][C][track][xyz]
    act = np.sqrt((v ** 2).sum(-1))
    seen = set()
    for th in list(CONF) + [HIGH]:
        sed = act > th
        for u in UNIFY:
            for f in range(T):
                for k in range(c):
                    pairs = []
                    for (i, j) in ((0, 1), (1, 2), (2, 0)):
                        pairs.append(bool(sed[f, k, i] and sed[f, k, j] and _dist64(v[f, k, i], v[f, k, j]) < u))
                    n = sum(pairs)
                    if n == 0 and sed[f, k].any():
                        seen.add("none")
                    if n == 0 and not sed[f, k].all():
                        seen.add("inactive")
                    if n == 1:
                        seen.add("single%d" % pairs.index(True))
                    if n == 2:
                        seen.add("two")
                    if n == 3:
                        seen.add("three")
                    if n >= 1 and th >= 1.0:
                        seen.add("unified_at_high")
                    if u == 45.0 and n >= 1:
                        for (i, j) in ((0, 1), (1, 2), (2, 0)):
                            d = _dist64(v[f, k, i], v[f, k, j])
                            if sed[f, k, i] and sed[f, k, j] and 15.0 < d < 45.0:
                                seen.add("45_not_15")
    return seen


def _ref_rows(pp, out):
    res = pp.postprocess(torch.from_numpy(out.copy()))
    rows = [[fr, float(d[0])] + [float(x) for x in d[1:]] for fr, dets in res.items() for d in dets]
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), 5)


def _np_decode(output):
    from classwise_decode_np import decode
    return decode(output.numpy(), "adpit", 12)


def gen_postprocess_classwise():
    from datasets import LabelPostProcessor
    rng = np.random.default_rng(2024)
    out = {"conf_thresholds": CONF, "high_thresh": np.asarray(HIGH), "unify_thresholds": np.asarray(UNIFY)}
    for c in (12, 13):
        planted = {"seddoa": planted_seddoa(rng, c), "accdoa": planted_accdoa(rng, c)}
        planted["adpit"], _ = planted_adpit(rng, c)
        cov = _coverage(planted["adpit"], c)
        need = {"none", "inactive", "single0", "single1", "single2", "two", "three", "unified_at_high", "45_not_15"}
        assert need <= cov, need - cov
        for loss, o in planted.items():
            out["out_%s_C%d" % (loss, c)] = o
            pp = LabelPostProcessor(_params(loss, c))
            ths = list(CONF) + ([] if loss == "seddoa" else [HIGH])
            for i, th in enumerate(ths):
                pp.conf_thresh = th
                for u in (UNIFY if loss == "adpit" else (None,)):
                    key = "rows_%s_C%d_t%d" % (loss, c, i) + ("" if u is None else "_u%d" % int(u))
                    if u is not None:
                        pp.unify_thresh = u
                    out[key] = _ref_rows(pp, o)
            print("postprocess_classwise C=%d %s: rows per threshold %s" % (
                c, loss, [len(out["rows_%s_C%d_t%d" % (loss, c, i) + ("_u15" if loss == "adpit" else "")]) for i in range(len(ths))]))
    np.savez_compressed(os.path.join(HERE, "postprocess_classwise.npz"), **out)


def gen_seld_chain_adpit():
    """``gen_seld_chain`` with ``loss='adpit'``: WAV files + DCASE metadata -> reference ``Dataset('test')`` with the default
    collate -> ``WrapperModel`` (se-resnet34 + ADPIT head, filler weights, eval mode) -> ``WrapperCriterion`` ->
    ``LabelPostProcessor`` -> CSVs -> ``ComputeSELDResults``.  The conf and unify thresholds sit in wide gaps of the track
    activities and pair distances; the rows must be stable under 1e-3 output noise before anything is written."""
    import shutil
    import scipy.io.wavfile as wavfile
    from torch.utils.data import DataLoader
    mg._install_torchvision_stub()
    mg._oracle_stft_shims()
    import datasets as ref_datasets
    from wrapper import WrapperModel, WrapperCriterion
    from utils.seld_metrics import ComputeSELDResults
    from seld_chain_inputs import CLIPS, chain_clip, crc
    tmp = os.path.join(HERE, "_chain_adpit_tmp")
    shutil.rmtree(tmp, ignore_errors=True)
    wdir, cdir = os.path.join(tmp, "foa_dev", "dev-test"), os.path.join(tmp, "metadata_dev", "dev-test")
    odir = os.path.join(tmp, "output_test")
    os.makedirs(wdir), os.makedirs(cdir)
    shutil.copy("/root/reference/data/DCASE2021_SELD/scaler_wts.pkl", os.path.join(tmp, "scaler_wts.pkl"))
    out = {"names": np.asarray([cl[0] for cl in CLIPS]), "seeds": np.asarray([cl[1] for cl in CLIPS]),
           "n_samples": np.asarray([cl[2] for cl in CLIPS])}
    crcs = []
    for name, seed, n in CLIPS:
        pcm = chain_clip(seed, n)
        crcs.append(crc(pcm))
        wavfile.write(os.path.join(wdir, name + ".wav"), 24000, pcm)
        open(os.path.join(cdir, name + ".csv"), "w").close()          # pass 1: no events yet
    out["crc32"] = np.asarray(crcs, dtype=np.int64)
    prm = _params("adpit", 12)
    prm["data_config"]["data_pth"] = tmp
    ds = ref_datasets.Dataset(prm, "test", is_valid=True)
    names = ds.get_filelist()
    model = WrapperModel((1, 7, 400, 64), (1, 100, 6, 4, 12), prm)
    mg.fill_module_(model)
    model.eval()
    outputs = {}
    with torch.no_grad():
        for i in range(len(ds)):
            feat, _ = ds[i]
            outputs[names[i]] = model(feat.unsqueeze(0).float())
    dec = {nm: _np_decode(o) for nm, o in outputs.items()}
    acts = np.concatenate([d[..., 0:3].reshape(-1) for d in dec.values()])

    def widest_gap(vals, lo, hi):
        vals = np.sort(vals[(vals > lo) & (vals < hi)])
        k = int(np.argmax(np.diff(vals)))
        return 0.5 * float(vals[k] + vals[k + 1]), float(vals[k + 1] - vals[k])
    # the filler network's tanh tracks are dense above 0.3: the widest gap below 1 (the reference's double test keeps no
    # single track at a threshold >= 1) decides the conf threshold, the widest gap of the distances between two active
    # tracks below 15 degrees the unify threshold (15 / 30 / 45 all fall within 0.03 degree of some pair here)
    conf_thresh, gap = widest_gap(acts, 0.5, 0.95)
    conf_thresh = round(conf_thresh, 6)
    pair_d = np.concatenate([d[..., 12 + k][np.minimum(d[..., i], d[..., j]) > conf_thresh]
                             for d in dec.values() for k, (i, j) in enumerate(((0, 1), (1, 2), (2, 0)))])
    unify, gap_u = widest_gap(pair_d, 0.0, 15.0)
    unify = round(unify, 3)
    print("seld chain adpit: activities in [%.4f, %.4f], conf_thresh %.6f (gap %.2e), unify %.3f deg (gap %.3f, %d active pairs "
          "below it)" % (acts.min(), acts.max(), conf_thresh, gap, unify, gap_u, int((pair_d < unify).sum())))
    prm["train_config"].update(conf_thresh=conf_thresh, unify_thresh=unify)
    post = ref_datasets.LabelPostProcessor(prm)

    def rows_of(det):          # in the reference's order: frames, classes, tracks (no confidence ordering to tie here)
        return [[fr, int(d[0]), float(d[1]), float(d[2]), float(d[3])] for fr, dets in det.items() for d in dets]
    base = {nm: rows_of(post.postprocess(o.clone())) for nm, o in outputs.items()}
    g = torch.Generator().manual_seed(78)
    for trial in range(8):
        for nm, o in outputs.items():
            noisy = o + (torch.rand(o.shape, generator=g) * 2.0 - 1.0) * 1e-3
            r = rows_of(post.postprocess(noisy))
            assert [x[:2] for x in r] == [x[:2] for x in base[nm]], "rows unstable under 1e-3 output noise: " + nm
            if r:
                d = np.abs(np.asarray(r)[:, 2:] - np.asarray(base[nm])[:, 2:]).max()
                assert d < 2e-3, d
    print("seld chain adpit: rows per clip", {nm: len(r) for nm, r in base.items()}, "stable under 1e-3 output noise")
    assert all(len(r) for r in base.values())
    rng = np.random.default_rng(4343)
    for nm, rows in base.items():
        by_frame = {}
        for fr, cls, x, y, z in rows:
            by_frame.setdefault(fr, []).append((cls, x, y, z))
        nb_frames = outputs[nm].shape[1]
        lines = []
        for fr in range(nb_frames):
            src = 0
            for cls, x, y, z in by_frame.get(fr, []):
                u = rng.random()
                az = np.degrees(np.arctan2(y, x))
                el = np.degrees(np.arctan2(z, np.hypot(x, y)))
                if u < 0.65:
                    sd = 6.0 if rng.random() < 0.8 else 30.0
                    a2, e2 = az + rng.normal(0, sd), np.clip(el + rng.normal(0, sd), -80, 80)
                    lines.append((fr, cls, src, int(np.round(((a2 + 180) % 360) - 180)), int(np.round(e2))))
                    src += 1
                elif u < 0.75:
                    lines.append((fr, (cls + 5) % 12, src, int(np.round(az)), int(np.round(el))))
                    src += 1
            if rng.random() < 0.2:
                lines.append((fr, int(rng.integers(0, 12)), src, int(rng.integers(-180, 180)), int(rng.integers(-60, 60))))
        with open(os.path.join(cdir, nm + ".csv"), "w") as f:
            for ln in lines:
                f.write("%d,%d,%d,%d,%d\n" % ln)
        out["ref_" + nm] = np.asarray(lines, dtype=np.int64).reshape(len(lines), 5)
    # ---- pass 2: the reference's evaluation loop (test.py:33-60) with the default collate
    crit = WrapperCriterion(prm)
    loader = DataLoader(ds, batch_size=1, shuffle=False)
    os.makedirs(odir)
    test_loss, losses = 0.0, {}
    with torch.no_grad():
        for i, (feat, label) in enumerate(loader):
            output = model(feat)
            loss = crit(output, label)
            test_loss += loss.item()
            losses[names[i]] = loss.item()
            seld_output = post.postprocess(output.detach().cpu())
            with open(os.path.join(odir, names[i] + ".csv"), "w") as f:          # the line format of test.py:29
                for frame_idx in seld_output.keys():
                    for [class_idx, x, y, z] in seld_output[frame_idx]:
                        f.write("{},{},{},{},{},{}\n".format(int(frame_idx), int(class_idx), 0, float(x), float(y), float(z)))
            out["target_" + names[i]] = label.numpy()
            out["output_absmax_" + names[i]] = np.asarray(float(output.abs().max()))
            out["output_sample_" + names[i]] = output.reshape(-1)[mg.strided_sample(output.numel())].numpy()
    test_loss /= (i + 1)
    for nm in names:
        out["pred_" + nm] = mg._parse_rows(os.path.join(odir, nm + ".csv"))
        assert len(out["pred_" + nm]) == len(base[nm])
    res = ComputeSELDResults(prm, cdir).get_SELD_Results(odir)
    out.update(conf_thresh=np.asarray(conf_thresh), unify_thresh=np.asarray(unify), mean_loss=np.asarray(test_loss),
               losses=np.asarray([losses[nm] for nm in out["names"]]), scores=np.asarray([float(v) for v in res[:5]]),
               classwise=np.asarray(res[5], dtype=np.float64))
    np.savez_compressed(os.path.join(HERE, "seld_chain_adpit.npz"), **out)
    shutil.rmtree(tmp, ignore_errors=True)
    print("seld_chain_adpit.npz  ER F LE LR SELD =", out["scores"], " mean loss", test_loss,
          " rows", {nm: len(out["pred_" + nm]) for nm in names})


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mg._install_shims()
    if "--only" in sys.argv:
        globals()[sys.argv[sys.argv.index("--only") + 1]]()
        sys.exit(0)
    gen_postprocess_classwise()
    gen_seld_chain_adpit()
