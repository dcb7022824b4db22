"""CPU: the host halves of the device SELD scorer (``seld_metrics.DeviceSELDScorer``, csrc/seld.hip): the packed reference
table, the macro average and jackknife from per-file accumulators against the reference-made ``golden/metrics.npz``, and
the assignment of csrc/lsap.hpp (built with the host C++ compiler) against scipy, ties included."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

G = os.path.join(os.path.dirname(__file__), "golden")
CSRC = os.path.join(os.path.dirname(__file__), "..", "ad-yolo_amd", "csrc")
PRM = {"data_config": {"nb_classes": 12, "sr": 24000, "label_hop_len_s": 0.1}}


def _write_fixture(tmp_path):
    g = np.load(os.path.join(G, "metrics.npz"))
    ref_dir, pred_dir = tmp_path / "ref", tmp_path / "pred"
    ref_dir.mkdir()
    pred_dir.mkdir()
    for i, name in enumerate(g["names"]):
        with open(ref_dir / str(name), "w") as f:
            for r in g["ref_%d" % i]:
                f.write("%d,%d,%d,%d,%d\n" % tuple(int(v) for v in r))
        with open(pred_dir / str(name), "w") as f:
            for r in g["pred_%d" % i]:
                f.write("{},{},{},{},{},{}\n".format(int(r[0]), int(r[1]), 0, float(r[3]), float(r[4]), float(r[5])))
    return g, str(ref_dir), str(pred_dir)


def _host_accumulators(obj, pred_dir, names):
    """One ``SELDScorer.accumulator()`` per file, in ``names`` order (files the scorer leaves out are skipped)."""
    from adyolo_amd.seld_metrics import SELDScorer
    rows = []
    for name in names:
        labels = obj._pred_labels(pred_dir, name)
        if labels is None:
            continue
        sc = SELDScorer(obj._nb_classes, 20.0)
        sc.update(labels, obj._ref[name][0])
        rows.append(sc.accumulator())
    return np.asarray(rows)


def test_pack_reference_length_quirk_and_last_block():
    """blocks = ceil(max frame / 10): the largest frame index itself is not scored when it is a multiple of 10, and frames
    after the last started block are not held; within a frame the events are grouped by class in reference order."""
    from adyolo_amd.seld_metrics import pack_reference
    gt = {0: [[3, 0, 10.0, 5.0]], 4: [[1, 0, -170.0, 40.0], [2, 1, 180.0, -30.0], [1, 1, 90.0, 0.0]], 20: [[5, 0, 0.0, 0.0]]}
    gt2 = {0: [[0, 0, 0.0, 0.0]], 21: [[7, 0, 45.0, 45.0]]}
    p = pack_reference([(gt, 20), (gt2, 21)], 12, 10)
    assert p["file_info"].tolist() == [[0, 2], [20, 3]]           # 20 frames (frame 20 dropped), then 30 frames
    assert p["keep"] is None
    off = p["ref_off"]
    assert len(off) == 50 * 12 + 1 and off[-1] == 6                 # 4 + 2 events: frame 20 of the first file is not held
    assert off[4 * 12 + 1 + 1] - off[4 * 12 + 1] == 2                # class 1 of frame 4: two events
    ev = p["ref_ev"][off[4 * 12 + 1]:off[4 * 12 + 2]]
    np.testing.assert_array_equal(ev[:, 0], np.asarray([-170.0, 90.0]) * np.pi / 180.0)
    np.testing.assert_array_equal(ev[:, 1:], np.stack([np.sin([40.0 * np.pi / 180.0, 0.0]), np.cos([40.0 * np.pi / 180.0, 0.0])], 1))
    assert off[(20 + 21) * 12 + 7 + 1] - off[(20 + 21) * 12 + 7] == 1
    with pytest.raises(ValueError, match="reference events"):
        pack_reference([({3: [[2, k, 0.0, 0.0] for k in range(9)]}, 5)], 12, 10)
    pack_reference([({3: [[2, k, 0.0, 0.0] for k in range(8)]}, 5)], 12, 10)


def test_device_table_overlap_masks_match_reference(tmp_path):
    """The overlap variants keep the reference's frames (nb_overlap_files / nb_overlap_frames of metrics.npz) and hold
    events and keep marks only there; the recording length stays that of the full file."""
    from adyolo_amd.seld_metrics import ComputeSELDResultsFromEventOverlap, DeviceSELDScorer, load_output_format_file
    g, ref_dir, _ = _write_fixture(tmp_path)
    for tag, ov, flag in (("poly", "polyphony", False), ("homog", "homogenous", True)):
        dev = DeviceSELDScorer(PRM, ref_dir, device="cpu", overlap=ov)
        host = ComputeSELDResultsFromEventOverlap(PRM, ref_dir, classwise_overlap_test=flag)
        assert dev.nb_overlap_files == int(g["ov_%s_nfiles" % tag]) and dev.nb_overlap_frames == int(g["ov_%s_nframes" % tag])
        assert sorted(dev.names) == sorted(host._ref.keys())
        info = dev.table.file_info.numpy()
        keep = dev.table.keep.numpy()
        off = dev.table.ref_off.numpy()
        for k, name in enumerate(dev.names):
            nb = max(load_output_format_file(os.path.join(ref_dir, name)).keys())
            base, blocks = info[k]
            assert blocks == int(np.ceil(nb / 10.0)) == len(host._ref[name][0])
            kept = sorted(fr for fr in host._ov_frames[name] if fr < blocks * 10)
            assert np.flatnonzero(keep[base:base + blocks * 10]).tolist() == kept
            per_frame = (off[(base + np.arange(blocks * 10) + 1) * 12] - off[(base + np.arange(blocks * 10)) * 12])
            assert set(np.flatnonzero(per_frame).tolist()) <= set(kept)
        assert info[-1, 1] == 0                                       # the empty entry skipped files are scored against
    plain = DeviceSELDScorer(PRM, ref_dir, device="cpu")
    assert plain.table.keep is None and sorted(plain.names) == sorted(str(n) for n in g["names"])
    with pytest.raises(KeyError):
        plain.add_dict("no_such_file", {})


def test_macro_average_of_host_accumulators_matches_reference(tmp_path):
    from adyolo_amd.seld_metrics import ComputeSELDResults, ComputeSELDResultsFromEventOverlap, macro_average
    g, ref_dir, pred_dir = _write_fixture(tmp_path)
    names = [str(n) for n in g["names"]]
    res = macro_average(_host_accumulators(ComputeSELDResults(PRM, ref_dir), pred_dir, names).sum(0), 12)
    np.testing.assert_allclose([float(v) for v in res[:5]], g["scores"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res[5], g["classwise"], rtol=1e-9, atol=1e-9)
    for tag, flag in (("poly", False), ("homog", True)):
        obj = ComputeSELDResultsFromEventOverlap(PRM, ref_dir, classwise_overlap_test=flag)
        r = macro_average(_host_accumulators(obj, pred_dir, names).sum(0), 12)
        np.testing.assert_allclose([float(v) for v in r[:5]], g["ov_%s_scores" % tag], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(r[5], g["ov_%s_classwise" % tag], rtol=1e-9, atol=1e-9)
    host = ComputeSELDResults(PRM, ref_dir).get_SELD_Results(pred_dir)    # one scorer over all files: other sum order
    np.testing.assert_allclose([float(v) for v in host[:5]], [float(v) for v in res[:5]], rtol=1e-12)
    np.testing.assert_allclose(host[5], res[5], rtol=1e-12)


def test_jackknife_from_accumulators_matches_reference(tmp_path):
    from adyolo_amd.seld_metrics import ComputeSELDResults, jackknife_from_accumulators
    g, ref_dir, pred_dir = _write_fixture(tmp_path)
    order = [str(n) for n in g["jk_order"]]
    jk = jackknife_from_accumulators(_host_accumulators(ComputeSELDResults(PRM, ref_dir), pred_dir, order), 12)
    np.testing.assert_allclose(np.asarray([np.asarray(jk[i][1]) for i in range(5)]), g["jk_conf"], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(jk[5][1], g["jk_classwise_conf"], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose([float(jk[i][0]) for i in range(5)], g["jk_points"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(jk[5][0], g["jk_classwise"], rtol=1e-9, atol=1e-9)


_SHIM = r"""
#include "lsap.hpp"
#include <vector>
struct Seq {
    const double *c; int ld; bool tr;
    int lane() const { return 0; }
    int width() const { return 1; }
    void sync() const {}
    void reduce(double &, int &) const {}
    double cost(int i, int j) const { return tr ? c[j * ld + i] : c[i * ld + j]; }
};
extern "C" int lsap_pairs(int nr, int nc, const double *cost, int *a, int *b) {
    const bool tr = nc < nr;
    const int r = tr ? nc : nr, k = tr ? nr : nc;
    std::vector<double> u(r), v(k), spc(k);
    std::vector<int> path(k), c4r(r), r4c(k), rem(k);
    std::vector<unsigned char> sc(k);
    lsap::State s{u.data(), v.data(), spc.data(), path.data(), c4r.data(), r4c.data(), rem.data(), sc.data()};
    Seq cx{cost, nc, tr};
    if (lsap::solve(cx, r, k, s)) return -1;
    int n = 0;
    for (int i = 0; i < nr; ++i) {
        const int m = lsap::match_of_row(s, tr, i);
        if (m >= 0) { a[n] = i; b[n] = m; ++n; }
    }
    return n;
}
"""


def _tie_heavy(rng, t):
    nr, nc = (int(v) for v in rng.integers(1, 9, 2))
    kind = t % 4
    if kind == 3:
        return rng.random((nr, nc))
    c = rng.integers(0, 3 if kind < 2 else 2, (nr, nc)).astype(np.float64)
    if kind >= 1:                                                   # duplicated rows and columns
        for _ in range(2):
            if nr > 1:
                c[rng.integers(nr)] = c[rng.integers(nr)]
            if nc > 1:
                c[:, rng.integers(nc)] = c[:, rng.integers(nc)]
    return c


def test_lsap_matches_scipy_including_ties(tmp_path):
    """csrc/lsap.hpp (one lane) gives the (row, column) pairs of scipy.optimize.linear_sum_assignment on 12 000 seeded
    matrices: small integer costs, duplicated rows and columns, both orientations, plus continuous ones."""
    from scipy.optimize import linear_sum_assignment
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, lib = tmp_path / "lsap_shim.cpp", tmp_path / "liblsap_shim.so"
    src.write_text(_SHIM)
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(lib)], check=True)
    so = ctypes.CDLL(str(lib))
    so.lsap_pairs.restype = ctypes.c_int
    so.lsap_pairs.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    rng = np.random.default_rng(2016)
    a, b = np.zeros(8, np.int32), np.zeros(8, np.int32)
    ties = 0
    for t in range(12000):
        c = np.ascontiguousarray(_tie_heavy(rng, t))
        n = so.lsap_pairs(c.shape[0], c.shape[1], c.ctypes.data, a.ctypes.data, b.ctypes.data)
        ra, rb = linear_sum_assignment(c)
        assert n == len(ra), (t, c)
        assert a[:n].tolist() == ra.tolist() and b[:n].tolist() == rb.tolist(), (t, c, a[:n], b[:n], ra, rb)
        ties += int(len(np.unique(c)) < c.size)
    assert ties > 6000
