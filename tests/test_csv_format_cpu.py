"""CPU: the definition of the device CSV formatter.
  csrc/csv_format.hpp, built with the host C++ compiler and called in batches through ctypes, against
  ``repr(float(np.float32))``: 2 000 000 seeded random bit patterns and the structured edges (``structured_bits``), no case
  left out; its integer and line routines against the writer's format expression.
  ``postprocess.format_rows`` against the bytes ``write_seld_output_file`` writes after ``group_rows`` / ``split_pass_rows`` /
  ``track_groups``; the segment helpers; the loops' refusal of a ``device_csv`` that is no bool."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import adyolo_amd  # noqa: F401
from adyolo_amd import postprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ad-yolo_amd", "csrc")


def _f32_bits(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32)


def _with_neighbours(values):
    v = np.asarray(values, dtype=np.float32)
    return np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))])


def structured_bits():
    """The float32 bit patterns where a shortest-digits routine or repr's notation rule can go wrong, both signs:
    every power of two 2^-149 .. 2^127 (the rounding interval is half as wide below it) and the float32 nearest 10^k,
    k = -45 .. 38, each with both neighbours -- these hold both notation borders, 9.99..e-05 | 0.0001 and
    9999999198822400.0 | 1.0000000272564224e+16; the integers 0 .. 4096 and 2^24 -+ 1; +-0, the smallest and the largest
    subnormal, the largest finite; +-inf; NaNs of both signs with payloads."""
    pow2 = _with_neighbours([np.ldexp(np.float32(1), p) for p in range(-149, 128)])
    pow10 = _with_neighbours([np.float32(float("1e%d" % k)) for k in range(-45, 39)])
    ints = np.concatenate([np.arange(0, 4097), [2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1]]).astype(np.float32)
    finite = np.concatenate([pow2, pow10, ints]).astype(np.float32)
    finite = finite[np.isfinite(finite)]
    special = np.array([0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000, 0x7fc00000, 0x7f800001,
                        0x7fffffff, 0x7fa5a5a5], dtype=np.uint32)
    bits = np.concatenate([_f32_bits(finite), special])
    return np.concatenate([bits, bits | np.uint32(0x80000000)]).astype(np.uint32)


def python_reprs(bits):
    with np.errstate(invalid="ignore"):                            # (a signalling NaN is widened too)
        return [repr(v) for v in np.asarray(bits, dtype=np.uint32).view(np.float32).astype(np.float64).tolist()]


_SHIM = r"""
#include "csv_format.hpp"
// every value's repr followed by '\n' into out (25 bytes per value are enough) -> the bytes written, or -1 - i when the
// length-only routine disagrees with the writing one at value i
extern "C" long csvf_repr_join(const uint32_t *bits, long n, char *out) {
    long at = 0;
    for (long i = 0; i < n; ++i) {
        const int len = csvf::f32_put(out + at, bits[i]);
        if (len != csvf::f32_len(bits[i]) || len > 24) return -1 - i;
        at += len;
        out[at++] = '\n';
    }
    return at;
}
extern "C" long csvf_lines(const long long *frame, const long long *cls, const long long *id, const uint32_t *xyz, long n,
                           char *out) {
    long at = 0;
    for (long i = 0; i < n; ++i) {
        const int len = csvf::line_put(out + at, frame[i], cls[i], id[i], xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        if (len != csvf::line_len(frame[i], cls[i], id[i], xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]) || len > CSVF_LINE_MAX)
            return -1 - i;
        at += len;
    }
    return at;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("csvf")
    src, lib = d / "csvf_shim.cpp", d / "libcsvf_shim.so"
    src.write_text(_SHIM)
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(lib)],
                   check=True)
    so = ctypes.CDLL(str(lib))
    so.csvf_repr_join.restype = ctypes.c_long
    so.csvf_repr_join.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    so.csvf_lines.restype = ctypes.c_long
    so.csvf_lines.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_long, ctypes.c_void_p]
    return so


def _header_reprs(so, bits):
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    out = np.zeros(25 * len(bits) + 1, dtype=np.uint8)
    n = so.csvf_repr_join(bits.ctypes.data, len(bits), out.ctypes.data)
    assert n >= 0, "f32_len and f32_put disagree at value %d (0x%08x)" % (-1 - n, bits[-1 - n])
    return out[:n].tobytes().decode("ascii")


def _assert_all_match(so, bits):
    got, want = _header_reprs(so, bits), python_reprs(bits)
    if got != "".join(w + "\n" for w in want):
        got = got.split("\n")
        bad = [(hex(int(b)), g, w) for b, g, w in zip(bits, got, want) if g != w]
        raise AssertionError("%d of %d values differ from repr, the first: %r" % (len(bad), len(bits), bad[:5]))


def test_header_matches_repr_on_the_structured_edges(shim):
    bits = structured_bits()
    assert len(bits) > 2 * (3 * 277 + 3 * 84 + 4100)
    want = dict(zip(bits.tolist(), python_reprs(bits)))
    # the list holds what it claims: both notation borders, the widest and the narrowest text, the specials
    for text in ("9.999999747378752e-05", "0.00010000000474974513", "9999999198822400.0", "1.0000000272564224e+16",
                 "0.10000000149011612", "1.401298464324817e-45", "-1.1754943508222875e-38", "3.4028234663852886e+38", "-0.0", "inf", "-inf",
                 "nan", "16777216.0", "1.0"):
        assert text in want.values(), text
    assert max(len(t) for t in want.values()) == 23
    _assert_all_match(shim, bits)


def test_header_matches_repr_on_two_million_random_patterns(shim):
    rng = np.random.default_rng(20240611)
    bits = rng.integers(0, 2 ** 32, size=2_000_000, dtype=np.uint64).astype(np.uint32)
    _assert_all_match(shim, bits)


def test_header_lines_match_the_writers_format_expression(shim):
    rng = np.random.default_rng(5)
    edges = structured_bits()
    n = 6000
    frame = np.concatenate([[0, 9, 10, 99, 100, 999, 1000, 2 ** 31 - 1], rng.integers(0, 100000, n - 8)]).astype(np.int64)
    cls = np.concatenate([[0, 9, 10, 12, -1, -(2 ** 31) + 1, 2 ** 31 - 1, 7], rng.integers(0, 13, n - 8)]).astype(np.int64)
    ids = np.concatenate([[0, 7, 2 ** 31 - 1, 10, 99, 100, 1, 0], rng.integers(0, 50, n - 8)]).astype(np.int64)
    xyz = rng.choice(edges, size=(n, 3)).astype(np.uint32)
    xyz[0] = _f32_bits([-1.1754943508222875e-38] * 3)              # the longest line next to the shortest
    frame[0], cls[0], ids[0] = 2 ** 31 - 1, -(2 ** 31) + 1, 2 ** 31 - 1
    xyz[1] = np.uint32(0x7fc00000)
    frame[1], cls[1], ids[1] = 0, 0, 0
    out = np.zeros(pp.CSV_LINE_MAX * n, dtype=np.uint8)
    got = shim.csvf_lines(frame.ctypes.data, cls.ctypes.data, ids.ctypes.data, xyz.ctypes.data, n, out.ctypes.data)
    assert got >= 0, "line_len and line_put disagree (or a line is longer than CSVF_LINE_MAX) at line %d" % (-1 - got)
    with np.errstate(invalid="ignore"):
        vals = xyz.view(np.float32).astype(np.float64).tolist()
    want = "".join("{},{},{},{},{},{}\n".format(int(f), int(c), int(i), float(x), float(y), float(z))
                   for f, c, i, (x, y, z) in zip(frame.tolist(), cls.tolist(), ids.tolist(), vals))
    assert out[:got].tobytes().decode("ascii") == want
    assert len(want.split("\n")[0]) + 1 == 106 <= pp.CSV_LINE_MAX and want.split("\n")[1] == "0,0,0,nan,nan,nan"


def test_the_constants_agree_in_every_place():
    """The status bits and the longest line: the C header, the formatting header, ``postprocess`` (the one Python
    definition) and ``ops`` (which imports it and words the bits)."""
    import re
    from adyolo_amd import ops
    with open(os.path.join(ROOT, "include", "adyolo_hip.h")) as f:
        abi = dict(re.findall(r"#define\s+ADYOLO_CSV_(OVERFLOW|BAD_COUNTS|BAD_VALUE|BAD_TABLE|LINE_MAX)\s+(\d+)", f.read()))
    with open(os.path.join(CSRC, "csv_format.hpp")) as f:
        line_max = int(re.search(r"#define\s+CSVF_LINE_MAX\s+(\d+)", f.read()).group(1))
    assert {k: int(v) for k, v in abi.items()} == {"OVERFLOW": pp.CSV_OVERFLOW, "BAD_COUNTS": pp.CSV_BAD_COUNTS,
                                                   "BAD_VALUE": pp.CSV_BAD_VALUE, "BAD_TABLE": pp.CSV_BAD_TABLE,
                                                   "LINE_MAX": pp.CSV_LINE_MAX}
    assert line_max == pp.CSV_LINE_MAX == ops.CSV_LINE_MAX and ops.CSV_OVERFLOW == pp.CSV_OVERFLOW
    assert sorted(bit for bit, _ in ops.CSV_STATUS) == sorted([pp.CSV_OVERFLOW, pp.CSV_BAD_COUNTS, pp.CSV_BAD_VALUE,
                                                               pp.CSV_BAD_TABLE])


def test_the_committed_power_table_is_the_generators():
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_csv_pow5.py"), "--check"], check=True)


# ------------------------------------------------------------------------------------------------------------ format_rows
def _random_rows(rng, counts, nb_classes=13):
    n = int(np.sum(counts))
    edges = structured_bits()
    edges = edges[np.isfinite(edges.view(np.float32))]
    rows = np.zeros((n, 5), dtype=np.float32)
    rows[:, 0] = rng.integers(0, 7, n)                             # the frame column is NOT what the writer uses
    rows[:, 1] = rng.integers(0, nb_classes, n)
    rows[:, 2:] = rng.standard_normal((n, 3)).astype(np.float32)
    pick = rng.random((n, 3)) < 0.3
    rows[:, 2:][pick] = rng.choice(edges, size=int(pick.sum())).view(np.float32)
    return rows


def _files(tmp_path, tag, groups, id_groups=None):
    out = []
    for k, g in enumerate(groups):
        pth = str(tmp_path / ("%s_%d.csv" % (tag, k)))
        pp.write_seld_output_file(pth, g, None if id_groups is None else id_groups[k])
        with open(pth, "rb") as f:
            out.append(f.read())
    return out


def _spans(data, seg_bytes):
    return [data[int(a):int(b)] for a, b in zip(seg_bytes[:-1], seg_bytes[1:])]


@pytest.mark.parametrize("with_ids", [False, True], ids=["no-ids", "ids"])
def test_format_rows_writes_the_clip_files_bytes(tmp_path, with_ids):
    rng = np.random.default_rng(11)
    t = 130
    counts = rng.integers(0, 4, 3 * t)
    counts[t:2 * t] = 0                                            # a clip without rows: an empty file
    counts[7] = 65
    rows = _random_rows(rng, counts)
    ids = rng.integers(0, 40, len(rows)).astype(np.int32) if with_ids else None
    want = _files(tmp_path, "clip", pp.group_rows(rows, counts, 3), pp.track_groups(ids, counts, 3) if with_ids else None)
    data, seg_bytes = pp.format_rows(rows, counts, pp.csv_segments_clips(3, t), ids)
    assert seg_bytes.shape == (4,) and seg_bytes[0] == 0 and seg_bytes[-1] == len(data)
    assert _spans(data, seg_bytes) == want and want[1] == b"" and len(want[0]) > 0 and len(want[2]) > 0
    assert data.count(b"\n") == len(rows)


@pytest.mark.parametrize("with_ids", [False, True], ids=["no-ids", "ids"])
def test_format_rows_writes_the_run_files_bytes(tmp_path, with_ids):
    """A run that starts inside recording 1 and crosses two recording boundaries, recording 2 without a frame."""
    from adyolo_amd.corpus import split_pass_rows
    rng = np.random.default_rng(12)
    frame_start = np.array([0, 20, 50, 50, 75, 110, 130])
    base, n = 33, 60                                               # frames [33, 93): recordings 1, (2,) 3 and 4
    counts = rng.integers(0, 4, n)
    counts[0], counts[50 - base], counts[75 - base], counts[-1] = 2, 1, 3, 2
    rows = _random_rows(rng, counts)
    ids = rng.integers(0, 40, len(rows)).astype(np.int32) if with_ids else None
    r0, table = pp.csv_segments_run(base, n, frame_start)
    assert r0 == 1 and table.tolist() == [[0, 13], [17, 0], [17, 0], [42, 0]] and table.dtype == np.int32
    split = split_pass_rows(rows, counts, base, frame_start)
    assert sorted(split) == [1, 3, 4]
    id_groups = None
    if with_ids:                                                   # the ids on each recording's frame axis, as _write_pass does
        id_groups = [{} for _ in range(4)]
        ends = np.cumsum(counts)
        for f in np.flatnonzero(counts).tolist():
            r = int(np.searchsorted(frame_start, base + f, "right")) - 1
            id_groups[r - r0][base + f - int(frame_start[r])] = ids[ends[f] - counts[f]:ends[f]].tolist()
    want = _files(tmp_path, "run", [split.get(r, {}) for r in range(1, 5)], id_groups)
    data, seg_bytes = pp.format_rows(rows, counts, table, ids)
    assert _spans(data, seg_bytes) == want and want[1] == b"" and all(len(want[k]) for k in (0, 2, 3))
    assert want[0].startswith(b"13,") and want[2].startswith(b"0,") and want[3].startswith(b"0,")


def test_format_rows_on_an_empty_call_and_its_refusals():
    empty = np.zeros((0, 5), dtype=np.float32)
    data, seg_bytes = pp.format_rows(empty, np.zeros(8, dtype=np.int32), pp.csv_segments_clips(2, 4))
    assert data == b"" and seg_bytes.tolist() == [0, 0, 0]
    data, seg_bytes = pp.format_rows(empty, np.zeros(8, dtype=np.int32), [[0, 5]], ids=np.zeros(0, dtype=np.int32))
    assert data == b"" and seg_bytes.tolist() == [0, 0]
    row = np.array([[0, 3, 1, 0, 0]], dtype=np.float32)
    assert pp.format_rows(row, [0, 1], [[0, 5]])[0] == b"6,3,0,1.0,0.0,0.0\n"
    for bad_cls in (np.nan, np.inf, -np.inf, 2.0 ** 31):
        bad = row.copy()
        bad[0, 1] = bad_cls
        with pytest.raises(ValueError):
            pp.format_rows(bad, [0, 1], [[0, 0]])
    with pytest.raises(ValueError):
        pp.format_rows(row, [0, 1], [[0, 0]], ids=[-1])
    with pytest.raises(ValueError):
        pp.format_rows(row, [0, 2], [[0, 0]])
    with pytest.raises(ValueError):
        pp.format_rows(row, [2, -1], [[0, 0]])
    for table in ([[1, 0]], [[0, 0], [2, 0], [1, 0]], [[0, -1]], [0, 0], [[0, 0], [3, 0]]):
        with pytest.raises(ValueError):
            pp.format_rows(row, [0, 1], table)


def test_segment_helpers():
    assert pp.csv_segments_clips(1, 600).tolist() == [[0, 0]]
    assert pp.csv_segments_clips(3, 130).tolist() == [[0, 0], [130, 0], [260, 0]]
    assert pp.csv_segments_clips(3, 130).dtype == np.int32
    fs = [0, 20, 50, 50, 75]
    r0, table = pp.csv_segments_run(0, 75, fs)
    assert r0 == 0 and table.tolist() == [[0, 0], [20, 0], [50, 0], [50, 0]]
    r0, table = pp.csv_segments_run(20, 30, fs)                    # a boundary on the first frame, the run ends on the last
    assert r0 == 1 and table.tolist() == [[0, 0]]
    r0, table = pp.csv_segments_run(49, 2, fs)                     # ... on the last frame, behind a recording without frames
    assert r0 == 1 and table.tolist() == [[0, 29], [1, 0], [1, 0]]
    r0, table = pp.csv_segments_run(60, 5, fs)                     # inside one recording: K = 1
    assert r0 == 3 and table.tolist() == [[0, 10]]
    for base, n in ((-1, 3), (70, 6), (0, 0)):
        with pytest.raises(ValueError):
            pp.csv_segments_run(base, n, fs)
    with pytest.raises(ValueError):
        pp.csv_segments_clips(0, 5)


@pytest.mark.parametrize("loop", ["test_epoch_corpus", "sweep_conf_thresh_corpus", "test_epoch_windows",
                                  "sweep_conf_thresh_windows", "infer_epoch_corpus"])
def test_the_loops_refuse_a_device_csv_that_is_no_bool(loop):
    """Checked before anything else is touched, so no corpus, model or device is needed to see it."""
    import inspect
    from adyolo_amd import test as atest
    fn = getattr(atest, loop)
    sig = inspect.signature(fn)
    assert sig.parameters["device_csv"].default is False
    args = [None] * sum(1 for p in sig.parameters.values() if p.default is inspect.Parameter.empty)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="device_csv"):
            fn(*args, device_csv=bad)
    with pytest.raises(TypeError):
        fn(*args, device_csvs=True)
