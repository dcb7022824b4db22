"""CPU side of the device selection of the AD-YOLO head: the C entry point is declared, exported and bound; the grouping of
its rows into per-clip dicts (``postprocess.group_rows``); the float32 rounding of the thresholds (``ops.np_f32_threshold``)
that makes the device compare exactly as NumPy compares the host path's float32 arrays."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from adyolo_amd import _lib, ops  # noqa: E402
from adyolo_amd.postprocess import LabelPostProcessor, group_rows  # noqa: E402


def test_select_entry_points_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adyolo_hip.h")).read(), flags=re.S)
    for name in ("adyolo_yolo_select", "adyolo_yolo_select_workspace_words"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    assert "#define ADYOLO_SELECT_MAX_N 1024" in open(os.path.join(ROOT, "include", "adyolo_hip.h")).read()
    lib = _lib.load()
    assert lib.adyolo_abi_version() == 4
    assert lib.adyolo_yolo_select_workspace_words(600, 160, 12) == 600 * 12 * (3 * 160 + 2)
    assert lib.adyolo_yolo_select_workspace_words(0, 160, 12) == 0


def test_group_rows_on_hand_built_rows():
    # two clips of three frames: clip 0 -> frames 0 (two rows) and 2 (one row); clip 1 -> frame 1 (local), three rows
    rows = np.asarray([[0, 3, 0.1, 0.2, 0.3],
                       [0, 5, 0.4, 0.5, 0.6],
                       [2, 1, 1.0, 0.0, 0.0],
                       [4, 0, 0.0, 1.0, 0.0],
                       [4, 0, 0.0, 0.0, 1.0],
                       [4, 7, -1.0, 0.0, 0.0]], dtype=np.float32)
    counts = np.asarray([2, 0, 1, 0, 3, 0], dtype=np.int32)
    one = group_rows(rows, counts)
    assert len(one) == 1 and list(one[0].keys()) == [0, 2, 4]
    two = group_rows(rows, counts, n_clips=2)
    assert [list(d.keys()) for d in two] == [[0, 2], [1]]
    f32 = lambda *v: [float(np.float32(x)) for x in v]                               # noqa: E731
    assert two[0][0] == [f32(3, 0.1, 0.2, 0.3), f32(5, 0.4, 0.5, 0.6)]
    assert two[0][2] == [f32(1, 1, 0, 0)]
    assert two[1][1] == [f32(0, 0, 1, 0), f32(0, 0, 0, 1), f32(7, -1, 0, 0)]
    assert all(isinstance(k, int) for d in two for k in d)
    assert group_rows(np.zeros((0, 5), np.float32), np.zeros(4, np.int32), n_clips=2) == [{}, {}]
    with pytest.raises(ValueError):
        group_rows(rows, counts[:4])                                                 # counts do not add up to the rows
    with pytest.raises(ValueError):
        group_rows(rows, counts, n_clips=4)                                          # 6 frames are not 4 clips


@pytest.mark.parametrize("t", [0.1, 0.2, 0.5, 0.9, 0.1 * 3, 1.0 / 3.0, 10.0, 15.0, 45.0, 0.3,
                               *np.arange(0.1, 1.0, 0.1), np.float64(20.000000001), np.float32(0.7), 1])
def test_threshold_rounding_reproduces_numpy_compares(t):
    t32 = np.float32(t)
    near = [np.nextafter(t32, np.float32(-np.inf)), t32, np.nextafter(t32, np.float32(np.inf))]
    x = np.asarray(near + list(np.random.RandomState(0).uniform(0, 2 * float(t) + 1, 1000)), dtype=np.float32)
    for op, fn in ((">", np.greater), ("<", np.less), ("<=", np.less_equal)):
        thr = np.float32(ops.np_f32_threshold(t, op))
        np.testing.assert_array_equal(fn(x, thr), fn(x, t), err_msg="%r %s" % (t, op))


def test_device_select_refuses_cpu_tensors_and_class_wise_heads():
    with pytest.raises(_lib.AdyoloHipError):
        ops.yolo_select(torch.zeros(2, 160, 15), 12, 0.5, 0.5, 20.0, "conn-merge")
    prm = {"args": {"loss": "accdoa"}, "data_config": {"nb_classes": 12}, "train_config": {"conf_thresh": 0.5}}
    with pytest.raises(NotImplementedError):
        LabelPostProcessor(prm).select_device(torch.zeros(2, 12, 4))
