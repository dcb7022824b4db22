"""CPU side of the device selection of the class-wise heads (seddoa / masked-seddoa / accdoa / adpit): the C entry points are
declared, exported and bound; ``ops.classwise_select`` refuses what it cannot run before anything is launched; a class-wise
``select_device`` on a host tensor keeps raising ``NotImplementedError`` (``select`` is the host path)."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from adyolo_amd import _lib, ops  # noqa: E402
from adyolo_amd.postprocess import CLASSWISE, LabelPostProcessor  # noqa: E402

NAMES = ("adyolo_classwise_select", "adyolo_classwise_select_workspace_words")


def test_classwise_select_entry_points_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adyolo_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    for mode in (0, 1, 2):                                                           # counts and offsets only
        assert lib.adyolo_classwise_select_workspace_words(600, 13, mode) == 2 * 600 * 13
    assert lib.adyolo_classwise_select_workspace_words(0, 13, 2) == 0
    assert lib.adyolo_classwise_select_workspace_words(600, 0, 2) == 0
    assert lib.adyolo_classwise_select_workspace_words(600, 13, 3) == 0


@pytest.mark.parametrize("loss", CLASSWISE)
def test_classwise_select_has_no_cpu_path(loss):
    rec = ops.CLASSWISE_REC[ops.CLASSWISE_MODES[loss]]
    with pytest.raises(_lib.AdyoloHipError):
        ops.classwise_select(torch.zeros(5, 12, rec), 12, loss, 0.5, unify=15.0)
    with pytest.raises(_lib.AdyoloHipError):
        ops.classwise_select(torch.zeros(5, 12, rec), 12, loss, 0.5, unify=15.0, trim=False)


def test_adpit_needs_a_unify_threshold():
    with pytest.raises(ValueError):
        ops.classwise_select(torch.zeros(5, 12, 16), 12, "adpit", 0.5)
    with pytest.raises(ValueError):
        ops.classwise_select(torch.zeros(5, 12, 16), 12, 2, 0.5, unify=None)
    with pytest.raises(_lib.AdyoloHipError):                                         # not needed elsewhere: the tensor is refused
        ops.classwise_select(torch.zeros(5, 12, 4), 12, "accdoa", 0.5)


@pytest.mark.parametrize("loss,shape", [("adpit", (5, 12, 4)), ("accdoa", (5, 12, 16)), ("seddoa", (5, 12, 3)),
                                        ("adpit", (5, 13, 16)), ("adpit", (5, 12 * 16))])
def test_wrong_record_width_is_refused(loss, shape):
    with pytest.raises(_lib.AdyoloHipError):
        ops.classwise_select(torch.zeros(*shape), 12, loss, 0.5, unify=15.0)


@pytest.mark.parametrize("loss", CLASSWISE)
def test_classwise_select_device_keeps_refusing_host_tensors(loss):
    prm = {"args": {"loss": loss}, "data_config": {"nb_classes": 12},
           "train_config": {"conf_thresh": 0.5, "unify_thresh": 15.0}}
    rec = ops.CLASSWISE_REC[ops.CLASSWISE_MODES[loss]]
    pp = LabelPostProcessor(prm)
    with pytest.raises(NotImplementedError):
        pp.select_device(torch.zeros(2, 12, rec))
    with pytest.raises(NotImplementedError):
        pp.select_device_rows(torch.zeros(2, 12, rec), trim=False)
    assert pp.select(torch.zeros(2, 12, rec).numpy()) == {}                          # the host path
