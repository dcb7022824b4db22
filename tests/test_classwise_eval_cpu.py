"""CPU: the host half of the class-wise evaluation path (``--loss seddoa | masked-seddoa | accdoa | adpit``).

* ``LabelPostProcessor.select`` on a decode made with NumPy from the planted outputs of ``golden/postprocess_classwise.npz``
  gives the rows of the REAL reference's ``LabelPostProcessor`` (make_golden_classwise.py) exactly: frame, class and order
  exact, xyz bit-equal, for every conf threshold and, for adpit, every unify threshold.
* ``FoaDataset`` returns the ``ClasswiseLabelEncoder`` labels (rotated with the rotation augmentation on) and
  ``audio_collate_fn`` stacks them."""
import os
import sys

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, G)
from classwise_decode_np import decode as np_decode  # noqa: E402

LOSSES = ("seddoa", "masked-seddoa", "accdoa", "adpit")


def _params(loss, nb_classes=12, data_pth=None, rotate=False):
    return {"args": {"device": "cuda:0", "encoder": "se-resnet34", "loss": loss},
            "data_config": {"nb_classes": nb_classes, "sr": 24000, "label_hop_len_s": 0.1, "data_pth": str(data_pth)},
            "aug_config": {"rotation_augment": rotate, "spec_augment": False},
            "train_config": {"conf_thresh": 0.5, "unify_thresh": 15.0}}


def _flat(res):
    rows = [[fr] + [float(v) for v in r] for fr, rr in res.items() for r in rr]
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), 5)


def _cases(g, loss, c):
    src = "seddoa" if loss == "masked-seddoa" else loss
    ths = list(g["conf_thresholds"]) + ([] if src == "seddoa" else [float(g["high_thresh"])])
    for i, th in enumerate(ths):
        for u in (g["unify_thresholds"] if src == "adpit" else (None,)):
            yield th, u, "rows_%s_C%d_t%d" % (src, c, i) + ("" if u is None else "_u%d" % int(u))


@pytest.mark.parametrize("c", [12, 13])
@pytest.mark.parametrize("loss", LOSSES)
def test_select_matches_the_reference_rows(loss, c):
    from adyolo_amd.postprocess import LabelPostProcessor
    g = np.load(os.path.join(G, "postprocess_classwise.npz"))
    src = "seddoa" if loss == "masked-seddoa" else loss
    out = g["out_%s_C%d" % (src, c)]
    dec = np_decode(out, loss, c)
    pp = LabelPostProcessor(_params(loss, c))
    n = 0
    for th, u, key in _cases(g, loss, c):
        pp.set_conf_thresh(th)
        if u is not None:
            pp.unify_thresh = float(u)            # read at select time, as the reference's test.py sets it
        got, ref = _flat(pp.select(dec)), g[key]
        assert got.shape == ref.shape, (key, got.shape, ref.shape)
        np.testing.assert_array_equal(got[:, :2], ref[:, :2], err_msg=key)              # frame, class, order
        np.testing.assert_array_equal(got[:, 2:].astype(np.float32).view(np.int32),
                                      ref[:, 2:].astype(np.float32).view(np.int32), err_msg=key)
        assert np.array_equal(got[:, 2:], ref[:, 2:])
        n += len(ref)
    assert n > 0


def test_select_reaches_every_adpit_case():
    """The fixture's adpit rows include single tracks, pair means and three-track means (so the comparison above covers
    every branch): count rows that are not a copy of one track."""
    g = np.load(os.path.join(G, "postprocess_classwise.npz"))
    out = g["out_adpit_C12"]
    v = np_decode(out, "adpit", 12)[..., 3:12].reshape(-1, 12, 3, 3)
    rows = g["rows_adpit_C12_t4_u45"]
    copies = 0
    for fr, cl, x, y, z in rows:
        tracks = v[int(fr), int(cl)].astype(np.float64)
        copies += any(np.array_equal(t, [x, y, z]) for t in tracks)
    assert 0 < copies < len(rows)
    assert len(g["rows_adpit_C12_t9_u15"]) > 0 and len(g["rows_accdoa_C12_t9"]) == 0     # threshold >= 1: unified rows only


def test_unknown_losses_still_raise(tmp_path):
    from adyolo_amd.datasets import FoaDataset
    from adyolo_amd.postprocess import LabelPostProcessor
    with pytest.raises(NotImplementedError):
        LabelPostProcessor(_params("masked-accdoa"))
    os.makedirs(os.path.join(tmp_path, "foa_dev", "dev-test"))
    with pytest.raises(NotImplementedError):
        FoaDataset(_params("masked-accdoa", data_pth=tmp_path), "test", is_valid=True)


# ------------------------------------------------------------------------------------------------------------- data
def _write_split(root, split, n_files=3):
    from scipy.io import wavfile
    wdir, cdir = os.path.join(root, "foa_dev", "dev-" + split), os.path.join(root, "metadata_dev", "dev-" + split)
    os.makedirs(wdir), os.makedirs(cdir)
    rs = np.random.RandomState(5)
    for i in range(n_files):
        name = "fold1_room1_mix%03d" % i
        wavfile.write(os.path.join(wdir, name + ".wav"), 24000, rs.randint(-900, 900, size=(24000 * 2, 4)).astype(np.int16))
        with open(os.path.join(cdir, name + ".csv"), "w") as f:
            for fr in range(0, 20):
                for src in range(int(rs.randint(0, 4))):
                    cls = int(rs.randint(0, 3)) if src else int(rs.randint(0, 12))          # same-class overlaps for ADPIT
                    f.write("%d,%d,%d,%d,%d\n" % (fr, cls, src, rs.randint(-180, 181), rs.randint(-60, 61)))
            f.write("25,3,0,10,20\n")                   # beyond the clip's 20 label frames: dropped
    return cdir


_LABEL = {"seddoa": "get_seddoa_label", "masked-seddoa": "get_seddoa_label", "accdoa": "get_accdoa_label",
          "adpit": "get_adpit_label"}


@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("loss", LOSSES)
def test_foa_dataset_returns_classwise_labels(tmp_path, loss, rotate):
    import random
    from adyolo_amd.augmentations import rotate_labels
    from adyolo_amd.datasets import ClasswiseLabelEncoder, FoaDataset, audio_collate_fn
    cdir = _write_split(tmp_path, "valid")
    random.seed(11)
    ds = FoaDataset(_params(loss, data_pth=tmp_path, rotate=rotate), "valid", is_valid=False)
    enc = ClasswiseLabelEncoder(12)
    items, combs = [], set()
    for i in range(len(ds)):
        pcm, comb, lab = ds[i]
        assert pcm.dtype == np.int16 and pcm.shape == (48000, 4)
        label = FoaDataset.load_csv2dict(os.path.join(cdir, ds.get_filelist()[i] + ".csv"))
        if rotate:
            label = rotate_labels(label, comb)
        else:
            assert comb == 0
        combs.add(comb)
        want = getattr(enc, _LABEL[loss])(label, 20)
        assert isinstance(lab, torch.Tensor) and lab.dtype == torch.float32
        assert torch.equal(lab, want), (loss, i)
        items.append((pcm, comb, lab))
    if rotate:
        assert combs != {0}
    pcm_b, comb_b, tgt = audio_collate_fn(items)
    assert tuple(pcm_b.shape) == (len(items), 48000, 4) and comb_b == [it[1] for it in items]
    assert torch.equal(tgt, torch.stack([it[2] for it in items]))
    assert tgt.shape[:2] == (len(items), 20)


def test_foa_dataset_infer_has_zero_labels(tmp_path):
    from adyolo_amd.datasets import FoaDataset
    _write_split(tmp_path, "test", n_files=1)
    prm = _params("adpit", data_pth=tmp_path)
    prm["args"]["infer_pth"] = os.path.join(tmp_path, "foa_dev", "dev-test")
    ds = FoaDataset(prm, "infer", is_valid=True)
    _, _, lab = ds[0]
    assert tuple(lab.shape) == (20, 6, 4, 12) and not lab.any()
