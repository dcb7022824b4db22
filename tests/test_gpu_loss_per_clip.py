"""GPU: the per-clip AD-YOLO loss of a batched evaluation pass (csrc/loss.hip ``adyolo_loss_per_clip``) against B calls of the
existing entry point, one per clip with that clip's logits and rows alone (``ops.adyolo_loss(need_grad=False)``, which the
float64 tests of test_gpu_loss_stage.py pin): every loss is compared as int32 BITS.  The shapes are the smallest at which the
decomposition into workgroups can differ: 0 / 1 / 31 / 32 / 33 / 257 rows (one assign workgroup takes 32), 32 800 rows (past
32 x 1024: the assign grid-stride), 160 anchors per frame with T' = 1 / 2 / 8 (under one 256-anchor tile, a ragged second tile,
five exact tiles) and T' = 3300 (more than 2048 tiles per clip: the main kernel's grid-stride), C = 12 / 13 (the two
``loss_main`` instantiations)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID, ANCHORS = (8, 4), 5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def _rows(rs, n, clip, t_frames, c, far=False):
    """n target rows [b, t, gi, gj, cls, U, V] of one clip; far: directions a long way from their cell (positives by arg-min)."""
    r = np.zeros((n, 7), dtype=np.float32)
    r[:, 0] = clip
    r[:, 1] = rs.randint(0, t_frames, n)
    r[:, 2] = rs.randint(0, GRID[0], n)
    r[:, 3] = rs.randint(0, GRID[1], n)
    r[:, 4] = rs.randint(0, c, n)
    if far:
        r[:, 5] = ((r[:, 2] * 45.0 - 180.0 + 22.5) + 180.0 + 180.0) % 360.0 - 180.0       # the opposite azimuth
        r[:, 6] = -(r[:, 3] * 45.0 - 90.0 + 22.5)
    else:
        r[:, 5] = r[:, 2] * 45.0 - 180.0 + rs.uniform(-20.0, 65.0, n)
        r[:, 6] = np.clip(r[:, 3] * 45.0 - 90.0 + rs.uniform(-20.0, 65.0, n), -90.0, 90.0)
        r[:, 5] = (r[:, 5] + 180.0) % 360.0 - 180.0
    return r


def _case(seed, counts, t_frames, c, pad=5, far=()):
    rs = np.random.RandomState(seed)
    b = len(counts)
    g = torch.Generator().manual_seed(seed)
    logit = (torch.randn(b, t_frames, GRID[0] * GRID[1] * ANCHORS * (c + 3), generator=g) * 1.5).to("cuda:0")
    clips = [_rows(rs, n, k, t_frames, c, far=k in far) for k, n in enumerate(counts)]
    padding = _rows(rs, pad, -1, t_frames, c)                                  # b = -1 rows that look like real ones
    target = torch.from_numpy(np.concatenate(clips + [padding], 0)).to("cuda:0")
    row_start = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).to("cuda:0")
    return logit, target, row_start, clips


def _reference(ops, logit, clips, c):
    """B calls of the existing entry point -> (int32 bits per clip, valid flags)."""
    bits, valid = [], []
    for k, rows in enumerate(clips):
        if len(rows) == 0:
            bits.append(0)
            valid.append(0)
            continue
        own = rows.copy()
        own[:, 0] -= k                                                         # clip k alone: its rows carry b = 0
        loss = ops.adyolo_loss(logit[k:k + 1].contiguous(), torch.from_numpy(own).to("cuda:0"), c, GRID, ANCHORS,
                               need_grad=False)[0]
        bits.append(int(loss.view(torch.int32).item()))
        valid.append(1)
    return bits, valid


def _check(ops, logit, target, row_start, clips, c, acc=None):
    want, want_valid = _reference(ops, logit, clips, c)
    loss, valid = ops.adyolo_loss_per_clip(logit, target, row_start, c, GRID, ANCHORS, acc=acc)
    torch.cuda.synchronize()
    got = loss.view(torch.int32).cpu().tolist()
    print("per-clip bits", [hex(v & 0xffffffff) for v in got], "reference", [hex(v & 0xffffffff) for v in want])
    assert valid.cpu().tolist() == want_valid
    assert got == want
    return loss.cpu().numpy(), want_valid


@pytest.mark.parametrize("counts", [(33,), (0,), (32, 0, 257), (0, 1, 31, 0, 32, 33, 257, 0)],
                         ids=["B1", "B1-empty", "B3", "B8-empty-first-middle-last"])
def test_row_counts_mixed_within_a_batch(ops, counts):
    logit, target, row_start, clips = _case(11 + len(counts), counts, 2, 12)
    _check(ops, logit, target, row_start, clips, 12)


@pytest.mark.parametrize("c", [12, 13])
@pytest.mark.parametrize("t_frames", [1, 2, 8])
def test_anchor_tiles_and_class_counts(ops, t_frames, c):
    logit, target, row_start, clips = _case(100 * c + t_frames, (33, 0, 257), t_frames, c)
    _check(ops, logit, target, row_start, clips, c)


def test_assign_grid_stride_past_32_x_1024_rows(ops):
    logit, target, row_start, clips = _case(7, (32800, 33), 8, 12)
    _check(ops, logit, target, row_start, clips, 12)


def test_main_grid_stride_past_2048_tiles_per_clip(ops):
    logit, target, row_start, clips = _case(8, (257, 33), 3300, 12)
    assert 3300 * GRID[0] * GRID[1] * ANCHORS > 2048 * 256
    _check(ops, logit, target, row_start, clips, 12)


def test_positives_by_arg_min_alone_and_no_positive_at_all(ops):
    """Clip 0: every row far from its cell, so no anchor is inside 10 degrees and the positives of that threshold are the
    arg-min anchors alone.  Clip 1: every row in a frame past the output (what a CSV with late frames gives): no positive at
    any threshold -- the existing call's bits (a 0 / 0), whatever they are, are the per-clip call's bits."""
    logit, target, row_start, clips = _case(21, (33, 31, 32), 2, 12, far=(0,))
    clips[1][:, 1] += 2
    target[33:64, 1] += 2
    _check(ops, logit, target, row_start, clips, 12)


def test_padding_and_neighbouring_clips_do_not_contribute(ops):
    """A row inside clip 0's range that names clip 1 is skipped (as the one-clip call skips a row with b = 1) and marks no
    anchor of clip 1; rows past row_start[B] (b = -1 or not) are never read."""
    logit, target, row_start, clips = _case(31, (33, 32), 2, 12, pad=40)
    clips[0][5, 0] = 1.0
    target[5, 0] = 1.0
    target[65 + 3, 0] = 1.0                                                    # a padding row that names a real clip
    _check(ops, logit, target, row_start, clips, 12)
    dirty = target.clone()
    dirty[65:, 1:] = 0.0
    dirty[65:, 0] = 0.0                                                        # padding that looks like rows of clip 0, cell (0, 0, 0)
    _check(ops, logit, dirty, row_start, clips, 12)


def test_accumulator_is_the_sequential_float32_sum(ops):
    counts = (0, 1, 31, 0, 32, 33, 257, 0)
    logit, target, row_start, clips = _case(41, counts, 2, 12)
    acc = ops.loss_accumulator("cuda:0")
    losses, valid = _check(ops, logit, target, row_start, clips, 12, acc=acc)
    total, n = np.float32(0.0), 0
    for v, ok in zip(losses, valid):
        if ok:
            total = np.float32(total + np.float32(v))
            n += 1
    got = acc.cpu().numpy()
    assert got[0].view(np.int32) == total.view(np.int32) and got[1] == n == 5
    _check(ops, logit, target, row_start, clips, 12, acc=acc)                  # a second batch runs on from the first
    for v, ok in zip(losses, valid):
        if ok:
            total = np.float32(total + np.float32(v))
    one = torch.tensor([0.375], device="cuda:0")
    ops.loss_accumulate(acc, one)                                              # a class-wise clip's loss through the same accumulator
    ops.loss_accumulate(acc, torch.tensor([1.5, 2.5], device="cuda:0"), torch.tensor([0, 1], dtype=torch.int32, device="cuda:0"))
    total = np.float32(np.float32(total + np.float32(0.375)) + np.float32(2.5))
    got = acc.cpu().numpy()
    assert got[0].view(np.int32) == total.view(np.int32) and got[1] == 12
    assert float(got[0]) / int(got[1]) == float(total) / 12
