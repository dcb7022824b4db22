"""Bars shared by the GPU test modules that compare a kernel with float64 (tests/test_gpu_block_stage.py,
tests/test_gpu_conformer_stage.py).  Neither bar is taken from what a kernel returns:

* value: err = max |q - q64| / max |q64| must stay below max(4 err_ref, 16 * 2^-24), err_ref being the same error of a plain
  float32 PyTorch-CPU evaluation of the same formula on the same inputs (``value_check``);
* sums: |sum - sum64| <= bound per entry, bound computed from the inputs (``oracle.seresnet.fp32_sum_bound``; ``sum_check``).

Every check prints its figures."""
import torch

U = 2.0 ** -24                    # unit roundoff of float32
FLOOR = 16 * U


def d64(t):
    return t.detach().cpu().double()


def value_check(what, got, ref64, ref32, keep=None):
    """err_gpu <= max(4 err_ref, 16 * 2^-24), both relative to max |ref64|.  keep (bool tensor): the elements compared."""
    got, ref64, ref32 = d64(got), d64(ref64), d64(ref32)
    assert got.shape == ref64.shape == ref32.shape, "%s: shapes %s %s %s" % (what, tuple(got.shape), tuple(ref64.shape), tuple(ref32.shape))
    assert bool(torch.isfinite(got).all()), "%s: not finite" % what
    scale = float(ref64.abs().max())
    dg, dr = (got - ref64).abs(), (ref32 - ref64).abs()
    if keep is not None:
        dg, dr = dg[keep], dr[keep]
    err_gpu = float(dg.max()) / scale if scale > 0 else float(dg.max())
    err_ref = float(dr.max()) / scale if scale > 0 else float(dr.max())
    bar = max(4 * err_ref, FLOOR)
    print("%-58s err_gpu %.3e  err_ref %.3e  bar %.3e  (float64 absmax %.3e)" % (what, err_gpu, err_ref, bar, scale))
    assert err_gpu <= bar, "%s: err_gpu %.3e > bar %.3e (err_ref %.3e, float64 absmax %.3e)" % (what, err_gpu, bar, err_ref, scale)
    return err_gpu


def sum_check(what, got, ref64, bound):
    """|got - ref64| <= bound, entry by entry (bound: a tensor computed from the inputs)."""
    got, ref64, bound = d64(got), d64(ref64), d64(bound)
    assert got.shape == ref64.shape == bound.shape, "%s: shapes %s %s %s" % (what, tuple(got.shape), tuple(ref64.shape), tuple(bound.shape))
    assert bool(torch.isfinite(got).all()), "%s: not finite" % what
    err = (got - ref64).abs()
    ok = err <= bound
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    scale = float(ref64.abs().max())
    print("%-58s worst err / bound %.3e  (max err %.3e, float64 absmax %.3e)" % (what, worst, float(err.max()), scale))
    assert bool(ok.all()), "%s: %d of %d entries over the a-priori bound, worst err / bound %.3e (max err %.3e, absmax %.3e)" % (
        what, int((~ok).sum()), ok.numel(), worst, float(err.max()), scale)
    return worst


def value_check_heads(what, got, ref64, ref32s, heads, allow=None):
    """``value_check`` for attention tensors [B][T][heads * D]: the same bar head by head, every error relative to the float64
    absmax of that head's columns over the samples given.  ref32s: one float32 evaluation or a tuple of them (err_ref = the
    largest).  allow: an element-wise absolute allowance derived from the inputs (same shape), taken off |got - ref64| before
    the comparison; the raw figure is printed as well.  Returns the worst (err_gpu, err_ref, bar) by err_gpu / bar."""
    if not isinstance(ref32s, (tuple, list)):
        ref32s = (ref32s,)
    got, ref64 = d64(got), d64(ref64)
    assert got.shape == ref64.shape, "%s: shapes %s %s" % (what, tuple(got.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(got).all()), "%s: not finite" % what
    b, t, e = ref64.shape
    hv = lambda z: z.reshape(b, t, heads, e // heads)                       # noqa: E731
    scale = hv(ref64).abs().amax(dim=(0, 1, 3))
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    raw = (got - ref64).abs()
    if allow is not None:
        print("%-58s raw err %.3e, the allowance covers up to %.3e (of each head's absmax)" % (
            what, float((hv(raw).amax(dim=(0, 1, 3)) / scale).max()), float((hv(d64(allow)).amax(dim=(0, 1, 3)) / scale).max())))
        raw = (raw - d64(allow)).clamp(min=0)
    err_gpu = hv(raw).amax(dim=(0, 1, 3)) / scale
    err_ref = torch.zeros_like(err_gpu)
    for r in ref32s:
        r = d64(r)
        assert r.shape == ref64.shape
        err_ref = torch.maximum(err_ref, hv((r - ref64).abs()).amax(dim=(0, 1, 3)) / scale)
    bar = torch.clamp(4 * err_ref, min=FLOOR)
    i = int(torch.argmax(err_gpu / bar))
    print("%-58s err_gpu %.3e  err_ref %.3e  bar %.3e  (worst head %d of %d, its float64 absmax %.3e)" % (
        what, float(err_gpu[i]), float(err_ref[i]), float(bar[i]), i, heads, float(scale[i])))
    assert bool((err_gpu <= bar).all()), "%s: head %d err_gpu %.3e > bar %.3e (err_ref %.3e)" % (
        what, i, float(err_gpu[i]), float(bar[i]), float(err_ref[i]))
    return float(err_gpu[i]), float(err_ref[i]), float(bar[i])


class Collect:
    """Run several checks of one test to the end, so that a run prints every figure, then fail with all their messages."""

    def __init__(self):
        self.failed = []

    def __call__(self, check, *args, **kw):
        try:
            return check(*args, **kw)
        except AssertionError as e:
            self.failed.append(str(e).splitlines()[0])
            return None

    def finish(self):
        assert not self.failed, "; ".join(self.failed)
