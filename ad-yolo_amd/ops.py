"""Tensor-level wrappers over the C ABI (include/adyolo_hip.h).

PyTorch is used here only as plumbing: device memory (caching allocator), the current HIP stream and,
in ``dist.py``, torch.distributed/RCCL.  Every function launches hand-written gfx950 kernels through
``libadyolo_hip.so``; nothing in this module computes with ATen ops.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib

_c = _lib.call
NULL = ctypes.c_void_p(0)


def _p(t):
    if t is None:
        return NULL
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.AdyoloHipError("adyolo ops need tensors on a HIP device (got %s); there is no CPU path" % t.device)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.AdyoloHipError("adyolo ops need contiguous float32 tensors (got %s, contiguous=%s)"
                                      % (t.dtype, t.is_contiguous()))


def _new(like, *shape):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _zeros(like, *shape):
    return torch.zeros(shape, dtype=torch.float32, device=like.device)


# ---------------------------------------------------------------------------------------------- exact data parallelism
class ExactDP:
    """Switch + collectives of EXACT data parallelism (``train.TrainStep(exact=True)`` / ADYOLO_DP_EXACT=1): every quantity
    the reference normalises over the batch is formed over the batch of ALL ranks, so N ranks on N equal shards compute what
    one device computes on the concatenated batch (SURVEY.md section 8e "optional"; the reference itself is single-device,
    src/train.py:40-62).  Three places need an exchange, all tiny:
      * BatchNorm forward (36 layers): the per-sample sums (sum, sum of squares) [B][C] of every rank are all-gathered in rank
        order and finished by the same kernel as on one device -> bit-identical batch statistics and running statistics;
      * BatchNorm backward (36 layers, incl. the BatchNorm folded into the SE tail): the two per-channel sums are all-reduced
        for the dx formula; the parameter gradients written to the flat buffer stay local (the bucket all-reduce sums them);
      * the AD-YOLO loss: the four counts (distinct positives per threshold, responsible pairs) are all-reduced between the
        assignment and the pass over the logits; the returned loss is the sum of the ranks' shares.
    Gradients are then SUMMED over the ranks (not averaged).  Off (world 1, or not enabled): everything is local, the
    DDP-conventional semantics of ``dist.py``."""

    def __init__(self):
        self.on, self.world, self.group = False, 1, None

    def enable(self, group=None):
        import torch.distributed as dist
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.on = self.world > 1
        return self.on

    def disable(self):
        self.on = False

    def all_reduce(self, t):
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    def gather_rows(self, t):
        """[n][c] of every rank -> [world * n][c] in rank order (== the row order of the concatenated batch)."""
        import torch.distributed as dist
        parts = [torch.empty_like(t) for _ in range(self.world)]
        dist.all_gather(parts, t.contiguous(), group=self.group)
        return torch.cat(parts, 0)


EXACT = ExactDP()


def EXACT_world_mean(t, group=None):
    """``t`` averaged over the ranks (in place; a no-op without a process group)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        t /= dist.get_world_size(group)
    return t


# Device -> host through page-locked staging buffers (one per shape and dtype, reused): a pageable ``tensor.cpu()`` of the decoded
# predictions (5.8 MB per 60 s clip) runs at a fifth of the PCIe rate and was a third of an eight-clip evaluation pass.
_PINNED = {}


def to_host(t):
    """``t`` copied into a reused page-locked host tensor of its shape (valid until the next ``to_host`` of that shape)."""
    key = (tuple(t.shape), t.dtype)
    buf = _PINNED.get(key)
    if buf is None:
        if len(_PINNED) >= 16:                       # clips of many different lengths: keep the page-locked pool bounded
            _PINNED.pop(next(iter(_PINNED)))
        buf = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        _PINNED[key] = buf
    buf.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return buf


# Results whose size the device decides (the selected detection rows): page-locked buffers that grow to the largest request.
_PINNED_GROW = {}


def to_host_many(*ts):
    """Device tensors of any shape copied into reused, growing page-locked host tensors (one per argument position and
    dtype) with ONE synchronisation; the returned views are valid until the next ``to_host_many``."""
    outs = []
    for i, t in enumerate(ts):
        key = (i, t.dtype)
        buf = _PINNED_GROW.get(key)
        if buf is None or buf.numel() < t.numel():
            buf = torch.empty(1 << max(16, (t.numel() - 1).bit_length()), dtype=t.dtype, pin_memory=True)
            _PINNED_GROW[key] = buf
        view = buf[:t.numel()].view(t.shape)
        view.copy_(t, non_blocking=True)
        outs.append(view)
    if ts:
        torch.cuda.current_stream(ts[0].device).synchronize()
    return outs


# Parameter / buffer epoch: bumped by everything that writes parameters or BatchNorm buffers IN PLACE through a kernel (no
# torch version bump): the optimizer step, the training-mode BatchNorm statistics, the start-up broadcast.  Evaluation-mode
# caches (BatchNorm affines, ``functional._BNState.eval_affine``; recorded forward graphs, ``graph.ForwardGraphs``) are keyed on it.
PARAMS_EPOCH = [0]


def params_changed():
    PARAMS_EPOCH[0] += 1


# ---------------------------------------------------------------------------------------------- conv
def conv_algo():
    """'winograd4' (default since round 4: F(4x4,3x3) on the fp32 MFMA where ``_w4_eligible`` says so -- 4x fewer matrix FLOPs
    than the direct form -- and F(2x2,3x3) elsewhere), 'winograd' (F(2x2,3x3) everywhere, 2.25x fewer) or 'direct' (implicit
    GEMM); chosen per call of ``pack_w3x3`` / ``WinoPackSet.refresh`` from ADYOLO_CONV_ALGO."""
    a = os.environ.get("ADYOLO_CONV_ALGO", "winograd4").lower()
    if a not in ("winograd4", "winograd", "direct"):
        raise _lib.AdyoloHipError("ADYOLO_CONV_ALGO must be 'winograd4', 'winograd' or 'direct' (got %r)" % a)
    return a


# Dispatch switches of the 3x3 convolutions, read from the environment ONCE -- at import, and again by ``reload_thresholds()``
# (tests and A/B tools that move one call it; README "Switches") -- into ONE table that every launch consults: the numeric
# thresholds AND the on / off switches (round 5 ADVICE: ADYOLO_W4_PERSIST / _NARROW / ADYOLO_WINO1D used to be read per launch,
# three getenv calls inside every adyolo_wino4_fwd, while the thresholds were frozen).  The library reads no environment: the two
# switches it consults are pushed from this table (``_push_switches``: when the library is loaded and on every reload), so host
# and library cannot differ (round 6 ADVICE: they used to read the environment at different moments).  ADYOLO_CONV_ALGO stays a
# per-call read (``conv_algo``): it selects the algorithm, is validated where it is read and is part of the graph stamp on its own.
W4_THRESHOLDS = {}
_THRESHOLD_KEYS = ("min_k", "min_k_addend", "min_wgs", "min_wgrad_work", "min_k_32")


def reload_thresholds():
    """ADYOLO_W4_MIN_K (32; 64 until round 6 -- with the persistent kernel the 32 -> 64 stage transition runs 0.56 -> 0.42 ms on
    F(4x4)): smallest contraction that gets the F(4x4) form packed; ADYOLO_W4_MIN_K_ADDEND (32; 128 until the
    persistent kernel of round 5): the same for launches that add a tensor in their epilogue; ADYOLO_W4_MIN_WGS (200): below
    that many 64-channel x patch work items a launch stays on the F(2x2) kernel (two workgroups per CU); ADYOLO_W4W_MIN_WORK
    (6 M): smallest (tile rows of 16-column runs) x Cin x Cout = N W/16 H/4 Cin Cout for the F(4x4)-domain weight gradient
    (``wgrad_form``; measured crossover with the F(2x2)-domain kernel at 3.3-6.5 M at every stage since the kernel stages between
    its MFMA groups -- 16 x 20 s: 1.18-1.41 x at every block shape, 8 x 20 s: 0.8-0.9 x at the 3.3 M stage transitions, 1.0-1.3 x
    from 6.5 M on: profiles/r05_w4w_small_shapes.txt; 2^24 with the first version of the kernel);
    ADYOLO_W4_MIN_K_32 (32): smallest contraction for the F(4x4) form with 32-channel OUTPUT blocks (stage 1's 32 -> 32 layers
    and the 64 -> 32 data-gradient: 1.04-1.14 x the F(2x2) kernel per launch, profiles/r05_w4p_nb1_ab.txt).
    On / off switches in the same table: ADYOLO_W4_PERSIST (persistent F(4x4) kernel; 0 = the one-patch form), ADYOLO_W4_NARROW
    (patches one / two tiles wide on maps up to 8 bins wide), ADYOLO_WINO1D (1-D Winograd along time on one-bin-wide maps),
    ADYOLO_WGRAD_ALGO (weight-gradient algorithm when it differs from ADYOLO_CONV_ALGO).
    Returns the numeric thresholds (``switch_table()``: everything)."""
    env = os.environ.get
    W4_THRESHOLDS.update(min_k=int(env("ADYOLO_W4_MIN_K", "32")),
                         min_k_addend=int(env("ADYOLO_W4_MIN_K_ADDEND", "32")),
                         min_wgs=int(env("ADYOLO_W4_MIN_WGS", "200")),
                         min_wgrad_work=int(env("ADYOLO_W4W_MIN_WORK", "6000000")),
                         min_k_32=int(env("ADYOLO_W4_MIN_K_32", "32")),
                         persist=env("ADYOLO_W4_PERSIST", "1") != "0",
                         narrow=env("ADYOLO_W4_NARROW", "1") != "0",
                         wino1d=env("ADYOLO_WINO1D", "1") != "0",
                         wgrad_algo=(env("ADYOLO_WGRAD_ALGO") or "").lower() or None)
    if _lib.loaded():                                  # (not loaded yet: ``_lib.load()`` pushes them, ``_lib.ON_LOAD``)
        _push_switches(_lib.load())
    return {k: W4_THRESHOLDS[k] for k in _THRESHOLD_KEYS}


def _push_switches(lib):
    lib.adyolo_set_switches((1 if W4_THRESHOLDS["persist"] else 0) | (2 if W4_THRESHOLDS["narrow"] else 0))


_lib.ON_LOAD.append(_push_switches)


def switch_table():
    """Every cached dispatch switch + the algorithm: what a recorded graph's kernel choice depends on besides its input shape
    (``graph.ForwardGraphs._stamp`` / ``StepGraphs`` key on it) and what bench.py echoes in ``dispatch``."""
    t = dict(W4_THRESHOLDS)
    t["conv_algo"] = conv_algo()
    return t


def switch_stamp():
    return tuple(sorted((k, str(v)) for k, v in switch_table().items()))


reload_thresholds()

# When set to a dict, ``conv3x3`` counts its launches in it: key = (kernel name, Cin, Cout, operand bits) -- the table bench.py prints as
# ``dispatch`` and tests/test_gpu_parity_scale.py asserts at the bench shape.
DISPATCH_LOG = None


def w4_narrow_ok(cin, cout):
    """A stride-1 3x3 convolution on a map at most 8 bins wide gets the persistent F(4x4) kernel with patches one / two tiles
    wide (``adyolo_wino4_fwd``, plain launches, 64-channel output blocks in both directions) -- the ResNet-Conformer's middle
    stages: 2.9 x the implicit GEMM at 32 x 800 x 4 x 128 (tools/wino4/narrow_check.py)."""
    return (conv_algo() == "winograd4" and cin % 64 == 0 and cout % 64 == 0 and _w4_eligible(cin, cout) and _w4_eligible(cout, cin)
            and W4_THRESHOLDS["narrow"] and W4_THRESHOLDS["persist"])


def _w4_eligible(k_gemm, n_gemm, allow32=False):
    """Does this GEMM direction (contraction over k_gemm channels, n_gemm output channels) get the F(4x4,3x3) form
    (csrc/wino4.hip, wino4p.hpp) packed beside the F(2x2) one?  The kernels take 16-channel pairs of the contraction and 64
    output channels per workgroup -- or 32 (round 5; the persistent kernel only, which deals 1 / 2 / 4 / 8 channel blocks to
    the XCDs: ``DualPack.pick`` keeps such a launch on F(2x2) when its operand combination has no persistent form).  One
    workgroup per CU: it wins by more the longer the contraction -- per launch at the bench shapes (round 5, persistent form)
    1.4-1.6 x the F(2x2) kernel at 256 channels, 1.3-1.4 x at 128, 1.2-1.4 x at 64; DESIGN.md, "F(4x4,3x3), round 5".
    ADYOLO_W4_MIN_K moves the threshold (``reload_thresholds``).  allow32: also 32-channel output blocks (``WinoPackSet``, whose
    ``DualPack`` can fall back; plain ``pack_w3x3`` packs them only on request)."""
    if k_gemm % 32 or k_gemm > 512:
        return False
    if n_gemm % 64 == 0:
        return k_gemm >= W4_THRESHOLDS["min_k"]
    return allow32 and n_gemm % 32 == 0 and n_gemm // 32 in (1, 2, 4, 8) and k_gemm >= W4_THRESHOLDS["min_k_32"]


def pack_w3x3(w, cin_pad, want_dgrad=True, algo=None, allow32=False):
    """w [Cout][Cin][3][3] -> (fwd pack, dgrad pack or None).

    direct:   wpk_fwd [Cout][9][cin_pad], wpk_dgrad [cin_pad][9][Cout]
    winograd: u_fwd [16][Cout/32][cin_pad/8][256], u_dgrad [16][cin_pad/32][Cout/8][256]  (needs both channel
              counts to be multiples of 32; the 8-channel stem stays direct).  ``conv3x3`` tells them apart by rank.
    winograd4: per direction the F(4x4,3x3) form [36][N/32][K/8][256] where ``_w4_eligible`` says so, else the F(2x2) form."""
    _chk(w)
    cout, cin = w.shape[0], w.shape[1]
    algo = algo or conv_algo()
    if algo == "winograd4" and cin_pad % 32 == 0 and cout % 32 == 0:
        # per direction: the F(4x4) form [36][N/32][K/8][256] where it applies, else the F(2x2) form
        f4, d4 = _w4_eligible(cin_pad, cout, allow32), want_dgrad and _w4_eligible(cout, cin_pad, allow32)
        uf = _new(w, 36 if f4 else 16, cout // 32, cin_pad // 8, 256)
        ud = _new(w, 36 if d4 else 16, cin_pad // 32, cout // 8, 256) if want_dgrad else None
        if f4 or d4:
            _c("adyolo_wino4_pack_w", _p(w), _p(uf if f4 else None), _p(ud if d4 else None), cout, cin, cin_pad, _stream())
        if not f4 or (want_dgrad and not d4):
            _c("adyolo_wino_pack_w", _p(w), _p(None if f4 else uf), _p(None if (d4 or not want_dgrad) else ud), cout, cin,
               cin_pad, _stream())
        return uf, ud
    if algo == "winograd" and cin_pad % 32 == 0 and cout % 32 == 0:
        uf = _new(w, 16, cout // 32, cin_pad // 8, 256)
        ud = _new(w, 16, cin_pad // 32, cout // 8, 256) if want_dgrad else None
        _c("adyolo_wino_pack_w", _p(w), _p(uf), _p(ud), cout, cin, cin_pad, _stream())
        return uf, ud
    wf = _new(w, cout, 9, cin_pad)
    wd = _new(w, cin_pad, 9, cout) if want_dgrad else None
    _c("adyolo_pack_w3x3", _p(w), _p(wf), _p(wd), cout, cin, cin_pad, _stream())
    return wf, wd


class DualPack:
    """Both Winograd forms of one filter direction: ``f4`` [36][N/32][K/8][256] for the F(4x4,3x3) kernel, ``f2`` [16][...] for
    the F(2x2) kernel.  ``conv3x3`` takes the F(4x4) form when its launch fills the chip and the F(2x2) form for small grids
    (one workgroup per CU and 32 x 16 / 16 x 32-pixel patches: a single 60 s clip is 76 workgroups at stage 4)."""
    __slots__ = ("f4", "f2")

    def __init__(self, f4, f2):
        self.f4, self.f2 = f4, f2

    def pick(self, n, h, w, cout, addend=False, persistent_ok=True):
        """addend: the launch adds a tensor in its epilogue (the data-gradient of a block's first convolution); until round 5 the
        F(2x2) kernel was the faster one there below 128 channels (ADYOLO_W4_MIN_K_ADDEND, now 32: no effect by default).  persistent_ok: the
        library takes the persistent form for the launch's operands (``adyolo_wino4_fwd_form`` == 2, asked by ``conv3x3``) -- with
        32-channel output blocks (cout % 64 != 0) there is no other F(4x4) kernel."""
        if cout % 64 and not (persistent_ok and W4_THRESHOLDS["persist"]):
            return self.f2
        wgs = _lib.load().adyolo_wino4_tiles(n, h, w) * ((cout + 63) // 64)
        if wgs < W4_THRESHOLDS["min_wgs"]:
            return self.f2
        if addend and self.f4.shape[2] * 8 < W4_THRESHOLDS["min_k_addend"]:
            return self.f2
        return self.f4


class WinoPackSet:
    """The Winograd-packed forms (forward + data-gradient) of a fixed list of 3x3 filters, refreshed by ONE launch
    (``adyolo_wino_pack_many``) instead of two per filter: ``refresh()`` at the start of a forward pass, ``get(i)`` ->
    (u_fwd, u_dgrad) of filter i.  The buffers and the descriptor table are allocated once and rebuilt only when a filter's
    storage moves (``.to()``, re-homing into a flat parameter buffer)."""

    def __init__(self):
        self.key = self.stamp = None

    def refresh(self, weights, frozen=False):
        """frozen (evaluation mode): skip the launch when nothing was written to the filters since the last one
        (``PARAMS_EPOCH`` for in-place kernels, the tensors' version counters for ``copy_`` / ``load_state_dict``)."""
        w4 = conv_algo() == "winograd4"
        key = (w4, W4_THRESHOLDS["min_k"], W4_THRESHOLDS["min_k_32"]) + tuple(w.data_ptr() for w in weights)
        stamp = (PARAMS_EPOCH[0],) + tuple(w._version for w in weights)
        if frozen and key == self.key and stamp == self.stamp:
            return self
        self.stamp = stamp
        if key != self.key:
            dev = weights[0].device
            self.packs, rows, rows4 = [], [], []
            for w in weights:
                _chk(w)
                cout, cin = w.shape[0], w.shape[1]
                if cout % 32 or cin % 32:
                    raise _lib.AdyoloHipError("WinoPackSet: channel counts must be multiples of 32")
                # per direction: the F(2x2) form always, the F(4x4) form [36][N/32][K/8][256] beside it where it applies
                # (winograd4): ``conv3x3`` picks by the size of the launch (``DualPack``)
                f4, d4 = w4 and _w4_eligible(cin, cout, True), w4 and _w4_eligible(cout, cin, True)
                uf = _new(w, 16, cout // 32, cin // 8, 256)
                ud = _new(w, 16, cin // 32, cout // 8, 256)
                rows.append([w.data_ptr(), uf.data_ptr(), ud.data_ptr(), cout, cin, cin, 0, 0])
                if f4 or d4:
                    uf4 = _new(w, 36, cout // 32, cin // 8, 256) if f4 else None
                    ud4 = _new(w, 36, cin // 32, cout // 8, 256) if d4 else None
                    rows4.append([w.data_ptr(), uf4.data_ptr() if f4 else 0, ud4.data_ptr() if d4 else 0, cout, cin, cin, 0, 0])
                    uf = DualPack(uf4, uf) if f4 else uf
                    ud = DualPack(ud4, ud) if d4 else ud
                self.packs.append((uf, ud))
            self.table = torch.tensor(rows, dtype=torch.int64, device=dev) if rows else None
            self.table4 = torch.tensor(rows4, dtype=torch.int64, device=dev) if rows4 else None
            self.nrows, self.nrows4 = len(rows), len(rows4)
            self.max_cout = max(w.shape[0] for w in weights)
            self.max_cin = max(w.shape[1] for w in weights)
            self.key = key
        if self.table is not None:
            _c("adyolo_wino_pack_many", _p(self.table), self.nrows, self.max_cout, self.max_cin, _stream())
        if self.table4 is not None:
            _c("adyolo_wino4_pack_many", _p(self.table4), self.nrows4, self.max_cout, self.max_cin, _stream())
        return self

    def get(self, i):
        return self.packs[i]


# first axis of the pack (transform points of a Winograd form; 0: the direct pack, rank 3) -> entry point, its patch count, kernel name
_CONV3X3_FORMS = {36: ("adyolo_wino4_fwd", "adyolo_wino4_tiles", None),                     # (named by the library's form: below)
                  16: ("adyolo_wino_fwd", "adyolo_wino_tiles", "wino_fwd_kernel"),
                  0: ("adyolo_conv3x3_fwd", "adyolo_conv3x3_tiles", "conv3x3_fwd_kernel")}
_W4_KERNELS = {1: "wino4_fwd_kernel", 2: "wino4p_fwd_kernel"}                             # by ``adyolo_wino4_fwd_form``


def conv3x3(x, wpk, cout, bias=None, addend=None, relu=False, addend_mask=None, in_affine=None, want_stats=False,
            stat_bn=None, stat_mask=None):
    """x [N][H][W][Cin] -> [N][H][W][cout];  wpk from ``pack_w3x3`` (direct [cout][9][Cin] or Winograd, rank 4).

    in_affine=(scale, shift): the producer's BatchNorm affine is applied while staging x (padding stays 0);
    addend_mask: addend is multiplied by (mask > 0); want_stats: also return the per-patch channel sums
    [2][tiles][cout] of the output for ``bn_stats_tiles``; stat_bn=(aux, mean, invstd): the second per-patch sum
    becomes sum(y * xhat(aux)) (the output is a gradient, aux the BatchNorm input) for ``bn_bwd(..., tile_stats=)``;
    stat_mask: both sums are taken of y * (stat_mask > 0) (for ``se_tail_bwd(..., tile_stats=)`` of the block below).
    addend_mask / stat_mask may also be the int64 ReLU-mask BITS ``se_tail_fwd(..., want_mask=True)`` returned."""
    mbits = 0
    if addend_mask is not None and addend_mask.dtype == torch.int64:
        mbits |= 1
    if stat_mask is not None and stat_mask.dtype == torch.int64:
        mbits |= 2
    n, h, w, cin = x.shape
    # operands present, as the ADYOLO_W4_* bits of include/adyolo_hip.h: 1 statistics, 2 addend, 4 addend mask, 8 stat_bn, 16 stat mask
    epi = (1 if want_stats else 0) | (2 if addend is not None else 0) | (4 if addend_mask is not None else 0) | \
          (8 if stat_bn is not None else 0) | (16 if stat_mask is not None else 0)
    lib = _lib.load()
    # the library decides which F(4x4) kernel such a launch gets -- 2 persistent, 1 one-patch, 0 none -- and the host asks
    w4_form = lib.adyolo_wino4_fwd_form(cout, epi | (32 if bias is not None else 0), mbits)
    if isinstance(wpk, DualPack):
        wpk = wpk.pick(n, h, w, cout, addend is not None, w4_form == 2)
    form = wpk.shape[0] if wpk.dim() == 4 else 0
    if form == 36 and not w4_form:
        raise _lib.AdyoloHipError("conv3x3: a F(4x4) pack with %d output channels needs an operand combination the persistent kernel "
                                  "is built for (pack with ops.DualPack / WinoPackSet to fall back to F(2x2))" % cout)
    fn, tiles_fn, name = _CONV3X3_FORMS[form]
    _chk(x, wpk, bias, addend, None if mbits & 1 else addend_mask, None if mbits & 2 else stat_mask)
    y = _new(x, n, h, w, cout)
    stats = _new(x, 2, getattr(lib, tiles_fn)(n, h, w), cout) if want_stats else None
    sc, sh = in_affine if in_affine is not None else (None, None)
    sa, sm, si = stat_bn if stat_bn is not None else (None, None, None)
    _c(fn, _p(x), _p(wpk), _p(bias), _p(addend), _p(addend_mask),
       _p(sc), _p(sh), _p(y), _p(stats), _p(sa), _p(sm), _p(si), _p(stat_mask), n, h, w, cin, cout, int(relu), mbits,
       _stream())
    if DISPATCH_LOG is not None:
        k = (name or _W4_KERNELS[w4_form], cin, cout, epi)
        DISPATCH_LOG[k] = DISPATCH_LOG.get(k, 0) + 1
    return (y, stats) if want_stats else y


def wgrad_form(cin, cout, algo=None, shape=None):
    """-> (kernel name, matrix FLOPs issued / direct-convolution FLOPs) of the weight-gradient ``conv3x3_wgrad`` launches for these
    channel counts (and, with ``shape`` = (N, H, W), this launch): the Winograd F(4x4,3x3) domain (csrc/wino4w.hip, round 5: 9
    multiplies per 36) under 'winograd4' when the kernel takes the shape (Cout % 32, W % 16, H % 4) and the launch is large
    enough (ADYOLO_W4W_MIN_WORK; one workgroup per CU: small launches stay on the two-per-CU kernel); else
    the F(2x2,3x3) domain (16 per 36) when both channel counts are multiples of 32; else the direct implicit GEMM.  The ONE
    place that decides it -- ``conv3x3_wgrad`` and bench.py both ask here."""
    algo = algo or W4_THRESHOLDS["wgrad_algo"] or conv_algo()
    if algo == "winograd4" and shape is not None and cin % 32 == 0 and cout % 32 == 0:
        n, h, w = shape
        if (w % 16 == 0 or w in (4, 8)) and h % 4 == 0 and n * w // 16 * (h // 4) * cin * cout >= W4_THRESHOLDS["min_wgrad_work"] and \
                _lib.load().adyolo_wino4_wgrad_slabs(n, h, w, cin, cout) > 0:
            return "wino4_wgrad_kernel", 9.0 / 36.0
    if algo in ("winograd", "winograd4") and cin % 32 == 0 and cout % 32 == 0:
        return "wino_wgrad_kernel", 16.0 / 36.0
    return "conv3x3_wgrad_kernel", 1.0


_WGRAD_FORMS = {"wino4_wgrad_kernel": ("adyolo_wino4_wgrad", 36), "wino_wgrad_kernel": ("adyolo_wino_wgrad", 16)}   # entry point, points


def conv3x3_wgrad(x, dy, cin_real, in_affine=None, algo=None, out=None):
    """x [N][H][W][Cin], dy [N][H][W][Cout] -> dw [Cout][cin_real][3][3] (x optionally seen through an affine).

    Winograd form (default) when both channel counts are multiples of 32, else the direct implicit GEMM."""
    _chk(x, dy)
    n, h, w, cin = x.shape
    cout = dy.shape[3]
    sc, sh = in_affine if in_affine is not None else (None, None)
    dw = out if out is not None else _new(x, cout, cin_real, 3, 3)      # out: e.g. the parameter's slice of the flat gradient buffer
    form = wgrad_form(cin, cout, algo, (n, h, w))[0]
    if DISPATCH_LOG is not None:
        k = (form, cin, cout, 1 if in_affine is not None else 0)
        DISPATCH_LOG[k] = DISPATCH_LOG.get(k, 0) + 1
    if form in _WGRAD_FORMS:
        fn, points = _WGRAD_FORMS[form]
        nslab = getattr(_lib.load(), fn + "_slabs")(n, h, w, cin, cout)
        if nslab <= 0:
            raise _lib.AdyoloHipError("%s_slabs rejected the shape" % fn)
        slabs = _new(x, nslab, points, cin, cout)
        du = _new(x, points, cin, cout)
        _c(fn, _p(x), _p(dy), _p(sc), _p(sh), _p(slabs), _p(du), _p(dw), n, h, w, cin, cin_real, cout, _stream())
        return dw
    nslab = _lib.load().adyolo_conv3x3_wgrad_slabs(n, h, w, cin, cout)
    if nslab <= 0:
        raise _lib.AdyoloHipError("conv3x3_wgrad_slabs rejected the shape")
    cinp = ((cin + 31) // 32) * 32
    slabs = _new(x, nslab, cout, 9, cinp)
    _c("adyolo_conv3x3_wgrad", _p(x), _p(dy), _p(sc), _p(sh), _p(slabs), _p(dw), n, h, w, cin, cin_real, cout, _stream())
    return dw


# ---------------------------------------------------------------------------------------------- gemm
def gemm(a, b, m, n, k, lda, ldb, trans_a=False, trans_b=False, bias=None, out=None, ldc=None, accumulate=False,
         splits=1):
    """C[m][n] = sum_k opA(m,k) opB(n,k) (+bias).  ``a``/``b``/``out`` may be views with an offset."""
    if ldc is None:
        ldc = n
    if out is None:
        out = _new(a, m, n)
        ldc = n
    slabs = None
    if splits > 1:
        slabs = _new(a, splits, m, n)
    _c("adyolo_gemm", _p(a), _p(b), _p(bias), _p(out), _p(slabs), m, n, k, lda, ldb, ldc, int(trans_a), int(trans_b),
       splits, int(accumulate), _stream())
    return out


def wgrad_splits(m, n, k):
    """Split-K factor for a weight-gradient GEMM (m x n output, contraction k = rows of the batch): enough 128 x 64 output
    tiles x splits to put ~2 workgroups on each of the 256 CUs, at least 512 contraction rows per split, at most 256
    (a 64 x 32 output over 2.5 M rows -- the 1x1 shortcut convolution of stage 2 -- ran on 64 workgroups with the old cap
    of 64: 1.54 ms for a 0.94 GB read)."""
    tiles = ((m + 127) // 128) * ((n + 63) // 64)
    want = (512 + tiles - 1) // tiles
    return max(1, min(256, want, k // 512))


def linear(x2d, w, bias=None):
    """x2d [R][K] @ w[N][K]^T + bias."""
    _chk(x2d, w, bias)
    r, k = x2d.shape
    return gemm(x2d, w, r, w.shape[0], k, k, k, bias=bias)


def linear_bwd(x2d, w, dy2d, need_dx=True, out_dw=None, out_db=None, need_db=True):
    """-> dx [R][K], dw [N][K], db [N].  out_dw / out_db: write there instead (e.g. the parameters' slices of the flat
    gradient buffer, ``functional.GradSink``)."""
    _chk(x2d, w, dy2d)
    r, k = x2d.shape
    n = w.shape[0]
    if n % 4:
        return _linear_bwd_padded(x2d, w, dy2d, need_dx, out_dw, out_db, need_db)
    dx = gemm(dy2d, w, r, k, n, n, k, trans_b=True) if need_dx else None
    dw = gemm(dy2d, x2d, n, k, r, n, k, trans_a=True, trans_b=True, splits=wgrad_splits(n, k, r), out=out_dw)
    db = colsum(dy2d, out=out_db) if need_db else None
    return dx, dw, db


def _linear_bwd_padded(x2d, w, dy2d, need_dx, out_dw, out_db, need_db):
    """``linear_bwd`` for an output width n that is no multiple of 4 (class-wise heads at 13 classes: 13, 39, 117).  dy is
    operand A of both GEMMs with lda = n, which the 16-byte fetches refuse; they run on copies padded to roundup4(n) with
    exact zeros -- dy [R][n4], w [n4][K] -- which add nothing to any sum, and dW's first n rows are copied out."""
    r, k = x2d.shape
    n = w.shape[0]
    n4 = (n + 3) // 4 * 4
    dyp = _zeros(dy2d, r, n4)
    dyp[:, :n].copy_(dy2d)
    dx = None
    if need_dx:
        wp = _zeros(w, n4, k)
        wp[:n].copy_(w)
        dx = gemm(dyp, wp, r, k, n4, n4, k, trans_b=True)
    dw = gemm(dyp, x2d, n4, k, r, n4, k, trans_a=True, trans_b=True, splits=wgrad_splits(n4, k, r))[:n]
    if out_dw is not None:
        out_dw.view(n, k).copy_(dw)
        dw = out_dw
    db = colsum(dy2d, out=out_db) if need_db else None
    return dx, dw, db


def colsum(a2d, out=None, accumulate=False):
    r, c = a2d.shape
    if out is None:
        out = _new(a2d, c)
        accumulate = False
    partial = _new(a2d, 1024, c)
    _c("adyolo_colsum", _p(a2d), _p(out), _p(partial), r, c, a2d.stride(0), int(accumulate), _stream())
    return out


def add(a, b):
    _chk(a, b)
    y = torch.empty_like(a)
    _c("adyolo_add", _p(a), _p(b), _p(y), a.numel(), _stream())
    return y


def scale_dev(a, scalar_dev):
    """a * scalar_dev[0], the scalar staying on the device (no host sync)."""
    _chk(a, scalar_dev)
    y = torch.empty_like(a)
    _c("adyolo_scale_dev", _p(a), _p(scalar_dev), _p(y), a.numel(), _stream())
    return y


def mul(a, b):
    _chk(a, b)
    y = torch.empty_like(a)
    _c("adyolo_mul", _p(a), _p(b), _p(y), a.numel(), _stream())
    return y


# ---------------------------------------------------------------------------------------------- norm
def bn_stats(x, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """x [N][H][W][C] -> per-sample sums [N][C], mean [C], invstd [C]; updates running stats in place."""
    _chk(x, running_mean, running_var)
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    ssum, mean, invstd = _new(x, n, c), _new(x, c), _new(x, c)
    partial = _new(x, 4 * 1024 * c)
    if EXACT.on and running_mean is not None:         # training statistics over the batch of all ranks
        _c("adyolo_bn_stats", _p(x), _p(ssum), _p(mean), _p(invstd), NULL, NULL, _p(partial), n, hw, c, momentum, eps, _stream())
        ps1 = partial[3 * 1024 * c:3 * 1024 * c + n * c].view(n, c)          # per-sample sums of squares (layout of the C side)
        g0, g1 = EXACT.gather_rows(ssum), EXACT.gather_rows(ps1)
        _c("adyolo_bn_finish", _p(g0), _p(g1), _p(mean), _p(invstd), _p(running_mean), _p(running_var), NULL, NULL, NULL, NULL,
           g0.shape[0], hw, c, momentum, eps, _stream())
        return ssum, mean, invstd
    _c("adyolo_bn_stats", _p(x), _p(ssum), _p(mean), _p(invstd), _p(running_mean), _p(running_var), _p(partial), n,
       hw, c, momentum, eps, _stream())
    return ssum, mean, invstd


def bn_stats_tiles(tile_stats, n, hw, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, gamma=None,
                   beta=None):
    """BatchNorm statistics from the per-patch sums of a convolution epilogue ([2][tiles][C]) -> ssum, mean, invstd
    (+ scale = gamma*invstd, shift = beta - mean*scale from the same finishing launch when gamma / beta are given)."""
    _chk(tile_stats, running_mean, running_var, gamma, beta)
    tiles, c = tile_stats.shape[1], tile_stats.shape[2]
    ssum, mean, invstd = _new(tile_stats, n, c), _new(tile_stats, c), _new(tile_stats, c)
    scale, shift = (_new(tile_stats, c), _new(tile_stats, c)) if gamma is not None else (None, None)
    if EXACT.on and running_mean is not None:         # training statistics over the batch of all ranks
        ps1 = _new(tile_stats, n, c)
        _c("adyolo_bn_persample", _p(tile_stats), _p(ssum), _p(ps1), n, tiles // n, c, _stream())
        g0, g1 = EXACT.gather_rows(ssum), EXACT.gather_rows(ps1)
        _c("adyolo_bn_finish", _p(g0), _p(g1), _p(mean), _p(invstd), _p(running_mean), _p(running_var), _p(gamma), _p(beta),
           _p(scale), _p(shift), g0.shape[0], hw, c, momentum, eps, _stream())
    else:
        partial = _new(tile_stats, 2 * 1024 * c)
        _c("adyolo_bn_stats_tiles", _p(tile_stats), _p(ssum), _p(mean), _p(invstd), _p(running_mean), _p(running_var),
           _p(gamma), _p(beta), _p(scale), _p(shift), _p(partial), n, tiles // n, hw, c, momentum, eps, _stream())
    if gamma is not None:
        return ssum, mean, invstd, scale, shift
    return ssum, mean, invstd


def bn_eval_stats(running_mean, running_var, eps=1e-5):
    _chk(running_mean, running_var)
    c = running_mean.numel()
    mean, invstd = _new(running_mean, c), _new(running_mean, c)
    _c("adyolo_bn_eval_stats", _p(running_mean), _p(running_var), _p(mean), _p(invstd), c, eps, _stream())
    return mean, invstd


def bn_scale_shift(gamma, beta, mean, invstd):
    _chk(gamma, beta, mean, invstd)
    c = gamma.numel()
    scale, shift = _new(gamma, c), _new(gamma, c)
    _c("adyolo_bn_scale_shift", _p(gamma), _p(beta), _p(mean), _p(invstd), _p(scale), _p(shift), c, _stream())
    return scale, shift


def affine(x, scale, shift):
    _chk(x, scale, shift)
    c = x.shape[-1]
    y = torch.empty_like(x)
    _c("adyolo_affine_nhwc", _p(x), _p(scale), _p(shift), _p(y), x.numel() // c, c, _stream())
    return y


def bn_bwd(dy, x, gamma, mean, invstd, relu_mask=False, tile_stats=None, out_dgamma=None, out_dbeta=None,
           want_dx_colsum=False):
    """-> dx, dgamma, dbeta.  relu_mask: additionally multiply dx by (x > 0) (x is a ReLU output).
    tile_stats: per-patch (sum dy, sum dy*xhat) written by the convolution that produced dy (skips the reduce pass)."""
    _chk(dy, x, gamma, mean, invstd)
    c = x.shape[-1]
    rows = x.numel() // c
    sdy = out_dbeta if out_dbeta is not None else _new(x, c)          # = dbeta
    sdyx = out_dgamma if out_dgamma is not None else _new(x, c)       # = dgamma
    if tile_stats is not None:
        _c("adyolo_bn_bwd_tiles", _p(tile_stats), _p(sdy), _p(sdyx), _p(_new(tile_stats, 2, 256, c)), tile_stats.shape[1], c,
           _stream())
    else:
        partial = _new(x, 2 * 1024 * c)
        _c("adyolo_bn_bwd_reduce", _p(dy), _p(x), _p(mean), _p(invstd), _p(sdy), _p(sdyx), _p(partial), rows, c,
           _stream())
    dx = torch.empty_like(x)
    colsum = part = None
    if want_dx_colsum:          # channel sums of dx from the same pass (e.g. the bias gradient of the producing convolution)
        colsum, part = _new(x, c), _new(x, 8192, c)
    a_sdy, a_sdyx, cs = sdy, sdyx, 1.0
    if EXACT.on:                # the dx formula needs the sums over the batch of ALL ranks; sdy / sdyx (= the parameter
        glob = EXACT.all_reduce(torch.stack([sdy, sdyx]))      # gradients, possibly slices of the flat buffer) stay local
        a_sdy, a_sdyx, cs = glob[0], glob[1], float(EXACT.world)
    _c("adyolo_bn_bwd_apply", _p(dy), _p(x), _p(gamma), _p(mean), _p(invstd), _p(a_sdy), _p(a_sdyx), _p(dx), NULL, NULL,
       _p(colsum), _p(part), rows, c, int(relu_mask), cs, _stream())
    if want_dx_colsum:
        return dx, sdyx, sdy, colsum
    return dx, sdyx, sdy


def se_fc_fwd(ssum, scale, shift, w1, b1, w2, b2, hw):
    _chk(ssum, scale, shift, w1, b1, w2, b2)
    n, c = ssum.shape
    cr = w1.shape[0]
    pooled, hid, s = _new(ssum, n, c), _new(ssum, n, cr), _new(ssum, n, c)
    _c("adyolo_se_fc_fwd", _p(ssum), _p(scale), _p(shift), _p(w1), _p(b1), _p(w2), _p(b2), _p(pooled), _p(hid), _p(s),
       n, hw, c, cr, _stream())
    return pooled, hid, s


def se_tail_pool_ok(h, w, ch):
    """True when ``se_tail_fwd(..., pool_hw=(h, w))`` takes the shape (adyolo_se_tail_fwd_pool_ok)."""
    return bool(_lib.load().adyolo_se_tail_fwd_pool_ok(int(h), int(w), int(ch)))


def se_tail_fwd(c_t, r_t, scale, shift, s, want_mask=False, r_affine=None, pool_hw=None):
    """e = relu((c*scale+shift)*s + r), r seen through r_affine = (scale, shift) per channel when given.  want_mask: also return the ReLU mask (e > 0) as bits (int64 words, 1/32 of the
    bytes of e) for ``se_tail_bwd(..., mask=)``; None when the shape does not support it (HW*C/4 % 64 != 0).
    pool_hw = (H, W): return avgpool2(e) [N][H/2][W/2][C] INSTEAD of e (the block in front of a pooled stage boundary; e is
    never written), always as a pair (pooled, mask or None); the caller checks ``se_tail_pool_ok`` first."""
    _chk(c_t, r_t, scale, shift, s)
    n, ch = c_t.shape[0], c_t.shape[-1]
    hw = c_t.numel() // (n * ch)
    mask = None
    if want_mask:
        words = _lib.load().adyolo_relu_mask_words(n, hw, ch)
        if words > 0:
            mask = torch.empty(words, dtype=torch.int64, device=c_t.device)
    rs, rt = r_affine if r_affine is not None else (None, None)
    if pool_hw is not None:
        h, w = pool_hw
        if want_mask and mask is None:
            raise _lib.AdyoloHipError("se_tail_fwd(pool_hw=): the shape has no mask bits")
        pooled = _new(c_t, n, h // 2, w // 2, ch)
        _c("adyolo_se_tail_fwd_pool", _p(c_t), _p(r_t), _p(scale), _p(shift), _p(s), _p(rs), _p(rt), _p(pooled), _p(mask), n, h, w,
           ch, _stream())
        return pooled, mask
    e = torch.empty_like(c_t)
    _c("adyolo_se_tail_fwd", _p(c_t), _p(r_t), _p(scale), _p(shift), _p(s), _p(rs), _p(rt), _p(e), _p(mask), n, hw, ch,
       _stream())
    return (e, mask) if want_mask else e


def se_tail_bwd(de, e, c_t, gamma, beta, mean, invstd, ssum, pooled, hid, s, w1, w2, want_dr=True, tile_stats=None,
                mask=None, packed_out=None, pooled_hw=None, de_out=None):
    """Backward of  e = relu(bn2(c) * s + r)  incl. the SE FCs.
    -> dc, dr, dgamma, dbeta, dw1, db1, dw2, db2
    tile_stats: per-patch sums [2][tiles][C] of de * (e > 0) and de * (e > 0) * xhat(c) from the convolution epilogue
    that produced ``de`` (``conv3x3(..., stat_bn=(c, mean, invstd), stat_mask=e)``): the reduction pass is skipped.
    mask: the bits ``se_tail_fwd(..., want_mask=True)`` returned; both passes then read them instead of e.
    pooled_hw = (H, W): the block's output was avgpool2(e) (``se_tail_fwd(pool_hw=)``) and ``de`` is the gradient of THAT,
    [N][H/2][W/2][C]; needs ``mask``.  de_out (optional, [N][H][W][C]) receives the gradient of e itself (avgpool2's backward),
    which no pass here reads."""
    _chk(de, e, c_t, gamma, beta, mean, invstd, ssum, pooled, hid, s, w1, w2, de_out)
    if pooled_hw is not None and mask is None:
        raise _lib.AdyoloHipError("se_tail_bwd(pooled_hw=) needs the ReLU-mask bits")
    n, ch = c_t.shape[0], c_t.shape[-1]
    hw = c_t.numel() // (n * ch)
    cr = w1.shape[0]
    sg, sgx = _new(c_t, n, ch), _new(c_t, n, ch)
    if tile_stats is not None:
        _c("adyolo_se_tail_bwd_tiles", _p(tile_stats), _p(sg), _p(sgx), n, tile_stats.shape[1] // n, ch, _stream())
    else:
        partial = _new(c_t, 2 * 1024 * ch)
        if pooled_hw is not None:
            _c("adyolo_se_tail_bwd_reduce_pooled", _p(de), _p(mask), _p(c_t), _p(mean), _p(invstd), _p(sg), _p(sgx), _p(partial),
               n, pooled_hw[0], pooled_hw[1], ch, _stream())
        else:
            _c("adyolo_se_tail_bwd_reduce", _p(de), _p(e), _p(mask), _p(c_t), _p(mean), _p(invstd), _p(sg), _p(sgx), _p(partial),
               n, hw, ch, _stream())
    pw = 2 * ch * cr + cr + 3 * ch
    part, cws = _new(c_t, n, pw), _new(c_t, 1024, pw)
    packed = packed_out if packed_out is not None else _new(c_t, pw)    # packed_out: the six gradients' slice of the flat buffer
    dpool = _new(c_t, n, ch)
    _c("adyolo_se_fc_bwd", _p(sg), _p(sgx), _p(ssum), _p(gamma), _p(beta), _p(mean), _p(invstd), _p(pooled), _p(hid),
       _p(s), _p(w1), _p(w2), _p(dpool), _p(part), _p(packed), _p(cws), n, hw, ch, cr, _stream())
    o = 0
    db2 = packed[o:o + ch]; o += ch
    dw2 = packed[o:o + ch * cr].view(ch, cr); o += ch * cr
    db1 = packed[o:o + cr]; o += cr
    dw1 = packed[o:o + cr * ch].view(cr, ch); o += cr * ch
    sdd = packed[o:o + ch]; o += ch
    sddx = packed[o:o + ch]
    dgamma, dbeta = sddx, sdd
    dc = torch.empty_like(c_t)
    dr = torch.empty_like(c_t) if want_dr else None
    a_sdd, a_sddx, cs = sdd, sddx, 1.0
    if EXACT.on:                # BN2's batch sums over all ranks for the dc formula; the packed parameter gradients stay local
        glob = EXACT.all_reduce(torch.stack([sdd, sddx]))
        a_sdd, a_sddx, cs = glob[0], glob[1], float(EXACT.world)
    if pooled_hw is not None:
        _c("adyolo_se_tail_bwd_apply_pooled", _p(de), _p(mask), _p(c_t), _p(gamma), _p(mean), _p(invstd), _p(s), _p(dpool),
           _p(a_sdd), _p(a_sddx), _p(dc), _p(dr), _p(de_out), n, pooled_hw[0], pooled_hw[1], ch, cs, _stream())
    else:
        _c("adyolo_se_tail_bwd_apply", _p(de), _p(e), _p(mask), _p(c_t), _p(gamma), _p(mean), _p(invstd), _p(s), _p(dpool),
           _p(a_sdd), _p(a_sddx), _p(dc), _p(dr), n, hw, ch, cs, _stream())
    return dc, dr, dgamma, dbeta, dw1, db1, dw2, db2


def avgpool2(x):
    _chk(x)
    n, h, w, c = x.shape
    y = _new(x, n, h // 2, w // 2, c)
    _c("adyolo_avgpool2_fwd", _p(x), _p(y), n, h, w, c, _stream())
    return y


def avgpool2_bwd(dy, h, w):
    _chk(dy)
    n, c = dy.shape[0], dy.shape[3]
    dx = _new(dy, n, h, w, c)
    _c("adyolo_avgpool2_bwd", _p(dy), _p(dx), n, h, w, c, _stream())
    return dx


# ---------------------------------------------------------------------------------------------- sequence
def sap_fwd(x, w, b):
    """x [R][F][256] -> y [R][256], attn [R][F]."""
    _chk(x, w, b)
    r, f, c = x.shape
    y, attn = _new(x, r, c), _new(x, r, f)
    _c("adyolo_sap_fwd", _p(x), _p(w), _p(b), _p(y), _p(attn), r, f, c, _stream())
    return y, attn


def sap_bwd(dy, x, w, attn, out_dw=None, out_db=None):
    """out_dw [C] / out_db [1]: accumulators the kernel ADDS the two gradients into instead of fresh zeros (``functional.GradSink``:
    the parameters' slices of the flat gradient buffer, zero since ``zero_grad``)."""
    _chk(dy, x, w, attn)
    r, f, c = x.shape
    dx = torch.empty_like(x)
    dw = out_dw if out_dw is not None else _zeros(x, c)
    db = out_db if out_db is not None else _zeros(x, 1)
    partial = _new(x, 1024 * 260)
    _c("adyolo_sap_bwd", _p(dy), _p(x), _p(w), _p(attn), _p(dx), _p(dw), _p(db), _p(partial), r, f, c, _stream())
    return dx, dw, db


def gru_fwd(gx, whh, bhh, save):
    """gx [B][T][2][384], whh [2][384][128], bhh [2][384] -> out [B][T][256] (+ gates, hprev when ``save``)."""
    _chk(gx, whh, bhh)
    b, t = gx.shape[0], gx.shape[1]
    out = _new(gx, b, t, 256)
    gates = _new(gx, b, t, 2, 4, 128) if save else None
    hprev = _new(gx, b, t, 2, 128) if save else None
    _c("adyolo_gru_fwd", _p(gx), _p(whh), _p(bhh), _p(out), _p(gates), _p(hprev), b, t, _stream())
    return out, gates, hprev


def gru_bwd(dout, gates, hprev, whh):
    _chk(dout, gates, hprev, whh)
    b, t = dout.shape[0], dout.shape[1]
    dgx, dgh = _new(dout, b, t, 2, 384), _new(dout, b, t, 2, 384)
    _c("adyolo_gru_bwd", _p(dout), _p(gates), _p(hprev), _p(whh), _p(dgx), _p(dgh), b, t, _stream())
    return dgx, dgh


def ln_tanh_fwd(x2d, gamma, beta, eps=1e-5):
    _chk(x2d, gamma, beta)
    r, c = x2d.shape
    y = torch.empty_like(x2d)
    _c("adyolo_ln_tanh_fwd", _p(x2d), _p(gamma), _p(beta), _p(y), r, c, eps, _stream())
    return y


def ln_tanh_bwd(dy2d, x2d, y2d, gamma, eps=1e-5, out_dgamma=None, out_dbeta=None):
    """out_dgamma / out_dbeta [C]: accumulators the kernel ADDS the two gradients into instead of fresh zeros (see ``sap_bwd``)."""
    _chk(dy2d, x2d, y2d, gamma)
    r, c = x2d.shape
    dx = torch.empty_like(x2d)
    dgamma = out_dgamma if out_dgamma is not None else _zeros(x2d, c)
    dbeta = out_dbeta if out_dbeta is not None else _zeros(x2d, c)
    partial = _new(x2d, 1024 * 512)
    _c("adyolo_ln_tanh_bwd", _p(dy2d), _p(x2d), _p(y2d), _p(gamma), _p(dx), _p(dgamma), _p(dbeta), _p(partial), r, c,
       eps, _stream())
    return dx, dgamma, dbeta


def dropout_mask(like, p, seed, offset):
    mask = torch.empty_like(like)
    _c("adyolo_dropout_mask", _p(mask), mask.numel(), float(p), ctypes.c_uint64(seed), ctypes.c_uint64(offset), _stream())
    return mask


def dropout_apply(x, p, seed, offset, offset_dev=None):
    """x * mask, mask = dropout_mask(x, p, seed, offset) generated on the fly (no mask tensor).
    offset_dev (int64 tensor of one element on the device, or None): its value is added to ``offset`` inside the kernel --
    the form a launch recorded in a hipGraph needs (``rng.DropoutStream`` while a step is being captured)."""
    _chk(x)
    y = torch.empty_like(x)
    if offset_dev is None:
        _c("adyolo_dropout_apply", _p(x), _p(y), x.numel(), float(p), ctypes.c_uint64(seed), ctypes.c_uint64(offset), _stream())
    else:
        _c("adyolo_dropout_apply_dev", _p(x), _p(y), x.numel(), float(p), ctypes.c_uint64(seed),
           ctypes.c_uint64(offset & 0xFFFFFFFFFFFFFFFF), _p(offset_dev), _stream())
    return y


def counter_add_(counter, inc):
    """counter[0] += inc on the device (int64 tensor of one element): advances a device-side dropout offset."""
    if not counter.is_cuda or counter.dtype != torch.int64 or counter.numel() != 1:
        raise _lib.AdyoloHipError("counter_add_ needs a one-element int64 tensor on the device")
    _c("adyolo_counter_add", _p(counter), ctypes.c_uint64(int(inc) & 0xFFFFFFFFFFFFFFFF), _stream())
    return counter


# ---------------------------------------------------------------------------------------------- loss / optim
def _thr_gains(thr, gains):
    """The three thresholds and the four gains of the AD-YOLO loss as host float arrays, the way the entry points take them."""
    return (ctypes.cast((ctypes.c_float * 3)(*[float(v) for v in thr]), ctypes.c_void_p),
            ctypes.cast((ctypes.c_float * 4)(*[float(v) for v in gains]), ctypes.c_void_p))


def adyolo_loss(logit, target, nb_classes, grid=(8, 4), anchors=5, thr=(45.0, 25.0, 10.0),
                gains=(5.0, 1.0, 5.0, 3.0), grid_size=(45.0, 45.0), g_overlap=0.5, need_grad=True, grad_scale=1.0,
                want_dist=False):
    """logit [B][T][G*A*(C+3)], target [M][7] (device) -> loss (1,), dlogit (or None), dist (or None)."""
    _chk(logit, target)
    b, t = logit.shape[0], logit.shape[1]
    m = target.shape[0]
    words = _lib.load().adyolo_loss_workspace_words(b * t, grid[0] * grid[1], anchors, m)
    ws = _new(logit, words)
    loss = _new(logit, 1)
    dlogit = torch.empty_like(logit) if need_grad else None
    dist = _new(logit, m, anchors) if want_dist else None
    thr_h, gains_h = _thr_gains(thr, gains)
    args = (_p(logit), _p(target), _p(ws), _p(loss), _p(dlogit), _p(dist), b, t, grid[0], grid[1],
            anchors, nb_classes, m, thr_h, gains_h,
            float(grid_size[0]), float(grid_size[1]), float(g_overlap), float(grad_scale))
    if EXACT.on:                # counts over the batch of all ranks between the assignment and the pass over the logits
        _c("adyolo_loss_phase", *args, 1, 0, _stream())
        EXACT.all_reduce(ws[:4].view(torch.int32))
        na = b * t * grid[0] * grid[1] * anchors
        _c("adyolo_loss_phase", *args, 2, na * EXACT.world, _stream())
        EXACT.all_reduce(loss)                          # the ranks' shares add up to the loss of the concatenated batch
    else:
        _c("adyolo_loss_fwd_bwd", *args, _stream())
    return loss, dlogit, dist


def loss_accumulator(device):
    """A running device accumulator float32 (2,) {sum, count} for ``adyolo_loss_per_clip`` / ``loss_accumulate``, zeroed."""
    return torch.zeros(2, dtype=torch.float32, device=device)


def loss_accumulate(acc, loss, valid=None):
    """acc {sum, count} += the losses of ``loss`` (any shape, float32) whose ``valid`` word (int32, same count; None: all) is
    not zero, added one after the other in float32 by one device thread: an evaluation loop's ``total + loss`` without the
    host.  No sync."""
    _chk(acc, loss)
    n = loss.numel()
    if acc.numel() != 2 or n < 1:
        raise _lib.AdyoloHipError("loss_accumulate: acc must hold 2 floats and loss at least one")
    if valid is not None and (valid.dtype != torch.int32 or not valid.is_cuda or not valid.is_contiguous()
                              or valid.numel() != n):
        raise _lib.AdyoloHipError("loss_accumulate: valid must be %d contiguous int32 words on the device" % n)
    _c("adyolo_loss_accumulate", _p(loss), _p(valid), n, _p(acc), _stream())
    return acc


def adyolo_loss_per_clip(logit, target, row_start, nb_classes, grid=(8, 4), anchors=5, thr=(45.0, 25.0, 10.0),
                         gains=(5.0, 1.0, 5.0, 3.0), grid_size=(45.0, 45.0), g_overlap=0.5, acc=None):
    """The AD-YOLO loss of every clip of a batched evaluation pass, forward only: logit [B][T][G*A*(C+3)], target (cap, 7) with
    clip b's rows at [row_start[b], row_start[b + 1]) and b in their first column, row_start int32 (B + 1,), all on the
    device -> loss (B,) float32, valid (B,) int32.  loss[b] carries the bits of ``adyolo_loss(logit[b:b+1], rows of clip b with
    b = 0, need_grad=False)``; a clip without rows gets loss 0 and valid 0.  acc: a ``loss_accumulator`` the valid losses are
    added to in clip order.  No sync."""
    _chk(logit, target, acc)
    if logit.dim() != 3 or target.dim() != 2 or target.shape[1] != 7 or target.shape[0] < 1:
        raise _lib.AdyoloHipError("adyolo_loss_per_clip: logit %s / target %s are not [B][T][K] / (cap, 7)"
                                  % (tuple(logit.shape), tuple(target.shape)))
    b, t = logit.shape[0], logit.shape[1]
    if logit.shape[2] != grid[0] * grid[1] * anchors * (nb_classes + 3):
        raise _lib.AdyoloHipError("adyolo_loss_per_clip: %d logits per frame, expected %d x %d x %d x (%d + 3)"
                                  % (logit.shape[2], grid[0], grid[1], anchors, nb_classes))
    if row_start.dtype != torch.int32 or not row_start.is_cuda or not row_start.is_contiguous() or row_start.numel() != b + 1:
        raise _lib.AdyoloHipError("adyolo_loss_per_clip: row_start must be %d contiguous int32 words on the device" % (b + 1))
    if acc is not None and acc.numel() != 2:
        raise _lib.AdyoloHipError("adyolo_loss_per_clip: acc must hold 2 floats")
    words = _lib.load().adyolo_loss_per_clip_workspace_words(b, t, grid[0] * grid[1], anchors)
    ws = _new(logit, words)
    loss = _new(logit, b)
    valid = torch.empty(b, dtype=torch.int32, device=logit.device)
    thr_h, gains_h = _thr_gains(thr, gains)
    _c("adyolo_loss_per_clip", _p(logit), _p(target), _p(row_start), _p(ws), _p(loss), _p(valid), _p(acc), b, t, grid[0],
       grid[1], anchors, nb_classes, target.shape[0], thr_h, gains_h, float(grid_size[0]), float(grid_size[1]),
       float(g_overlap), _stream())
    return loss, valid


def act_fwd(x2d, n_sigmoid_cols):
    """columns [0, n_sigmoid_cols) -> sigmoid, the rest -> tanh."""
    _chk(x2d)
    y = torch.empty_like(x2d)
    _c("adyolo_act_fwd", _p(x2d), _p(y), x2d.shape[0], x2d.shape[1], int(n_sigmoid_cols), _stream())
    return y


def act_bwd(dy2d, y2d, n_sigmoid_cols):
    _chk(dy2d, y2d)
    dx = torch.empty_like(y2d)
    _c("adyolo_act_bwd", _p(dy2d), _p(y2d), _p(dx), y2d.shape[0], y2d.shape[1], int(n_sigmoid_cols), _stream())
    return dx


def seddoa_loss(out2d, tgt2d, nsed, masked, w_bce, w_mse, need_grad=True):
    _chk(out2d, tgt2d)
    loss = _new(out2d, 1)
    dout = torch.empty_like(out2d) if need_grad else None
    partial = _new(out2d, 2 * 1024)
    _c("adyolo_seddoa_loss", _p(out2d), _p(tgt2d), _p(loss), _p(dout), _p(partial), out2d.shape[0], out2d.shape[1],
       int(nsed), int(masked), float(w_bce), float(w_mse), _stream())
    return loss, dout


def adpit_loss(out2d, tgt, nb_classes, need_grad=True):
    """out2d [rows][9*C], tgt [rows][6][4][C]."""
    _chk(out2d, tgt)
    loss = _new(out2d, 1)
    dout = torch.empty_like(out2d) if need_grad else None
    partial = _new(out2d, 1024)
    _c("adyolo_adpit_loss", _p(out2d), _p(tgt), _p(loss), _p(dout), _p(partial), out2d.shape[0], int(nb_classes), _stream())
    return loss, dout


CLASSWISE_MODES = {"seddoa": 0, "masked-seddoa": 0, "accdoa": 1, "adpit": 2}     # ADYOLO_CLASSWISE_* in adyolo_hip.h
CLASSWISE_WIDTH = {0: 4, 1: 3, 2: 9}                                               # output columns per class
CLASSWISE_REC = {0: 4, 1: 4, 2: 16}                                                # decoded floats per (frame, class)


def classwise_decode(output, nb_classes, mode):
    """output [...][W*C] of a seddoa / accdoa / adpit head -> decoded [frames][C][rec] (adyolo_hip.h, ``adyolo_classwise_decode``:
    activities, copied xyz and, for adpit, the angular distances of the track pairs).  mode: a loss name or its integer code."""
    _chk(output)
    m = CLASSWISE_MODES[mode] if isinstance(mode, str) else int(mode)
    k = CLASSWISE_WIDTH.get(m, 1) * int(nb_classes)
    frames = output.numel() // k if k > 0 else 0
    if k <= 0 or output.numel() != frames * k:
        raise _lib.AdyoloHipError("classwise_decode: %d output values are not a whole number of frames of %d" % (output.numel(), k))
    dec = _new(output, frames, int(nb_classes), CLASSWISE_REC.get(m, 4))
    _c("adyolo_classwise_decode", _p(output), _p(dec), frames, int(nb_classes), m, _stream())
    return dec


def yolo_decode(logit, nb_classes, grid=(8, 4), anchors=5, grid_size=(45.0, 45.0), g_overlap=0.5):
    """logit [...][G*A*(C+3)] -> decoded [frames][Gaz][Gel][A][C+3] (conf, class-confidence scores, U, V)."""
    _chk(logit)
    ch = nb_classes + 3
    frames = logit.numel() // (grid[0] * grid[1] * anchors * ch)
    out = _new(logit, frames, grid[0], grid[1], anchors, ch)
    _c("adyolo_yolo_decode", _p(logit), _p(out), frames, grid[0], grid[1], anchors, nb_classes, float(grid_size[0]),
       float(grid_size[1]), float(g_overlap), _stream())
    return out


SELECT_MODES = {"conn-merge": 1, "soft-merge": 2}                                   # ADYOLO_SELECT_* in adyolo_hip.h; else 0


def np_f32_threshold(t, op):
    """The float32 value t32 with ``(x op t32) == (x op t)`` for every float32 array x under NumPy's promotion rules, op one of
    '>', '<', '<='.  A Python float (NumPy 2: a weak scalar) is rounded to float32 before the compare, so 0.1 * 3 acts as
    float32(0.3); a float64 NumPy scalar such as an ``np.arange`` threshold is compared in float64, which float32 reproduces
    with the threshold rounded down ('>', '<=') or up ('<')."""
    if np.result_type(np.float32, t) == np.float32:
        return float(np.float32(t))
    t = float(t)
    lo = np.float32(t)
    if float(lo) > t:
        lo = np.nextafter(lo, np.float32(-np.inf))
    hi = lo if float(lo) == t else np.nextafter(lo, np.float32(np.inf))
    return float(lo if op in (">", "<=") else hi)


def yolo_select(decoded, nb_classes, conf, clss, unify, nms="conn-merge", trim=True):
    """decoded [frames][Gaz][Gel][A][C+3] (``yolo_decode``) -> (rows (N, 5) [frame, class, x, y, z], counts (frames,) int32),
    both on the device (adyolo_hip.h, ``adyolo_yolo_select``): the thresholds and the per-class NMS of
    ``postprocess.nms_decoded`` with the same rows in the same order.  The thresholds are compared as NumPy compares them
    with the host path's float32 arrays (``np_f32_threshold``).  One 4-byte read of the row total synchronises the stream.
    trim=False: no read and no synchronisation; rows is the whole capacity buffer, of which the first counts.sum() rows are
    written (what ``seld_score`` takes)."""
    _chk(decoded)
    ch = int(nb_classes) + 3
    frames = decoded.shape[0] if decoded.dim() > 0 else 0
    if frames <= 0 or decoded.numel() % (frames * ch) != 0 or decoded.shape[-1] != ch:
        raise _lib.AdyoloHipError("yolo_select: decoded %s is not [frames][...][%d]" % (tuple(decoded.shape), ch))
    n_anchor = decoded.numel() // (frames * ch)               # above ADYOLO_SELECT_MAX_N the C call refuses it (ENOSUP)
    mode = SELECT_MODES.get(nms, 0)
    ws = _new(decoded, max(1, _lib.load().adyolo_yolo_select_workspace_words(frames, n_anchor, int(nb_classes))))
    rows = _new(decoded, frames * int(nb_classes) * n_anchor, 5)
    counts = torch.empty(frames + 1, dtype=torch.int32, device=decoded.device)
    _c("adyolo_yolo_select", _p(decoded), _p(ws), _p(rows), _p(counts), frames, n_anchor, int(nb_classes),
       np_f32_threshold(conf, ">"), np_f32_threshold(clss, ">"), np_f32_threshold(unify, "<" if mode == 1 else "<="),
       float(np.float32(clss)), mode, _stream())
    if not trim:
        return rows, counts[:frames]
    total = int(to_host(counts[frames:])[0])
    return rows[:total], counts[:frames]


def classwise_select(decoded, nb_classes, mode, conf, unify=None, trim=True):
    """decoded [frames][C][rec] (``classwise_decode``) -> (rows (N, 5) [frame, class, x, y, z], counts (frames,) int32), both
    on the device (adyolo_hip.h, ``adyolo_classwise_select``): the thresholds and, for adpit, the unification of
    ``postprocess.classwise_select`` with the same rows in the same order, bit for bit.  mode: a loss name or its integer code;
    unify: needed for adpit, not read otherwise.  The thresholds are compared as NumPy compares them with the host path's
    float32 arrays (``np_f32_threshold``).  One 4-byte read of the row total synchronises the stream.  trim=False: no read and
    no synchronisation; rows is the whole capacity buffer, of which the first counts.sum() rows are written (what
    ``seld_score`` takes)."""
    m = CLASSWISE_MODES[mode] if isinstance(mode, str) else int(mode)
    if m not in CLASSWISE_REC:
        raise _lib.AdyoloHipError("classwise_select: unknown mode %r" % (mode,))
    if m == CLASSWISE_MODES["adpit"] and unify is None:
        raise ValueError("classwise_select: adpit needs a unify threshold")
    _chk(decoded)
    c, rec = int(nb_classes), CLASSWISE_REC[m]
    frames = decoded.shape[0] if decoded.dim() > 0 else 0
    if frames <= 0 or c <= 0 or tuple(decoded.shape) != (frames, c, rec):
        raise _lib.AdyoloHipError("classwise_select: decoded %s is not [frames][%d][%d]" % (tuple(decoded.shape), c, rec))
    per_class = 3 if m == CLASSWISE_MODES["adpit"] else 1
    ws = _new(decoded, _lib.load().adyolo_classwise_select_workspace_words(frames, c, m))
    rows = _new(decoded, frames * c * per_class, 5)
    counts = torch.empty(frames + 1, dtype=torch.int32, device=decoded.device)
    _c("adyolo_classwise_select", _p(decoded), _p(ws), _p(rows), _p(counts), frames, c, m, np_f32_threshold(conf, ">"),
       np_f32_threshold(unify, "<") if m == CLASSWISE_MODES["adpit"] else 0.0, _stream())
    if not trim:
        return rows, counts[:frames]
    total = int(to_host(counts[frames:])[0])
    return rows[:total], counts[:frames]


TTA_STATUS = ((1, "more rows of one view in one frame than the pool holds (enlarge tta_max_rows_per_frame)"),   # ADYOLO_TTA_*
              (2, "more than 1024 candidates in one frame and class"),
              (4, "a selected row with a zero or non-finite vector was dropped"),
              (8, "frame counts negative or past the rows given, or a class outside [0, nb_classes)"))
TTA_BAD_VECTOR = 4
TTA_MAX_VIEWS = 16                                            # ADYOLO_TTA_MAX_VIEWS


def tta_matrix_word(matrix):
    """A view's 3x3 signed permutation M (``augmentations.view_matrix``) -> the word ``adyolo_tta_collect`` takes: component i of
    M^T xyz is sign_i * xyz[src_i], src_i in bits [4 i, 4 i + 2), bit 4 i + 2 set for a negative sign."""
    m = np.asarray(matrix)
    if m.shape != (3, 3) or not np.isin(m, (-1, 0, 1)).all() or not (np.abs(m).sum(0) == 1).all() \
            or not (np.abs(m).sum(1) == 1).all():
        raise ValueError("tta_matrix_word: %r is no 3x3 signed permutation" % (matrix,))
    word = 0
    for i in range(3):
        j = int(np.abs(m[:, i]).argmax())
        word |= (j | (4 if m[j, i] < 0 else 0)) << (4 * i)
    return word


def tta_status_check(word):
    """Raise ``AdyoloHipError`` for the ADYOLO_TTA_* bits of a status word already read to the host; a dropped vector alone
    (a NaN in the network's output, which the plain pass writes out as it is) only warns."""
    word = int(word)
    why = "; ".join(msg for bit, msg in TTA_STATUS if word & bit)
    if word & ~TTA_BAD_VECTOR:
        raise _lib.AdyoloHipError("adyolo test-time augmentation failed (status 0x%x): %s" % (word, why))
    if word:
        import warnings
        warnings.warn("adyolo test-time augmentation (status 0x%x): %s" % (word, why))


def tta_buffers(device, n_views, frames, nb_classes, rows_per_frame, min_views=1):
    """The buffers one batch shape of ``tta_collect`` / ``tta_merge`` needs, allocated once: {'pool' (V, frames, P, 4) float32,
    'pool_counts' (V, frames) int32, 'ws', 'rows' (frames * (V * P // min_views), 5) float32, 'counts' (frames + 1,) int32}."""
    v, f, c, p = int(n_views), int(frames), int(nb_classes), int(rows_per_frame)
    dev = torch.device(device)
    return {"pool": torch.empty((v, f, p, 4), dtype=torch.float32, device=dev),
            "pool_counts": torch.empty((v, f), dtype=torch.int32, device=dev),
            "ws": torch.empty(max(1, _lib.load().adyolo_tta_merge_workspace_words(f, c)), dtype=torch.float32, device=dev),
            "rows": torch.empty((max(1, f * (v * p // max(1, int(min_views)))), 5), dtype=torch.float32, device=dev),
            "counts": torch.empty(f + 1, dtype=torch.int32, device=dev)}


def _tta_pool(name, pool, pool_counts, status, ws, nb_classes):
    """The checks both TTA calls share -> (V, frames, P)."""
    _chk(pool, ws)
    if pool.dim() != 4 or pool.shape[3] != 4 or not 1 <= pool.shape[0] <= TTA_MAX_VIEWS or pool.shape[1] < 1 or pool.shape[2] < 1:
        raise _lib.AdyoloHipError("%s: pool %s is not (views <= %d, frames, rows per frame, 4)"
                                  % (name, tuple(pool.shape), TTA_MAX_VIEWS))
    v, frames, p, _ = pool.shape
    for what, t, shape in (("pool_counts", pool_counts, (v, frames)), ("status", status, None)):
        if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.device != pool.device \
                or (shape is not None and tuple(t.shape) != shape) or t.numel() < 1:
            raise _lib.AdyoloHipError("%s: %s must be a contiguous int32 tensor%s on %s"
                                      % (name, what, "" if shape is None else " %s" % (shape,), pool.device))
    if int(nb_classes) < 1 or ws.device != pool.device \
            or ws.numel() < _lib.load().adyolo_tta_merge_workspace_words(frames, int(nb_classes)):
        raise _lib.AdyoloHipError("%s: the workspace needs %d words on %s (adyolo_tta_merge_workspace_words)"
                                  % (name, _lib.load().adyolo_tta_merge_workspace_words(frames, max(1, int(nb_classes))), pool.device))
    return v, frames, p


def tta_collect(rows, counts, view, matrix, nb_classes, pool, pool_counts, status, ws):
    """One view's selection -- rows (capacity, 5) and counts (frames,) int32 as ``yolo_select`` / ``classwise_select`` return them
    with ``trim=False`` -- turned back by ``matrix`` (``augmentations.view_matrix`` of the view, or its ``tta_matrix_word``) into
    slot ``view`` of pool (V, frames, P, 4) {class, x, y, z} / pool_counts (V, frames) (adyolo_hip.h ``adyolo_tta_collect``;
    ``tta_buffers`` makes the buffers).  A frame with more than P rows keeps its first P and sets status bit 1.  No allocation,
    no synchronisation."""
    name = "tta_collect"
    v, frames, p = _tta_pool(name, pool, pool_counts, status, ws, nb_classes)
    _chk(rows)
    if rows.dim() != 2 or rows.shape[1] != 5 or rows.device != pool.device:
        raise _lib.AdyoloHipError("%s: rows %s are not (N, 5) on %s" % (name, tuple(rows.shape), pool.device))
    if not counts.is_cuda or counts.dtype != torch.int32 or not counts.is_contiguous() or counts.device != pool.device \
            or counts.numel() != frames:
        raise _lib.AdyoloHipError("%s: counts must be a contiguous int32 tensor (%d,) on %s" % (name, frames, pool.device))
    if not 0 <= int(view) < v:
        raise _lib.AdyoloHipError("%s: view %r of %d" % (name, view, v))
    word = int(matrix) if isinstance(matrix, int) else tta_matrix_word(matrix)
    _c("adyolo_tta_collect", _p(rows) if rows.numel() else _p(pool), rows.shape[0], _p(counts), _p(ws), _p(pool),
       _p(pool_counts), _p(status), frames, int(nb_classes), v, int(view), p, word, _stream())


def tta_merge(pool, pool_counts, nb_classes, cos_t, min_views, status, ws, rows=None, counts=None, trim=True):
    """The pool ``tta_collect`` filled for every view -> (rows (N, 5) [frame, class, x, y, z], counts (frames,) int32), both on
    the device, in the layout of ``yolo_select`` (adyolo_hip.h ``adyolo_tta_merge``): ``postprocess.merge_view_rows`` bit for
    bit.  cos_t: ``postprocess.tta_cos`` of the cluster distance.  rows / counts: the buffers to write, (>= frames * (V * P //
    min_views), 5) float32 and (frames + 1,) int32 (``tta_buffers``); None: new ones.  trim as ``yolo_select``: True reads the
    row total (one 4-byte copy, synchronises); False neither allocates (given buffers) nor synchronises."""
    name = "tta_merge"
    v, frames, p = _tta_pool(name, pool, pool_counts, status, ws, nb_classes)
    if isinstance(min_views, bool) or int(min_views) != min_views or not 1 <= int(min_views) <= v:
        raise _lib.AdyoloHipError("%s: min_views %r with %d views" % (name, min_views, v))
    need = frames * (v * p // int(min_views))
    if rows is None:
        rows = _new(pool, max(1, need), 5)
    if counts is None:
        counts = torch.empty(frames + 1, dtype=torch.int32, device=pool.device)
    _chk(rows)
    if rows.dim() != 2 or rows.shape[1] != 5 or rows.shape[0] < need or rows.device != pool.device:
        raise _lib.AdyoloHipError("%s: rows %s are not (>= %d, 5) on %s" % (name, tuple(rows.shape), need, pool.device))
    if not counts.is_cuda or counts.dtype != torch.int32 or not counts.is_contiguous() or counts.device != pool.device \
            or counts.numel() != frames + 1:
        raise _lib.AdyoloHipError("%s: counts must be a contiguous int32 tensor (%d,) on %s" % (name, frames + 1, pool.device))
    _c("adyolo_tta_merge", _p(pool), _p(pool_counts), _p(ws), _p(rows), rows.shape[0], _p(counts), _p(status), frames,
       int(nb_classes), v, p, float(np.float32(cos_t)), int(min_views), _stream())
    if not trim:
        return rows, counts[:frames]
    total = int(to_host(counts[frames:])[0])
    return rows[:total], counts[:frames]


TRACK_STATUS = ((1, "more than 64 rows in one frame and class: the first 64 were linked"),                       # ADYOLO_TRACK_*
                (2, "more than 8 concurrent tracks of one class: a detection was dropped"),
                (4, "a selected row with a zero or non-finite vector was dropped"),
                (8, "frame counts negative or past the rows given, or a class outside [0, nb_classes)"))
TRACK_BAD_ROWS = 8
TRACK_SLOTS = 8                                               # ADYOLO_TRACK_SLOTS


def track_status_check(word):
    """Raise ``AdyoloHipError`` for ADYOLO_TRACK_BAD_ROWS in a status word already read to the host.  The two overflows and a
    dropped vector are defined behaviour (caps of ``postprocess.track_rows``; an untrained model's twenty rows per class and
    frame pass through) and only warn."""
    word = int(word)
    why = "; ".join(msg for bit, msg in TRACK_STATUS if word & bit)
    if word & TRACK_BAD_ROWS:
        raise _lib.AdyoloHipError("adyolo tracking failed (status 0x%x): %s" % (word, why))
    if word:
        import warnings
        warnings.warn("adyolo tracking (status 0x%x): %s" % (word, why))


def track_buffers(device, frames, nb_classes):
    """The buffers one batch shape of ``track_rows`` needs, allocated once: {'ws', 'rows' (frames * C * 8, 5) float32, 'ids'
    (frames * C * 8,) int32, 'counts' (frames + 1,) int32}."""
    f, c = int(frames), int(nb_classes)
    dev = torch.device(device)
    return {"ws": torch.empty(max(4, _lib.load().adyolo_track_workspace_words(f, c)), dtype=torch.float32, device=dev),
            "rows": torch.empty((max(1, f * c * TRACK_SLOTS), 5), dtype=torch.float32, device=dev),
            "ids": torch.empty(max(1, f * c * TRACK_SLOTS), dtype=torch.int32, device=dev),
            "counts": torch.empty(f + 1, dtype=torch.int32, device=dev)}


def track_rows(rows, counts, n_clips, nb_classes, opts, buf=None, status=None, trim=True):
    """A selection -- rows (capacity, 5) [frame, class, x, y, z] and counts (n_clips * T',) int32 on the device, as
    ``yolo_select`` / ``classwise_select`` / ``tta_merge`` return them, trimmed or not -- linked into tracks (adyolo_hip.h
    ``adyolo_track_rows``): ``postprocess.track_rows`` bit for bit -> (rows' (N', 5), counts' (n_clips * T',) int32, ids (N',)
    int32), all on the device.  opts: the dict of ``augmentations.track_options`` {'gate_deg', 'max_gap', 'min_len', 'smooth'}.
    buf: ``track_buffers`` of this shape (None: new ones); status: one int32 on the device the ADYOLO_TRACK_* bits are ORed into
    (None: a new word, read and passed to ``track_status_check`` here when trim is True).  trim as ``yolo_select``: True reads
    the row total (one 4-byte copy, synchronises); False with given buffers neither allocates nor synchronises, and rows' / ids
    are the capacity buffers of which the first counts'.sum() are written."""
    from .postprocess import track_cos
    name = "track_rows"
    _chk(rows)
    frames, c, n_clips = int(counts.numel()), int(nb_classes), int(n_clips)
    if rows.dim() != 2 or rows.shape[1] != 5:
        raise _lib.AdyoloHipError("%s: rows %s are not (N, 5)" % (name, tuple(rows.shape)))
    if not counts.is_cuda or counts.dtype != torch.int32 or not counts.is_contiguous() or counts.device != rows.device:
        raise _lib.AdyoloHipError("%s: counts must be a contiguous int32 tensor on %s" % (name, rows.device))
    if n_clips < 1 or frames < 1 or frames % n_clips or c < 1:
        raise _lib.AdyoloHipError("%s: %d frame counts, %d clips, %d classes" % (name, frames, n_clips, c))
    if buf is None:
        buf = track_buffers(rows.device, frames, c)
    own_status = status is None
    if own_status:
        status = torch.zeros(1, dtype=torch.int32, device=rows.device)
    need = frames * c * TRACK_SLOTS
    ws, out, ids, out_counts = buf["ws"], buf["rows"], buf["ids"], buf["counts"]
    _chk(ws, out)
    if ws.numel() < _lib.load().adyolo_track_workspace_words(frames, c) or out.dim() != 2 or out.shape[1] != 5 \
            or out.shape[0] < need or ids.numel() < need or out_counts.numel() != frames + 1 \
            or any(t.device != rows.device for t in (ws, out, ids, out_counts, status)) \
            or any(t.dtype != torch.int32 or not t.is_contiguous() for t in (ids, out_counts, status)) or status.numel() < 1:
        raise _lib.AdyoloHipError("%s: the buffers are not track_buffers(%s, %d, %d) / status no int32 word there"
                                  % (name, rows.device, frames, c))
    a = np.float32(opts["smooth"])
    _c("adyolo_track_rows", _p(rows) if rows.numel() else _p(out), rows.shape[0], _p(counts), n_clips, frames // n_clips, c,
       float(track_cos(opts["gate_deg"])), int(opts["max_gap"]), int(opts["min_len"]), float(a),
       float(np.float32(np.float32(1) - a)), _p(ws), _p(out), _p(ids), out.shape[0], _p(out_counts), _p(status), _stream())
    if not trim:
        return out, out_counts[:frames], ids
    if own_status:
        total_h, status_h = to_host_many(out_counts[frames:], status)
        track_status_check(int(status_h[0]))
        total = int(total_h[0])
    else:
        total = int(to_host(out_counts[frames:])[0])
    return out[:total], out_counts[:frames], ids[:total]


CSV_STATUS = ((1, "more bytes than the buffer holds: nothing was written (seg_bytes[-1] is the capacity needed)"),   # ADYOLO_CSV_*
              (2, "frame counts negative or past the rows given"),
              (4, "a class that is not finite or not within int32, or a negative track id"),
              (8, "a segment table that does not ascend from frame 0 within the frames"))
from .postprocess import CSV_LINE_MAX, CSV_OVERFLOW          # noqa: E402  (defined once, beside format_rows; a test holds them to the headers)


def csv_status_check(word):
    """Raise ``AdyoloHipError`` for any ADYOLO_CSV_* bit in a status word already read to the host: every one of them means
    the bytes are not the files'."""
    word = int(word)
    if word:
        raise _lib.AdyoloHipError("adyolo csv_format failed (status 0x%x): %s"
                                  % (word, "; ".join(msg for bit, msg in CSV_STATUS if word & bit)))


def csv_workspace_words(frames, n_rows):
    """ADYOLO_CSV_WORKSPACE_WORDS in adyolo_hip.h."""
    return 2 * ((int(n_rows) + 255) // 256) + 4 + int(frames)


def csv_buffers(device, frames, n_rows, n_segments, n_bytes):
    """The buffers one shape of ``csv_format`` needs, allocated once: {'ws' int32, 'out' (n_bytes rounded up to 16,) uint8,
    'seg_bytes' (n_segments + 1,) int64}.  n_rows * CSV_LINE_MAX bytes always suffice; fewer may (``csv_format`` reports it)."""
    dev = torch.device(device)
    return {"ws": torch.empty(csv_workspace_words(frames, n_rows), dtype=torch.int32, device=dev),
            "out": torch.empty(max(16, (int(n_bytes) + 15) // 16 * 16), dtype=torch.uint8, device=dev),
            "seg_bytes": torch.empty(int(n_segments) + 1, dtype=torch.int64, device=dev)}


def csv_format(rows, counts, segments, ids=None, buf=None, status=None):
    """A selection -- rows (capacity, 5) [frame, class, x, y, z] and counts (frames,) int32 on the device, as ``yolo_select`` /
    ``classwise_select`` / ``tta_merge`` / ``track_rows`` / ``track_run`` return them, trimmed or not -- as the bytes of its CSV
    files (adyolo_hip.h ``adyolo_csv_format``): ``postprocess.format_rows`` byte for byte -> (out (capacity,) uint8, seg_bytes
    (K + 1,) int64), both on the device: segment k's file is out[seg_bytes[k]:seg_bytes[k + 1]].  segments: (K, 2) int32 on the
    device (``postprocess.csv_segments_clips`` / ``csv_segments_run``, uploaded by the caller once).  ids: (>= capacity,) int32
    track ids or None.  buf: ``csv_buffers`` (None: new ones for rows.shape[0] * CSV_LINE_MAX bytes, which always suffice).
    status: one int32 on the device the ADYOLO_CSV_* bits are ORed into (None: a new word).  Neither allocates (given buffers)
    nor synchronises; the caller reads seg_bytes and status (``csv_status_check``) before it trusts a byte.
    -> (out, seg_bytes, status)"""
    name = "csv_format"
    _chk(rows)
    if rows.dim() != 2 or rows.shape[1] != 5:
        raise _lib.AdyoloHipError("%s: rows %s are not (N, 5)" % (name, tuple(rows.shape)))
    dev, frames = rows.device, int(counts.numel())
    if not counts.is_cuda or counts.dtype != torch.int32 or not counts.is_contiguous() or counts.device != dev or frames < 1:
        raise _lib.AdyoloHipError("%s: counts must be a contiguous int32 tensor of at least one frame on %s" % (name, dev))
    if not torch.is_tensor(segments) or segments.dtype != torch.int32 or segments.dim() != 2 or segments.shape[1] != 2 \
            or segments.shape[0] < 1 or not segments.is_contiguous() or segments.device != dev:
        raise _lib.AdyoloHipError("%s: segments must be a contiguous (K >= 1, 2) int32 tensor on %s" % (name, dev))
    if ids is not None and (not torch.is_tensor(ids) or ids.dtype != torch.int32 or not ids.is_contiguous() or ids.device != dev
                            or ids.numel() < rows.shape[0]):
        raise _lib.AdyoloHipError("%s: ids must be a contiguous int32 tensor of at least %d on %s" % (name, rows.shape[0], dev))
    k = int(segments.shape[0])
    if buf is None:
        buf = csv_buffers(dev, frames, rows.shape[0], k, rows.shape[0] * CSV_LINE_MAX)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws, out, seg_bytes = buf["ws"], buf["out"], buf["seg_bytes"]
    if ws.dtype != torch.int32 or ws.numel() < csv_workspace_words(frames, rows.shape[0]) or out.dtype != torch.uint8 \
            or seg_bytes.dtype != torch.int64 or seg_bytes.numel() < k + 1 or status.dtype != torch.int32 or status.numel() < 1 \
            or any(t.device != dev or not t.is_contiguous() for t in (ws, out, seg_bytes, status)):
        raise _lib.AdyoloHipError("%s: the buffers are not csv_buffers(%s, %d, %d, %d, ...) / status no int32 word there"
                                  % (name, dev, frames, rows.shape[0], k))
    _c("adyolo_csv_format", _p(rows) if rows.numel() else _p(ws), rows.shape[0], _p(counts), frames, _p(ids), _p(segments), k,
       _p(ws), _p(out) if out.numel() else _p(ws), out.numel(), _p(seg_bytes), _p(status), _stream())   # (no bytes: not written)
    return out, seg_bytes[:k + 1], status


def track_carry(device, nb_classes, hold):
    """An empty carry for ``track_run``: the state of one stream of recordings between two runs (the open recording's slots,
    next ids and held frames' cells), adyolo_hip.h ``adyolo_track_carry_words`` float32 words, all zero.  ``zero_()`` empties
    it again."""
    return torch.zeros(max(4, _lib.load().adyolo_track_carry_words(int(nb_classes), int(hold))), dtype=torch.float32,
                       device=torch.device(device))


def track_run_buffers(device, run_frames, nb_classes, hold):
    """The buffers one run length of ``track_run`` needs, allocated once: {'ws', 'rows' ((hold + run_frames) * C * 8, 5)
    float32, 'ids' int32, 'counts' (hold + run_frames + 2,) int32}."""
    f, c, d = int(run_frames), int(nb_classes), int(hold)
    dev = torch.device(device)
    n = max(1, (f + d) * c * TRACK_SLOTS)
    return {"ws": torch.empty(max(4, _lib.load().adyolo_track_run_workspace_words(f, c, d)), dtype=torch.float32, device=dev),
            "rows": torch.empty((n, 5), dtype=torch.float32, device=dev), "ids": torch.empty(n, dtype=torch.int32, device=dev),
            "counts": torch.empty(f + d + 2, dtype=torch.int32, device=dev)}


def track_run(rows, counts, segments, nb_classes, opts, hold, carry, buf=None, status=None, trim=True, emitted=None):
    """``track_rows`` on one run of a stream of recordings, the state carried in ``carry`` from call to call (adyolo_hip.h
    ``adyolo_track_run``): ``postprocess.track_run`` bit for bit -> (rows' (N', 5), counts' (emitted frames,) int32, ids (N',)
    int32) on the device.  rows / counts (run frames,) / opts / status / trim as ``track_rows``.  segments: (S, 4) int32 on the
    device, {first frame in the run, frames, continues, open} per recording of the run (``corpus.track_plan`` uploads them
    once).  hold: D >= ``postprocess.track_hold``.  carry: ``track_carry(device, nb_classes, hold)``, read and rewritten here.
    buf: ``track_run_buffers`` of this run length.  emitted: the number of emitted frames when the caller knows it (the plan
    does); None with trim=False returns all hold + run frames counts, zeros behind the emitted ones; trim=True reads the row
    total and the emitted frames in one 8-byte copy."""
    from .postprocess import track_cos
    name = "track_run"
    _chk(rows)
    frames, c, d = int(counts.numel()), int(nb_classes), int(hold)
    if rows.dim() != 2 or rows.shape[1] != 5:
        raise _lib.AdyoloHipError("%s: rows %s are not (N, 5)" % (name, tuple(rows.shape)))
    if not counts.is_cuda or counts.dtype != torch.int32 or not counts.is_contiguous() or counts.device != rows.device:
        raise _lib.AdyoloHipError("%s: counts must be a contiguous int32 tensor on %s" % (name, rows.device))
    if not torch.is_tensor(segments) or segments.dtype != torch.int32 or segments.dim() != 2 or segments.shape[1] != 4 \
            or segments.shape[0] < 1 or not segments.is_contiguous() or segments.device != rows.device:
        raise _lib.AdyoloHipError("%s: segments must be a contiguous (S >= 1, 4) int32 tensor on %s" % (name, rows.device))
    if frames < 1 or c < 1 or d < 0:
        raise _lib.AdyoloHipError("%s: %d frame counts, %d classes, hold %d" % (name, frames, c, d))
    if buf is None:
        buf = track_run_buffers(rows.device, frames, c, d)
    own_status = status is None
    if own_status:
        status = torch.zeros(1, dtype=torch.int32, device=rows.device)
    n_out = frames + d
    need = n_out * c * TRACK_SLOTS
    ws, out, ids, out_counts = buf["ws"], buf["rows"], buf["ids"], buf["counts"]
    _chk(ws, out)
    lib = _lib.load()
    if ws.numel() < lib.adyolo_track_run_workspace_words(frames, c, d) or out.dim() != 2 or out.shape[1] != 5 \
            or out.shape[0] < need or ids.numel() < need or out_counts.numel() != n_out + 2 \
            or any(t.device != rows.device for t in (ws, out, ids, out_counts, status, carry)) \
            or any(t.dtype != torch.int32 or not t.is_contiguous() for t in (ids, out_counts, status)) or status.numel() < 1 \
            or carry.dtype != torch.float32 or not carry.is_contiguous() or carry.numel() < lib.adyolo_track_carry_words(c, d):
        raise _lib.AdyoloHipError("%s: the buffers are not track_run_buffers(%s, %d, %d, %d) / carry not track_carry of that "
                                  "shape / status no int32 word there" % (name, rows.device, frames, c, d))
    a = np.float32(opts["smooth"])
    _c("adyolo_track_run", _p(rows) if rows.numel() else _p(out), rows.shape[0], _p(counts), frames, _p(segments),
       segments.shape[0], c, float(track_cos(opts["gate_deg"])), int(opts["max_gap"]), int(opts["min_len"]), float(a),
       float(np.float32(np.float32(1) - a)), d, _p(carry), _p(ws), _p(out), _p(ids), out.shape[0], _p(out_counts), _p(status),
       _stream())
    if not trim:
        return out, out_counts[:n_out if emitted is None else int(emitted)], ids
    if own_status:
        tail_h, status_h = to_host_many(out_counts[n_out:], status)
        track_status_check(int(status_h[0]))
    else:
        tail_h = to_host(out_counts[n_out:])
    total = int(tail_h[0])
    return out[:total], out_counts[:int(tail_h[1]) if emitted is None else int(emitted)], ids[:total]


SELD_STATUS =((1, "more than 1024 predictions in one frame and class"),      # ADYOLO_SELD_* in adyolo_hip.h
               (2, "more than 8 reference events in one frame and class"),
               (4, "frame counts negative or summing past the rows given"),
               (8, "a file index outside the reference table"),
               (16, "no finite assignment (NaN coordinates)"),
               (32, "a run segment off the block grid, outside the run or beyond seg_blocks"))
SELD_ENOSUP_BITS = 1 | 2                                      # ADYOLO_SELD_PRED_OVERFLOW | ADYOLO_SELD_REF_OVERFLOW


def seld_status_check(status):
    """Raise ``AdyoloHipError`` for the ADYOLO_SELD_* bits of a ``seld_score`` status word (one 4-byte copy, synchronises)."""
    word = int(to_host(status.reshape(-1)[:1])[0])
    if word:
        why = "; ".join(msg for bit, msg in SELD_STATUS if word & bit)
        code = -2 if word & SELD_ENOSUP_BITS else -1
        raise _lib.AdyoloHipError("adyolo_seld_score failed (rc=%d, status 0x%x): %s" % (code, word, why))


def seld_score(rows, counts, table, file_ids, t_clip, out, status=None):
    """Adds the SELD accumulators of n_clips = counts.numel() // t_clip clips into out [files][9 C + 3] float64
    (adyolo_hip.h, ``adyolo_seld_score``).  rows (N, 5) float32 or float64 [frame, class, x, y, z] with per-frame counts
    (int32, clip after clip: what ``yolo_select(..., trim=False)`` returns; rows beyond counts.sum() are not read), table a
    ``seld_metrics.SELDRefTable`` on the same device, file_ids (n_clips,) int32 on the device.  status: an int32 word on the
    device that collects errors across calls (the caller checks it with ``seld_status_check``; while it is set nothing is
    added); None: a fresh word, checked before returning (synchronises)."""
    if not rows.is_cuda or rows.dtype not in (torch.float32, torch.float64) or not rows.is_contiguous():
        raise _lib.AdyoloHipError("seld_score: rows must be a contiguous float32 or float64 tensor on the device")
    if rows.numel() % 5 or (rows.dim() == 2 and rows.shape[1] != 5):
        raise _lib.AdyoloHipError("seld_score: rows %s are not (N, 5)" % (tuple(rows.shape),))
    for name, t, dt in (("counts", counts, torch.int32), ("file_ids", file_ids, torch.int32), ("out", out, torch.float64)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or t.device != rows.device:
            raise _lib.AdyoloHipError("seld_score: %s must be a contiguous %s tensor on %s" % (name, dt, rows.device))
    t_clip = int(t_clip)
    n_clips = file_ids.numel()
    if t_clip <= 0 or counts.numel() != n_clips * t_clip:
        raise _lib.AdyoloHipError("seld_score: %d frame counts for %d clips of %d frames" % (counts.numel(), n_clips, t_clip))
    if out.shape != (table.n_files, 9 * table.nb_classes + 3):
        raise _lib.AdyoloHipError("seld_score: out %s is not [%d][%d]" % (tuple(out.shape), table.n_files,
                                                                          9 * table.nb_classes + 3))
    own = status is None
    if own:
        status = torch.zeros(1, dtype=torch.int32, device=rows.device)
    words = _lib.load().adyolo_seld_score_workspace_words(n_clips, t_clip, table.max_blocks, table.nb_classes)
    ws = torch.empty(max(1, words), dtype=torch.float32, device=rows.device)
    _c("adyolo_seld_score", _p(rows) if rows.numel() else NULL, int(rows.dtype == torch.float64), rows.numel() // 5,
       _p(counts), n_clips, t_clip, _p(file_ids), _p(table.file_info), _p(table.ref_off), _p(table.ref_ev),
       _p(table.keep), table.n_files, table.nb_classes, table.frames_per_block, table.max_blocks, float(table.doa_threshold),
       _p(ws), _p(out), _p(status), _stream())
    if own:
        seld_status_check(status)
    return status


SELD_RUN_WORDS = 8                                            # ADYOLO_SELD_RUN_WORDS: {file, f0, r0, n, last, 0, 0, 0}
SELD_BAD_RUN = 32                                             # ADYOLO_SELD_BAD_RUN


def seld_score_runs(rows, counts, table, segments, seg_blocks, out, status=None):
    """Adds the SELD accumulators of the segments of ONE stitched run of frames into out [files][9 C + 3] float64 (adyolo_hip.h,
    ``adyolo_seld_score_runs``).  rows, table, out, status as for ``seld_score``; counts (run frames,) int32: rows per frame of
    the run (``select_device_rows(run, 1, trim=False)``); segments int32 (S, 8) on the device: {file id, f0, r0, n, last, 0, 0,
    0} per row (``seld_metrics.run_segments``); seg_blocks: at least the blocks any segment covers.  A file scored in ordered
    segments into a zeroed row ends with the bits of one ``seld_score`` call on the whole recording.  No sync with a status."""
    if not rows.is_cuda or rows.dtype not in (torch.float32, torch.float64) or not rows.is_contiguous():
        raise _lib.AdyoloHipError("seld_score_runs: rows must be a contiguous float32 or float64 tensor on the device")
    if rows.numel() % 5 or (rows.dim() == 2 and rows.shape[1] != 5):
        raise _lib.AdyoloHipError("seld_score_runs: rows %s are not (N, 5)" % (tuple(rows.shape),))
    for name, t, dt in (("counts", counts, torch.int32), ("segments", segments, torch.int32), ("out", out, torch.float64)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or t.device != rows.device:
            raise _lib.AdyoloHipError("seld_score_runs: %s must be a contiguous %s tensor on %s" % (name, dt, rows.device))
    if segments.dim() != 2 or segments.shape[0] < 1 or segments.shape[1] != SELD_RUN_WORDS:
        raise _lib.AdyoloHipError("seld_score_runs: segments %s are not (S, %d)" % (tuple(segments.shape), SELD_RUN_WORDS))
    run_frames, n_seg, seg_blocks = counts.numel(), segments.shape[0], int(seg_blocks)
    if run_frames < 1 or seg_blocks < 1:
        raise _lib.AdyoloHipError("seld_score_runs: a run of %d frames, %d blocks per segment" % (run_frames, seg_blocks))
    if out.shape != (table.n_files, 9 * table.nb_classes + 3):
        raise _lib.AdyoloHipError("seld_score_runs: out %s is not [%d][%d]" % (tuple(out.shape), table.n_files,
                                                                               9 * table.nb_classes + 3))
    own = status is None
    if own:
        status = torch.zeros(1, dtype=torch.int32, device=rows.device)
    words = _lib.load().adyolo_seld_score_runs_workspace_words(n_seg, run_frames, seg_blocks, table.nb_classes)
    ws = torch.empty(max(1, words), dtype=torch.float32, device=rows.device)
    _c("adyolo_seld_score_runs", _p(rows) if rows.numel() else NULL, int(rows.dtype == torch.float64), rows.numel() // 5,
       _p(counts), run_frames, _p(segments), n_seg, _p(table.file_info), _p(table.ref_off), _p(table.ref_ev), _p(table.keep),
       table.n_files, table.nb_classes, table.frames_per_block, seg_blocks, float(table.doa_threshold), _p(ws), _p(out),
       _p(status), _stream())
    if own:
        seld_status_check(status)
    return status


GRAD_SUMSQ_MAX_PARTS = 1024       # adyolo_grad_sumsq_parts(n) never exceeds this (csrc/optim.hip OX_SUMSQ_BLOCKS)
OPTIM_SCRATCH_FLOATS = 4          # st_dev of the calls below: {a, b, total_norm, clip_coef} (include/adyolo_hip.h, K11)


def grad_sumsq_parts(n):
    """number of float64 partials ``grad_sumsq`` writes for a gradient of n elements (what ``clip_partials`` must hold)"""
    return int(_lib.load().adyolo_grad_sumsq_parts(int(n)))


def _chk_optim_dev(what, n, step_dev, st_dev, partials):
    if step_dev is not None and (not step_dev.is_cuda or step_dev.dtype != torch.int64 or step_dev.numel() != 1):
        raise _lib.AdyoloHipError("%s needs a one-element int64 step counter on the device" % what)
    if st_dev is not None and st_dev.numel() < OPTIM_SCRATCH_FLOATS:
        raise _lib.AdyoloHipError("%s needs %d floats of scratch on the device" % (what, OPTIM_SCRATCH_FLOATS))
    if partials is not None and (not partials.is_cuda or partials.dtype != torch.float64 or not partials.is_contiguous()
                                 or partials.numel() < grad_sumsq_parts(n)):
        raise _lib.AdyoloHipError("%s needs %d contiguous float64 partials on the device" % (what, grad_sumsq_parts(n)))


def _max_norm(what, partials, max_norm):
    if (partials is None) != (max_norm is None):
        raise _lib.AdyoloHipError("%s: partials and max_norm go together (both or neither)" % what)
    return float(max_norm) if max_norm is not None else 0.0


def _optim_step(what, param, grad, states, hyper, step_dev, st_dev, grad_scale, partials, max_norm, sched=(), groups=(),
                momentum=None, guard=None, accum=None):
    """The checks and the call behind every optimizer wrapper below.  ``what``: the wrapper's name, in errors and (as
    ``adyolo_<what>``) the entry point.  states: the rule's state buffers; hyper: its scalars, in the entry point's order;
    sched: (sched_dev, sched_out, ema) of the scheduled forms; groups: (groups_dev, groups_out, group_map) of the grouped
    ones; momentum: SGD's, whose one state buffer is needed, and passed on, only when it is not 0; guard: the record of the
    guarded entry points, which take every form's arguments (null where the form has none) and a negative max_norm for
    "no clipping"; accum: (accum, accum_dev, accum_steps) of the accumulating entry points, which take the guarded ones'
    arguments with the guard optional."""
    _chk(param, grad, *states, st_dev)
    _chk_optim_dev(what, param.numel(), step_dev, st_dev, partials)
    form = ()                         # what the entry point takes after grad_scale: sched_dev, sched_out, ema, then
    if sched:                         # groups_dev, groups_out, n_groups, group_map
        _chk_sched(what, param, *sched)
        form = tuple(map(_p, sched))
    if groups:
        groups_dev, groups_out, group_map = groups
        form += (_p(groups_dev), _p(groups_out), _chk_groups(what, param, *groups), _p(group_map))
    if momentum is not None and momentum != 0.0 and states[0] is None:
        raise _lib.AdyoloHipError("%s with momentum needs a momentum buffer" % what)
    if momentum == 0.0:
        states = (None,)              # SGD without momentum: the buffer is not passed on
    if guard is not None or accum is not None:        # every form's arguments, null where the form has none
        if not sched:
            form = (_p(None),) * 3
        if not groups:
            form += (_p(None), _p(None), 0, _p(None))
        form += (_p(guard),)
    if accum is not None:
        form += (_p(accum[0]), _p(accum[1]), int(accum[2]))
    if guard is not None:
        if max_norm is not None and not float(max_norm) >= 0.0:
            raise _lib.AdyoloHipError("%s: max_norm must not be negative (None = no clipping)" % what)
        norm = -1.0 if max_norm is None else float(max_norm)
    else:
        norm = _max_norm(what, partials, max_norm)
    # every step entry point: param, grad, state..., n, hyper..., step_dev, st_dev, partials, max_norm, grad_scale, form..., stream
    _c("adyolo_" + what, _p(param), _p(grad), *map(_p, states), param.numel(), *hyper, _p(step_dev), _p(st_dev), _p(partials),
       norm, grad_scale, *form, _stream())


def grad_sumsq(grad, partials, grad_scale=1.0):
    """partials[k] = float64 sum of (grad * grad_scale)^2 over workgroup k's share: fixed grid, fixed order, no atomics."""
    _chk(grad)
    _chk_optim_dev("grad_sumsq", grad.numel(), None, None, partials)
    if partials is None:
        raise _lib.AdyoloHipError("grad_sumsq needs float64 partials")
    _c("adyolo_grad_sumsq", _p(grad), grad.numel(), grad_scale, _p(partials), _stream())
    return partials


def grad_norm_dev(grad, partials, st_dev, max_norm, grad_scale=1.0):
    """st_dev[2] = ||grad * grad_scale||_2 (summed in float64, written as fp32), st_dev[3] = min(1, max_norm / (norm + 1e-6)):
    the clipping part of an optimizer step on its own.  Returns st_dev; no host sync."""
    _chk(grad, st_dev)
    _chk_optim_dev("grad_norm_dev", grad.numel(), None, st_dev, partials)
    if partials is None:
        raise _lib.AdyoloHipError("grad_norm_dev needs float64 partials")
    _c("adyolo_grad_norm_dev", _p(grad), grad.numel(), grad_scale, _p(partials), max_norm, _p(st_dev), _stream())
    return st_dev


def adam_step_dev(param, grad, exp_avg, exp_avg_sq, step_dev, st_dev, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                  weight_decay=0.0, grad_scale=1.0, partials=None, max_norm=None, decoupled=False):
    """torch.optim.Adam (``decoupled``: torch.optim.AdamW) with the step counter on the device: step_dev (int64, one element) is
    incremented by the call, st_dev (``OPTIM_SCRATCH_FLOATS`` floats) receives the bias corrections.  No argument changes from
    step to step (hipGraph-replayable).  partials (``grad_sumsq_parts(n)`` float64) + max_norm: clip the gradient norm first
    (st_dev[2] = the pre-clip norm); partials None = no clipping, the same kernel with a coefficient of exactly 1."""
    _optim_step("adam_step_dev", param, grad, (exp_avg, exp_avg_sq), (lr, betas[0], betas[1], eps, weight_decay,
                int(bool(decoupled))), step_dev, st_dev, grad_scale, partials, max_norm)


def adamw_step_dev(param, grad, exp_avg, exp_avg_sq, step_dev, st_dev, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                   weight_decay=1e-2, grad_scale=1.0, partials=None, max_norm=None):
    """``adam_step_dev`` with torch.optim.AdamW's decoupled decay and its default weight decay."""
    adam_step_dev(param, grad, exp_avg, exp_avg_sq, step_dev, st_dev, lr, betas, eps, weight_decay, grad_scale, partials,
                  max_norm, decoupled=True)


def sgd_step_dev(param, grad, momentum_buf, step_dev, st_dev, lr=1e-3, weight_decay=0.0, momentum=0.0, dampening=0.0,
                 nesterov=False, grad_scale=1.0, partials=None, max_norm=None):
    """torch.optim.SGD.  momentum_buf: None when momentum == 0 (nothing is allocated or touched); the call that takes step_dev
    from 0 to 1 initialises it with the gradient (no dampening)."""
    _optim_step("sgd_step_dev", param, grad, (momentum_buf,), (lr, weight_decay, momentum, dampening, int(bool(nesterov))),
                step_dev, st_dev, grad_scale, partials, max_norm, momentum=momentum)


# The scheduled forms (include/adyolo_hip.h, "The scheduled forms"): the rate is derived on the device from the step counter
# and ``sched_dev``; the layout of that table, by index:
SCHED_TABLE_DOUBLES = 24          # float64 elements of sched_dev (adyolo_sched_table_doubles())
SCHED_OUT_FLOATS = 4              # float32 elements of sched_out: {lr, AdamW decay, EMA weight, EMA first flag}
SCHED_KINDS = {"constant": 0, "step": 1, "multistep": 2, "exponential": 3, "cosine": 4}
(SCHED_KIND, SCHED_BASE, SCHED_EVERY, SCHED_WARMUP, SCHED_START, SCHED_GAMMA, SCHED_STEP_SIZE, SCHED_T_MAX, SCHED_ETA_MIN,
 SCHED_N_MILESTONES, SCHED_MILESTONE0) = range(11)
SCHED_MAX_MILESTONES = 8
SCHED_OFFSET, SCHED_EMA_DECAY, SCHED_EMA_WARMUP, SCHED_EMA_OFFSET = 18, 19, 20, 21


def _chk_sched(what, param, sched_dev, sched_out, ema):
    if (not sched_dev.is_cuda or sched_dev.dtype != torch.float64 or not sched_dev.is_contiguous()
            or sched_dev.numel() < SCHED_TABLE_DOUBLES):
        raise _lib.AdyoloHipError("%s needs a schedule table of %d contiguous float64 on the device" % (what, SCHED_TABLE_DOUBLES))
    _chk(sched_out, ema)
    if sched_out.numel() < SCHED_OUT_FLOATS:
        raise _lib.AdyoloHipError("%s needs %d floats of sched_out on the device" % (what, SCHED_OUT_FLOATS))
    if ema is not None and ema.numel() != param.numel():
        raise _lib.AdyoloHipError("%s: the EMA buffer has %d elements, the parameters %d" % (what, ema.numel(), param.numel()))


def adam_step_sched_dev(param, grad, exp_avg, exp_avg_sq, step_dev, st_dev, sched_dev, sched_out, ema=None,
                        betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, partials=None, max_norm=None,
                        decoupled=False):
    """``adam_step_dev`` whose learning rate is computed by the step's prep kernel from step_dev and the table sched_dev
    (``SCHED_TABLE_DOUBLES`` float64) and written to sched_out[0] (``SCHED_OUT_FLOATS`` floats); a constant schedule gives
    ``adam_step_dev``'s bits.  ema: a buffer like param that receives the moving average of the parameters in the same launch."""
    _optim_step("adam_step_sched_dev", param, grad, (exp_avg, exp_avg_sq), (betas[0], betas[1], eps, weight_decay,
                int(bool(decoupled))), step_dev, st_dev, grad_scale, partials, max_norm, (sched_dev, sched_out, ema))


def sgd_step_sched_dev(param, grad, momentum_buf, step_dev, st_dev, sched_dev, sched_out, ema=None, weight_decay=0.0,
                       momentum=0.0, dampening=0.0, nesterov=False, grad_scale=1.0, partials=None, max_norm=None):
    """``sgd_step_dev`` with the learning rate from the device-side schedule (see ``adam_step_sched_dev``)."""
    _optim_step("sgd_step_sched_dev", param, grad, (momentum_buf,), (weight_decay, momentum, dampening, int(bool(nesterov))),
                step_dev, st_dev, grad_scale, partials, max_norm, (sched_dev, sched_out, ema), momentum=momentum)


# The scheduled forms with parameter groups (include/adyolo_hip.h): a base rate and a weight decay per group of elements
OPTIM_MAX_GROUPS = 16             # adyolo_optim_max_groups()
GROUP_OUT_FLOATS = 4              # per group in groups_out: {rate, rate / bc1 (Adam) or rate (SGD), AdamW decay, weight_decay}


def _chk_groups(what, param, groups_dev, groups_out, group_map):
    if (not groups_dev.is_cuda or groups_dev.dtype != torch.float64 or not groups_dev.is_contiguous() or groups_dev.dim() != 2
            or groups_dev.shape[1] != 2 or not 1 <= groups_dev.shape[0] <= OPTIM_MAX_GROUPS):
        raise _lib.AdyoloHipError("%s needs groups_dev (G, 2) contiguous float64 on the device, 1 <= G <= %d"
                                  % (what, OPTIM_MAX_GROUPS))
    _chk(groups_out)
    if tuple(groups_out.shape) != (groups_dev.shape[0], GROUP_OUT_FLOATS):
        raise _lib.AdyoloHipError("%s needs groups_out (%d, %d)" % (what, groups_dev.shape[0], GROUP_OUT_FLOATS))
    if (not group_map.is_cuda or group_map.dtype != torch.uint8 or not group_map.is_contiguous()
            or group_map.numel() != param.numel() or group_map.device != param.device):
        raise _lib.AdyoloHipError("%s needs a group map of %d contiguous uint8 on the parameters' device"
                                  % (what, param.numel()))
    return int(groups_dev.shape[0])


def adam_step_groups_dev(param, grad, exp_avg, exp_avg_sq, step_dev, st_dev, sched_dev, sched_out, groups_dev, groups_out,
                         group_map, ema=None, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, partials=None, max_norm=None,
                         decoupled=False):
    """``adam_step_sched_dev`` with a base rate and a weight decay per parameter group: groups_dev (G, 2) float64
    {base rate, weight_decay}, groups_out (G, ``GROUP_OUT_FLOATS``) float32 written every step (column 0: the groups' rates),
    group_map uint8, one entry per element of param.  The norm and the clip coefficient stay global."""
    _optim_step("adam_step_groups_dev", param, grad, (exp_avg, exp_avg_sq), (betas[0], betas[1], eps, int(bool(decoupled))),
                step_dev, st_dev, grad_scale, partials, max_norm, (sched_dev, sched_out, ema), (groups_dev, groups_out, group_map))


def sgd_step_groups_dev(param, grad, momentum_buf, step_dev, st_dev, sched_dev, sched_out, groups_dev, groups_out, group_map,
                        ema=None, momentum=0.0, dampening=0.0, nesterov=False, grad_scale=1.0, partials=None, max_norm=None):
    """``sgd_step_sched_dev`` with a base rate and a weight decay per parameter group (see ``adam_step_groups_dev``)."""
    _optim_step("sgd_step_groups_dev", param, grad, (momentum_buf,), (momentum, dampening, int(bool(nesterov))), step_dev,
                st_dev, grad_scale, partials, max_norm, (sched_dev, sched_out, ema), (groups_dev, groups_out, group_map),
                momentum=momentum)


# The guarded steps (include/adyolo_hip.h, "The guarded steps"): a step that does nothing when the gradient is not finite
OPTIM_GUARD_WORDS = 4             # int64 elements of the guard record: {attempts, skipped, last skipped, run} (adyolo_optim_guard_words())


def _chk_guard(what, param, guard, partials):
    if (guard is None or not guard.is_cuda or guard.dtype != torch.int64 or not guard.is_contiguous()
            or guard.numel() < OPTIM_GUARD_WORDS or guard.device != param.device):
        raise _lib.AdyoloHipError("%s needs a guard record of %d contiguous int64 on the parameters' device"
                                  % (what, OPTIM_GUARD_WORDS))
    if partials is None:
        raise _lib.AdyoloHipError("%s needs float64 partials: the guard always sums the squares" % what)


def _guard_forms(what, sched_dev, sched_out, ema, groups_dev, groups_out, group_map):
    """-> (sched, groups) for ``_optim_step``: what is not None decides the form, as in the entry point"""
    if sched_dev is None and (groups_dev is not None or ema is not None or sched_out is not None):
        raise _lib.AdyoloHipError("%s: groups, sched_out and the EMA need sched_dev" % what)
    if (groups_dev is None) != (groups_out is None) or (groups_dev is None) != (group_map is None):
        raise _lib.AdyoloHipError("%s: groups_dev, groups_out and group_map go together" % what)
    sched = () if sched_dev is None else (sched_dev, sched_out, ema)
    return sched, (() if groups_dev is None else (groups_dev, groups_out, group_map))


def adam_step_guard_dev(param, grad, exp_avg, exp_avg_sq, step_dev, st_dev, guard, partials, lr=1e-3, betas=(0.9, 0.999),
                        eps=1e-8, weight_decay=0.0, grad_scale=1.0, max_norm=None, decoupled=False, sched_dev=None,
                        sched_out=None, ema=None, groups_dev=None, groups_out=None, group_map=None):
    """``adam_step_dev`` / ``adam_step_sched_dev`` / ``adam_step_groups_dev`` (sched_dev / groups_dev given or not decide which;
    lr is ignored with sched_dev, weight_decay with groups_dev) behind the non-finite guard: the sum of squares always runs
    (partials is required; max_norm None = no clipping, coefficient exactly 1), st_dev[2] is the norm of every attempt, and
    when it is not finite the call changes nothing but st_dev[2] and guard (``OPTIM_GUARD_WORDS`` int64: attempts, skipped,
    last attempt skipped, run of consecutive skips) -- step_dev does not tick.  A finite gradient gives the unguarded bits."""
    what = "adam_step_guard_dev"
    _chk_guard(what, param, guard, partials)
    sched, groups = _guard_forms(what, sched_dev, sched_out, ema, groups_dev, groups_out, group_map)
    _optim_step(what, param, grad, (exp_avg, exp_avg_sq), (lr, betas[0], betas[1], eps, weight_decay, int(bool(decoupled))),
                step_dev, st_dev, grad_scale, partials, max_norm, sched, groups, guard=guard)


def sgd_step_guard_dev(param, grad, momentum_buf, step_dev, st_dev, guard, partials, lr=1e-3, weight_decay=0.0, momentum=0.0,
                       dampening=0.0, nesterov=False, grad_scale=1.0, max_norm=None, sched_dev=None, sched_out=None, ema=None,
                       groups_dev=None, groups_out=None, group_map=None):
    """``sgd_step_dev`` / ``sgd_step_sched_dev`` / ``sgd_step_groups_dev`` behind the non-finite guard (see
    ``adam_step_guard_dev``); a skipped first attempt leaves the next one the first (the momentum buffer's initialisation)."""
    what = "sgd_step_guard_dev"
    _chk_guard(what, param, guard, partials)
    sched, groups = _guard_forms(what, sched_dev, sched_out, ema, groups_dev, groups_out, group_map)
    _optim_step(what, param, grad, (momentum_buf,), (lr, weight_decay, momentum, dampening, int(bool(nesterov))), step_dev,
                st_dev, grad_scale, partials, max_norm, sched, groups, momentum=momentum, guard=guard)


# The accumulating steps (include/adyolo_hip.h, "The accumulating steps"): K micro-batches, one optimizer step
OPTIM_ACCUM_WORDS = 4             # int64 elements of the accumulation record: {next micro index, calls, cycles, last call held}
#                                   (adyolo_optim_accum_words())


def _chk_accum(what, param, accum, accum_dev, accum_steps, guard, partials):
    _chk(accum)
    if accum is None or accum.numel() != param.numel() or accum.device != param.device:
        raise _lib.AdyoloHipError("%s needs an accumulator of %d floats on the parameters' device" % (what, param.numel()))
    if (accum_dev is None or not accum_dev.is_cuda or accum_dev.dtype != torch.int64 or not accum_dev.is_contiguous()
            or accum_dev.numel() < OPTIM_ACCUM_WORDS or accum_dev.device != param.device):
        raise _lib.AdyoloHipError("%s needs an accumulation record of %d contiguous int64 on the parameters' device"
                                  % (what, OPTIM_ACCUM_WORDS))
    if isinstance(accum_steps, bool) or int(accum_steps) != accum_steps or int(accum_steps) < 1:
        raise _lib.AdyoloHipError("%s: accum_steps must be an integer >= 1, not %r" % (what, accum_steps))
    if guard is not None:
        _chk_guard(what, param, guard, partials)
    return accum, accum_dev, int(accum_steps)


def adam_step_accum_dev(param, grad, exp_avg, exp_avg_sq, step_dev, st_dev, accum, accum_dev, accum_steps, guard=None,
                        partials=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, max_norm=None,
                        decoupled=False, sched_dev=None, sched_out=None, ema=None, groups_dev=None, groups_out=None,
                        group_map=None):
    """One micro-step of a cycle of ``accum_steps`` calls.  Every call adds grad into accum (a buffer like grad; the cycle's
    first call overwrites it) in fp32, left to right.  All but the cycle's last call change nothing else but accum_dev
    (``OPTIM_ACCUM_WORDS`` int64: index of the next call in its cycle, calls, cycles, last call held).  The last call then takes
    the step of ``adam_step_dev`` / ``adam_step_sched_dev`` / ``adam_step_groups_dev`` (sched_dev / groups_dev decide which) --
    or, with guard, of ``adam_step_guard_dev`` -- on accum under ``float32(float64(grad_scale) / accum_steps)``, bit for bit.
    The position in the cycle is read on the device: the call is the same every time (hipGraph-replayable).  Without guard:
    partials and max_norm go together (both None = no clipping)."""
    what = "adam_step_accum_dev"
    acc = _chk_accum(what, param, accum, accum_dev, accum_steps, guard, partials)
    sched, groups = _guard_forms(what, sched_dev, sched_out, ema, groups_dev, groups_out, group_map)
    _optim_step(what, param, grad, (exp_avg, exp_avg_sq), (lr, betas[0], betas[1], eps, weight_decay, int(bool(decoupled))),
                step_dev, st_dev, grad_scale, partials, max_norm, sched, groups, guard=guard, accum=acc)


def sgd_step_accum_dev(param, grad, momentum_buf, step_dev, st_dev, accum, accum_dev, accum_steps, guard=None, partials=None,
                       lr=1e-3, weight_decay=0.0, momentum=0.0, dampening=0.0, nesterov=False, grad_scale=1.0, max_norm=None,
                       sched_dev=None, sched_out=None, ema=None, groups_dev=None, groups_out=None, group_map=None):
    """``sgd_step_dev`` / ``sgd_step_sched_dev`` / ``sgd_step_groups_dev`` (with guard: ``sgd_step_guard_dev``) once per cycle of
    ``accum_steps`` calls, on the accumulated gradient (see ``adam_step_accum_dev``)."""
    what = "sgd_step_accum_dev"
    acc = _chk_accum(what, param, accum, accum_dev, accum_steps, guard, partials)
    sched, groups = _guard_forms(what, sched_dev, sched_out, ema, groups_dev, groups_out, group_map)
    _optim_step(what, param, grad, (momentum_buf,), (lr, weight_decay, momentum, dampening, int(bool(nesterov))), step_dev,
                st_dev, grad_scale, partials, max_norm, sched, groups, momentum=momentum, guard=guard, accum=acc)


def nchw_to_nhwc8(x):
    _chk(x)
    b, c, h, w = x.shape
    y = _new(x, b, h, w, 8)
    _c("adyolo_nchw_to_nhwc8", _p(x), _p(y), b, c, h, w, _stream())
    return y


# ---------------------------------------------------------------------------------------------- conformer pieces
def _kp(kh, kw, c):
    return (kh * kw * c + 3) // 4 * 4


def conv_out_hw(h, w, kh, kw, sh, sw, ph, pw):
    return (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1


# ---------------------------------------------------------------------------------------------- 1-D Winograd F(4, 3) (K9w)
def wino1d_ok(n, h, cin, cout):
    """The 3 x 1 convolution along H (x [N][H][1][Cin]) takes the 1-D Winograd form: whole output tiles, GEMM-friendly channel
    counts and enough rows to fill the chip with the six position GEMMs (``ADYOLO_WINO1D=0`` switches it off)."""
    return (W4_THRESHOLDS["wino1d"] and h % 4 == 0 and cin % 64 == 0 and cout % 64 == 0
            and n * (h // 4) >= 2048)


def wino1d_conv(x3, u, n, h, cin, cout):
    """x3 [N][H][Cin], u [6][Cout][Cin] (``wino1d_filter`` mode 0 / 1) -> (y [N][H][Cout], V [6][N T][Cin])."""
    rows = n * (h // 4)
    v = _new(x3, 6, rows, cin)
    _c("adyolo_wino1d_in", _p(x3), _p(v), n, h, cin, _stream())
    m = _new(x3, 6, rows, cout)
    gemm_batched(v, u, m, rows, cout, cin, cin, cin, cout, False, False, 6, 1, rows * cin, 0, cout * cin, 0, rows * cout, 0)
    y = _new(x3, n, h, cout)
    _c("adyolo_wino1d_out", _p(m), _p(y), n, h, cout, _stream())
    return y, v


def wino1d_filter(w3, cout, cin, mode):
    """w3 [Cout][Cin][3] -> U [6][Cout][Cin] (mode 0) or [6][Cin][Cout] (mode 1: data gradient)."""
    u = _new(w3, 6, cin if mode else cout, cout if mode else cin)
    _c("adyolo_wino1d_filter", _p(w3), _p(u), cout, cin, mode, _stream())
    return u


def wino1d_wgrad(v, dy3, n, h, cin, cout, out=None):
    """v [6][N T][Cin] (the forward's transformed input), dy3 [N][H][Cout] -> dw [Cout][Cin][3] (into ``out`` when given)."""
    rows = n * (h // 4)
    e = _new(dy3, 6, rows, cout)
    _c("adyolo_wino1d_dy", _p(dy3), _p(e), n, h, cout, _stream())
    du = _new(dy3, 6, cout, cin)
    gemm_batched(e, v, du, cout, cin, rows, cout, cin, cin, True, True, 6, 1, rows * cout, 0, rows * cin, 0, cout * cin, 0)
    dw = out if out is not None else _new(dy3, cout, cin, 3)
    _c("adyolo_wino1d_filter", _p(dw), _p(du), cout, cin, 2, _stream())
    return dw


def conv_gemm(mode, src, other, n, h, w, cin, cout, kh, kw, sh, sw, ph, pw):
    """General strided convolution as an implicit GEMM (no column buffer), channels-last.
    mode 0: src x [N][H][W][Cin], other wk = pack_wk(w) -> y [N][Ho][Wo][Cout]
    mode 1: src dy [N][Ho][Wo][Cout], other wkT = pack_wk(w.transpose(0, 1)) -> dx [N][H][W][Cin]
    mode 2: src x, other dy -> dwk [Cout][Kp] (split-K over the output pixels, summed in a fixed order)."""
    _chk(src, other)
    ho, wo = conv_out_hw(h, w, kh, kw, sh, sw, ph, pw)
    splits, slabs = 1, None
    if mode == 0:
        out = _new(src, n, ho, wo, cout)
    elif mode == 1:
        out = _new(src, n, h, w, cin)
    else:
        kp = _kp(kh, kw, cin)
        out = _new(src, cout, kp)
        splits = wgrad_splits(cout, kp, n * ho * wo)
        if splits > 1:
            slabs = _new(src, splits, cout, kp)
    _c("adyolo_conv_gemm", _p(src), _p(other), _p(out), _p(slabs), mode, n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, splits,
       _stream())
    return out


def pack_wk(w):
    """w [Cout][Cin][KH][KW] -> [Cout][Kp] with k = (kh*KW+kw)*Cin + ci."""
    _chk(w)
    cout, cin, kh, kw = w.shape
    wk = _new(w, cout, _kp(kh, kw, cin))
    _c("adyolo_pack_wk", _p(w), _p(wk), cout, cin, kh, kw, 1, _stream())
    return wk


def unpack_wk(wk, cout, cin, kh, kw, out=None):
    w = out if out is not None else _new(wk, cout, cin, kh, kw)
    _c("adyolo_pack_wk", _p(w), _p(wk), cout, cin, kh, kw, 0, _stream())
    return w


def maxpool3_fwd(x):
    _chk(x)
    n, h, w, c = x.shape
    wo = (w + 2 - 3) // 2 + 1
    y = _new(x, n, h, wo, c)
    arg = torch.empty((n, h, wo, c), dtype=torch.uint8, device=x.device)
    _c("adyolo_maxpool3_fwd", _p(x), _p(y), _p(arg), n, h, w, c, _stream())
    return y, arg


def maxpool3_bwd(dy, arg, w):
    _chk(dy)
    n, h, _, c = dy.shape
    dx = _new(dy, n, h, w, c)                   # (gather form: every element is written)
    _c("adyolo_maxpool3_bwd", _p(dy), _p(arg), _p(dx), n, h, w, c, _stream())
    return dx


def affine_relu(x, scale, shift):
    _chk(x, scale, shift)
    c = x.shape[-1]
    y = torch.empty_like(x)
    _c("adyolo_affine_relu_nhwc", _p(x), _p(scale), _p(shift), _p(y), x.numel() // c, c, _stream())
    return y


def relu_bwd(dy, y):
    _chk(dy, y)
    dx = torch.empty_like(y)
    _c("adyolo_relu_bwd", _p(dy), _p(y), _p(dx), y.numel(), _stream())
    return dx


def dropout_axpby(x, z, a, b, p, seed, offset, offset_dev=None):
    """a * dropout(x) + b * z in one pass (z None: a * dropout(x)); the mask of ``dropout_apply(x, p, seed, offset, offset_dev)``."""
    _chk(x, z)
    y = torch.empty_like(x)
    _c("adyolo_dropout_axpby", _p(x), _p(z), _p(y), x.numel(), float(p), ctypes.c_uint64(seed),
       ctypes.c_uint64(offset & 0xFFFFFFFFFFFFFFFF), _p(offset_dev), float(a), float(b), _stream())
    return y


def axpby(x, z, a, b):
    _chk(x, z)
    y = torch.empty_like(x)
    _c("adyolo_axpby", _p(x), _p(z), _p(y), float(a), float(b), x.numel(), _stream())
    return y


def swish_fwd(x):
    _chk(x)
    y = torch.empty_like(x)
    _c("adyolo_swish_fwd", _p(x), _p(y), x.numel(), _stream())
    return y


def swish_bwd(dy, x):
    _chk(dy, x)
    dx = torch.empty_like(x)
    _c("adyolo_swish_bwd", _p(dy), _p(x), _p(dx), x.numel(), _stream())
    return dx


def glu_fwd(x2d):
    _chk(x2d)
    r, c2 = x2d.shape
    y = _new(x2d, r, c2 // 2)
    _c("adyolo_glu_fwd", _p(x2d), _p(y), r, c2 // 2, _stream())
    return y


def glu_bwd(dy2d, x2d):
    _chk(dy2d, x2d)
    dx = torch.empty_like(x2d)
    _c("adyolo_glu_bwd", _p(dy2d), _p(x2d), _p(dx), x2d.shape[0], x2d.shape[1] // 2, _stream())
    return dx


def dwconv3(x, w, bias, dilation, flip=False):
    """x [B][T][C], w [C][3] (or [C][1][3]), bias [C] or None."""
    _chk(x, w, bias)
    b, t, c = x.shape
    y = torch.empty_like(x)
    _c("adyolo_dwconv3_fwd", _p(x), _p(w), _p(bias), _p(y), b, t, c, int(dilation), int(flip), _stream())
    return y


def dwconv3_wgrad(dy, x, dilation, out_dw=None, out_db=None):
    _chk(dy, x)
    b, t, c = x.shape
    dw = out_dw if out_dw is not None else _new(x, c, 3)
    db = out_db if out_db is not None else _new(x, c)
    partial, cws = _new(x, 1024, 4 * c), _new(x, 1024, 3 * c)
    _c("adyolo_dwconv3_wgrad", _p(dy), _p(x), _p(dw), _p(db), _p(partial), _p(cws), b, t, c, int(dilation), _stream())
    return dw, db


def softmax_fwd(s2d, scale):
    _chk(s2d)
    p = torch.empty_like(s2d)
    _c("adyolo_softmax_fwd", _p(s2d), _p(p), s2d.shape[0], s2d.shape[1], float(scale), _stream())
    return p


def softmax_bwd(dp2d, p2d, scale):
    _chk(dp2d, p2d)
    ds = torch.empty_like(p2d)
    _c("adyolo_softmax_bwd", _p(dp2d), _p(p2d), _p(ds), p2d.shape[0], p2d.shape[1], float(scale), _stream())
    return ds


def avgpool1d(x, k, fac):
    _chk(x)
    b, t, c = x.shape
    y = _new(x, b, t // k, c)
    _c("adyolo_avgpool1d_fwd", _p(x), _p(y), b, t, c, k, float(fac), _stream())
    return y


def avgpool1d_bwd(dy, t, k, fac):
    _chk(dy)
    b, _, c = dy.shape
    dx = _new(dy, b, t, c)
    _c("adyolo_avgpool1d_bwd", _p(dy), _p(dx), b, t, c, k, float(fac), _stream())
    return dx


def ln_fwd(x2d, gamma, beta, eps=1e-5):
    _chk(x2d, gamma, beta)
    y = torch.empty_like(x2d)
    _c("adyolo_ln_fwd", _p(x2d), _p(gamma), _p(beta), _p(y), x2d.shape[0], x2d.shape[1], eps, _stream())
    return y


def ln_bwd(dy2d, x2d, gamma, eps=1e-5, acc_dgamma=None, acc_dbeta=None):
    """acc_dgamma / acc_dbeta: the kernel ADDS the two gradients into these (the parameters' slices of the flat gradient
    buffer, zeroed at the start of the step) instead of into fresh zeros."""
    _chk(dy2d, x2d, gamma)
    r, c = x2d.shape
    dx = torch.empty_like(x2d)
    dgamma = acc_dgamma if acc_dgamma is not None else _zeros(x2d, c)
    dbeta = acc_dbeta if acc_dbeta is not None else _zeros(x2d, c)
    partial = _new(x2d, 1024 * 512)
    _c("adyolo_ln_bwd", _p(dy2d), _p(x2d), _p(gamma), _p(dx), _p(dgamma), _p(dbeta), _p(partial), r, c, eps, _stream())
    return dx, dgamma, dbeta


def gemm_batched(a, b, c, m, n, k, lda, ldb, ldc, trans_a, trans_b, outer, inner, oa, ia, ob, ib, oc, ic, alpha=1.0,
                 accumulate=False):
    _c("adyolo_gemm_batched", _p(a), _p(b), _p(c), m, n, k, lda, ldb, ldc, int(trans_a), int(trans_b), outer, inner,
       oa, ia, ob, ib, oc, ic, float(alpha), int(accumulate), _stream())
    return c


# ---------------------------------------------------------------------------------------------- attention (flash style)
def _seed_args(seed):
    """seed: an int, or a one-element int32 tensor on the device holding the 32-bit seed (``seed32_dev``: hipGraph replays)"""
    if isinstance(seed, torch.Tensor):
        return ctypes.c_uint32(0), _p(seed)
    return ctypes.c_uint32(seed & 0xFFFFFFFF), None


def seed32_dev(seed, offset, offset_dev):
    """The value ``rng.DropoutStream.seed32`` computes on the host, computed on the device from (seed, offset + *offset_dev) into a
    one-element int32 tensor: a recorded step replays it with the stream's current offset."""
    out = torch.empty(1, dtype=torch.int32, device=offset_dev.device)
    _c("adyolo_seed32_dev", ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), ctypes.c_uint64(offset & 0xFFFFFFFFFFFFFFFF), _p(offset_dev),
       _p(out), _stream())
    return out


def attn_fwd(q, k, v, heads, scale, dropout_p=0.0, seed=0, want_lse=True):
    """q, k, v [B][T][heads*64] -> ctx [B][T][heads*64], lse2 [B][heads][T] (or None); scores never reach HBM."""
    _chk(q, k, v)
    b, t, e = q.shape
    ctxv = torch.empty_like(q)
    lse = _new(q, b, heads, t) if want_lse else None
    sv, sp = _seed_args(seed)
    _c("adyolo_attn_fwd", _p(q), _p(k), _p(v), _p(ctxv), _p(lse), b, t, heads, e // heads, float(scale), float(dropout_p),
       sv, sp, _stream())
    return ctxv, lse


def attn_bwd(q, k, v, ctxv, dctx, lse, heads, scale, dropout_p=0.0, seed=0):
    _chk(q, k, v, ctxv, dctx, lse)
    b, t, e = q.shape
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = _new(q, b, heads, t)
    sv, sp = _seed_args(seed)
    _c("adyolo_attn_bwd", _p(q), _p(k), _p(v), _p(ctxv), _p(dctx), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), b, t, heads,
       e // heads, float(scale), float(dropout_p), sv, sp, _stream())
    return dq, dk, dv


def attn_dropout_mask(like, b, t, heads, dropout_p, seed):
    """The (B, heads, T, T) mask (0 or 1/(1-p)) that attn_fwd / attn_bwd apply for (dropout_p, seed) -- tests only."""
    mask = torch.empty((b, heads, t, t), dtype=torch.float32, device=like.device)
    _c("adyolo_attn_dropout_mask", _p(mask), b, t, heads, float(dropout_p), ctypes.c_uint32(seed & 0xFFFFFFFF), _stream())
    return mask


# ---------------------------------------------------------------------------------------------- input pipeline (8f rows 2-3)
def pcm16_to_f32(pcm, out=None):
    """int16 samples (any shape, contiguous, on the GPU) -> float32 ``x / 32768 + 1e-8`` (datasets.py:105)."""
    if not pcm.is_cuda or pcm.dtype != torch.int16 or not pcm.is_contiguous():
        raise _lib.AdyoloHipError("pcm16_to_f32 needs a contiguous int16 tensor on a HIP device")
    if out is None:
        out = torch.empty(pcm.shape, dtype=torch.float32, device=pcm.device)
    _c("adyolo_pcm16_to_f32", _p(pcm), _p(out), pcm.numel(), _stream())
    return out


CORPUS_ITEM_WORDS = 8                                     # ADYOLO_CORPUS_ITEM_WORDS / _ROT_WORDS in adyolo_hip.h
CORPUS_STATUS = ((1, "more AD-YOLO rows than the target capacity"), (2, "an item outside the corpus"),
                 (4, "an event class outside [0, nb_classes)"), (8, "an Inf or NaN sample in a float32 recording"))
CORPUS_XYZ_SLOTS = 17                                     # ADYOLO_CORPUS_XYZ_SLOTS: no rotation + the 16 FOA combinations
CORPUS_FORMATS = {"seddoa": 0, "masked-seddoa": 0, "accdoa": 1, "adpit": 2}     # ADYOLO_CORPUS_SEDDOA / _ACCDOA / _ADPIT


def corpus_rot_table(combinations):
    """augmentations.COMBINATIONS -> the host table [16][8] float {sy, sz, sx, swap, az weight, az offset, el weight, 0}."""
    vals = []
    for (sy, sz, sx), swap, pw, dpi, tw in combinations:
        vals += [float(sy), float(sz), float(sx), float(swap), float(pw), float(dpi), float(tw), 0.0]
    return (ctypes.c_float * len(vals))(*vals)


def _corpus_i64(name, t, device):
    if not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous() or t.device != device:
        raise _lib.AdyoloHipError("%s must be a contiguous int64 tensor on %s" % (name, device))


def _corpus_tables(name, items, mates, device):
    """The item table of a corpus call and, where the call has one, its table of mates: rows like the items'."""
    _corpus_i64("%s: items" % name, items, device)
    if mates is not None:
        _corpus_i64("%s: mates" % name, mates, device)
        if tuple(mates.shape) != tuple(items.shape):
            raise _lib.AdyoloHipError("%s: mates %s do not match items %s" % (name, tuple(mates.shape), tuple(items.shape)))


def _corpus_gather_args(name, pcm, items, out, status, mates=None):
    """The argument checks of the gather family -> B."""
    dev = pcm.device
    if not pcm.is_cuda or pcm.dtype != torch.int16 or not pcm.is_contiguous() or pcm.dim() != 2 or pcm.shape[1] != 4:
        raise _lib.AdyoloHipError("%s: pcm must be a contiguous int16 tensor (S, 4) on the device" % name)
    _corpus_tables(name, items, mates, dev)
    _chk(out)
    b = items.shape[0] if items.dim() == 2 else 0
    if items.dim() != 2 or items.shape[1] != CORPUS_ITEM_WORDS or out.dim() != 3 or out.shape[0] != b or out.shape[2] != 4:
        raise _lib.AdyoloHipError("%s: items %s / out %s are not (B, %d) / (B, n, 4)"
                                  % (name, tuple(items.shape), tuple(out.shape), CORPUS_ITEM_WORDS))
    if status.dtype != torch.int32 or status.device != dev:
        raise _lib.AdyoloHipError("%s: status must be an int32 word on %s" % (name, dev))
    return b


def _host_table(tab):
    return NULL if tab is None else ctypes.cast(tab, ctypes.c_void_p)


def corpus_gather(pcm, items, rot, out, status, *, mates=None, mic_src=None, yaw_tab=None):
    """pcm int16 (S, 4) and items int64 (B, 8) on the device -> out (B, n, 4) float32: the int16 windows at the items' sample
    offsets as ``x / 32768 + 1e-8`` (adyolo_hip.h ``adyolo_corpus_gather``), then
    * FOA-rotated by their combinations (rot: ``corpus_rot_table``), or
    * ``mic_src`` (``corpus_mic_table``; rot may be None): MIC-format audio, the four capsules permuted by the combinations
      instead -- bit for bit ``pcm16_to_f32`` then ``mic_swap``; a combination that is no symmetry: a bad item;
    * ``yaw_tab`` (``corpus_yaw_table``; FOA only): every source yawed after its combination by word 7 of its row, whole degrees
      in [-180, 180) -- bit for bit ``pcm16_to_f32`` then ``augmentations.rotate_audio_yaw``; a yaw outside the range: a bad item;
    * ``mates`` int64 (B, 8) on the device: a second window per item summed in, rows like ``items`` with their own combinations
      (and yaws), the float32 bits of the gain in word 6, offset -1 = no mate -> out = a + g * m, bit for bit two plain gathers
      and that expression on float32 tensors.
    A bad item or mate: zeros for the sample and status bit 2.  status: int32 word on the device the call ORs its bits into.  No
    allocation, no sync."""
    name = "corpus_gather"
    b = _corpus_gather_args(name, pcm, items, out, status, mates)
    if mic_src is None and rot is None:
        raise _lib.AdyoloHipError("%s: the FOA form needs the rotation table" % name)
    if yaw_tab is not None:
        if mic_src is not None:
            raise _lib.AdyoloHipError("%s: yaw_tab with mic_src (there is no MIC yaw)" % name)
        _corpus_yaw_tab(name, yaw_tab, pcm.device, torch.float32, (360, 2))
    _c("adyolo_corpus_gather", _p(pcm), pcm.shape[0], _p(items), _p(mates), b, out.shape[1], _host_table(rot),
       _host_table(mic_src), _p(yaw_tab), _p(out), _p(status), _stream())
    return out


MIC_SWAP_NONE = 0xFFFFFFFF                                # ADYOLO_MIC_SWAP_NONE: a combination that is no symmetry of the array


def corpus_mic_table(sources):
    """{combination: (s0, s1, s2, s3)} (``augmentations.mic_swap_source`` of every symmetry) -> the host table uint32 [16] of
    ``corpus_gather``'s ``mic_src``: s_j in bits [8 j, 8 j + 2), ``MIC_SWAP_NONE`` for every other combination."""
    words = [MIC_SWAP_NONE] * 16
    for comb, src in sources.items():
        src = tuple(int(v) for v in src)
        if not 0 <= int(comb) < 16 or sorted(src) != [0, 1, 2, 3]:
            raise ValueError("corpus_mic_table: combination %r -> %r is not a permutation of the four channels" % (comb, src))
        words[int(comb)] = src[0] | src[1] << 8 | src[2] << 16 | src[3] << 24
    return (ctypes.c_uint32 * 16)(*words)


def audio_mix(audio, mate, gains, mixed, out=None):
    """audio, mate (B, n, 4) float32, gains float32 (B,), mixed bool (B,), all on the device ->
    ``mixed[b] ? audio[b] + gains[b] * mate[b] : audio[b]`` (a new tensor unless ``out`` is given; ``out`` may be ``audio`` itself).
    The product is rounded before the sum; an unmixed clip keeps its bits (adyolo_hip.h ``adyolo_audio_mix``)."""
    _chk(audio, mate)
    if audio.dim() != 3 or audio.shape[2] != 4 or tuple(mate.shape) != tuple(audio.shape) or mate.device != audio.device:
        raise _lib.AdyoloHipError("audio_mix: audio %s / mate %s are not two (B, n, 4) tensors on one device"
                                  % (tuple(audio.shape), tuple(mate.shape)))
    b, n, _ = audio.shape
    if gains.dtype != torch.float32 or gains.device != audio.device or not gains.is_contiguous() or tuple(gains.shape) != (b,):
        raise _lib.AdyoloHipError("audio_mix: gains must be a contiguous float32 tensor (%d,) on %s" % (b, audio.device))
    if mixed.dtype != torch.bool or mixed.device != audio.device or not mixed.is_contiguous() or tuple(mixed.shape) != (b,):
        raise _lib.AdyoloHipError("audio_mix: mixed must be a contiguous bool tensor (%d,) on %s" % (b, audio.device))
    if out is None:
        out = torch.empty_like(audio)
    else:
        _chk(out)
        if tuple(out.shape) != tuple(audio.shape) or out.device != audio.device:
            raise _lib.AdyoloHipError("audio_mix: out %s does not match audio %s" % (tuple(out.shape), tuple(audio.shape)))
    _c("adyolo_audio_mix", _p(audio), _p(mate), _p(gains), _p(mixed), _p(out), b, n, _stream())
    return out


def mic_swap(audio, src, out=None):
    """audio (B, n, 4) float32 and src int32 (B, 4) on the device -> out[b, i, j] = audio[b, i, src[b, j] & 3] (a new tensor
    unless ``out``, which must not overlap audio, is given).  The values are moved bit for bit (adyolo_hip.h ``adyolo_mic_swap``)."""
    _chk(audio)
    if audio.dim() != 3 or audio.shape[2] != 4:
        raise _lib.AdyoloHipError("mic_swap: audio %s is not (B, n, 4)" % (tuple(audio.shape),))
    b, n, _ = audio.shape
    if src.dtype != torch.int32 or src.device != audio.device or not src.is_contiguous() or tuple(src.shape) != (b, 4):
        raise _lib.AdyoloHipError("mic_swap: src must be a contiguous int32 tensor (%d, 4) on %s" % (b, audio.device))
    if out is None:
        out = torch.empty_like(audio)
    else:
        _chk(out)
        if tuple(out.shape) != tuple(audio.shape) or out.device != audio.device:
            raise _lib.AdyoloHipError("mic_swap: out %s does not match audio %s" % (tuple(out.shape), tuple(audio.shape)))
    _c("adyolo_mic_swap", _p(audio), _p(out), _p(src), b, n, _stream())
    return out


def corpus_labels_workspace_words(batch, max_events, mix=False):
    return int(_lib.load().adyolo_corpus_yolo_labels_workspace_words(int(batch), int(max_events), int(bool(mix))))


def _corpus_events(name, events, items, mates):
    """The checks every label call makes of its tables and of the event table -> (B, E)."""
    dev = items.device
    _corpus_tables(name, items, mates, dev)
    if not events.is_cuda or events.dtype != torch.float64 or not events.is_contiguous() or events.dim() != 2 \
            or events.shape[1] != 4 or events.device != dev:
        raise _lib.AdyoloHipError("%s: events must be a contiguous float64 tensor (E, 4) on %s" % (name, dev))
    return items.shape[0], events.shape[0]


def _corpus_yolo_args(name, events, items, max_events, bounds, grid, ws, target, count, status, mates=None):
    """The argument checks of the AD-YOLO label family -> (B, E, Gaz, Gel)."""
    dev = items.device
    b, n_ev = _corpus_events(name, events, items, mates)
    gaz, gel = int(grid[0]), int(grid[1])
    if bounds.dtype != torch.float64 or bounds.device != dev or not bounds.is_contiguous() or bounds.numel() != 2 * (gaz + gel):
        raise _lib.AdyoloHipError("%s: bounds must be float64 (2 Gaz + 2 Gel,) on %s" % (name, dev))
    _chk(target)
    if target.dim() != 2 or target.shape[1] != 7:
        raise _lib.AdyoloHipError("%s: target %s is not (cap, 7)" % (name, tuple(target.shape)))
    ws_words = corpus_labels_workspace_words(b, max_events, mix=mates is not None)
    for what, t, words in (("ws", ws, ws_words), ("count", count, 1), ("status", status, 1)):
        if t.dtype != torch.int32 or t.device != dev or not t.is_contiguous() or t.numel() < words:
            raise _lib.AdyoloHipError("%s: %s must be at least %d int32 words on %s" % (name, what, words, dev))
    return b, n_ev, gaz, gel


def corpus_yolo_labels(events, items, max_events, n_label_frames, bounds, grid, rot, ws, target, count, status, *, mates=None,
                       yaw=False):
    """The AD-YOLO rows of a batch on the device (adyolo_hip.h ``adyolo_corpus_yolo_labels``): events float64 (E, 4) {frame,
    class, az, el}, items int64 (B, 8), bounds float64 (2 Gaz + 2 Gel,), grid (Gaz, Gel), ws int32 of
    ``corpus_labels_workspace_words(B, max_events, mix=mates is not None)`` words -> target (cap, 7) float32 (b = -1 past the
    total), count int32 word = total rows.  ``mates`` (as for ``corpus_gather``): the rows of ``augmentations.merge_labels(item,
    mate)`` per item, each event under its own source's combination and frame offset, column 0 the item.  ``yaw``:
    ``augmentations.yaw_labels`` by word 7 of each row after its combination.  status: int32 word the call ORs its bits into.
    No allocation, no sync."""
    b, n_ev, gaz, gel = _corpus_yolo_args("corpus_yolo_labels", events, items, max_events, bounds, grid, ws, target, count, status,
                                          mates)
    _c("adyolo_corpus_yolo_labels", _p(events), n_ev, _p(items), _p(mates), b, int(max_events),
       int(n_label_frames), _p(bounds), gaz, gel, ctypes.cast(rot, ctypes.c_void_p), int(bool(yaw)), _p(ws), _p(target),
       target.shape[0], _p(count), _p(status), _stream())
    return target


def corpus_classwise_shape(loss, batch, n_label_frames, nb_classes):
    """The dense target of ``datasets.ClasswiseLabelEncoder`` stacked over a batch: (B, T', 4C) seddoa / masked-seddoa,
    (B, T', 3C) accdoa, (B, T', 6, 4, C) adpit."""
    if loss not in CORPUS_FORMATS:
        raise _lib.AdyoloHipError("corpus_classwise: loss %r is not one of %s" % (loss, sorted(CORPUS_FORMATS)))
    b, t, c = int(batch), int(n_label_frames), int(nb_classes)
    return {0: (b, t, 4 * c), 1: (b, t, 3 * c), 2: (b, t, 6, 4, c)}[CORPUS_FORMATS[loss]]


def _corpus_classwise_args(name, events, items, xyz, n_label_frames, nb_classes, loss, target, status, mates=None):
    """The argument checks of the class-wise label family -> (B, E)."""
    dev = items.device
    b, n_ev = _corpus_events(name, events, items, mates)
    if xyz.dtype != torch.float32 or xyz.device != dev or not xyz.is_contiguous() \
            or tuple(xyz.shape) != (n_ev, CORPUS_XYZ_SLOTS, 3):
        raise _lib.AdyoloHipError("%s: xyz must be a contiguous float32 tensor (%d, %d, 3) on %s"
                                  % (name, n_ev, CORPUS_XYZ_SLOTS, dev))
    want = corpus_classwise_shape(loss, b, n_label_frames, nb_classes)
    _chk(target)
    if tuple(target.shape) != want or target.device != dev:
        raise _lib.AdyoloHipError("%s: target %s on %s, expected %s on %s for %s"
                                  % (name, tuple(target.shape), target.device, want, dev, loss))
    if status.dtype != torch.int32 or status.device != dev or not status.is_contiguous() or status.numel() < 1:
        raise _lib.AdyoloHipError("%s: status must be an int32 word on %s" % (name, dev))
    return b, n_ev


def corpus_classwise_labels(events, items, xyz, max_events, n_label_frames, nb_classes, loss, target, status, *, mates=None,
                            rot=None, yaw_xyz=None):
    """The dense class-wise targets of a batch on the device (adyolo_hip.h ``adyolo_corpus_classwise_labels``): events float64
    (E, 4) {frame, class, az, el}, items int64 (B, 8), xyz float32 (E, 17, 3) (``corpus.xyz_table``) -> target float32 of
    ``corpus_classwise_shape(loss, B, n_label_frames, nb_classes)``, every element written.  ``mates`` (as for
    ``corpus_gather``): the targets of the host encoders on ``augmentations.merge_labels(item, mate)``, each event's direction
    vector from its own source's combination.  ``yaw_xyz`` (``corpus_yaw_xyz_tables``; needs rot: ``corpus_rot_table``): yawed
    sources (word 7 of each row), z from the event's xyz slot, x and y from the tables at the event's moved whole-degree angles.
    status: int32 word the call ORs its bits into.  No allocation, no sync."""
    name = "corpus_classwise_labels"
    b, n_ev = _corpus_classwise_args(name, events, items, xyz, n_label_frames, nb_classes, loss, target, status, mates)
    az = el = None
    if yaw_xyz is not None:
        if rot is None:
            raise _lib.AdyoloHipError("%s: yaw_xyz needs the rotation table" % name)
        az, el = _corpus_yaw_xyz_args(name, yaw_xyz, items.device)
    _c("adyolo_corpus_classwise_labels", _p(events), _p(xyz), n_ev, _p(items), _p(mates), b,
       int(max_events), int(n_label_frames), int(nb_classes), CORPUS_FORMATS[loss], _host_table(rot), _p(az), _p(el), _p(target),
       _p(status), _stream())
    return target


# ---- yaw rotation (aug_config.yaw_rotation_augment): with a yaw table the calls read each row's yaw, whole degrees, from word 7
CORPUS_YAW_WORD = 7                                       # ADYOLO_CORPUS_YAW_WORD


def corpus_yaw_table(device):
    """float32 (360, 2) on ``device``: {cos, sin} of the yaws -180 .. 179 degrees (``augmentations.yaw_cos_sin``), the
    ``yaw_tab`` of ``corpus_gather``."""
    from .augmentations import yaw_cos_sin
    return torch.tensor([[float(v) for v in yaw_cos_sin(phi)] for phi in range(-180, 180)], dtype=torch.float32).to(device)


def corpus_yaw_xyz_tables(device):
    """(az float64 (361, 2) = {cos, sin} of the azimuths -180 .. 180 degrees, el float64 (181,) = cos of the elevations -90 ..
    90) on ``device``, each value by the expressions of ``datasets._polar_to_xyz`` on a Python float: the ``yaw_xyz`` of
    ``corpus_classwise_labels``."""
    import numpy as np
    az = [[float(np.cos(float(a) * np.pi / 180)), float(np.sin(float(a) * np.pi / 180))] for a in range(-180, 181)]
    el = [float(np.cos(float(e) * np.pi / 180.0)) for e in range(-90, 91)]
    return torch.tensor(az, dtype=torch.float64).to(device), torch.tensor(el, dtype=torch.float64).to(device)


def _corpus_yaw_tab(name, tab, device, dtype, shape):
    if tab.dtype != dtype or tab.device != device or not tab.is_contiguous() or tuple(tab.shape) != shape:
        raise _lib.AdyoloHipError("%s: the yaw table must be a contiguous %s tensor %s on %s" % (name, dtype, shape, device))


def _corpus_yaw_xyz_args(name, yaw_xyz, device):
    az, el = yaw_xyz
    _corpus_yaw_tab(name, az, device, torch.float64, (361, 2))
    _corpus_yaw_tab(name, el, device, torch.float64, (181,))
    return az, el


WINDOW_WORDS = 8                                          # ADYOLO_WINDOW_WORDS: {offset, valid, src_lo, dst, n, recording, 0, 0}


def _window_table(name, windows, device):
    _corpus_i64("%s: windows" % name, windows, device)
    if windows.dim() != 2 or windows.shape[0] < 1 or windows.shape[1] != WINDOW_WORDS:
        raise _lib.AdyoloHipError("%s: windows %s are not (W, %d)" % (name, tuple(windows.shape), WINDOW_WORDS))
    return int(windows.shape[0])


def _gather_windows_args(name, pcm, windows, out, status):
    """The argument checks of both window gathers -> W."""
    dev = pcm.device
    if not pcm.is_cuda or pcm.dtype != torch.int16 or not pcm.is_contiguous() or pcm.dim() != 2 or pcm.shape[1] != 4:
        raise _lib.AdyoloHipError("%s: pcm must be a contiguous int16 tensor (S, 4) on the device" % name)
    w = _window_table(name, windows, dev)
    _chk(out)
    if out.dim() != 3 or out.shape[0] != w or out.shape[1] < 1 or out.shape[2] != 4 or out.device != dev:
        raise _lib.AdyoloHipError("%s: out %s is not (%d, n, 4) on %s" % (name, tuple(out.shape), w, dev))
    if status.dtype != torch.int32 or status.device != dev or status.numel() < 1:
        raise _lib.AdyoloHipError("%s: status must be an int32 word on %s" % (name, dev))
    return w


def corpus_gather_windows(pcm, windows, out, status):
    """pcm int16 (S, 4) and windows int64 (W, 8) on the device -> out (W, n, 4) float32: each window's ``valid`` int16 frames
    from its offset as ``x / 32768 + 1e-8``, the rest of the window the conversion of int16 zero, not read from pcm
    (adyolo_hip.h ``adyolo_corpus_gather_windows``).  An odd or negative offset, or a window past the stream: zeros for it and
    status bit 2.  out may be a recorded graph's static input.  No allocation, no sync."""
    w = _gather_windows_args("corpus_gather_windows", pcm, windows, out, status)
    _c("adyolo_corpus_gather_windows", _p(pcm), pcm.shape[0], _p(windows), w, out.shape[1], _p(out), _p(status), _stream())
    return out


def corpus_gather_windows_view(pcm, windows, comb, rot, out, status, *, mic_src=None):
    """``corpus_gather_windows`` under ONE combination ``comb`` for all windows (rotation test-time augmentation through
    windows; adyolo_hip.h ``adyolo_corpus_gather_windows_view``): FOA-rotated (rot: ``corpus_rot_table``) -- bit for bit the
    plain window gather then ``augmentations.rotate_audio``, the padding past ``valid`` turned too -- or with ``mic_src``
    (``corpus_mic_table``; rot may be None) the four capsules permuted -- bit for bit the plain gather then ``swap_audio``; a
    combination that is no symmetry: zeros and status bit 2.  comb <= 0: the bits of ``corpus_gather_windows``; comb >= 16
    raises.  Bad windows as in the plain gather.  No allocation, no sync."""
    name = "corpus_gather_windows_view"
    w = _gather_windows_args(name, pcm, windows, out, status)
    if mic_src is None and rot is None:
        raise _lib.AdyoloHipError("%s: the FOA form needs the rotation table" % name)
    _c("adyolo_corpus_gather_windows_view", _p(pcm), pcm.shape[0], _p(windows), w, out.shape[1], int(comb), _host_table(rot),
       _host_table(mic_src), _p(out), _p(status), _stream())
    return out


def stream_gather_windows(ring, head, windows, out, status, *, comb=0, rot=None, mic_src=None):
    """ring int16 (capacity, 4) on the device, absolute sample s of a live stream at ``ring[s % capacity]``, ``head`` samples
    pushed so far; windows int64 (W, 8) with ABSOLUTE sample offsets -> out (W, n, 4) float32: the bits of
    ``corpus_gather_windows`` (comb <= 0) or ``corpus_gather_windows_view`` (comb > 0: rot / mic_src as there) on the stream
    laid out linearly (adyolo_hip.h ``adyolo_stream_gather_windows``).  A window that is odd, not pushed yet (offset + valid >
    head) or already overwritten (offset < head - capacity): zeros and status bit 2.  capacity odd or < n, comb >= 16: raises.
    No allocation, no sync."""
    name = "stream_gather_windows"
    w = _gather_windows_args(name, ring, windows, out, status)
    if int(comb) > 0 and mic_src is None and rot is None:
        raise _lib.AdyoloHipError("%s: the FOA form needs the rotation table" % name)
    _c("adyolo_stream_gather_windows", _p(ring), ring.shape[0], int(head), _p(windows), w, out.shape[1], int(comb),
       _host_table(rot), _host_table(mic_src), _p(out), _p(status), _stream())
    return out


def decode_stitch(decoded, windows, window_frames, pass_base, out, status):
    """decoded (W * window_frames, ...) float32 (``LabelPostProcessor.decode_device`` of a pass of W windows) and windows int64
    (W, 8) on the device -> out (capacity, ...) float32 with the same trailing shape: window w's frames [src_lo, src_lo + n)
    copied to out[dst - pass_base ...], the kept frames of the pass as one run in window order (adyolo_hip.h
    ``adyolo_decode_stitch``).  A window whose frames are outside its own window or outside out is skipped and sets status
    bit 2.  No allocation, no sync."""
    _chk(decoded, out)
    dev = decoded.device
    w = _window_table("decode_stitch", windows, dev)
    wf = int(window_frames)
    if wf < 1 or decoded.dim() < 2 or decoded.shape[0] != w * wf:
        raise _lib.AdyoloHipError("decode_stitch: decoded %s is not (%d * %d, ...)" % (tuple(decoded.shape), w, wf))
    if out.dim() != decoded.dim() or out.shape[0] < 1 or tuple(out.shape[1:]) != tuple(decoded.shape[1:]) or out.device != dev:
        raise _lib.AdyoloHipError("decode_stitch: out %s does not hold frames of %s on %s"
                                  % (tuple(out.shape), tuple(decoded.shape[1:]), dev))
    if status.dtype != torch.int32 or status.device != dev or status.numel() < 1:
        raise _lib.AdyoloHipError("decode_stitch: status must be an int32 word on %s" % dev)
    rec = decoded.numel() // decoded.shape[0]
    _c("adyolo_decode_stitch", _p(decoded), _p(windows), w, wf, rec, int(pass_base), _p(out), out.shape[0], _p(status), _stream())
    return out


RESAMPLE_WORDS = 4                                        # ADYOLO_RESAMPLE_WORDS: {src offset, src frames, dst offset, dst frames}
RESAMPLE_TILE = 256                                       # ADYOLO_RESAMPLE_TILE: output frames per workgroup pass
RESAMPLE_KINDS = {torch.int16: 0, torch.int32: 1, torch.float32: 2}     # ADYOLO_RESAMPLE_INT16 / _INT32 / _FLOAT32


def resample_pcm(src, recs, taps, m, centre, dst, status):
    """src int16 / int32 (24-bit PCM left-justified) / float32 (S, 4), recs int64 (R, 4) {src offset, src frames, dst offset, dst
    frames} and taps int32 (L, K) (``resample.plan``) on the device -> dst int16 (D, 4): every row's recording converted by L / m
    into its place, bit for bit the integer polyphase filter of adyolo_hip.h ``adyolo_resample_pcm``; nothing outside the rows'
    destinations is written.  A row outside either stream, or whose dst frames are not (src frames * L + m - 1) // m: not
    written, status bit 2; a non-finite float sample: taken as 0, status bit 8.  No allocation, no sync."""
    dev = src.device
    if not src.is_cuda or src.dtype not in RESAMPLE_KINDS or not src.is_contiguous() or src.dim() != 2 or src.shape[1] != 4:
        raise _lib.AdyoloHipError("resample_pcm: src must be a contiguous int16, int32 or float32 tensor (S, 4) on the device")
    _corpus_i64("resample_pcm: recs", recs, dev)
    if recs.dim() != 2 or recs.shape[0] < 1 or recs.shape[1] != RESAMPLE_WORDS:
        raise _lib.AdyoloHipError("resample_pcm: recs %s are not (R, %d)" % (tuple(recs.shape), RESAMPLE_WORDS))
    if taps.dtype != torch.int32 or taps.device != dev or not taps.is_contiguous() or taps.dim() != 2 or taps.numel() < 1:
        raise _lib.AdyoloHipError("resample_pcm: taps must be a contiguous int32 tensor (L, K) on %s" % dev)
    if dst.dtype != torch.int16 or dst.device != dev or not dst.is_contiguous() or dst.dim() != 2 or dst.shape[1] != 4:
        raise _lib.AdyoloHipError("resample_pcm: dst must be a contiguous int16 tensor (D, 4) on %s" % dev)
    if status.dtype != torch.int32 or status.device != dev or status.numel() < 1:
        raise _lib.AdyoloHipError("resample_pcm: status must be an int32 word on %s" % dev)
    if int(m) < 1 or int(centre) < 0:
        raise _lib.AdyoloHipError("resample_pcm: M %r, centre %r" % (m, centre))
    _c("adyolo_resample_pcm", _p(src), RESAMPLE_KINDS[src.dtype], src.shape[0], _p(recs), recs.shape[0], _p(taps), taps.numel(),
       taps.shape[0], int(m), taps.shape[1], int(centre), _p(dst), dst.shape[0], _p(status), _stream())
    return dst


def corpus_status_check(word):
    """Raise ``AdyoloHipError`` for the ADYOLO_CORPUS_* bits of a status word already read to the host."""
    word = int(word)
    if word:
        raise _lib.AdyoloHipError("adyolo corpus batch failed (status 0x%x): %s"
                                  % (word, "; ".join(msg for bit, msg in CORPUS_STATUS if word & bit)))


def mask_ranges_(feat, ranges):
    """In-place SpecAug masking of feat [B][T][F][C]: ranges int32 [B][4] = {t0, t1, f0, f1} per sample."""
    _chk(feat)
    if ranges.dtype != torch.int32 or not ranges.is_cuda or not ranges.is_contiguous():
        raise _lib.AdyoloHipError("mask_ranges_ needs contiguous int32 ranges on the device")
    b, t, f, c = feat.shape
    _c("adyolo_mask_ranges", _p(feat), _p(ranges), b, t, f, c, _stream())
    return feat


def mask_groups_(feat, ranges, group_quads):
    """In-place SpecAug masking of feat [B][T][F][C] per channel group: ranges int32 [B][G][4] = {t0, t1, f0, f1} on the device
    (clamped to the tensor by the kernel), group_quads G pairs (q0, q1) of float4 quads (channels 4 q0 .. 4 q1 - 1)."""
    _chk(feat)
    if feat.dim() != 4 or feat.shape[3] % 4 != 0:
        raise _lib.AdyoloHipError("mask_groups_ needs feat (B, T, F, C) with C %% 4 == 0 (got %s)" % (tuple(feat.shape),))
    b, t, f, c = feat.shape
    gq = [(int(q0), int(q1)) for q0, q1 in group_quads]
    g = len(gq)
    if ranges.dtype != torch.int32 or not ranges.is_contiguous() or ranges.device != feat.device:
        raise _lib.AdyoloHipError("mask_groups_ needs contiguous int32 ranges on the device of feat")
    if tuple(ranges.shape) != (b, g, 4):
        raise _lib.AdyoloHipError("mask_groups_: ranges must be (%d, %d, 4) (got %s)" % (b, g, tuple(ranges.shape)))
    if not 0 < g <= 8 or any(not 0 <= q0 <= q1 <= c // 4 for q0, q1 in gq):
        raise _lib.AdyoloHipError("mask_groups_: 1..8 groups of quads within [0, %d] (got %s)" % (c // 4, gq))
    quads = (ctypes.c_int32 * (2 * g))(*[q for pair in gq for q in pair])
    _c("adyolo_mask_groups", _p(feat), _p(ranges), b, g, t, f, c, ctypes.cast(quads, ctypes.c_void_p), _stream())
    return feat


def feat_augment_(feat, table, group_quads, shift_groups):
    """In-place frequency shift + SpecAug stripes + cutout of feat [B][T][64][C] in one launch (``adyolo_feat_augment``; the
    definition is ``augmentations.apply_feature_aug_host``).  table int32 [B][G + 2][4] on the device: rows 0..G-1 the SpecAug
    ranges of ``mask_groups_``, row G the cutout rectangle {t0, t1, f0, f1} over all channels, row G + 1 = {shift, 0, 0, 0}
    (every value clamped by the kernel); group_quads G pairs (q0, q1) of float4 quads; shift_groups one bool per group (the
    groups whose bin axis moves)."""
    _chk(feat)
    if feat.dim() != 4 or feat.shape[3] % 4 != 0:
        raise _lib.AdyoloHipError("feat_augment_ needs feat (B, T, F, C) with C %% 4 == 0 (got %s)" % (tuple(feat.shape),))
    b, t, f, c = feat.shape
    gq = [(int(q0), int(q1)) for q0, q1 in group_quads]
    g = len(gq)
    if table.dtype != torch.int32 or not table.is_contiguous() or table.device != feat.device:
        raise _lib.AdyoloHipError("feat_augment_ needs a contiguous int32 table on the device of feat")
    if tuple(table.shape) != (b, g + 2, 4):
        raise _lib.AdyoloHipError("feat_augment_: table must be (%d, %d, 4) (got %s)" % (b, g + 2, tuple(table.shape)))
    if not 0 < g <= 8 or any(not 0 <= q0 <= q1 <= c // 4 for q0, q1 in gq):
        raise _lib.AdyoloHipError("feat_augment_: 1..8 groups of quads within [0, %d] (got %s)" % (c // 4, gq))
    shift = [bool(s) for s in shift_groups]
    if len(shift) != g:
        raise _lib.AdyoloHipError("feat_augment_: shift_groups must have one entry per group (%d; got %d)" % (g, len(shift)))
    quads = (ctypes.c_int32 * (2 * g))(*[q for pair in gq for q in pair])
    _c("adyolo_feat_augment", _p(feat), _p(table), b, g, t, f, c, ctypes.cast(quads, ctypes.c_void_p),
       sum(1 << i for i, s in enumerate(shift) if s), _stream())
    return feat


def colstats(a2d):
    """[rows][cols] fp32 -> float64 [4][cols]: column sum, sum of squares, max, min."""
    _chk(a2d)
    rows, cols = a2d.shape
    out = torch.empty((4, cols), dtype=torch.float64, device=a2d.device)
    partial = _new(a2d, 4, 1024, cols)
    _c("adyolo_colstats", _p(a2d), _p(partial), _p(out), rows, cols, _stream())
    return out
