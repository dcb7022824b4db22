"""GPU tests of the sequence stage (run with ``-m gpu`` on an MI355X): self-attention pooling, the BiGRU recurrence and
its backward, the whole BiGRU layer, LayerNorm (+ tanh) and the head / long-contraction GEMMs, each against a float64
reference on the CPU at the shapes where the kernels change path: several 16-step GRU chunks (exact multiples, one step
over, the reverse direction crossing a boundary), backward reductions whose workgroups loop over many rows (R up to the
bench's 64 x 600 = 38400), saturated softmax / sigmoid / tanh, LayerNorm rows far from zero mean.

Every error is max |kernel - float64| / max |float64| over the checked tensor; each bar is at most 4x the worst error
measured on an MI355X (written next to it) and never looser than the bars of test_gpu_kernels.py for the same kernel."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import seresnet as onet

pytestmark = pytest.mark.gpu

H = 128
GRU_BOUND = 1.0 / math.sqrt(H)          # nn.GRU's init (GRUParams): U(-1/sqrt(H), 1/sqrt(H)) for every weight and bias
BENCH_B, BENCH_T = 64, 600              # bench.py: 64 clips x 60 s -> 600 sequence steps
BENCH_R = BENCH_B * BENCH_T
BENCH_PICK = [0, 37, BENCH_B - 1]       # samples checked against float64 at the bench shape (first, a middle one, last)
GRU_SHAPES = [(b, t) for t in (1, 2, 15, 16, 17, 31, 32, 33, 47, 200) for b in (1, 3)] + [(BENCH_B, BENCH_T)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


def dev(t):
    return t.to("cuda:0").contiguous()


class Err:
    """Running max |got - ref| and max |ref| over chunks of one tensor (got: kernel output, ref: float64)."""

    def __init__(self):
        self.err = 0.0
        self.scale = 0.0

    def add(self, got, ref):
        got = got.detach().cpu().double()
        ref = ref.detach().cpu().double()
        assert got.shape == ref.shape, "shape %s vs %s" % (tuple(got.shape), tuple(ref.shape))
        if got.numel() == 0:
            return self
        self.err = max(self.err, float((got - ref).abs().max()))
        if not bool(torch.isfinite(got).all()):
            self.err = float("inf")
        self.scale = max(self.scale, float(ref.abs().max()))
        return self

    @property
    def rel(self):
        return self.err / self.scale if self.scale > 0 else self.err


def check(what, got, ref, bar):
    """got / ref: tensors, or an Err already filled."""
    e = got if isinstance(got, Err) else Err().add(got, ref)
    print("%-40s rel err %.3e (bar %.1e, float64 absmax %.3e)" % (what, e.rel, bar, e.scale))
    assert np.isfinite(e.rel) and e.rel <= bar, "%s: rel err %.3e > %.1e (float64 absmax %.3e)" % (what, e.rel, bar, e.scale)


# ---------------------------------------------------------------------------------------------------------- GRU
def gru_inputs(b, t, seed):
    """gx [B][T][2][384] = x W_ih^T + b_ih with x ~ N(0, 1) and the model's init, W_hh [2][384][128], b_hh [2][384]:
    fp32, the values the kernels see (the float64 references start from the same fp32 numbers)."""
    g = torch.Generator().manual_seed(seed)

    def u(*s):
        return (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * GRU_BOUND
    x = torch.randn(b, t, 256, generator=g, dtype=torch.float64)
    wih, bih = u(2, 3 * H, 256), u(2, 3 * H)
    gx = torch.einsum("btc,dgc->btdg", x, wih) + bih
    return gx.float(), u(2, 3 * H, H).float(), u(2, 3 * H).float()


def gru_ref(gx, whh, bhh, pick, dout=None):
    """float64 recurrence of samples ``pick``, per direction: the dict of ``onet.gru_gate_steps`` (time order); with ``dout``
    also "dgx" = d/d(gx) = (dr_pre, dz_pre, dn_pre) and "dgh" = d/d(h_prev W_hh^T + b_hh) = (dr_pre, dz_pre, dhn)."""
    res = []
    for d in (0, 1):
        gxd = gx[pick, :, d].double().requires_grad_(dout is not None)
        with torch.set_grad_enabled(dout is not None):
            # (W_hh / b_hh require grad so that the first step's pre-activations, from h = 0, are in the graph too)
            whd, bhd = (v[d].double().requires_grad_(dout is not None) for v in (whh, bhh))
            st = onet.gru_gate_steps(gxd, whd, bhd, reverse=bool(d))
            if dout is not None:
                for gh in st["gh"]:
                    gh.retain_grad()
                (st["h"] * dout[pick][..., d * H:(d + 1) * H].double()).sum().backward()
                dgh = torch.stack([gh.grad for gh in st["gh"]], dim=1)        # step order
                st["dgh"] = dgh.flip(1) if d else dgh
                st["dgx"] = gxd.grad
        res.append({k: (v.detach() if torch.is_tensor(v) else v) for k, v in st.items()})
    return res


def pick_of(b):
    return BENCH_PICK if b == BENCH_B else list(range(b))


@pytest.mark.parametrize("b,t", GRU_SHAPES)
def test_gru_fwd_matches_float64(ops, b, t):
    gx, whh, bhh = gru_inputs(b, t, 1000 + 7 * t + b)
    out, gates, hprev = ops.gru_fwd(dev(gx), dev(whh), dev(bhh), True)
    out_nosave, _, _ = ops.gru_fwd(dev(gx), dev(whh), dev(bhh), False)
    torch.cuda.synchronize()
    assert torch.equal(out, out_nosave), "gru_fwd: save=False changes out"
    pick = pick_of(b)
    ref = gru_ref(gx, whh, bhh, pick)
    out, gates, hprev = out.cpu()[pick], gates.cpu()[pick], hprev.cpu()[pick]
    e = {k: Err() for k in ("out", "r", "z", "n", "hn", "hprev")}
    for d in (0, 1):
        e["out"].add(out[..., d * H:(d + 1) * H], ref[d]["h"])
        for i, k in enumerate(("r", "z", "n", "hn")):
            e[k].add(gates[:, :, d, i], ref[d][k])
        e["hprev"].add(hprev[:, :, d], ref[d]["hprev"])
        first = t - 1 if d else 0
        assert torch.equal(hprev[:, first, d], torch.zeros(len(pick), H)), "hprev at the first step of direction %d" % d
    # measured worst over the shapes: out 2.4e-7 (B=64 T=600), r 9.7e-8, z 9.6e-8, n 2.0e-7, hn 2.1e-7, hprev 2.4e-7
    bars = {"out": 8e-7, "r": 3e-7, "z": 3e-7, "n": 8e-7, "hn": 8e-7, "hprev": 8e-7}
    for k in ("out", "r", "z", "n", "hn", "hprev"):
        check("gru fwd (B=%d T=%d) %s" % (b, t, k), e[k], None, bars[k])


@pytest.mark.parametrize("k", [0, 15, 16, 20, 32, 46])
def test_gru_fwd_one_step_changes_only_what_it_reaches(ops, k):
    """A change of gx at (sample 1, time k) reaches the forward half at t >= k and the reverse half at t <= k of sample 1
    only: everything else is bit-identical."""
    b, t = 3, 47
    gx, whh, bhh = gru_inputs(b, t, 77)
    gx2 = gx.clone()
    gx2[1, k] += 0.5
    o1, _, _ = ops.gru_fwd(dev(gx), dev(whh), dev(bhh), True)
    o2, _, _ = ops.gru_fwd(dev(gx2), dev(whh), dev(bhh), True)
    o1, o2 = o1.cpu(), o2.cpu()
    assert torch.equal(o1[0], o2[0]) and torch.equal(o1[2], o2[2]), "another sample changed"
    assert torch.equal(o1[1, :k, :H], o2[1, :k, :H]), "forward half changed before the perturbed step"
    assert torch.equal(o1[1, k + 1:, H:], o2[1, k + 1:, H:]), "reverse half changed after the perturbed step"
    assert not torch.equal(o1[1, k, :H], o2[1, k, :H]) and not torch.equal(o1[1, k, H:], o2[1, k, H:])


@pytest.mark.parametrize("amp", [30.0, 90.0])
def test_gru_fwd_saturated_gates(ops, amp):
    """Pre-activations up to +-amp: exp overflows to inf / underflows to 0 inside the fast sigmoid / tanh."""
    b, t = 3, 40
    gx, whh, bhh = gru_inputs(b, t, 5)
    gx = (gx * (amp / float(gx.abs().max()))).float()
    out, gates, _ = ops.gru_fwd(dev(gx), dev(whh), dev(bhh), True)
    out, gates = out.cpu(), gates.cpu()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gates).all())
    ref = gru_ref(gx, whh, bhh, list(range(b)))
    e, eg = Err(), Err()
    for d in (0, 1):
        e.add(out[..., d * H:(d + 1) * H], ref[d]["h"])
        for i, k in enumerate(("r", "z", "n", "hn")):
            eg.add(gates[:, :, d, i], ref[d][k])
    check("gru fwd saturated out (amp %g)" % amp, e, None, 1.2e-6)          # measured 4.0e-7 (amp 30)
    check("gru fwd saturated gates (amp %g)" % amp, eg, None, 5e-7)         # measured 1.5e-7 (amp 30)


@pytest.mark.parametrize("b,t", GRU_SHAPES)
def test_gru_bwd_matches_float64(ops, b, t):
    gx, whh, bhh = gru_inputs(b, t, 2000 + 7 * t + b)
    dout = torch.randn(b, t, 2 * H, generator=torch.Generator().manual_seed(t + b))
    pick = pick_of(b)
    ref = gru_ref(gx, whh, bhh, pick, dout)
    whh_d, dout_d = dev(whh), dev(dout)
    # (a) the model's path: the kernel's own saved forward tensors
    _, gates, hprev = ops.gru_fwd(dev(gx), whh_d, dev(bhh), True)
    dgx_a, dgh_a = ops.gru_bwd(dout_d, gates, hprev, whh_d)
    # (b) the float64 forward quantities rounded to fp32 (samples `pick`): the backward kernel alone
    gates_b, hprev_b = gates.clone(), hprev.clone()
    for d in (0, 1):
        gates_b[pick, :, d] = dev(torch.stack([ref[d][k] for k in ("r", "z", "n", "hn")], dim=2).float())
        hprev_b[pick, :, d] = dev(ref[d]["hprev"].float())
    dgx_b, dgh_b = ops.gru_bwd(dout_d, gates_b, hprev_b, whh_d)
    torch.cuda.synchronize()
    # measured worst over the shapes: own fwd dgx 2.2e-7, dgh 2.6e-7; float64 fwd dgx 1.8e-7, dgh 1.8e-7
    for tag, dgx, dgh, bar in (("own fwd", dgx_a, dgh_a, 8e-7), ("float64 fwd", dgx_b, dgh_b, 6e-7)):
        dgx, dgh = dgx.cpu()[pick], dgh.cpu()[pick]
        ex, eh = Err(), Err()
        for d in (0, 1):
            ex.add(dgx[:, :, d], ref[d]["dgx"])
            eh.add(dgh[:, :, d], ref[d]["dgh"])
        check("gru bwd (B=%d T=%d) dgx, %s" % (b, t, tag), ex, None, bar)
        check("gru bwd (B=%d T=%d) dgh, %s" % (b, t, tag), eh, None, bar)


GRU_NAMES = ["weight_ih", "weight_hh", "bias_ih", "bias_hh"]


@pytest.mark.parametrize("b,t", [(2, 200), (BENCH_B, BENCH_T)])
def test_bigru_layer_matches_float64_nn_gru(ops, b, t):
    """BiGRULayerFn (input GEMMs, both recurrence kernels, split-K weight-gradient GEMMs, colsum biases, accumulated dx)
    against float64 nn.GRU autograd."""
    from adyolo_amd import functional as Fn
    rows = b * t
    if b == BENCH_B:      # the split-K weight-gradient path must stay exercised here
        assert ops.wgrad_splits(384, 256, rows) > 1 and ops.wgrad_splits(384, 128, rows) > 1
    g = torch.Generator().manual_seed(rows)
    gru = torch.nn.GRU(256, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for p in gru.parameters():
            p.copy_(((torch.rand(p.shape, generator=g, dtype=torch.float64) * 2 - 1) * GRU_BOUND).float())
    x = torch.randn(b, t, 256, generator=g)
    probe = torch.randn(b, t, 2 * H, generator=g)
    x64 = x.double().requires_grad_(True)
    y64, _ = gru(x64)
    (y64 * probe.double()).sum().backward()
    names = ["%s_l0%s" % (n, s) for s in ("", "_reverse") for n in GRU_NAMES]
    prm = [dev(getattr(gru, n).detach().float()).requires_grad_(True) for n in names]
    xg = dev(x).requires_grad_(True)
    yg = Fn.BiGRULayerFn.apply(xg, *prm, True)
    (yg * dev(probe)).sum().backward()
    torch.cuda.synchronize()
    nm = "bigru layer (B=%d T=%d) " % (b, t)
    check(nm + "out", yg, y64, 4e-6)                   # measured 1.3e-6 (B=64 T=600)
    check(nm + "dx", xg.grad, x64.grad, 2e-6)          # measured 5.6e-7 (B=64 T=600)
    # measured worst: weights 7.3e-7 .. 1.08e-6 (B=2 T=200), biases 2.0e-7 .. 2.6e-7 (B=64 T=600)
    for n, p in zip(names, prm):
        check(nm + "d" + n, p.grad, getattr(gru, n).grad, 2.5e-6 if n.startswith("weight") else 8e-7)


# ---------------------------------------------------------------------------------------------------------- SAP
SAP_R = [1, 3, 5, 4097, BENCH_R]
CHUNK = 4096            # rows per float64 reference chunk


def sap_inputs(r, f, seed):
    """x [R][F][256] ~ N(0, 1), w ~ nn.Linear(256, 1)'s init, and (R >= 3) saturated rows: logits from -5 to 95 (a spread of
    100; exp(95) overflows fp32, so only the max subtraction keeps the softmax finite)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(r, f, 256, generator=g)
    w = (torch.rand(256, generator=g) * 2 - 1) / 16
    b = torch.randn(1, generator=g) * 0.1
    w64 = w.double()
    sat = [] if r < 3 else sorted({r // 2, r - 1})
    for row in sat:
        c = torch.linspace(-5.0, 95.0, f, dtype=torch.float64)[torch.randperm(f, generator=g)] - float(b)
        xr = x[row].double()
        x[row] = (xr + (c - xr @ w64)[:, None] * w64[None, :] / float(w64 @ w64)).float()
    return x, w, b, sat


def sap_bwd_ref(x, attn, w, dy):
    """float64 SAP backward for the given weights ``attn`` [R][F] (the softmax of the forward pass, or any weights):
    dl_f = a_f (da_f - sum_g a_g da_g), da_f = x_f . dy -> dx, dW = sum dl x, db = sum dl, and sum |dl|."""
    x, attn, dy, w = x.double(), attn.double(), dy.double(), w.double()
    da = torch.einsum("rfc,rc->rf", x, dy)
    dl = attn * (da - (attn * da).sum(-1, keepdim=True))
    dx = attn[..., None] * dy[:, None, :] + dl[..., None] * w
    return dx, torch.einsum("rf,rfc->c", dl, x), dl.sum().view(1), float(dl.abs().sum())


@pytest.mark.parametrize("r", SAP_R)
@pytest.mark.parametrize("f", [4, 8, 16])
def test_sap_matches_float64(ops, f, r):
    x, w, b, sat = sap_inputs(r, f, 300 + f + r)
    dy = torch.randn(r, 256, generator=torch.Generator().manual_seed(r))
    xg, wg, bg = dev(x), dev(w), dev(b)
    y, attn = ops.sap_fwd(xg, wg, bg)
    dx, dw, db = ops.sap_bwd(dev(dy), xg, wg, attn)
    torch.cuda.synchronize()
    y, attn, dx, dw, db = y.cpu(), attn.cpu(), dx.cpu(), dw.cpu(), db.cpu()
    del xg
    plain = torch.ones(r, dtype=torch.bool)
    plain[sat] = False
    # float64 autograd through the oracle, chunk by chunk (dW / db accumulate in w64.grad / b64.grad)
    w64 = w.double().view(1, 256).requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    sd = {"attention.W.weight": w64, "attention.W.bias": b64}
    e = {k: Err() for k in ("y", "y sat", "attn", "dx", "dx sat")}
    l1 = 0.0
    for s in range(0, r, CHUNK):
        sl, pl = slice(s, s + CHUNK), plain[s:s + CHUNK]
        xc = x[sl].double().requires_grad_(True)
        yr = onet.self_attention_pooling(sd, xc.unsqueeze(0)).squeeze(0)
        (yr * dy[sl].double()).sum().backward()
        with torch.no_grad():
            ar = torch.softmax(F.linear(xc, w64, b64).squeeze(-1), dim=-1)
        l1 += sap_bwd_ref(x[sl], ar, w, dy[sl])[3]
        e["attn"].add(attn[sl], ar)
        e["y"].add(y[sl][pl], yr.detach()[pl])
        e["dx"].add(dx[sl][pl], xc.grad[pl])
        if not bool(pl.all()):       # saturated rows: y ~ one x row (|x| ~ 20) -- checked on their own scale
            e["y sat"].add(y[sl][~pl], yr.detach()[~pl])
            e["dx sat"].add(dx[sl][~pl], xc.grad[~pl])
    for row in sat:                  # saturated for real: one weight ~1, the smallest underflows
        assert float(attn[row].max()) > 0.99 and float(attn[row].min()) < 1e-30
    nm = "sap (F=%d R=%d) " % (f, r)
    check(nm + "y", e["y"], None, 8e-7)                          # measured 2.6e-7 (F=16 R=4097)
    check(nm + "attn", e["attn"], None, 4e-7)                    # measured 1.1e-7 (F=4 R=38400)
    check(nm + "dx", e["dx"], None, 8e-7)                        # measured 2.2e-7 (F=16 R=38400)
    if sat:
        check(nm + "y saturated rows", e["y sat"], None, 8e-7)   # measured 2.2e-7 (F=16 R=38400)
        check(nm + "dx saturated rows", e["dx sat"], None, 1.5e-6)   # measured 4.5e-7 (F=16 R=38400)
    check(nm + "dW", dw, w64.grad.view(-1), 6e-5)                # measured 1.9e-5 (F=16 R=3: saturated rows, cancellation)
    # the bias gradient is 0 exactly (softmax is shift-invariant): what is left is rounding, measured against sum |dl|
    db_err = abs(float(db) - float(b64.grad)) / l1
    print("%-40s err / sum|dl| %.3e (bar 4e-6)" % (nm + "db", db_err))
    assert db_err <= 4e-6                                        # measured 1.3e-6 (F=16 R=3)


@pytest.mark.parametrize("r", [5, 4097, BENCH_R])
def test_sap_bwd_reduces_db_for_any_weights(ops, r):
    """db = sum of dl over all rows and positions.  With softmax weights that sum is 0, so the db reduction is only
    observable with weights that do not sum to one: sap_bwd is linear in the dl it forms from the weights it is given."""
    f = 4
    x, w, b, _ = sap_inputs(r, f, 500 + r)
    g = torch.Generator().manual_seed(r + 2)
    attn = torch.rand(r, f, generator=g)
    dy = torch.randn(r, 256, generator=g)
    xg, wg = dev(x), dev(w)
    dx, dw, db = ops.sap_bwd(dev(dy), xg, wg, dev(attn))
    torch.cuda.synchronize()
    dxr, dwr, dbr, _ = sap_bwd_ref(x, attn, w, dy)
    check("sap bwd, any weights (R=%d) dx" % r, dx, dxr, 8e-7)   # measured 2.6e-7 (R=38400)
    check("sap bwd, any weights (R=%d) dW" % r, dw, dwr, 8e-7)   # measured 2.4e-7 (R=5)
    check("sap bwd, any weights (R=%d) db" % r, db, dbr, 8e-7)   # measured 2.2e-7 (R=5)


def test_sap_bwd_adds_into_the_given_accumulators(ops):
    """out_dw / out_db (GradSink: the parameters' slices of the flat gradient buffer) receive acc + gradient."""
    x, w, b, _ = sap_inputs(4097, 4, 9)
    xg, wg = dev(x), dev(w)
    g = torch.Generator().manual_seed(3)
    dyg = dev(torch.randn(4097, 256, generator=g))
    attn = dev(torch.rand(4097, 4, generator=g))          # weights that do not sum to one: db is not 0
    _, dw, db = ops.sap_bwd(dyg, xg, wg, attn)
    acc_w = dev(torch.randn(256, generator=g))
    acc_b = dev(torch.randn(1, generator=g))
    want_w, want_b = acc_w + dw, acc_b + db
    _, dw2, db2 = ops.sap_bwd(dyg, xg, wg, attn, out_dw=acc_w, out_db=acc_b)
    torch.cuda.synchronize()
    assert float(db.abs()) > 0.0
    assert dw2.data_ptr() == acc_w.data_ptr() and db2.data_ptr() == acc_b.data_ptr()
    assert torch.equal(acc_w, want_w) and torch.equal(acc_b, want_b)


# ---------------------------------------------------------------------------------------------------- LayerNorm
LN_R = [1, 3, 4, 5, 4097, BENCH_R]
EPS = 1e-5


def ln_inputs(r, seed):
    """x [R][256]; special rows: mean 1e3 / std 1e-2 ("offset"), constant (var = 0), one spike (x_hat ~ 16, tanh saturated
    with |gamma| up to 3), mean 3 / 5 std."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(r, 256, generator=g) * 2 + 0.5
    sign = torch.where(torch.rand(256, generator=g) < 0.5, -1.0, 1.0)
    gamma = sign * (0.5 + 2.5 * torch.rand(256, generator=g))
    beta = torch.randn(256, generator=g) * 0.5
    special = {r - 1: "offset"}
    if r >= 3:
        special[r // 2] = "const"
    if r >= 4:
        special[r // 3] = "spike"
    if r >= 4097:
        special[1] = "offset"
        special[r - 2] = "const"
        special[2] = "mean 3 std"          # either side of the kernel's |mean| > 4 std switch to corrected centring
        special[3] = "mean 5 std"
    for row, kind in special.items():
        if kind == "offset":
            x[row] = 1e3 + 1e-2 * torch.randn(256, generator=g)
        elif kind.startswith("mean"):
            z = torch.randn(256, generator=g, dtype=torch.float64)
            z = (z - z.mean()) / z.std(unbiased=False)
            x[row] = (float(kind.split()[1]) + z).float()
        elif kind == "const":
            x[row] = 0.75
        else:
            x[row] = 0.0
            x[row, int(torch.randint(256, (1,), generator=g))] = 40.0
    return x, gamma, beta, sorted(special)


def ln_ref(x, gamma, beta, dy, tanh):
    x64 = x.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True)
    b64 = beta.double().requires_grad_(True)
    y = F.layer_norm(x64, (256,), g64, b64, EPS)
    if tanh:
        y = torch.tanh(y)
    (y * dy.double()).sum().backward()
    return y.detach(), x64.grad, g64.grad, b64.grad


@pytest.mark.parametrize("r", LN_R)
@pytest.mark.parametrize("tanh", [True, False])
def test_layernorm_matches_float64(ops, tanh, r):
    x, gamma, beta, special = ln_inputs(r, 400 + r)
    dy = torch.randn(r, 256, generator=torch.Generator().manual_seed(r + 1))
    xg, gg, bg, dyg = dev(x), dev(gamma), dev(beta), dev(dy)
    if tanh:
        y = ops.ln_tanh_fwd(xg, gg, bg, EPS)
        dx, dgamma, dbeta = ops.ln_tanh_bwd(dyg, xg, y, gg, EPS)
    else:
        y = ops.ln_fwd(xg, gg, bg, EPS)
        dx, dgamma, dbeta = ops.ln_bwd(dyg, xg, gg, EPS)
    torch.cuda.synchronize()
    yr, dxr, dgr, dbr = ln_ref(x, gamma, beta, dy, tanh)
    y, dx = y.cpu(), dx.cpu()
    plain = torch.ones(r, dtype=torch.bool)
    plain[special] = False
    nm = "ln%s (R=%d) " % ("+tanh" if tanh else "", r)
    # measured worst over R, LN + tanh / plain LN: y 3.3e-7 / 1.5e-7, dx 1.8e-7 / 1.5e-7, special rows y 1.6e-7 / 1.0e-7,
    # dx 1.7e-7 / 1.2e-7, dgamma 1.7e-7 / 1.2e-7, dbeta 1.2e-7 / 8.9e-8.  (Before the corrected two-pass centring, the
    # rows of mean 1e3 and std 1e-2 had y off by up to 1.7e-2 / 2.6e-3.)
    bars = {"y": 1e-6, "dx": 6e-7, "y row": 5e-7, "dx row": 6e-7, "dgamma": 6e-7, "dbeta": 4e-7} if tanh else \
        {"y": 5e-7, "dx": 5e-7, "y row": 3.5e-7, "dx row": 4e-7, "dgamma": 4e-7, "dbeta": 3e-7}
    if bool(plain.any()):
        check(nm + "y", y[plain], yr[plain], bars["y"])
        check(nm + "dx", dx[plain], dxr[plain], bars["dx"])
    # offset / constant / spike rows on their own scale (dx ~ 1/std of the row: up to 1/sqrt(eps) ~ 316)
    for row in special:
        check(nm + "y row %d" % row, y[row], yr[row], bars["y row"])
        check(nm + "dx row %d" % row, dx[row], dxr[row], bars["dx row"])
    check(nm + "dgamma", dgamma, dgr, bars["dgamma"])
    check(nm + "dbeta", dbeta, dbr, bars["dbeta"])


@pytest.mark.parametrize("tanh", [True, False])
def test_layernorm_bwd_adds_into_the_given_accumulators(ops, tanh):
    x, gamma, beta, _ = ln_inputs(4097, 8)
    xg, gg, bg = dev(x), dev(gamma), dev(beta)
    dyg = dev(torch.randn(4097, 256, generator=torch.Generator().manual_seed(6)))
    acc_g = dev(torch.randn(256, generator=torch.Generator().manual_seed(7)))
    acc_b = dev(torch.randn(256, generator=torch.Generator().manual_seed(8)))
    if tanh:
        y = ops.ln_tanh_fwd(xg, gg, bg, EPS)
        _, dg, db = ops.ln_tanh_bwd(dyg, xg, y, gg, EPS)
        want_g, want_b = acc_g + dg, acc_b + db
        _, dg2, db2 = ops.ln_tanh_bwd(dyg, xg, y, gg, EPS, out_dgamma=acc_g, out_dbeta=acc_b)
    else:
        _, dg, db = ops.ln_bwd(dyg, xg, gg, EPS)
        want_g, want_b = acc_g + dg, acc_b + db
        _, dg2, db2 = ops.ln_bwd(dyg, xg, gg, EPS, acc_dgamma=acc_g, acc_dbeta=acc_b)
    torch.cuda.synchronize()
    assert dg2.data_ptr() == acc_g.data_ptr() and db2.data_ptr() == acc_b.data_ptr()
    assert torch.equal(acc_g, want_g) and torch.equal(acc_b, want_b)


# ------------------------------------------------------------------------------------------ head / long-K GEMMs
def test_head_gemms_at_the_bench_shape(ops):
    """The YOLO head (256 -> 256 -> 2400, bias) forward and backward over the bench's 38400 rows: dW contracts over all
    rows with the split-K factor linear_bwd picks (asserted > 1), db is a colsum."""
    g = torch.Generator().manual_seed(11)
    k_out = 2400
    x = torch.tanh(torch.randn(BENCH_R, 256, generator=g))          # LayerNorm + tanh output
    w0 = (torch.rand(256, 256, generator=g) * 2 - 1) * math.sqrt(6.0 / 512)
    w1 = (torch.rand(k_out, 256, generator=g) * 2 - 1) * math.sqrt(6.0 / (256 + k_out))
    b0, b1 = torch.randn(256, generator=g) * 0.1, torch.randn(k_out, generator=g) * 0.1
    dy1 = torch.randn(BENCH_R, k_out, generator=g)
    assert ops.wgrad_splits(256, 256, BENCH_R) > 1 and ops.wgrad_splits(k_out, 256, BENCH_R) > 1
    xg, w0g, w1g = dev(x), dev(w0), dev(w1)
    y0 = ops.linear(xg, w0g, dev(b0))
    y1 = ops.linear(y0, w1g, dev(b1))
    dx1, dw1, db1 = ops.linear_bwd(y0, w1g, dev(dy1))
    dx0, dw0, db0 = ops.linear_bwd(xg, w0g, dx1)
    torch.cuda.synchronize()
    y0c, dx1c = y0.cpu().double(), dx1.cpu().double()
    x64, dy64 = x.double(), dy1.double()
    check("head linear 256->256", y0, x64 @ w0.double().T + b0.double(), 2e-6)           # measured 7.1e-7
    check("head linear 256->2400", y1, y0c @ w1.double().T + b1.double(), 2e-6)         # measured 7.2e-7
    check("head bwd dx (2400->256)", dx1, dy64 @ w1.double(), 8e-6)                     # measured 2.7e-6
    check("head bwd dW (2400x256, K=38400)", dw1, dy64.T @ y0c, 6e-6)                   # measured 1.8e-6
    check("head bwd db (2400, 38400 rows)", db1, dy64.sum(0), 2.5e-7)                   # measured 8.2e-8
    check("head bwd dx (256->256)", dx0, dx1c @ w0.double(), 3e-6)                      # measured 9.0e-7
    check("head bwd dW (256x256, K=38400)", dw0, dx1c.T @ x64, 1.5e-6)                  # measured 4.8e-7
    check("head bwd db (256, 38400 rows)", db0, dx1c.sum(0), 2.5e-7)                    # measured 6.6e-8


def test_colsum_over_a_strided_view_at_the_bench_shape(ops):
    """colsum over the GRU's gate-gradient layout: [38400][768], a 384-column half at lda 768 (both halves)."""
    a = torch.randn(BENCH_R, 768, generator=torch.Generator().manual_seed(12))
    ag = dev(a)
    a64 = a.double()
    for lo in (0, 384):
        s = ops.colsum(ag[:, lo:lo + 384])
        check("colsum [38400][384] lda 768 at %d" % lo, s, a64[:, lo:lo + 384].sum(0), 2.5e-7)   # measured 8.8e-8 / 6.8e-8
    acc = dev(torch.randn(384, generator=torch.Generator().manual_seed(13)))
    want = acc + ops.colsum(ag[:, 384:])
    ops.colsum(ag[:, 384:], out=acc, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(acc, want)
