"""Sample-rate conversion for inference on recordings at any rate: the host half (NumPy only) of ``adyolo_resample_pcm``
(csrc/resample.hip, DESIGN section 5 "Sample-rate conversion").

``plan(rate_in, rate_out)`` designs a Kaiser-windowed sinc prototype and cuts it into the L phase rows of a polyphase filter,
quantised to Q30 integers with every row summing to exactly 2**30; the kernel multiplies Q23 samples by those rows in int64
and rounds half-even to int16, so the result is defined bit for bit (adyolo_hip.h) and a constant input is reproduced exactly.
``corpus.load_infer_split(..., resample=True)`` + ``corpus.InferDeviceCorpus`` use it for whole folders; ``resample_device``
converts one device tensor for callers that feed ``test_epoch_audio`` or ``FeatureExtractor`` themselves.

zeros = 32, beta = 9.0 and rolloff = 0.95 are configuration defaults, not tuned values: 32 zero crossings of the sinc on each
side, a Kaiser window of about 90 dB, the cutoff at 0.95 of the lower Nyquist rate.
"""
from math import gcd

import numpy as np

MAX_P = 320                     # max(L, M): every standard rate against 24 kHz (8 ... 192 kHz); the table is then 81 KB
TAP_BITS = 30                   # the taps are Q30
KINDS = {np.dtype(np.int16): 0, np.dtype(np.int32): 1, np.dtype(np.float32): 2}      # ADYOLO_RESAMPLE_INT16 / _INT32 / _FLOAT32


def ratio(rate_in, rate_out):
    """(L, M): rate_out / rate_in in lowest terms.  ``ValueError`` unless both rates are positive integers."""
    if int(rate_in) != rate_in or int(rate_out) != rate_out or int(rate_in) < 1 or int(rate_out) < 1:
        raise ValueError("resample: rates %r -> %r Hz are not positive integers" % (rate_in, rate_out))
    g = gcd(int(rate_in), int(rate_out))
    return int(rate_out) // g, int(rate_in) // g


def n_out(n, l, m):
    """Frames a recording of ``n`` frames has after conversion by L / M: ceil(n L / M)."""
    return (int(n) * int(l) + int(m) - 1) // int(m)


def plan(rate_in, rate_out, zeros=32, beta=9.0, rolloff=0.95):
    """The polyphase filter of a conversion rate_in -> rate_out: {L, M, K, centre, taps}.

    L / M is the ratio in lowest terms and P = max(L, M).  The prototype has N = 2 zeros P + 1 points about its centre c =
    zeros P, in float64: h[n] = L fc sinc(fc (n - c)) kaiser(N, beta)[n] with fc = rolloff / P.  Row p of the (L, K) table,
    K = ceil(N / L), is h[p::L] zero-padded, divided by its own sum (DC gain 1 in every phase); taps = rint(table * 2**30) as
    int32, the largest-magnitude tap of each row then adjusted so that the row sums to exactly 2**30.  Output frame j reads
    t = j M + centre: phase t % L, newest input t // L (adyolo_hip.h ``adyolo_resample_pcm``).

    ``ValueError`` naming both rates for equal rates (there is nothing to filter: callers skip the kernel) and for P > 320."""
    l, m = ratio(rate_in, rate_out)
    if l == m:
        raise ValueError("resample.plan: %d -> %d Hz is no conversion (equal rates: skip the filter)" % (rate_in, rate_out))
    p_max = max(l, m)
    if p_max > MAX_P:
        raise ValueError("resample.plan: %d -> %d Hz is the ratio %d / %d; max(L, M) = %d is more than %d"
                         % (rate_in, rate_out, l, m, p_max, MAX_P))
    zeros = int(zeros)
    if zeros < 1 or not 0.0 < float(rolloff) <= 1.0:
        raise ValueError("resample.plan: zeros %r, rolloff %r (%d -> %d Hz)" % (zeros, rolloff, rate_in, rate_out))
    n = 2 * zeros * p_max + 1
    c = zeros * p_max
    fc = float(rolloff) / p_max
    h = l * fc * np.sinc(fc * (np.arange(n, dtype=np.float64) - c)) * np.kaiser(n, float(beta))
    k = -(-n // l)
    table = np.zeros((l, k), dtype=np.float64)
    for p in range(l):
        row = h[p::l]
        table[p, :len(row)] = row
    table /= table.sum(axis=1, keepdims=True)
    taps = np.rint(table * float(1 << TAP_BITS)).astype(np.int64)
    big = np.abs(taps).argmax(axis=1)
    taps[np.arange(l), big] += (1 << TAP_BITS) - taps.sum(axis=1)
    if taps.max() > np.iinfo(np.int32).max or taps.min() < np.iinfo(np.int32).min:
        raise ValueError("resample.plan: %d -> %d Hz: a tap does not fit int32" % (rate_in, rate_out))
    return {"L": l, "M": m, "K": int(k), "centre": int(c), "taps": np.ascontiguousarray(taps.astype(np.int32))}


def format_plan():
    """The plan that only converts the sample format (equal rates, an int32 or float32 source): one tap of 2**30, so that the
    kernel's rounding is round-half-even of q / 256."""
    return {"L": 1, "M": 1, "K": 1, "centre": 0, "taps": np.full((1, 1), 1 << TAP_BITS, dtype=np.int32)}


def plan_for(rate_in, rate_out):
    """``plan`` for two different rates, ``format_plan`` for equal ones."""
    l, m = ratio(rate_in, rate_out)
    return format_plan() if l == m else plan(rate_in, rate_out)


def resample_device(pcm, rate_in, rate_out, out=None):
    """pcm (n, 4) int16 / int32 (24-bit PCM left-justified) / float32 on the device, recorded at ``rate_in`` -> int16 (n_out, 4)
    at ``rate_out``, the bits ``InferDeviceCorpus`` holds for the same recording.  Equal rates and int16: ``pcm`` itself.  out:
    write into this int16 (n_out, 4) tensor.  A non-finite float sample counts as 0 and raises ``AdyoloHipError`` after the
    conversion (the status word is read: one host synchronisation)."""
    import torch
    from . import ops
    if not torch.is_tensor(pcm) or pcm.dim() != 2 or pcm.shape[1] != 4 or pcm.dtype not in ops.RESAMPLE_KINDS:
        raise ValueError("resample_device: pcm must be an int16, int32 or float32 tensor (n, 4) (got %s %s)"
                         % (getattr(pcm, "dtype", type(pcm).__name__), tuple(getattr(pcm, "shape", ()))))
    l, m = ratio(rate_in, rate_out)
    if l == m and pcm.dtype == torch.int16:
        return pcm
    pl = plan_for(rate_in, rate_out)
    n = int(pcm.shape[0])
    frames = n_out(n, l, m)
    if out is None:
        out = torch.empty((frames, 4), dtype=torch.int16, device=pcm.device)
    elif tuple(out.shape) != (frames, 4) or out.dtype != torch.int16:
        raise ValueError("resample_device: out %s %s, expected int16 %s" % (out.dtype, tuple(out.shape), (frames, 4)))
    if n == 0:
        return out
    dev = pcm.device
    recs = torch.tensor([[0, n, 0, frames]], dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.resample_pcm(pcm.contiguous(), recs, torch.from_numpy(pl["taps"]).to(dev), pl["M"], pl["centre"], out, status)
    ops.corpus_status_check(int(ops.to_host(status)[0]))
    return out
