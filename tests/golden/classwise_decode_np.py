"""NumPy float32 statement of the class-wise decode record (include/adyolo_hip.h, ``adyolo_classwise_decode``): the CPU tests
feed it to ``classwise_select``, the GPU tests compare the kernel with it.  Test-side code of this project; the distances
follow ``distance_between_cartesian_coordinates`` (utils/seld_metrics.py:97-114) in float32."""
import numpy as np

F32 = np.float32


def _act(x, y, z):
    return np.sqrt(x ** 2 + y ** 2 + z ** 2)


def _dist(a, b):
    n1 = np.sqrt(a[..., 0] ** 2 + a[..., 1] ** 2 + a[..., 2] ** 2 + F32(1e-10))
    n2 = np.sqrt(b[..., 0] ** 2 + b[..., 1] ** 2 + b[..., 2] ** 2 + F32(1e-10))
    d = (a[..., 0] / n1) * (b[..., 0] / n2) + (a[..., 1] / n1) * (b[..., 1] / n2) + (a[..., 2] / n1) * (b[..., 2] / n2)
    return (np.arccos(np.clip(d, F32(-1), F32(1))) * F32(180) / F32(np.pi)).astype(F32)


def decode(output, loss, c):
    """output (..., W*C) float32 -> [frames][C][rec] float32."""
    o = np.asarray(output, dtype=F32).reshape(-1, {"adpit": 9, "accdoa": 3}.get(loss, 4), c)
    if loss in ("seddoa", "masked-seddoa"):
        return np.ascontiguousarray(o.transpose(0, 2, 1))
    if loss == "accdoa":
        return np.stack([_act(o[:, 0], o[:, 1], o[:, 2]), o[:, 0], o[:, 1], o[:, 2]], axis=-1)
    v = o.reshape(-1, 3, 3, c).transpose(0, 3, 1, 2)                  # [frames][C][track][xyz]
    dec = np.zeros((o.shape[0], c, 16), dtype=F32)
    dec[..., 0:3] = _act(v[..., 0], v[..., 1], v[..., 2])
    dec[..., 3:12] = v.reshape(-1, c, 9)
    dec[..., 12] = _dist(v[:, :, 0], v[:, :, 1])
    dec[..., 13] = _dist(v[:, :, 1], v[:, :, 2])
    dec[..., 14] = _dist(v[:, :, 2], v[:, :, 0])
    return dec
