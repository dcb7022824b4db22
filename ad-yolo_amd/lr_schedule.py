"""Host side of the device-computed learning-rate schedules and the parameter EMA (csrc/optim.hip, the ``*_sched`` entry
points): ``train_config['lr_schedule']`` -> the float64 table the step's prep kernel reads, and the host mirror of the closed
forms the kernel evaluates (for logging without a device read, and for the tests).

With t the 1-based schedule step and e = floor((t - 1) / every)::

    lr(t) = base * warm(t) * main(e)                  (double; rounded to float32 once)
    warm(t) = s + (1 - s) * min(t - 1, W) / W         (W warm-up STEPS, 0 = none: LinearLR(start_factor=s, total_iters=W))
    main(e) = 1                                       constant
              gamma ** floor(e / step_size)           step         (StepLR)
              gamma ** #{milestones <= e}             multistep    (MultiStepLR, at most 8 milestones)
              gamma ** e                              exponential  (ExponentialLR)
              (eta_min + (base - eta_min) * (1 + cos(pi * min(e, T_max) / T_max)) / 2) / base
                                                      cosine       (CosineAnnealingLR's closed form, held after T_max)

Step 1 runs at the base rate: torch's convention when ``scheduler.step()`` follows ``optimizer.step()``, with one
``scheduler.step()`` per unit of ``every`` optimizer steps.
"""
import math

import numpy as np

from . import ops

_COMMON = {"name", "every", "warmup_steps", "warmup_start_factor"}
_OWN = {"constant": set(), "step": {"gamma", "step_size"}, "multistep": {"gamma", "milestones"}, "exponential": {"gamma"},
        "cosine": {"T_max", "eta_min"}}


def _whole(cfg, key, default, least):
    v = cfg.get(key, default)
    if v is None or isinstance(v, bool) or int(v) != v or int(v) < least:
        raise ValueError("lr_schedule: %s must be a whole number >= %d (got %r)" % (key, least, v))
    return int(v)


def normalise(cfg):
    """-> the schedule's configuration with every key of its kind present.  Unknown names raise NotImplementedError (like
    ``optim``), unknown keys and impossible values ValueError."""
    cfg = dict(cfg)
    name = cfg.get("name")
    if name not in _OWN:
        raise NotImplementedError("lr_schedule name %r (known: %s)" % (name, ", ".join(sorted(_OWN))))
    extra = set(cfg) - _COMMON - _OWN[name]
    if extra:
        raise ValueError("lr_schedule %r does not take %s" % (name, sorted(extra)))
    out = {"name": name, "every": _whole(cfg, "every", 1, 1), "warmup_steps": _whole(cfg, "warmup_steps", 0, 0)}
    s = float(cfg.get("warmup_start_factor", 1.0 / 3.0))                     # torch.optim.lr_scheduler.LinearLR's default
    if not 0.0 < s <= 1.0:
        raise ValueError("lr_schedule: warmup_start_factor must be in (0, 1] (got %r)" % s)
    out["warmup_start_factor"] = s
    if "gamma" in _OWN[name]:
        if name == "exponential" and "gamma" not in cfg:
            raise ValueError("lr_schedule 'exponential' needs gamma")
        g = float(cfg.get("gamma", 0.1))
        if not (g > 0.0 and math.isfinite(g)):
            raise ValueError("lr_schedule: gamma must be positive (got %r)" % g)
        out["gamma"] = g
    if name == "step":
        out["step_size"] = _whole(cfg, "step_size", None, 1)
    if name == "multistep":
        ms = [_whole({"milestones": m}, "milestones", None, 0) for m in cfg.get("milestones", ())]
        if not ms or len(ms) > ops.SCHED_MAX_MILESTONES or ms != sorted(ms):
            raise ValueError("lr_schedule 'multistep' needs 1 to %d milestones in increasing order (got %r)"
                             % (ops.SCHED_MAX_MILESTONES, cfg.get("milestones")))
        out["milestones"] = ms
    if name == "cosine":
        out["T_max"] = _whole(cfg, "T_max", None, 1)
        lo = float(cfg.get("eta_min", 0.0))
        if not (lo >= 0.0 and math.isfinite(lo)):
            raise ValueError("lr_schedule: eta_min must be >= 0 (got %r)" % lo)
        out["eta_min"] = lo
    return out


def check_base(cfg, base):
    base = float(base)
    if not math.isfinite(base) or base < 0.0 or (cfg["name"] == "cosine" and base <= 0.0):
        raise ValueError("learning rate %r is not usable with lr_schedule %r" % (base, cfg["name"]))
    return base


def check_ema_decay(decay):
    decay = float(decay)
    if not 0.0 <= decay < 1.0:
        raise ValueError("ema_decay must be in [0, 1) (got %r)" % decay)
    return decay


def table(cfg, base, offset=0, ema_decay=None, ema_warmup=False, ema_offset=0):
    """the ``ops.SCHED_TABLE_DOUBLES`` doubles of ``sched_dev`` for a normalised configuration"""
    tb = [0.0] * ops.SCHED_TABLE_DOUBLES
    tb[ops.SCHED_KIND] = float(ops.SCHED_KINDS[cfg["name"]])
    tb[ops.SCHED_BASE] = check_base(cfg, base)
    tb[ops.SCHED_EVERY] = float(cfg["every"])
    tb[ops.SCHED_WARMUP] = float(cfg["warmup_steps"])
    tb[ops.SCHED_START] = cfg["warmup_start_factor"]
    tb[ops.SCHED_GAMMA] = cfg.get("gamma", 1.0)
    tb[ops.SCHED_STEP_SIZE] = float(cfg.get("step_size", 1))
    tb[ops.SCHED_T_MAX] = float(cfg.get("T_max", 1))
    tb[ops.SCHED_ETA_MIN] = cfg.get("eta_min", 0.0)
    ms = cfg.get("milestones", [])
    tb[ops.SCHED_N_MILESTONES] = float(len(ms))
    for i, m in enumerate(ms):
        tb[ops.SCHED_MILESTONE0 + i] = float(m)
    tb[ops.SCHED_OFFSET] = float(offset)
    tb[ops.SCHED_EMA_DECAY] = 0.0 if ema_decay is None else check_ema_decay(ema_decay)
    tb[ops.SCHED_EMA_WARMUP] = 1.0 if ema_warmup else 0.0
    tb[ops.SCHED_EMA_OFFSET] = float(ema_offset)
    return tb


def lr_double(tb, t):
    """lr(t) before its rounding to float32, from the table, in the kernel's order of operations (t: 1-based schedule step)"""
    t = float(t)
    base, w, s = tb[ops.SCHED_BASE], tb[ops.SCHED_WARMUP], tb[ops.SCHED_START]
    e = math.floor((t - 1.0) / tb[ops.SCHED_EVERY])
    warm = s + (1.0 - s) * min(t - 1.0, w) / w if w > 0.0 else 1.0
    kind = int(tb[ops.SCHED_KIND])
    main = 1.0
    if kind == ops.SCHED_KINDS["step"]:
        main = math.pow(tb[ops.SCHED_GAMMA], math.floor(e / tb[ops.SCHED_STEP_SIZE]))
    elif kind == ops.SCHED_KINDS["multistep"]:
        n = int(tb[ops.SCHED_N_MILESTONES])
        main = math.pow(tb[ops.SCHED_GAMMA], float(sum(1 for m in tb[ops.SCHED_MILESTONE0:ops.SCHED_MILESTONE0 + n] if m <= e)))
    elif kind == ops.SCHED_KINDS["exponential"]:
        main = math.pow(tb[ops.SCHED_GAMMA], float(e))
    elif kind == ops.SCHED_KINDS["cosine"]:
        tm, lo = tb[ops.SCHED_T_MAX], tb[ops.SCHED_ETA_MIN]
        main = (lo + (base - lo) * (1.0 + math.cos(math.pi * min(float(e), tm) / tm)) / 2.0) / base
    return base * warm * main


def lr_at(tb, t):
    """the float32 the prep kernel hands to the update at schedule step t, as a Python float"""
    return float(np.float32(lr_double(tb, t)))


def ema_weight(tb, k):
    """(w, first) of the EMA update that follows k earlier ones: ema = first ? p : fma(p - ema, w, ema)"""
    keep = tb[ops.SCHED_EMA_DECAY]
    if tb[ops.SCHED_EMA_WARMUP] != 0.0:
        keep = min(keep, (1.0 + k) / (10.0 + k))
    return float(np.float32(1.0 - keep)), k <= 0
