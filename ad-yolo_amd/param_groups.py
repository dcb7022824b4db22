"""Host side of the fused optimizers' parameter groups (csrc/optim.hip, the ``*_groups`` entry points):
``train_config['param_groups']`` -> the resolved groups the optimizers take, and the group map the update launch reads.

An entry is ``{name, match, ndim_max, lr, weight_decay}``: ``match`` a list of ``fnmatch`` patterns on the names of
``model.named_parameters()``, ``ndim_max`` selects parameters with ``p.ndim <= ndim_max`` (``ndim_max: 1`` = BatchNorm and
LayerNorm scales and every bias: the usual no-decay rule); an entry with both selects what satisfies both.  A parameter
goes to the FIRST entry that selects it; what no entry selects forms the default group with ``train_config``'s ``lr`` and
``weight_decay``, which are also the defaults of an entry's own.  ``lr`` is the group's absolute base rate, as in torch.
Group order: the default group first if it is non-empty, then the entries in list order.

A resolved group is ``{name, lr, weight_decay, params}`` with ``params`` the members' indices in ``flat.module_params``
(``model.parameters()`` order), increasing.
"""
import fnmatch
import math

import torch

from . import ops

MAX_ENTRIES = ops.OPTIM_MAX_GROUPS - 1           # + the default group
_KEYS = {"name", "match", "ndim_max", "lr", "weight_decay"}


def _value(entry_name, key, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError("param_groups entry %r: %s must be a finite number >= 0 (got %r)" % (entry_name, key, v))
    return float(v)


def resolve(entries, flat, lr, weight_decay):
    """``train_config['param_groups']`` (None or empty: no groups -> None) on the parameters of ``flat`` -> the resolved groups"""
    if not entries:
        return None
    if len(entries) > MAX_ENTRIES:
        raise ValueError("param_groups has %d entries, at most %d are possible" % (len(entries), MAX_ENTRIES))
    resolved = []
    for k, e in enumerate(entries):
        name = e.get("name", k) if isinstance(e, dict) else k
        if not isinstance(e, dict) or set(e) - _KEYS:
            raise ValueError("param_groups entry %r: unknown key(s) %s (known: %s)"
                             % (name, sorted(set(e) - _KEYS) if isinstance(e, dict) else e, sorted(_KEYS)))
        match = e.get("match")
        if isinstance(match, str):
            match = [match]
        ndim_max = e.get("ndim_max")
        if ndim_max is not None and (isinstance(ndim_max, bool) or int(ndim_max) != ndim_max or ndim_max < 0):
            raise ValueError("param_groups entry %r: ndim_max must be a whole number >= 0 (got %r)" % (name, ndim_max))
        resolved.append({"name": name, "match": match, "ndim_max": ndim_max,
                         "lr": _value(name, "lr", e.get("lr", lr)),
                         "weight_decay": _value(name, "weight_decay", e.get("weight_decay", weight_decay)), "params": []})
    if len({g["name"] for g in resolved} | {"default"}) != len(resolved) + 1:
        raise ValueError("param_groups: entry names must differ from each other and from 'default' (got %r)"
                         % [g["name"] for g in resolved])
    default = {"name": "default", "lr": float(lr), "weight_decay": float(weight_decay), "params": []}
    for i, (pname, p) in enumerate(zip(flat.names, flat.module_params)):
        for g in resolved:
            if g["match"] is not None and not any(fnmatch.fnmatchcase(pname, pat) for pat in g["match"]):
                continue
            if g["ndim_max"] is not None and p.ndim > g["ndim_max"]:
                continue
            g["params"].append(i)
            break
        else:
            default["params"].append(i)
    for g in resolved:
        if not g["params"]:
            raise ValueError("param_groups entry %r selects no parameter" % (g["name"],))
    groups = ([default] if default["params"] else []) + resolved
    return [{"name": g["name"], "lr": g["lr"], "weight_decay": g["weight_decay"], "params": g["params"]} for g in groups]


def check(groups, flat):
    """resolved groups handed to an optimizer: every parameter of ``flat`` in exactly one of at most 16 groups"""
    if not 1 <= len(groups) <= ops.OPTIM_MAX_GROUPS:
        raise ValueError("%d parameter groups, 1 to %d are possible" % (len(groups), ops.OPTIM_MAX_GROUPS))
    members = sorted(i for g in groups for i in g["params"])
    if members != list(range(len(flat.module_params))):
        raise ValueError("param_groups must hold every parameter of the flat buffer exactly once")
    out = []
    for k, g in enumerate(groups):
        name = g.get("name", k)
        out.append({"name": name, "lr": _value(name, "lr", g["lr"]), "weight_decay": _value(name, "weight_decay", g["weight_decay"]),
                    "params": sorted(int(i) for i in g["params"])})
    return out


def group_map(groups, flat):
    """one uint8 per element of the padded flat buffer, on its device: the element's group (the padding belongs to group 0)"""
    where = {id(p): k for k, p in enumerate(flat.params)}
    m = torch.zeros(flat.flat.numel(), dtype=torch.uint8)
    for k, g in enumerate(groups):
        for i in g["params"]:
            off, n = flat.offsets[where[id(flat.module_params[i])]]
            m[off:off + n] = k
    return m.to(flat.flat.device)
