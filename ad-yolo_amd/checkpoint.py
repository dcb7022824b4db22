"""Checkpoint / resume in the reference's file format (src/train.py:145-159, 225-248; src/utils/utility.py:22-50), so that
result folders are interchangeable: ``model_ckpt.h5`` = {start_epoch_nb, model_state_dict, optim_state_dict,
confidence_thresh, rng_state, best_log, train_remaining_file}, ``model_best.h5`` = {epoch_nb, model_state_dict,
optim_state_dict, confidence_thresh}.  ``model_state_dict`` has the reference's 305 keys (WrapperModel.state_dict()),
``optim_state_dict`` is the layout of the optimizer's torch.optim counterpart (Adam, AdamW or SGD) with parameter indices in
``model.parameters()`` order.

With a learning-rate schedule or an EMA on the optimizer (``train_config['lr_schedule']`` / ``['ema_decay']``), and only then,
both files gain ``sched_state_dict`` (the optimizer's ``sched_state_dict()``: configuration, current base rate, the schedule's
step, the EMA's update count) and, with an EMA, ``ema_state_dict``: the layout of ``model_state_dict`` with the parameters taken
from the EMA and the buffers from the live model, so that the reference loads it as a model.  With the non-finite guard
(``train_config['skip_nonfinite']``) both files gain ``guard_state_dict``: {attempts, skipped}, the counts of the optimizer's
guard record; a file without it loads with zeros, and a file with it loads into an unguarded optimizer, which ignores it.
Without them the files are what they always were.

Unlike the reference the RNG helpers do not touch ``torch.cuda`` when the device is the CPU.
"""
import os
import random

import numpy as np
import torch


def get_rng_state(device, model=None):
    """utility.py:32-39 plus, when ``model`` is given, the encoders' counter-based dropout streams (``rng.DropoutStream``:
    they replace the draws the reference takes from torch's generator)."""
    dev = torch.device(device)
    state = {"rand_state": random.getstate(), "numpy_state": np.random.get_state(),
             "torch_state": torch.random.get_rng_state(), "os_hash_state": str(os.environ.get("PYTHONHASHSEED", "100"))}
    if model is not None:
        from . import rng
        state["dropout_streams"] = rng.collect(model)
    state["cuda_state"] = torch.cuda.get_rng_state(device=dev) if dev.type == "cuda" and torch.cuda.is_available() else None
    return state


def seed_resume(rng_state, device, model=None):
    dev = torch.device(device)
    if model is not None and rng_state.get("dropout_streams"):
        from . import rng
        rng.restore(model, rng_state["dropout_streams"])
    random.setstate(rng_state["rand_state"])
    np.random.set_state(rng_state["numpy_state"])
    torch.random.set_rng_state(rng_state["torch_state"])
    if rng_state.get("cuda_state") is not None and dev.type == "cuda" and torch.cuda.is_available():
        torch.cuda.set_rng_state(rng_state["cuda_state"], device=dev)
    os.environ["PYTHONHASHSEED"] = str(rng_state["os_hash_state"])


def _indexed_params(optimizer, model):
    """-> [(index in model.parameters() order, parameter, offset in the flat buffer, numel)]: the order torch.optim's
    ``state_dict()`` uses, independent of the flat buffer's internal (reversed) order."""
    flat = optimizer.flat
    where = {id(p): k for k, p in enumerate(flat.params)}
    params = [p for p in model.parameters() if p.requires_grad] if model is not None else flat.module_params
    return [(i, p) + tuple(flat.offsets[where[id(p)]]) for i, p in enumerate(params)]


def _grouping(optimizer, params):
    """-> [(the optimizer's group or None, [positions in ``params``])] in group order, and the torch id of every position:
    torch numbers the parameters consecutively group by group, inside a group in the order they were handed over
    (``model.parameters()`` order here).  Without parameter groups: one group, ids = positions."""
    groups = getattr(optimizer, "groups", None)
    if groups is None:
        return [(None, list(range(len(params))))], list(range(len(params)))
    members = [(g, list(g["params"])) for g in groups]
    ids = [None] * len(params)
    for k, i in enumerate(i for _, mem in members for i in mem):
        ids[i] = k
    return members, ids


def _shape_of(groups):
    return [len(g["params"]) for g in groups]


def _match_groups(optimizer, params, sd):
    """-> (file ids by position in ``params``, the file's groups to take ``lr`` / ``weight_decay`` from or None = keep the
    optimizer's own).  File groups of the optimizer's sizes, in order: state goes through the ids.  A one-group file into a
    grouped optimizer (fine-tuning from an ungrouped run): by ``model.parameters()`` order.  Anything else is refused."""
    members, ids = _grouping(optimizer, params)
    file_groups = sd["param_groups"]
    mine, theirs = [len(mem) for _, mem in members], _shape_of(file_groups)
    if sum(theirs) != len(params):
        raise ValueError("optimizer state has %d parameters, the model %d" % (sum(theirs), len(params)))
    if theirs == mine:
        file_ids = [None] * len(params)
        for (_, mem), fg in zip(members, file_groups):
            for i, fid in zip(mem, fg["params"]):
                file_ids[i] = fid
        return file_ids, file_groups
    if len(theirs) == 1:
        return list(file_groups[0]["params"]), None
    raise ValueError("optimizer state has parameter groups of sizes %s, this optimizer %s" % (theirs, mine))


def _shared(file_groups, keys):
    """the hyper-parameters the flat optimizers keep ONE of must agree over the file's groups"""
    g0 = file_groups[0]
    for g in file_groups[1:]:
        for k in keys:
            if g.get(k) != g0.get(k):
                raise ValueError("optimizer state has per-group %s (%r and %r): only lr and weight_decay may differ between "
                                 "groups" % (k, g0.get(k), g.get(k)))
    return g0


def _take_group_values(optimizer, file_groups):
    """``lr`` / ``weight_decay``: the file's, group by group (``file_groups`` None: a grouped optimizer keeps its own)"""
    if getattr(optimizer, "groups", None) is None:
        optimizer.lr, optimizer.weight_decay = file_groups[0]["lr"], file_groups[0].get("weight_decay", 0.0)
    elif file_groups is not None:
        for g, fg in zip(optimizer.groups, file_groups):
            g["lr"], g["weight_decay"] = float(fg["lr"]), float(fg.get("weight_decay", 0.0))
        optimizer.lr, optimizer.weight_decay = optimizer.groups[0]["lr"], optimizer.groups[0]["weight_decay"]


def _cpu_slice(buf, off, n, p):
    return buf[off:off + n].view(p.shape).detach().cpu().clone()


def optimizer_state_dict(optimizer, model):
    """The fused optimizer's state in the layout of its torch.optim counterpart (``optimizer.kind``): FusedAdam ->
    torch.optim.Adam, FusedAdamW -> torch.optim.AdamW (Adam's state, ``decoupled_weight_decay: True`` in the group), FusedSGD ->
    torch.optim.SGD (``momentum_buffer`` per parameter once a step with momentum was taken, no entries otherwise).  Indices
    follow ``model.parameters()``; with parameter groups there is one torch group per group, each with its own ``lr`` and
    ``weight_decay``, and torch's numbering: consecutive group by group, ``model.parameters()`` order inside a group.
    ``clip_grad_norm`` is configuration, not state: it is not written.  Under the non-finite guard
    (``train_config['skip_nonfinite']``) the optimizer reconciles first: ``step`` is the number of APPLIED steps, what
    torch.optim under a ``GradScaler`` would hold.  Under gradient accumulation (``train_config['accum_steps']``) a state in the
    middle of a cycle is refused with ValueError: the accumulator is not part of a checkpoint."""
    if getattr(optimizer, "micro_index", 0) != 0:
        optimizer._refuse_mid_cycle("optimizer state_dict")
    if getattr(optimizer, "guard_dev", None) is not None:
        optimizer.reconcile()
    params = _indexed_params(optimizer, model)
    members, ids = _grouping(optimizer, params)
    kind = getattr(optimizer, "kind", "adam")
    state = {}
    if kind == "sgd":
        if optimizer.momentum != 0 and optimizer.step_count > 0:
            for i, p, off, n in params:
                state[ids[i]] = {"momentum_buffer": _cpu_slice(optimizer.momentum_buffer, off, n, p)}
    elif optimizer.step_count > 0:
        for i, p, off, n in params:
            state[ids[i]] = {"step": torch.tensor(float(optimizer.step_count)),
                             "exp_avg": _cpu_slice(optimizer.exp_avg, off, n, p),
                             "exp_avg_sq": _cpu_slice(optimizer.exp_avg_sq, off, n, p)}
    if getattr(optimizer, "groups", None) is not None:
        state = {k: state[k] for k in sorted(state)}
    out = []
    for g, mem in members:
        lr, wd = (optimizer.lr, optimizer.weight_decay) if g is None else (g["lr"], g["weight_decay"])
        if kind == "sgd":
            group = {"lr": lr, "momentum": optimizer.momentum, "dampening": optimizer.dampening, "weight_decay": wd,
                     "nesterov": optimizer.nesterov, "maximize": False, "foreach": None, "differentiable": False, "fused": None}
        else:
            group = {"lr": lr, "betas": tuple(optimizer.betas), "eps": optimizer.eps, "weight_decay": wd, "amsgrad": False,
                     "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None}
            if kind == "adamw":
                group["decoupled_weight_decay"] = True
        group["params"] = [ids[i] for i in mem]
        out.append(group)
    return {"state": state, "param_groups": out}


def _load_sgd_state(optimizer, params, sd, g, file_ids, file_groups):
    """torch.optim.SGD's state holds no step count: whether the next step is "the first" (momentum buffer := gradient) is
    decided by the presence of buffers, and ``step_count`` -- from which the device-side flag is derived -- is set to agree."""
    if (g.get("momentum", 0.0) != 0) != (optimizer.momentum != 0):        # (the buffer exists or not since construction)
        raise ValueError("SGD state was written with momentum %r, this optimizer has %r"
                         % (g.get("momentum", 0.0), optimizer.momentum))
    _take_group_values(optimizer, file_groups)
    optimizer.momentum, optimizer.dampening = g.get("momentum", 0.0), g.get("dampening", 0.0)
    optimizer.nesterov = bool(g.get("nesterov", False))
    have = []
    for i, p, off, n in params:
        st = sd["state"].get(file_ids[i], sd["state"].get(i) if len(sd["param_groups"]) == 1 else None)
        buf = None if st is None else st.get("momentum_buffer")
        have.append(buf is not None)
        if buf is None or optimizer.momentum == 0:
            continue
        if tuple(buf.shape) != tuple(p.shape):
            raise ValueError("optimizer state %d has shape %s, parameter %s" % (i, tuple(buf.shape), tuple(p.shape)))
        optimizer.momentum_buffer[off:off + n].copy_(buf.reshape(-1))
    if optimizer.momentum != 0 and any(have) and not all(have):
        raise ValueError("some parameters have a momentum buffer and some have none: the flat SGD keeps ONE first-step flag")
    resumed = optimizer.momentum != 0 and bool(have) and all(have)
    if optimizer.momentum != 0 and not resumed:
        optimizer.momentum_buffer.zero_()
    optimizer.step_count = 1 if resumed else 0
    _refresh_schedule(optimizer)


def _refresh_schedule(optimizer):
    """the loaded group's ``lr`` is the schedule's base rate: rewrite the device table (scheduled optimizers only)"""
    if getattr(optimizer, "sched_dev", None) is not None:
        optimizer._write_table()


def load_optimizer_state_dict(optimizer, model, sd):
    """A file whose groups have the sizes of the optimizer's, in order, is taken group by group (state through the ids, ``lr``
    and ``weight_decay`` per group from the file); a one-group file into a grouped optimizer is taken by
    ``model.parameters()`` order and the optimizer keeps its own group values; any other grouping raises ValueError.  An
    accumulating optimizer starts a new cycle."""
    if getattr(optimizer, "accum_dev", None) is not None:
        optimizer.reset_accumulation()
    params = _indexed_params(optimizer, model)
    file_ids, file_groups = _match_groups(optimizer, params, sd)
    kind = getattr(optimizer, "kind", "adam")
    if kind == "sgd":
        if any("betas" in fg for fg in sd["param_groups"]):
            raise ValueError("an Adam-family optimizer state cannot be loaded into FusedSGD")
        g = _shared(sd["param_groups"], ("momentum", "dampening", "nesterov"))
        return _load_sgd_state(optimizer, params, sd, g, file_ids, file_groups)
    if any("betas" not in fg for fg in sd["param_groups"]):
        raise ValueError("an SGD optimizer state cannot be loaded into %s" % type(optimizer).__name__)
    g = _shared(sd["param_groups"], ("betas", "eps", "amsgrad", "decoupled_weight_decay"))
    if kind == "adamw" and g.get("decoupled_weight_decay", True) is False:
        raise ValueError("a torch.optim.Adam state (coupled weight decay) cannot be loaded into FusedAdamW")
    optimizer.betas, optimizer.eps = tuple(g["betas"]), g["eps"]
    _take_group_values(optimizer, file_groups)
    if g.get("amsgrad", False):
        raise NotImplementedError("amsgrad Adam state is not supported by the fused gfx950 Adam")
    steps = set()
    for i, p, off, n in params:
        st = sd["state"].get(file_ids[i], sd["state"].get(i) if len(sd["param_groups"]) == 1 else None)
        if st is None:
            optimizer.exp_avg[off:off + n].zero_()
            optimizer.exp_avg_sq[off:off + n].zero_()
            continue
        if tuple(st["exp_avg"].shape) != tuple(p.shape):
            raise ValueError("optimizer state %d has shape %s, parameter %s" % (i, tuple(st["exp_avg"].shape), tuple(p.shape)))
        optimizer.exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1))
        optimizer.exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
        steps.add(int(st["step"]))
    if len(steps) > 1:
        raise ValueError("per-parameter step counts differ (%s): not a plain Adam run" % sorted(steps))
    optimizer.step_count = steps.pop() if steps else 0
    _refresh_schedule(optimizer)


def _flat_slices(optimizer, model):
    """-> [(state_dict key, parameter, offset in the flat buffer, numel)] of the parameters that live in the flat buffer"""
    flat = optimizer.flat
    where = {id(p): k for k, p in enumerate(flat.params)}
    return [(name, p) + tuple(flat.offsets[where[id(p)]]) for name, p in model.named_parameters() if id(p) in where]


def ema_state_dict(optimizer, model, model_sd=None):
    """``model_state_dict``'s layout and keys: parameters from the optimizer's EMA (the live ones while it has had no update),
    buffers -- BatchNorm running statistics among them -- from the live model (or from ``model_sd``, a state_dict to fill)."""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()} if model_sd is None else dict(model_sd)
    if optimizer.ema_updates > 0:
        for name, p, off, n in _flat_slices(optimizer, model):
            sd[name] = _cpu_slice(optimizer.ema, off, n, p)
    return sd


def load_ema_state_dict(optimizer, model, sd):
    for name, p, off, n in _flat_slices(optimizer, model):
        if tuple(sd[name].shape) != tuple(p.shape):
            raise ValueError("EMA state %s has shape %s, parameter %s" % (name, tuple(sd[name].shape), tuple(p.shape)))
        optimizer.ema[off:off + n].copy_(sd[name].reshape(-1))


def _schedule_entries(optimizer, model, sd):
    """the keys a scheduled / averaging / guarded optimizer adds to a checkpoint file (none otherwise)"""
    out = {}
    if getattr(optimizer, "guard_dev", None) is not None:
        out["guard_state_dict"] = optimizer.guard_state_dict()
    if getattr(optimizer, "sched_dev", None) is None:
        return out
    out["sched_state_dict"] = optimizer.sched_state_dict()
    if optimizer.ema is not None:
        out["ema_state_dict"] = ema_state_dict(optimizer, model, sd)
    return out


def _state_dict_for_save(model, group=None):
    """-> (this process writes?, the state_dict to write).

    Data parallelism: BatchNorm running statistics are per-rank (each rank sees its own shard).  The file holds their AVERAGE
    over the ranks, formed in temporary copies: the live buffers are not touched (round 4, ADVICE: averaging them in place
    made a run that saves follow another trajectory than one that does not).  THE ALL-RANKS CONTRACT: with a process group of
    more than one rank, ``save_checkpoint`` / ``save_best`` are COLLECTIVES -- every rank must call them (an
    ``if rank == 0: save_checkpoint(...)`` would leave rank 0 waiting in all_reduce for ever); only rank 0 writes the file.
    ``group``: the trainer's process group (``TrainStep.reducer.group``; None = the default group)."""
    import torch.distributed as dist
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    writes = True
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        world = dist.get_world_size(group)
        for name, buf in model.named_buffers():
            if name in sd and buf.is_floating_point():          # running_mean / running_var (num_batches_tracked is equal)
                t = buf.detach().clone()
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
                sd[name] = t / world
        writes = dist.get_rank(group) == 0
    return writes, {k: v.cpu() for k, v in sd.items()}


def save_checkpoint(path, model, optimizer, start_epoch_nb, conf_thresh, best_log, train_remaining_file, device, group=None):
    """``model_ckpt.h5`` in the reference's format (train.py:241-248).  A collective under data parallelism: see
    ``_state_dict_for_save``."""
    writes, sd = _state_dict_for_save(model, group)
    if not writes:
        return
    ck = {"start_epoch_nb": start_epoch_nb,
          "model_state_dict": sd,
          "optim_state_dict": optimizer_state_dict(optimizer, model),
          "confidence_thresh": float(conf_thresh), "rng_state": get_rng_state(device, model), "best_log": best_log,
          "train_remaining_file": train_remaining_file}
    ck.update(_schedule_entries(optimizer, model, sd))
    torch.save(ck, path)


def save_best(path, model, optimizer, epoch_nb, conf_thresh, group=None):
    """``model_best.h5`` (train.py:234-238).  A collective under data parallelism: see ``_state_dict_for_save``."""
    writes, sd = _state_dict_for_save(model, group)
    if not writes:
        return
    ck = {"epoch_nb": epoch_nb, "model_state_dict": sd,
          "optim_state_dict": optimizer_state_dict(optimizer, model), "confidence_thresh": float(conf_thresh)}
    ck.update(_schedule_entries(optimizer, model, sd))
    torch.save(ck, path)


def load_checkpoint(path, model, optimizer=None, device="cpu", restore_rng=True):
    """-> the checkpoint dictionary; model (strict) and optimizer are restored in place.  Parameters stay views of the
    flat buffer: ``load_state_dict`` copies into them.  An optimizer with a schedule / EMA continues both from
    ``sched_state_dict`` / ``ema_state_dict``; a file without ``ema_state_dict`` starts the EMA from the loaded parameters."""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    model.load_state_dict(ck["model_state_dict"], strict=True)
    if optimizer is not None and "optim_state_dict" in ck:
        load_optimizer_state_dict(optimizer, model, ck["optim_state_dict"])
    if optimizer is not None and getattr(optimizer, "sched_dev", None) is not None:
        if "sched_state_dict" in ck:
            optimizer.load_sched_state_dict(ck["sched_state_dict"])
        if optimizer.ema is not None:
            if "ema_state_dict" in ck:
                load_ema_state_dict(optimizer, model, ck["ema_state_dict"])
            else:
                optimizer.restart_ema()
    if optimizer is not None and getattr(optimizer, "guard_dev", None) is not None:
        optimizer.load_guard_state_dict(ck.get("guard_state_dict"))
    if restore_rng and ck.get("rng_state") is not None:
        seed_resume(ck["rng_state"], device, model)
    return ck
