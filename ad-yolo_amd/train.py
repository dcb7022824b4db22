"""Train step of the AD-YOLO hot path: features (K1) -> encoder+head forward -> AD-YOLO loss ->
backward -> [bucketed RCCL all-reduce] -> [gradient-norm clip] -> fused Adam / AdamW / SGD.  Mirror of ``get_optimizers`` / ``train_one_epoch``
(/root/reference/src/train.py:29-62) with the data-parallel layer the reference lacks.

FusedAdam keeps torch.optim.Adam's hyper-parameters and produces a ``state_dict`` in the stock Adam
format (train.py:149,236 save/restore it) while running one HIP launch over the flat parameter buffer.
"""
import contextlib
import os

import torch

from . import functional as Fn
from . import lr_schedule as _sched
from . import ops
from . import param_groups as _pgroups
from .dist import BucketedAllReduce, FlatParameters


class _FusedOptimizer:
    """What ``graph.StepGraphs`` and ``checkpoint`` use of an optimizer over a FlatParameters buffer: ``flat``, ``step_count``
    (settable), ``_dev_step_value``, ``step_dev``, ``sync_device_step()``, ``replayed()``, ``zero_grad()``,
    ``step(grad_scale=1.0)``, ``state_dict()`` / ``load_state_dict()``.

    The step counter lives ON THE DEVICE (incremented by the optimizer launch itself), so that no kernel argument changes from
    step to step and a whole train step can be replayed from a hipGraph; ``step_count`` is the host's mirror of it (checkpoints,
    torch.optim's state_dict layout).

    max_norm (None = off): ``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` in front of the update, on the device: one
    pass over the gradient buffer sums (g * grad_scale)^2 in float64 (fixed order, no atomics: the same bits on every call and
    on every rank that holds the same reduced gradients), the step's one-workgroup prep kernel turns the partials into
    ``clip_coef = min(1, max_norm / (norm + 1e-6))`` and the update multiplies it into ``grad_scale``.  ``grad_norm`` is then a
    device tensor of one float, the pre-clip norm of the last step (what ``clip_grad_norm_`` returns); reading it is an
    ordinary device read, nothing in here syncs.  ``max_norm`` is a constant of a recorded step, and so is ``lr`` unless the
    optimizer was built with a schedule.

    lr_schedule (None = off: the plain entry points, nothing more allocated): a ``lr_schedule`` configuration
    (``train_config['lr_schedule']``: ``{name, every, warmup_steps, warmup_start_factor, ...}``).  The rate is then computed
    ON THE DEVICE by the step's prep kernel from the step counter and a small table (``sched_dev``, float64, written by the
    host only), so it changes from step to step also under a replayed graph.  ``current_lr`` is a device view of one float, the
    rate the last step used (read it like ``grad_norm``); ``lr_at(t)`` is the host mirror of the same closed form, for logging
    without a device read; ``set_lr(x)`` writes a new base rate into the table -- it holds from the next step on, eager or
    replayed, with no new recording (the hook for a reduce-on-plateau policy in the caller's epoch loop).  ``lr`` is the BASE
    rate.  The schedule's clock is ``sched_step`` = ``step_count`` + an offset kept in the table, so it survives a resume
    that restarts ``step_count`` (FusedSGD).

    ema_decay (None = off): an exponential moving average of the parameters, ``ema`` (laid out like ``flat.flat``), updated by
    the update launch itself: a copy of the parameters after its first step, then ``ema += (p - ema) * (1 - decay_eff)`` with
    ``decay_eff = decay`` or, with ema_warmup, ``min(decay, (1 + k) / (10 + k))`` after k updates.  Without ``lr_schedule``
    the rate is a constant schedule.

    param_groups (None or empty = off: the entry points above with their arguments, nothing more allocated): resolved
    parameter groups, ``[{name, lr, weight_decay, params}]`` with ``params`` the members' indices in ``flat.module_params``
    (``param_groups.resolve`` makes them from ``train_config['param_groups']``).  Every group has its own base rate and weight
    decay; the schedule (constant without ``lr_schedule``), the counter, the clip -- ONE norm over all groups, as
    ``clip_grad_norm_(model.parameters())`` gives -- and the EMA are shared.  The step is then ``ops.*_step_groups_dev``: the
    prep kernel derives every group's rate from ``groups_dev`` (float64 (G, 2) {base rate, weight decay}, written by the host
    only) into ``groups_out``, and the update launch looks every element's group up in ``group_map`` (uint8, one entry per
    element of ``flat.flat``; a function of the layout alone, so identical on every rank).  ``groups`` lists
    ``{name, lr, weight_decay, params}``; ``current_lrs`` is a device view of the G rates the last step used; ``lr_at(t, group)``
    mirrors them on the host; ``set_lr(x, group=)`` / ``set_weight_decay(x, group=)`` (index or name) rewrite ``groups_dev``
    and hold from the next step on, eager or replayed -- a group built with rate 0 and decay 0 keeps its parameters bit for
    bit (its moments still move, its gradient still counts in the norm) until ``set_lr`` releases it.  ``lr`` and
    ``weight_decay`` mirror group 0's.

    skip_nonfinite (False = off: the entry points above, nothing more allocated): the step is ``ops.*_step_guard_dev``, which
    does NOTHING when the gradient is not finite -- the test is the fp32 total norm of ``grad * grad_scale``, so the sum of
    squares always runs (``clip_partials`` is allocated and ``grad_norm`` available with or without ``max_norm``), and it is
    made on the device inside the (recorded) step: a skipped attempt leaves parameters, state, EMA and the device counter
    untouched, so bias corrections, the schedule's clock, the EMA's count and SGD's first-step flag continue as if the batch
    had never been drawn.  ``guard_dev`` (int64, ``ops.OPTIM_GUARD_WORDS``) is the device's record {attempts, skipped, last
    attempt skipped, run of consecutive skips}.  The host cannot see a skip without reading it, so ``step_count`` counts
    ATTEMPTS until ``reconcile()`` is called: it takes the record's host copy (or reads it: one sync), subtracts the skips
    it has not seen yet from ``step_count`` and returns ``{attempts, skipped, last_skipped, run}``; ``lr_at(step_count)``,
    ``sched_step`` and ``ema_updates`` then agree with the device.  Everything that saves the counter or writes the device
    counter from the mirror reconciles first (``state_dict``, ``sched_state_dict``, setting ``step_count``, the fill of
    ``sync_device_step``, a graph capture).  Under data parallelism every rank holds the same reduced buffer and sums it in the
    same order, so every rank takes the same decision with no collective.  The guard protects what the optimizer owns:
    BatchNorm running statistics are written by the forward pass and are not rolled back.

    accum_steps (1 = off: the entry points above with their arguments, nothing more allocated): gradient accumulation over K
    micro-batches.  Every ``step()`` -- every ``TrainStep.step``, eager or replayed -- is then a MICRO-STEP,
    ``ops.*_step_accum_dev``: it adds ``flat.flat_grad`` into ``accum`` (laid out like it; fp32, left to right, as ``p.grad``
    accumulates in torch; the cycle's first micro-step overwrites), and all but the K-th of a cycle do nothing else.  The K-th
    takes the step the optimizer would take without accumulation on ``accum`` as its gradient under ``grad_scale / K`` (the
    mean of the micro-gradients): the norm, the clip, the guard's verdict -- one poisoned micro-gradient makes the whole cycle
    a skipped attempt --, the schedule's clock, the bias corrections and the EMA's count see one step per CYCLE.  Which
    micro-step a call is, is read by the kernels from ``accum_dev`` (int64, ``ops.OPTIM_ACCUM_WORDS``: {next micro index,
    calls, cycles, last call held}), so the call is the same every time and one recorded graph serves the whole cycle;
    ``micro_index`` (0 .. K-1, the next call's) is the host's mirror, and ``step_count`` advances on a cycle's last call
    only.  ``reset_accumulation()`` discards a partial cycle (the epoch loops call it when an epoch stops inside one);
    ``state_dict()`` and the checkpoint refuse a mid-cycle state with ValueError, ``load_state_dict`` starts a new cycle.
    BatchNorm statistics are per MICRO-batch, and the running statistics move on every micro-step, as in torch.  Under data
    parallelism every micro-gradient is all-reduced before it is accumulated."""

    kind = None                     # 'adam' | 'adamw' | 'sgd': the torch.optim layout ``checkpoint`` reads and writes

    def _init_common(self, flat, max_norm, skip_nonfinite=False, accum_steps=1):
        self.flat = flat
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        dev = flat.flat.device
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._step_count = 0
        self._dev_step_value = 0
        self.st_dev = torch.zeros(ops.OPTIM_SCRATCH_FLOATS, dtype=torch.float32, device=dev)
        self.clip_partials = self.grad_norm = None
        if self.max_norm is not None or self.skip_nonfinite:
            self.clip_partials = torch.zeros(ops.GRAD_SUMSQ_MAX_PARTS, dtype=torch.float64, device=dev)
            self.grad_norm = self.st_dev[2:3]
        if self.skip_nonfinite:
            self.guard_dev = torch.zeros(ops.OPTIM_GUARD_WORDS, dtype=torch.int64, device=dev)
        if _check_accum_steps(accum_steps) > 1:
            self.accum_steps = int(accum_steps)
            self.accum = torch.zeros_like(flat.flat_grad)
            self.accum_dev = torch.zeros(ops.OPTIM_ACCUM_WORDS, dtype=torch.int64, device=dev)

    @property
    def step_count(self):
        return self._step_count

    @step_count.setter
    def step_count(self, v):
        self.reconcile()                  # (guarded: skips not seen yet belong to the old value, not to the new one)
        self._step_count = int(v)

    def sync_device_step(self):
        if self._dev_step_value != self._step_count:
            self.reconcile()
            self.step_dev.fill_(self._step_count)
            self._dev_step_value = self._step_count

    def replayed(self):
        """A captured step (graph.py) was replayed: the optimizer launch inside it advanced the device counter (guarded: unless
        it skipped, which ``reconcile`` corrects later; accumulating: on a cycle's last micro-step)."""
        self._advance()

    def _advance(self):
        """the host's mirrors after one call of the step's launches, made now or replayed"""
        if self.accum_dev is not None:
            self.micro_index = (self.micro_index + 1) % self.accum_steps
            if self.micro_index != 0:         # a hold call: the device moved the accumulator and its record, nothing else
                return
        self._step_count += 1
        self._dev_step_value = self._step_count
        self._guard_dirty = True
        ops.params_changed()

    # ------------------------------------------------------------------------------------------ gradient accumulation
    accum_steps = 1
    accum = accum_dev = None
    micro_index = 0                 # which micro-step of its cycle the NEXT call is: the mirror of accum_dev[0]

    def reset_accumulation(self):
        """Discard a partial cycle: the next call is micro-step 0 of a new one, which overwrites the accumulator.  (A stream-
        ordered device write, no sync; nothing to do when accumulation is off.)"""
        if self.accum_dev is not None:
            self.accum_dev[0:1].zero_()
        self.micro_index = 0

    def _accum_kw(self):
        """what the accumulating entry points take beyond the guarded ones' arguments"""
        return dict(accum=self.accum, accum_dev=self.accum_dev, accum_steps=self.accum_steps, guard=self.guard_dev,
                    partials=self.clip_partials, max_norm=self.max_norm, sched_dev=self.sched_dev, sched_out=self.sched_out,
                    ema=self.ema, groups_dev=self.groups_dev, groups_out=self.groups_out, group_map=self.group_map)

    # ------------------------------------------------------------------------------------------ non-finite guard
    guard_dev = None
    skip_nonfinite = False
    _guard_seen = 0                 # skips of the record that ``step_count`` has been corrected for
    _guard_dirty = False            # an attempt was made since the record was last read
    _guard_record = (0, 0, 0, 0)    # the record as last seen

    def reconcile(self, guard=None):
        """guard: a host copy of ``guard_dev`` fetched after the last attempt (None: it is read here, one sync, and only if an
        attempt was made since the last time).  Subtracts the skips not yet seen from ``step_count`` and from the mirror of the
        device counter's value, once.  -> {attempts, skipped, last_skipped, run}; all zero on an unguarded optimizer."""
        if self.guard_dev is None:
            return {"attempts": 0, "skipped": 0, "last_skipped": False, "run": 0}
        if guard is not None:
            self._guard_record = tuple(int(x) for x in guard.reshape(-1)[:4].tolist())
        elif self._guard_dirty:
            self._guard_record = tuple(int(x) for x in self.guard_dev.tolist())
        self._guard_dirty = False
        attempts, skipped, last, run = self._guard_record
        unseen = skipped - self._guard_seen
        if unseen:
            self._step_count -= unseen
            self._dev_step_value -= unseen
            self._guard_seen = skipped
        return {"attempts": attempts, "skipped": skipped, "last_skipped": bool(last), "run": run}

    def guard_state_dict(self):
        """the counts a checkpoint carries (``checkpoint`` writes them as ``guard_state_dict``)"""
        rec = self.reconcile()
        return {"attempts": rec["attempts"], "skipped": rec["skipped"]}

    def load_guard_state_dict(self, sd=None):
        """the record continues from a checkpoint's counts (None or a file without them: zeros); the flag and the run start
        clean.  ``step_count`` is not touched: the loaded optimizer state already holds the number of APPLIED steps."""
        self.reconcile()
        sd = sd or {}
        rec = (int(sd.get("attempts", 0)), int(sd.get("skipped", 0)), 0, 0)
        if self.guard_dev is not None:
            self.guard_dev.copy_(torch.tensor(rec, dtype=torch.int64))
            self._guard_record, self._guard_seen, self._guard_dirty = rec, rec[1], False

    # ------------------------------------------------------------------------------------------ schedule / EMA
    sched_config = sched_dev = sched_out = current_lr = ema = ema_decay = None
    ema_warmup = False
    _sched_offset = _ema_offset = 0
    groups = group_map = groups_dev = groups_out = current_lrs = None

    def _init_sched(self, lr_schedule, ema_decay, ema_warmup, param_groups=None):
        if param_groups:
            self.groups = _pgroups.check(param_groups, self.flat)
            self.lr, self.weight_decay = self.groups[0]["lr"], self.groups[0]["weight_decay"]
            lr_schedule = {"name": "constant"} if lr_schedule is None else lr_schedule
        if lr_schedule is None and ema_decay is None:
            if ema_warmup:
                raise ValueError("ema_warmup without ema_decay")
            return
        self.sched_config = _sched.normalise({"name": "constant"} if lr_schedule is None else lr_schedule)
        if self.groups is None:
            _sched.check_base(self.sched_config, self.lr)
        self.ema_decay = None if ema_decay is None else _sched.check_ema_decay(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        if self.ema_warmup and self.ema_decay is None:
            raise ValueError("ema_warmup without ema_decay")
        dev = self.flat.flat.device
        self.sched_dev = torch.zeros(ops.SCHED_TABLE_DOUBLES, dtype=torch.float64, device=dev)
        self.sched_out = torch.zeros(ops.SCHED_OUT_FLOATS, dtype=torch.float32, device=dev)
        self.current_lr = self.sched_out[0:1]
        if self.ema_decay is not None:
            self.ema = torch.zeros_like(self.flat.flat)
        if self.groups is not None:
            self.group_map = _pgroups.group_map(self.groups, self.flat)
            self.groups_dev = torch.zeros(len(self.groups), 2, dtype=torch.float64, device=dev)
            self.groups_out = torch.zeros(len(self.groups), ops.GROUP_OUT_FLOATS, dtype=torch.float32, device=dev)
            self.current_lrs = self.groups_out[:, 0]
        self._write_table()

    def _table_for(self, base):
        """the schedule table with ``base`` as its rate.  A group's rate may be 0 under every schedule (the device then skips
        the closed form, and so does ``lr_at``): its table is built around a stand-in of 1."""
        zero = self.groups is not None and float(base) == 0.0
        tb = _sched.table(self.sched_config, 1.0 if zero else base, self._sched_offset, self.ema_decay, self.ema_warmup,
                          self._ema_offset)
        if zero:
            tb[ops.SCHED_BASE] = 0.0
        return tb

    def _write_table(self):
        """(re)write ``sched_dev`` (and ``groups_dev``) from the host's values: construction, ``set_lr``, ``load_state_dict``"""
        if self.groups is not None:
            for g in self.groups:
                self._table_for(g["lr"])                                      # (refuses what the schedule cannot run)
            self.groups[0]["lr"], self.groups[0]["weight_decay"] = float(self.lr), float(self.weight_decay)
            self.groups_dev.copy_(torch.tensor([[g["lr"], float(torch.tensor(g["weight_decay"], dtype=torch.float32))]
                                                for g in self.groups], dtype=torch.float64))
        self._table = self._table_for(self.lr)
        self.sched_dev.copy_(torch.tensor(self._table, dtype=torch.float64))

    def _group_index(self, group):
        if self.groups is None:
            raise ValueError("this optimizer was built without param_groups")
        if isinstance(group, int) and not isinstance(group, bool) and 0 <= group < len(self.groups):
            return group
        for k, g in enumerate(self.groups):
            if g["name"] == group and not isinstance(group, bool):
                return k
        raise ValueError("no parameter group %r (groups: %s)" % (group, [g["name"] for g in self.groups]))

    @property
    def sched_step(self):
        """the schedule's clock: the t of the LAST step taken (0 before the first)"""
        return self._step_count + self._sched_offset

    @property
    def ema_updates(self):
        return self._step_count + self._ema_offset if self.ema is not None else 0

    def lr_at(self, t, group=0):
        """the rate of schedule step t (1-based) as the device computes it: the closed form in double, rounded to float32.
        group (index or name; grouped optimizers only): whose rate -- a group whose base is 0 has rate 0.0 at every step"""
        if self.sched_dev is None:
            return _sched.lr_at(_sched.table(_sched.normalise({"name": "constant"}), self.lr), t)
        if self.groups is None:
            return _sched.lr_at(self._table, t)
        base = self.groups[self._group_index(group)]["lr"]
        return 0.0 if base == 0.0 else _sched.lr_at(self._table_for(base), t)

    def set_lr(self, lr, group=None):
        if self.sched_dev is None:
            raise ValueError("this optimizer was built without a schedule, its lr is a constant of the (recorded) step: "
                             "build it with lr_schedule: {name: constant} to change the rate between steps")
        if self.groups is None:
            if group is not None:
                raise ValueError("this optimizer was built without param_groups")
            self.lr = _sched.check_base(self.sched_config, lr)
        else:
            if group is None and len(self.groups) > 1:
                raise ValueError("this optimizer has %d parameter groups: say which, set_lr(lr, group=index or name) (groups: %s)"
                                 % (len(self.groups), [g["name"] for g in self.groups]))
            k = self._group_index(0 if group is None else group)
            lr = _pgroups._value(self.groups[k]["name"], "lr", lr)
            self._table_for(lr)
            self.groups[k]["lr"] = lr
            if k == 0:
                self.lr = lr
        self._write_table()

    def set_weight_decay(self, weight_decay, group=None):
        """a new weight decay for one parameter group, from the next step on (grouped optimizers: elsewhere the decay is a
        constant of the recorded step)"""
        if self.groups is None:
            raise ValueError("this optimizer was built without param_groups, its weight_decay is a constant of the (recorded) "
                             "step")
        if group is None and len(self.groups) > 1:
            raise ValueError("this optimizer has %d parameter groups: say which, set_weight_decay(x, group=index or name)"
                             % len(self.groups))
        k = self._group_index(0 if group is None else group)
        self.groups[k]["weight_decay"] = _pgroups._value(self.groups[k]["name"], "weight_decay", weight_decay)
        if k == 0:
            self.weight_decay = self.groups[k]["weight_decay"]
        self._write_table()

    def sched_state_dict(self):
        """configuration, current base rate(s) and clocks of the schedule / EMA (``checkpoint`` writes it beside the
        optimizer's)"""
        self.reconcile()
        sd = {"config": dict(self.sched_config), "base_lr": self.lr, "step": self.sched_step,
              "ema_decay": self.ema_decay, "ema_warmup": self.ema_warmup, "ema_updates": self.ema_updates}
        if self.groups is not None:
            sd["group_base_lrs"] = [g["lr"] for g in self.groups]
        return sd

    def load_sched_state_dict(self, sd):
        """After ``load_state_dict`` (it sets ``step_count``, which the offsets refer to).  The schedule continues at the saved
        step with the saved configuration and base rate; the EMA's decay stays this run's."""
        if self.sched_dev is None:
            raise ValueError("this optimizer was built without a schedule")
        self.sched_config = _sched.normalise(sd["config"])
        if self.groups is None:
            self.lr = _sched.check_base(self.sched_config, sd["base_lr"])
        elif "group_base_lrs" in sd:
            if len(sd["group_base_lrs"]) != len(self.groups):
                raise ValueError("the schedule state has %d group rates, this optimizer %d groups"
                                 % (len(sd["group_base_lrs"]), len(self.groups)))
            for g, lr in zip(self.groups, sd["group_base_lrs"]):
                g["lr"] = _pgroups._value(g["name"], "lr", lr)
            self.lr = self.groups[0]["lr"]
        self._sched_offset = int(sd["step"]) - self._step_count
        if self.ema is not None:
            self._ema_offset = int(sd.get("ema_updates", 0)) - self._step_count
        self._write_table()

    def restart_ema(self):
        """the EMA becomes a copy of the parameters as they are now, counted as its first update"""
        self.ema.copy_(self.flat.flat)
        self._ema_offset = 1 - self._step_count
        self._write_table()

    def zero_grad(self, set_to_none=False):
        self.flat.zero_grad()

    def step(self, grad_scale=1.0):
        self.sync_device_step()
        self._launch(grad_scale)
        self._advance()

    def state_dict(self):
        """The matching torch.optim layout with parameter indices in ``model.parameters()`` order -- the format this build
        reads and writes (``checkpoint.optimizer_state_dict``), interchangeable with the reference's
        ``optimizer.state_dict()`` / ``load_state_dict`` (train.py:149, 236)."""
        from . import checkpoint
        return checkpoint.optimizer_state_dict(self, None)

    def _refuse_mid_cycle(self, what):
        if self.micro_index != 0:
            raise ValueError("%s in the middle of an accumulation cycle (micro-step %d of %d): a partial cycle is not saved; "
                             "finish the cycle or drop it with reset_accumulation()"
                             % (what, self.micro_index, self.accum_steps))

    def load_state_dict(self, sd):
        """(with a schedule: the clocks keep their values relative to the loaded ``step_count``; ``load_sched_state_dict``
        sets them)"""
        from . import checkpoint
        checkpoint.load_optimizer_state_dict(self, None, sd)          # (starts a new accumulation cycle)


def _check_accum_steps(k):
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError("accum_steps must be an integer >= 1 (1 = no gradient accumulation), not %r" % (k,))
    return k


class FusedAdam(_FusedOptimizer):
    """Adam over a FlatParameters buffer (csrc/optim.hip); lr 1e-3, betas (0.9,0.999), eps 1e-8, wd 0 by
    default like the reference config (src/configs/hyp_train.yaml:7-9).  The step is ``ops.adam_step_dev``, with or without
    ``max_norm``: one kernel, whose clip coefficient is exactly 1 when clipping is off."""

    kind = "adam"

    def __init__(self, flat: FlatParameters, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None,
                 lr_schedule=None, ema_decay=None, ema_warmup=False, param_groups=None, skip_nonfinite=False, accum_steps=1):
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.exp_avg = torch.zeros_like(flat.flat)
        self.exp_avg_sq = torch.zeros_like(flat.flat)
        self._init_common(flat, max_norm, skip_nonfinite, accum_steps)
        self._init_sched(lr_schedule, ema_decay, ema_warmup, param_groups)

    def _launch(self, grad_scale):
        if self.accum_dev is not None:
            return ops.adam_step_accum_dev(self.flat.flat, self.flat.flat_grad, self.exp_avg, self.exp_avg_sq, self.step_dev,
                                           self.st_dev, lr=self.lr, betas=self.betas, eps=self.eps,
                                           weight_decay=self.weight_decay, grad_scale=grad_scale,
                                           decoupled=self.kind == "adamw", **self._accum_kw())
        if self.guard_dev is not None:
            return ops.adam_step_guard_dev(self.flat.flat, self.flat.flat_grad, self.exp_avg, self.exp_avg_sq, self.step_dev,
                                           self.st_dev, self.guard_dev, self.clip_partials, self.lr, self.betas, self.eps,
                                           self.weight_decay, grad_scale, self.max_norm, self.kind == "adamw", self.sched_dev,
                                           self.sched_out, self.ema, self.groups_dev, self.groups_out, self.group_map)
        if self.groups is not None:
            return ops.adam_step_groups_dev(self.flat.flat, self.flat.flat_grad, self.exp_avg, self.exp_avg_sq, self.step_dev,
                                            self.st_dev, self.sched_dev, self.sched_out, self.groups_dev, self.groups_out,
                                            self.group_map, self.ema, self.betas, self.eps, grad_scale, self.clip_partials,
                                            self.max_norm, decoupled=self.kind == "adamw")
        if self.sched_dev is not None:
            return ops.adam_step_sched_dev(self.flat.flat, self.flat.flat_grad, self.exp_avg, self.exp_avg_sq, self.step_dev,
                                           self.st_dev, self.sched_dev, self.sched_out, self.ema, self.betas, self.eps,
                                           self.weight_decay, grad_scale, self.clip_partials, self.max_norm,
                                           decoupled=self.kind == "adamw")
        ops.adam_step_dev(self.flat.flat, self.flat.flat_grad, self.exp_avg, self.exp_avg_sq, self.step_dev, self.st_dev,
                          self.lr, self.betas, self.eps, self.weight_decay, grad_scale, self.clip_partials, self.max_norm,
                          decoupled=self.kind == "adamw")


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW (decoupled weight decay, default 1e-2 like torch) over a FlatParameters buffer: Adam's state and
    checkpoint layout, the group carrying ``decoupled_weight_decay: True``."""

    kind = "adamw"

    def __init__(self, flat: FlatParameters, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None,
                 lr_schedule=None, ema_decay=None, ema_warmup=False, param_groups=None, skip_nonfinite=False, accum_steps=1):
        super().__init__(flat, lr, betas, eps, weight_decay, max_norm, lr_schedule, ema_decay, ema_warmup, param_groups,
                         skip_nonfinite, accum_steps)


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD over a FlatParameters buffer: weight_decay, momentum, dampening, nesterov.  With ``momentum == 0`` (the
    reference's own call, ``optim.SGD(lr=..., weight_decay=...)``) no buffer is allocated or touched.  With momentum the first
    step after construction -- or after loading a state without buffers -- sets ``momentum_buffer`` to the gradient (no
    dampening), as torch does; "first" is ``step_count == 0``, decided on the device from the step counter.  torch's SGD state
    holds no step count, so after loading a state WITH buffers ``step_count`` restarts at 1: it counts the steps since
    construction or load, and only whether it is zero matters."""

    kind = "sgd"

    def __init__(self, flat: FlatParameters, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                 max_norm=None, lr_schedule=None, ema_decay=None, ema_warmup=False, param_groups=None, skip_nonfinite=False,
                 accum_steps=1):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self._init_common(flat, max_norm, skip_nonfinite, accum_steps)
        self.lr, self.momentum, self.dampening, self.weight_decay = lr, momentum, dampening, weight_decay
        self.nesterov = bool(nesterov)
        self.momentum_buffer = torch.zeros_like(flat.flat) if momentum != 0 else None
        self._init_sched(lr_schedule, ema_decay, ema_warmup, param_groups)

    @property
    def first_step(self):
        """the next step initialises the momentum buffer instead of updating it"""
        return self._step_count == 0

    def _launch(self, grad_scale):
        if self.accum_dev is not None:
            return ops.sgd_step_accum_dev(self.flat.flat, self.flat.flat_grad, self.momentum_buffer, self.step_dev, self.st_dev,
                                          lr=self.lr, weight_decay=self.weight_decay, momentum=self.momentum,
                                          dampening=self.dampening, nesterov=self.nesterov, grad_scale=grad_scale,
                                          **self._accum_kw())
        if self.guard_dev is not None:
            return ops.sgd_step_guard_dev(self.flat.flat, self.flat.flat_grad, self.momentum_buffer, self.step_dev, self.st_dev,
                                          self.guard_dev, self.clip_partials, self.lr, self.weight_decay, self.momentum,
                                          self.dampening, self.nesterov, grad_scale, self.max_norm, self.sched_dev,
                                          self.sched_out, self.ema, self.groups_dev, self.groups_out, self.group_map)
        if self.groups is not None:
            return ops.sgd_step_groups_dev(self.flat.flat, self.flat.flat_grad, self.momentum_buffer, self.step_dev, self.st_dev,
                                           self.sched_dev, self.sched_out, self.groups_dev, self.groups_out, self.group_map,
                                           self.ema, self.momentum, self.dampening, self.nesterov, grad_scale,
                                           self.clip_partials, self.max_norm)
        if self.sched_dev is not None:
            return ops.sgd_step_sched_dev(self.flat.flat, self.flat.flat_grad, self.momentum_buffer, self.step_dev, self.st_dev,
                                          self.sched_dev, self.sched_out, self.ema, self.weight_decay, self.momentum,
                                          self.dampening, self.nesterov, grad_scale, self.clip_partials, self.max_norm)
        ops.sgd_step_dev(self.flat.flat, self.flat.flat_grad, self.momentum_buffer, self.step_dev, self.st_dev, self.lr,
                         self.weight_decay, self.momentum, self.dampening, self.nesterov, grad_scale, self.clip_partials,
                         self.max_norm)


def get_optimizers(params: dict, flat: FlatParameters):
    """reference train.py:29-37: ``optim`` 'Adam' | 'AdamW' | 'SGD' with ``lr`` / ``weight_decay``.  Optional keys of
    ``train_config``: ``momentum``, ``dampening``, ``nesterov`` (SGD; the reference passes none of them) and ``clip_grad_norm``
    (the max_norm of the reference's ``clip_grad_norm_`` line, train.py:54; absent or None = off); ``lr_schedule`` (a dict
    ``{name: constant | step | multistep | exponential | cosine, every, warmup_steps, warmup_start_factor, ...}``, see
    ``lr_schedule.py``; absent = the rate is a constant of the step), ``ema_decay`` (absent = no averaged weights) and
    ``ema_warmup`` (default false); ``param_groups`` (a list of at most 15 entries ``{name, match, ndim_max, lr,
    weight_decay}``, see ``param_groups.py``; absent or empty = one rate and one decay for all parameters);
    ``skip_nonfinite`` (default false: today's step; true: a step whose gradient is not finite is skipped on the device, see
    ``_FusedOptimizer``) and ``skip_nonfinite_patience`` (default 10, None = off: the epoch loops raise FloatingPointError
    when an epoch ends in that many consecutive skipped steps); ``accum_steps`` (an integer >= 1, default 1 = off: gradient
    accumulation, one optimizer step per that many calls of ``step``, see ``_FusedOptimizer``)."""
    tc = params["train_config"]
    name = tc.get("optim", "Adam")
    if name not in ("Adam", "AdamW", "SGD"):
        raise NotImplementedError(name)
    clip = tc.get("clip_grad_norm")
    extra = {"lr_schedule": tc.get("lr_schedule"), "ema_decay": tc.get("ema_decay"), "ema_warmup": tc.get("ema_warmup", False)}
    lr, wd = tc.get("lr", 1e-3), tc.get("weight_decay", 1e-2 if name == "AdamW" else 0.0)
    groups = _pgroups.resolve(tc.get("param_groups"), flat, lr, wd)
    if groups is not None:
        extra["param_groups"] = groups
    if tc.get("skip_nonfinite", False):
        extra["skip_nonfinite"] = True
    if _check_accum_steps(tc.get("accum_steps", 1)) > 1:
        extra["accum_steps"] = tc["accum_steps"]
    if name == "Adam":
        return FusedAdam(flat, lr=lr, weight_decay=wd, max_norm=clip, **extra)
    if name == "AdamW":
        return FusedAdamW(flat, lr=lr, weight_decay=wd, max_norm=clip, **extra)
    if name == "SGD":
        return FusedSGD(flat, lr=lr, weight_decay=wd,
                        momentum=tc.get("momentum", 0.0), dampening=tc.get("dampening", 0.0),
                        nesterov=tc.get("nesterov", False), max_norm=clip, **extra)
    raise NotImplementedError(name)


class TrainStep:
    """One data-parallel optimisation step on raw audio.

    step(audio (B, n_samples, 4) float32 on the GPU, target (M,7), spec_ranges=None) -> loss tensor (1,) on the device (no
    host sync).  spec_ranges: SpecAug tables int32 (B, 2, 4) (``FoaDataset`` items with ``spec_augment`` on) or the (B, 4, 4) tables
    of the frequency-shift / cutout augmentation (``aug_config.freq_shift_augment`` / ``cutout_augment``), handed to the
    feature extractor, which masks its output in the same call; None leaves the step exactly as without SpecAug (the
    feature callable is then called without the keyword).

    graph=True (default: the ADYOLO_GRAPH environment variable, off when unset): the whole step is recorded ONCE per input
    shape in a hipGraph and replayed (``graph.StepGraphs``) -- ~770 kernel launches per step leave the Python / ctypes /
    autograd path, which is what bounds the reference's own shapes (16 x 20 s chunks: the GPU work of a step is shorter than
    its launch sequence).  The first step at a new shape runs eagerly, the second is captured; results are bit-identical to
    the eager path.  Single-process only (under data parallelism the RCCL hooks stay eager).

    Gradient clipping (``train_config['clip_grad_norm']``) belongs to the optimizer: it acts on the REDUCED gradients times the
    ``grad_scale`` handed to ``optimizer.step`` (i.e. on the gradient the update uses).  Under data parallelism every rank holds
    the same reduced buffer and the norm is summed in a fixed order, so every rank derives the same coefficient, bit for bit,
    with no extra collective.  ``trainer.optimizer.grad_norm`` holds the pre-clip norm of the last step on the device.
    """

    def __init__(self, model, criterion, feature_extractor, params=None, n_buckets=4, lr=1e-3, graph=None, exact=None):
        self.model, self.criterion, self.features = model, criterion, feature_extractor
        self.flat = FlatParameters(model)
        self.flat.broadcast(0)                   # no-op on one rank: all ranks start from rank 0's parameters / buffers
        self.optimizer = get_optimizers(params, self.flat) if params is not None else FusedAdam(self.flat, lr=lr)
        self.reducer = BucketedAllReduce(self.flat, n_buckets=n_buckets)
        # exact=True (default: ADYOLO_DP_EXACT=1): batch statistics and loss normalisers over the batch of ALL ranks
        # (ops.ExactDP) -- N ranks on N equal shards == one device on the concatenated batch; gradients are summed
        self.exact = (os.environ.get("ADYOLO_DP_EXACT", "0") == "1") if exact is None else bool(exact)
        if graph is None:
            graph = os.environ.get("ADYOLO_GRAPH", "0") == "1"
        self.graphs = None
        if graph and not self.reducer.active:
            from .graph import StepGraphs
            self.graphs = StepGraphs(self)

    def step(self, audio, target, spec_ranges=None):
        if self.graphs is not None:
            return self.graphs.step(audio, target, spec_ranges)
        return self.step_eager(audio, target, spec_ranges)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the model's parameters are the optimizer's EMA (``train_config['ema_decay']``): the flat
        parameter buffer is stashed, overwritten with the averaged weights (device copies) and put back on exit, with
        ``ops.params_changed()`` both times so that cached weight packs and transformed filters are rebuilt.  Parameters keep
        their addresses, so evaluation code (``test_epoch_audio``, ``graph.ForwardGraphs``) runs unchanged.  BatchNorm running
        statistics are buffers, not parameters: inside the context they are the LIVE model's, they are not averaged.  Before
        the first optimizer step the EMA is the live weights.  Take no train step inside the context."""
        opt = self.optimizer
        if getattr(opt, "ema", None) is None:
            raise ValueError("no averaged weights: the optimizer was built without train_config['ema_decay']")
        if opt.ema_updates <= 0:
            yield
            return
        if getattr(self, "_ema_stash", None) is None:
            self._ema_stash = torch.empty_like(self.flat.flat)
        self._ema_stash.copy_(self.flat.flat)
        self.flat.flat.copy_(opt.ema)
        ops.params_changed()
        try:
            yield
        finally:
            self.flat.flat.copy_(self._ema_stash)
            ops.params_changed()

    def step_eager(self, audio, target, spec_ranges=None):
        self.model.train()
        exact = self.exact and ops.EXACT.enable(self.reducer.group)
        try:
            if spec_ranges is None:
                feat = self.features(audio, channels_last8=True)
            else:
                feat = self.features(audio, channels_last8=True, spec_ranges=spec_ranges)
            output = self.model(feat, channels_last8=True)
            self.optimizer.zero_grad()
            loss = self.criterion(output, target)
            Fn.SINK.begin(self.flat, self.reducer)       # weight / BatchNorm / SE gradients go straight into the flat buffer
            try:
                loss.backward()
            finally:
                Fn.SINK.end()
        finally:
            ops.EXACT.disable()
        scale = self.reducer.finish()
        # exact + AD-YOLO: the loss kernel normalises by the counts of ALL ranks, so the ranks' gradients ADD UP to the batch's.
        # The class-wise losses (seddoa / masked-seddoa / accdoa / adpit: means over the local rows, ops.*_loss) keep their
        # local normaliser: with equal shards the batch mean is the mean of the ranks' means, i.e. gradients are AVERAGED and
        # the reported loss is the ranks' average (round 4, ADVICE: they used to be summed -- world times too large)
        summed = exact and getattr(self.criterion, "loss_nm", "adyolo") == "adyolo"
        self.optimizer.step(grad_scale=1.0 if summed else scale)
        if exact and not summed:
            loss = ops.EXACT_world_mean(loss.detach().clone(), self.reducer.group)
        return loss.detach()


def train_one_epoch(params: dict, dataloader, model, optimizer, criterion, device):
    """Mirror of ``train_one_epoch`` (/root/reference/src/train.py:40-62) for loaders that yield pre-computed features:
    ``for feat (B,7,T,64), label in dataloader`` -> forward, zero_grad, loss, backward, step; returns the mean loss.
    Works with a ``torch.optim`` optimizer or ``FusedAdam`` / ``FusedAdamW`` / ``FusedSGD`` (``TrainStep`` is the faster raw-audio +
    flat-buffer path).
    The per-step ``loss.item()`` of the reference (a device sync every iteration, train.py:57) is replaced by one
    device-side accumulation and a single sync at the end of the epoch."""
    model.train()
    total = None
    n = 0
    for i, (feat, label) in enumerate(dataloader):
        feat = feat.to(device).float()
        output = model(feat)
        optimizer.zero_grad()
        loss = criterion(output, label)
        loss.backward()
        optimizer.step()
        total = loss.detach().reshape(-1)[:1].clone() if total is None else total + loss.detach().reshape(-1)[:1]
        n = i + 1
        if params.get("args", {}).get("quick_test") and i == 4:
            break
    return float(total) / max(n, 1) if total is not None else 0.0


class _EpochLoss:
    """The running loss of the raw-audio epoch loops, kept on the device and read ONCE at the end of the epoch.

    Without the non-finite guard (``train_config['skip_nonfinite']``): the sum of the steps' losses over their number.  With
    it: a step's loss counts only when the step was applied -- chosen by ``torch.where`` on the flag of the optimizer's guard
    record (a multiply would not do: NaN * 0 is NaN) -- the applied steps are counted on the device, the mean is over them,
    and the record comes to the host in the same read, where the optimizer reconciles its ``step_count`` with it.  An epoch
    that ENDS in ``train_config['skip_nonfinite_patience']`` (default 10; None = never) or more consecutive skipped steps
    raises FloatingPointError: a model whose weights are already not finite would otherwise skip for ever in silence.

    Under gradient accumulation (``train_config['accum_steps']``) every call of ``add`` is a micro-step.  Without the guard
    nothing changes: the mean over all micro-steps.  With it the guard's flag speaks for a whole cycle and only after the
    cycle's last micro-step, so the micro losses wait in a pending sum that is folded in, by the same ``torch.where``, when the
    cycle ends: the mean is over the micro-steps of the applied cycles.  ``drop_partial_cycle()`` ends an epoch that stops
    inside a cycle: the optimizer's accumulation is reset and the pending losses are dropped with it."""

    def __init__(self, params, trainer):
        self.optimizer = getattr(trainer, "optimizer", None)
        self.guard = getattr(self.optimizer, "guard_dev", None)
        self.cycles = self.guard is not None and getattr(self.optimizer, "accum_steps", 1) > 1
        self.patience = params.get("train_config", {}).get("skip_nonfinite_patience", 10)
        self.total = self.applied = self.pending = None
        self.n = self.n_pending = 0

    def add(self, loss):
        loss = loss.detach().reshape(-1)[:1]
        self.n += 1
        if self.guard is not None:
            count = 1
            if self.cycles:
                self.pending = loss.clone() if self.pending is None else self.pending + loss
                self.n_pending += 1
                if self.optimizer.micro_index != 0:           # the cycle goes on: the flag still speaks for the last one
                    return
                loss, count, self.pending, self.n_pending = self.pending, self.n_pending, None, 0
            ok = self.guard[2:3] == 0
            loss = torch.where(ok, loss, torch.zeros_like(loss))
            ok_n = ok.to(torch.int64) if count == 1 else ok * count
            self.applied = ok_n if self.applied is None else self.applied + ok_n
        self.total = loss.clone() if self.total is None else self.total + loss

    def drop_partial_cycle(self):
        if getattr(self.optimizer, "micro_index", 0) != 0:
            self.optimizer.reset_accumulation()
        self.pending, self.n_pending = None, 0

    def mean(self, *also):
        """-> (the mean loss, host copies of ``also``) with one device read"""
        if self.total is None and self.n == 0:
            return 0.0, list(also)
        if self.total is None:                                # (guarded accumulation: no cycle of this epoch came to its end)
            self.total, self.applied = torch.zeros_like(self.guard[:1], dtype=torch.float32), self.guard[:1] * 0
        mine = (self.total,) if self.guard is None else (self.total, self.applied, self.guard)
        host = ops.to_host_many(*mine, *also) if self.total.is_cuda else [t.clone() for t in mine + also]
        if self.guard is None:
            return float(host[0][0]) / max(self.n, 1), host[1:]
        total, applied, rec = float(host[0][0]), int(host[1][0]), self.optimizer.reconcile(host[2])
        if self.patience is not None and rec["run"] >= int(self.patience):
            raise FloatingPointError("the epoch ended in %d consecutive optimizer steps skipped for a non-finite gradient "
                                     "(skip_nonfinite_patience %d): %d of this epoch's %d steps were applied; %d of %d attempts "
                                     "skipped since the start" % (rec["run"], int(self.patience), applied, self.n,
                                                                  rec["skipped"], rec["attempts"]))
        return total / max(applied, 1), host[3:]


def train_one_epoch_audio(params: dict, dataloader, trainer, stager=None, rotate=True):
    """The raw-audio epoch: ``dataloader`` yields ``audio_collate_fn`` batches (pcm int16 (B,T,4), comb_nos, target[, SpecAug
    tables (B,2,4), or (B,4,4) with the frequency-shift / cutout rows]); each is staged to the GPU (int16 over PCIe on a side stream, double-buffered), converted, rotated (with
    ``aug_config.channel_swap_augment``: its channels permuted, ``swap_audio``; with ``aug_config.yaw_rotation_augment``: rotated
    and yawed by ``rotate_audio_yaw``, the batch's second element then holding (combination, yaw) pairs; with
    ``aug_config.time_mix_augment``: the batch's
    trailing dict of mates staged, moved by their own combinations and summed in by ``ops.audio_mix``) and handed with its
    tables to ``TrainStep.step``
    (features [+ SpecAug masks] + forward + loss + backward [+ all-reduce] + Adam).  Returns the mean loss with ONE device sync
    at the end of the epoch (the reference syncs every iteration, train.py:57); with ``train_config['skip_nonfinite']`` the
    mean over the APPLIED steps (``_EpochLoss``).  With ``train_config['accum_steps']`` every batch is a micro-step; an epoch whose number of batches is no multiple of it (or that
    ``quick_test`` cuts short) ends inside a cycle, and that partial cycle is DROPPED: its gradients take part in no step."""
    from .augmentations import channel_swap_enabled, rotate_audio, rotate_audio_yaw, swap_audio
    from .datasets import AudioStager
    move_audio = swap_audio if channel_swap_enabled(params) else rotate_audio     # MIC channel swap | FOA rotation

    def yawed(combs):
        """``aug_config.yaw_rotation_augment``: the batch carries (combination, yaw) pairs -> (combinations, yaws), else None."""
        if len(combs) and isinstance(combs[0], tuple):
            return [c for c, _ in combs], [p for _, p in combs]
        return None

    def split(rest):
        """The optional tail of a batch -> (SpecAug tables or None, mixing dict or None), told apart by type."""
        spec = [r for r in rest if isinstance(r, torch.Tensor)]
        mix = [r for r in rest if isinstance(r, dict)]
        return (spec[0] if spec else None), (mix[0] if mix else None)
    acc, n = _EpochLoss(params, trainer), 0
    it = iter(dataloader)
    try:
        pcm, combs, target, *rest = next(it)
    except StopIteration:
        return 0.0
    spec, mix = split(rest)
    device = trainer.flat.flat.device
    if stager is None:
        stager = AudioStager(pcm.shape[0], pcm.shape[1], device)
    stager.stage(pcm)
    mate_stager = None
    if mix is not None:                           # time-domain mixing: the mates cross PCIe through a stager of their own
        mate_stager = AudioStager(pcm.shape[0], pcm.shape[1], device)
        mate_stager.stage(mix["mate_pcm"])
    while True:
        audio = stager.get()
        mate = mate_stager.get() if mate_stager is not None else None
        cur_combs, cur_target, cur_spec, cur_mix = combs, target, spec, mix
        nxt = next(it, None)
        if nxt is not None:                       # the next batch crosses PCIe while this step runs
            pcm, combs, target, *rest = nxt
            spec, mix = split(rest)
            stager.stage(pcm)
            if mate_stager is not None:
                mate_stager.stage(mix["mate_pcm"])
        pairs = yawed(cur_combs)
        if pairs is not None:                     # FOA rotation, then the yaw, in one pass
            if rotate:
                audio = rotate_audio_yaw(audio, *pairs)
        elif rotate and any(int(c) != 0 for c in cur_combs):
            audio = move_audio(audio, cur_combs)
        if cur_mix is not None:                   # each side under its own combinations, then audio + gain * mate
            if "mate_yaws" in cur_mix:
                if rotate:
                    mate = rotate_audio_yaw(mate, cur_mix["mate_combs"], cur_mix["mate_yaws"])
            elif rotate and any(int(c) != 0 for c in cur_mix["mate_combs"]):
                mate = move_audio(mate, cur_mix["mate_combs"])
            audio = ops.audio_mix(audio, mate, cur_mix["gains"].to(device), cur_mix["mixed"].to(device), out=audio)
        acc.add(trainer.step(audio, cur_target, cur_spec))
        n += 1
        if nxt is None or (params.get("args", {}).get("quick_test") and n == 5):
            break
    acc.drop_partial_cycle()
    return acc.mean()[0]


def train_one_epoch_corpus(params: dict, corpus, trainer):
    """``train_one_epoch_audio`` on a ``corpus.DeviceCorpus`` or ``corpus.ClasswiseDeviceCorpus``: batches of ``batch_size`` over
    ``corpus.get_filelist()`` in order, each made on the device (gather + rotation of the audio; AD-YOLO rows into the
    fixed-capacity target, or the dense class-wise target) and handed with its SpecAug tables to ``TrainStep.step``.  With
    ``trainer.graphs`` the kernels write straight into the recorded step's input buffers (of ``corpus.target_shape``) once it
    exists (eager launches before the replay, no copy).  The host draws of batch k+1 (rotation, SpecAug) happen while step k
    runs, in the order the host path draws them.  Returns the mean loss with ONE device sync at the end, where the corpus' status
    word is read too: a batch with more rows than the capacity, an item outside the corpus or a class outside the model's
    raises.  With ``train_config['skip_nonfinite']``: the mean over the APPLIED steps, the guard record in the same read
    (``_EpochLoss``).  With ``train_config['accum_steps']``: micro-steps, and a partial cycle at the end of the epoch is dropped,
    as in ``train_one_epoch_audio``."""
    bs = int(params["train_config"]["batch_size"])
    files = corpus.get_filelist()
    starts = list(range(0, len(files), bs))
    if not starts:
        return 0.0
    graphs = trainer.graphs
    corpus.reset_status()
    acc, n = _EpochLoss(params, trainer), 0
    nxt = corpus.draw(range(starts[0], min(len(files), starts[0] + bs)))
    for k in range(len(starts)):
        drawn = nxt
        items, spec = drawn[0], drawn[1]          # a third element (mates: time-domain mixing) goes through to launch
        bufs = None
        if graphs is not None:
            target_like = torch.empty(corpus.target_shape(items.shape[0]), dtype=torch.float32, device="meta")
            bufs = graphs.static_inputs((items.shape[0], corpus.n_samples, 4), target_like,
                                        None if spec is None else tuple(spec.shape))
        audio, target, spec_dev = corpus.launch(drawn, *(bufs or ()))
        acc.add(trainer.step(audio, target, spec_dev))
        n += 1
        nxt = None
        if k + 1 < len(starts):                   # the next batch's host draws while this step runs
            nxt = corpus.draw(range(starts[k + 1], min(len(files), starts[k + 1] + bs)))
        if nxt is None or (params.get("args", {}).get("quick_test") and n == 5):
            break
    acc.drop_partial_cycle()
    mean, (status,) = acc.mean(corpus.status)
    corpus.check(int(status[0]))
    return mean
