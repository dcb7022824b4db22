"""CPU: the host side of gradient accumulation (``train_config['accum_steps']``): what ``get_optimizers`` allocates, how the
host's mirrors (``micro_index``, ``step_count`` and what follows from it) move with the calls, ``reset_accumulation``, the
refusal of a mid-cycle ``state_dict``, the interplay with the non-finite guard's ``reconcile`` and the epoch loops' folding of
micro losses.  No HIP call is made: optimizers live on CPU tensors (the pattern of test_nonfinite_guard_cpu), records are
written by hand and the epoch loops run a stub trainer that moves the records as the device would."""
import pytest
import torch

import adyolo_amd  # noqa: F401  (import shim at the repo root)


def _params(**train_config):
    tc = {"optim": "Adam", "lr": 1e-3, "weight_decay": 0.0, "batch_size": 2}
    tc.update(train_config)
    return {"args": {"device": "cpu"}, "train_config": tc}


def _small_flat(seed=5):
    from adyolo_amd.dist import FlatParameters
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))      # 26 parameters, padded to 28
    return net, FlatParameters(net)


SCHED = {"lr_schedule": {"name": "cosine", "T_max": 10, "warmup_steps": 3}, "ema_decay": 0.9, "ema_warmup": True}


def _calls(opt, k):
    """what k calls of the step's launches do to the host's mirrors"""
    for _ in range(k):
        opt.replayed()


# ------------------------------------------------------------------------------------------------ construction
@pytest.mark.parametrize("name", ["Adam", "AdamW", "SGD"])
def test_get_optimizers_allocates_the_accumulator_only_when_asked(name):
    """``accum_steps: 3`` allocates an accumulator like ``flat.flat_grad`` and the record; an absent key and 1 leave every
    attribute as it was: nothing allocated, and the same set of instance attributes as an optimizer built without the key."""
    from adyolo_amd import ops
    from adyolo_amd.train import get_optimizers
    _, flat = _small_flat()
    o = get_optimizers(_params(optim=name, accum_steps=3), flat)
    assert o.accum_steps == 3 and o.micro_index == 0 and o.step_count == 0
    assert o.accum.shape == flat.flat_grad.shape and o.accum.dtype == torch.float32
    assert o.accum.data_ptr() != flat.flat_grad.data_ptr() and not bool(o.accum.any())
    assert o.accum_dev.dtype == torch.int64 and o.accum_dev.tolist() == [0] * ops.OPTIM_ACCUM_WORDS
    assert o.guard_dev is None and o.clip_partials is None
    absent = get_optimizers(_params(optim=name), flat)
    one = get_optimizers(_params(optim=name, accum_steps=1), flat)
    for off in (absent, one):
        assert off.accum_steps == 1 and off.accum is None and off.accum_dev is None and off.micro_index == 0
    assert sorted(vars(absent)) == sorted(vars(one))
    assert "accum" not in vars(absent) and "accum_dev" not in vars(absent)
    both = get_optimizers(_params(optim=name, accum_steps=2, skip_nonfinite=True, clip_grad_norm=1.0), flat)
    assert both.accum_dev is not None and both.guard_dev is not None and both.clip_partials is not None


def test_accum_symbols_are_exported_and_bound():
    from adyolo_amd import _lib, ops
    lib = _lib.load()
    assert int(lib.adyolo_optim_accum_words()) == ops.OPTIM_ACCUM_WORDS == 4
    for name in ("adyolo_optim_accum_words", "adyolo_adam_step_accum_dev", "adyolo_sgd_step_accum_dev"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert callable(ops.adam_step_accum_dev) and callable(ops.sgd_step_accum_dev)
    guard, accum = _lib.SIGNATURES["adyolo_adam_step_guard_dev"][1], _lib.SIGNATURES["adyolo_adam_step_accum_dev"][1]
    assert accum == guard[:-1] + [_lib.P, _lib.P, _lib.I] + guard[-1:]           # the guarded list + accum, record, K
    guard, accum = _lib.SIGNATURES["adyolo_sgd_step_guard_dev"][1], _lib.SIGNATURES["adyolo_sgd_step_accum_dev"][1]
    assert accum == guard[:-1] + [_lib.P, _lib.P, _lib.I] + guard[-1:]


@pytest.mark.parametrize("bad", [0, -2, 2.0, 2.5, "2", True, None])
def test_get_optimizers_refuses_bad_values(bad):
    from adyolo_amd.train import FusedSGD, get_optimizers
    _, flat = _small_flat()
    with pytest.raises(ValueError, match="accum_steps"):
        get_optimizers(_params(accum_steps=bad), flat)
    with pytest.raises(ValueError, match="accum_steps"):
        FusedSGD(flat, accum_steps=bad)


# ------------------------------------------------------------------------------------------------ the host's mirrors
@pytest.mark.parametrize("via", ["replayed", "advance"])
def test_seven_calls_at_three_are_two_steps_and_one_micro_step(via):
    """``step_count`` advances on a cycle's last call only, and the schedule's clock and the EMA's count follow it; the
    mirror of the device counter's value follows too, so ``sync_device_step`` has nothing to write."""
    from adyolo_amd.train import FusedAdam
    _, flat = _small_flat()
    opt = FusedAdam(flat, accum_steps=3, **SCHED)
    seen = []
    for _ in range(7):
        opt.replayed() if via == "replayed" else opt._advance()
        seen.append((opt.micro_index, opt.step_count))
    assert seen == [(1, 0), (2, 0), (0, 1), (1, 1), (2, 1), (0, 2), (1, 2)]
    assert (opt.step_count, opt.micro_index, opt.sched_step, opt.ema_updates, opt._dev_step_value) == (2, 1, 2, 2, 2)
    assert opt.lr_at(opt.sched_step) == opt.lr_at(2) != opt.lr_at(7)
    opt.step_dev.fill_(-1)
    opt.sync_device_step()
    assert int(opt.step_dev) == -1


def test_hold_calls_leave_the_parameter_epoch_alone():
    """a hold call changes no parameter: the caches keyed on ``ops.PARAMS_EPOCH`` expire on a cycle's last call only"""
    from adyolo_amd import ops
    from adyolo_amd.train import FusedSGD
    _, flat = _small_flat()
    opt = FusedSGD(flat, accum_steps=2)
    e0 = ops.PARAMS_EPOCH[0]
    opt.replayed()
    assert ops.PARAMS_EPOCH[0] == e0
    opt.replayed()
    assert ops.PARAMS_EPOCH[0] == e0 + 1


def test_reset_accumulation_writes_index_zero_to_record_and_mirror():
    from adyolo_amd.train import FusedAdam
    _, flat = _small_flat()
    opt = FusedAdam(flat, accum_steps=3)
    _calls(opt, 4)
    opt.accum_dev.copy_(torch.tensor([1, 4, 1, 1]))                               # the record as the device leaves it after 4 calls
    opt.accum.fill_(float("nan"))
    opt.reset_accumulation()
    assert opt.micro_index == 0 and opt.step_count == 1
    assert opt.accum_dev.tolist() == [0, 4, 1, 1]                                 # the index alone: the counts are the device's
    _calls(opt, 3)                                                                # a whole new cycle
    assert (opt.micro_index, opt.step_count) == (0, 2)
    off = FusedAdam(flat)
    off.reset_accumulation()                                                      # nothing to do, nothing allocated
    assert off.micro_index == 0 and off.accum_dev is None


def test_state_dict_and_checkpoint_refuse_a_mid_cycle_state_and_loading_resets(tmp_path):
    from adyolo_amd import checkpoint as ck
    from adyolo_amd.train import get_optimizers
    net, flat = _small_flat()
    opt = get_optimizers(_params(accum_steps=3, **SCHED), flat)
    _calls(opt, 3)
    sd = opt.state_dict()                                                         # a cycle boundary: fine
    assert all(float(s["step"]) == 1.0 for s in sd["state"].values())
    path = str(tmp_path / "model_ckpt.h5")
    ck.save_checkpoint(path, net, opt, 1, 0.5, {}, [], "cpu")
    _calls(opt, 1)
    with pytest.raises(ValueError, match="middle of an accumulation cycle.*micro-step 1 of 3"):
        opt.state_dict()
    with pytest.raises(ValueError, match="accumulation cycle"):
        ck.save_checkpoint(str(tmp_path / "mid.h5"), net, opt, 1, 0.5, {}, [], "cpu")
    with pytest.raises(ValueError, match="accumulation cycle"):
        ck.save_best(str(tmp_path / "best.h5"), net, opt, 1, 0.5)
    opt.accum_dev[0] = 1
    opt.load_state_dict(sd)                                                       # starts a new cycle
    assert opt.micro_index == 0 and int(opt.accum_dev[0]) == 0 and opt.step_count == 1
    opt.state_dict()
    net2, flat2 = _small_flat(seed=6)
    fresh = get_optimizers(_params(accum_steps=3, **SCHED), flat2)
    _calls(fresh, 2)
    fresh.accum_dev[0] = 2
    ck.load_checkpoint(path, net2, fresh, restore_rng=False)
    assert (fresh.micro_index, int(fresh.accum_dev[0]), fresh.step_count, fresh.sched_step) == (0, 0, 1, 1)
    net3, flat3 = _small_flat(seed=7)
    plain = get_optimizers(_params(**SCHED), flat3)                               # the file is an ordinary one
    ck.load_checkpoint(path, net3, plain, restore_rng=False)
    assert plain.step_count == 1 and plain.accum_dev is None


# ------------------------------------------------------------------------------------------------ with the guard
def test_reconcile_counts_cycles_as_attempts():
    """Twelve calls at K = 3 are four attempts; a hand-written guard record that says one of them was skipped takes one off
    ``step_count`` -- once -- and leaves the micro mirror alone.  A hold call does not mark the record as moved."""
    from adyolo_amd.train import FusedAdam
    _, flat = _small_flat()
    opt = FusedAdam(flat, skip_nonfinite=True, accum_steps=3, **SCHED)
    _calls(opt, 2)
    assert opt._guard_dirty is False                                              # hold calls: the guard's record has not moved
    _calls(opt, 10)
    assert opt._guard_dirty is True and (opt.step_count, opt.micro_index) == (4, 0)
    rec = torch.tensor([4, 1, 0, 0], dtype=torch.int64)
    assert opt.reconcile(rec) == {"attempts": 4, "skipped": 1, "last_skipped": False, "run": 0}
    assert (opt.step_count, opt._dev_step_value, opt.sched_step, opt.ema_updates, opt.micro_index) == (3, 3, 3, 3, 0)
    assert opt.reconcile(rec)["skipped"] == 1 and opt.step_count == 3
    _calls(opt, 2)                                                                # mid-cycle: nothing new to reconcile
    opt.guard_dev.copy_(torch.tensor([9, 9, 1, 9]))
    assert opt.reconcile()["attempts"] == 4 and (opt.step_count, opt.micro_index) == (3, 2)
    _calls(opt, 1)
    opt.guard_dev.copy_(torch.tensor([5, 2, 1, 1]))
    assert opt.reconcile() == {"attempts": 5, "skipped": 2, "last_skipped": True, "run": 1} and opt.step_count == 3


# ------------------------------------------------------------------------------------------------ epoch loops
class _StubTrainer:
    """``step`` returns the scripted loss (None: NaN, a poisoned micro-batch) and moves the accumulation record, the guard
    record and the host's mirrors as an accumulating optimizer step does: a cycle with a poisoned micro-batch is a skipped
    attempt, decided on its last call."""
    graphs = None

    def __init__(self, script, **tc):
        from adyolo_amd.train import get_optimizers
        _, self.flat = _small_flat()
        self.optimizer = get_optimizers(_params(**tc), self.flat)
        self.script, self.calls, self.poisoned = list(script), 0, False

    def step(self, audio, target, spec=None):
        loss = self.script[self.calls]
        self.calls += 1
        opt = self.optimizer
        k, a, g = opt.accum_steps, opt.accum_dev, opt.guard_dev
        self.poisoned = (self.poisoned and opt.micro_index != 0) or loss is None
        last = opt.micro_index == k - 1
        if a is not None:
            a[0], a[1], a[2], a[3] = (0 if last else int(a[0]) + 1), int(a[1]) + 1, int(a[2]) + int(last), int(not last)
        if g is not None and last:
            skip = self.poisoned
            g[0] += 1
            g[1] += int(skip)
            g[2] = int(skip)
            g[3] = int(g[3]) + 1 if skip else 0
        opt.replayed()
        return torch.tensor([float("nan") if loss is None else loss])


class _StubStager:
    def stage(self, pcm):
        self.pcm = pcm

    def get(self):
        return self.pcm


class _StubCorpus:
    n_samples = 8

    def __init__(self, n_files):
        self.files, self.status, self.checked = list(range(n_files)), torch.zeros(1, dtype=torch.int32), None

    def get_filelist(self):
        return self.files

    def reset_status(self):
        self.status.zero_()

    def draw(self, items):
        return torch.tensor(list(items)), None

    def launch(self, drawn):
        return torch.zeros(len(drawn[0]), self.n_samples, 4), torch.zeros(1, 7), None

    def check(self, status):
        self.checked = status


def _audio_epoch(script, args=None, **tc):
    from adyolo_amd.train import train_one_epoch_audio
    tr = _StubTrainer(script, **tc)
    loader = [(torch.zeros(2, 8, 4, dtype=torch.int16), [0, 0], torch.zeros(1, 7)) for _ in script]
    prm = _params(**tc)
    prm["args"].update(args or {})
    return tr, lambda: train_one_epoch_audio(prm, loader, tr, stager=_StubStager(), rotate=False)


def _corpus_epoch(script, args=None, **tc):
    from adyolo_amd.train import train_one_epoch_corpus
    tr, corpus = _StubTrainer(script, **tc), _StubCorpus(2 * len(script))
    prm = _params(**tc)
    prm["args"].update(args or {})
    return tr, lambda: train_one_epoch_corpus(prm, corpus, tr)


@pytest.mark.parametrize("epoch", [_audio_epoch, _corpus_epoch])
def test_guarded_epoch_mean_is_over_the_micro_steps_of_applied_cycles(epoch):
    """K = 2, four cycles: (1, 3) applied, (NaN, 5) skipped, (7, NaN) skipped, (2, 4) applied -> (1 + 3 + 2 + 4) / 4.  A
    finite loss inside a skipped cycle does not count and its NaN does not leak."""
    tr, run = epoch([1.0, 3.0, None, 5.0, 7.0, None, 2.0, 4.0], skip_nonfinite=True, accum_steps=2)
    assert run() == 2.5 and tr.calls == 8
    opt = tr.optimizer
    assert opt.step_count == 2 and opt.micro_index == 0
    assert opt.reconcile() == {"attempts": 4, "skipped": 2, "last_skipped": False, "run": 0}
    assert opt.accum_dev.tolist() == [0, 8, 4, 0]


@pytest.mark.parametrize("epoch", [_audio_epoch, _corpus_epoch])
def test_unguarded_epoch_mean_is_over_all_micro_steps(epoch):
    tr, run = epoch([1.0, 2.0, 6.0, 7.0], accum_steps=2)
    assert run() == 4.0 and tr.optimizer.step_count == 2 and tr.optimizer.micro_index == 0
    tr, run = epoch([1.0, 2.0, 6.0, 7.0])                                         # and without accumulation, as it always was
    assert run() == 4.0 and tr.optimizer.step_count == 4


@pytest.mark.parametrize("epoch", [_audio_epoch, _corpus_epoch])
@pytest.mark.parametrize("guarded", [False, True])
def test_an_epoch_that_stops_inside_a_cycle_drops_the_partial_cycle(epoch, guarded):
    """Seven batches at K = 3: two cycles and one micro-step over, which ``reset_accumulation`` discards -- record and mirror
    read index 0.  With the guard its loss (a NaN here) is not part of the mean; without, the mean is over all seven."""
    tc = dict(accum_steps=3, skip_nonfinite=True) if guarded else dict(accum_steps=3)
    last = None if guarded else 8.0
    tr, run = epoch([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, last], **tc)
    assert run() == (3.5 if guarded else 29.0 / 7) and tr.calls == 7
    opt = tr.optimizer
    assert (opt.step_count, opt.micro_index, int(opt.accum_dev[0])) == (2, 0, 0)
    assert opt.accum_dev.tolist() == [0, 7, 2, 1]
    opt.state_dict()                                                              # not refused: no cycle is open


@pytest.mark.parametrize("epoch", [_audio_epoch, _corpus_epoch])
def test_quick_test_break_inside_a_cycle_resets_too(epoch):
    """``quick_test`` stops after five batches: at K = 2 that is two cycles and a dropped micro-step"""
    tr, run = epoch([1.0, 3.0, 5.0, 7.0, 100.0, 100.0, 100.0], args={"quick_test": True}, accum_steps=2, skip_nonfinite=True)
    assert run() == 4.0 and tr.calls == 5
    assert (tr.optimizer.step_count, tr.optimizer.micro_index, int(tr.optimizer.accum_dev[0])) == (2, 0, 0)


def test_guarded_epoch_with_no_finished_cycle_is_zero():
    tr, run = _audio_epoch([1.0, 2.0], skip_nonfinite=True, accum_steps=3)
    assert run() == 0.0 and tr.optimizer.step_count == 0 and tr.optimizer.micro_index == 0


def test_patience_counts_cycles():
    """the run of consecutive skips that ends an epoch is a run of CYCLES: 3 poisoned cycles of 2 at patience 3 raise"""
    tr, run = _audio_epoch([1.0, 1.0] + [None, 2.0] * 3, skip_nonfinite=True, accum_steps=2, skip_nonfinite_patience=3)
    with pytest.raises(FloatingPointError, match=r"3 consecutive.*2 of this epoch's 8 steps.*3 of 4 attempts"):
        run()
    tr, run = _audio_epoch([1.0, 1.0] + [None, 2.0] * 2, skip_nonfinite=True, accum_steps=2, skip_nonfinite_patience=3)
    assert run() == 1.0
