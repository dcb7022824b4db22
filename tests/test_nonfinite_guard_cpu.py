"""CPU: the host side of the non-finite guard (``train_config['skip_nonfinite']``): what ``get_optimizers`` allocates, how
``reconcile`` corrects the host's step mirror from a guard record, the checkpoint entries, and the epoch loops' masked mean and
patience rule.  No HIP call is made: optimizers live on CPU tensors (the pattern of test_optimizers_cpu), the records are
written by hand and the epoch loops run a stub trainer that writes the record as the device would."""
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


def _record(attempts, skipped, last, run):
    return torch.tensor([attempts, skipped, last, run], dtype=torch.int64)


# ------------------------------------------------------------------------------------------------ construction
@pytest.mark.parametrize("name", ["Adam", "AdamW", "SGD"])
@pytest.mark.parametrize("clip", [None, 3.0])
def test_get_optimizers_builds_guarded_optimizers(name, clip):
    """``skip_nonfinite: true`` allocates the record and the partials with and without ``clip_grad_norm`` and makes
    ``grad_norm`` available; an absent or false key allocates what it always did."""
    from adyolo_amd import ops
    from adyolo_amd.train import get_optimizers
    _, flat = _small_flat()
    o = get_optimizers(_params(optim=name, clip_grad_norm=clip, skip_nonfinite=True), flat)
    assert o.skip_nonfinite is True and o.max_norm == clip
    assert o.guard_dev.dtype == torch.int64 and o.guard_dev.tolist() == [0] * ops.OPTIM_GUARD_WORDS
    assert o.clip_partials.dtype == torch.float64 and o.clip_partials.numel() == ops.GRAD_SUMSQ_MAX_PARTS
    assert o.grad_norm.data_ptr() == o.st_dev[2:3].data_ptr() and tuple(o.grad_norm.shape) == (1,)
    assert o.reconcile() == {"attempts": 0, "skipped": 0, "last_skipped": False, "run": 0}
    for tc in (_params(optim=name, clip_grad_norm=clip), _params(optim=name, clip_grad_norm=clip, skip_nonfinite=False)):
        o = get_optimizers(tc, flat)
        assert o.guard_dev is None and o.skip_nonfinite is False
        assert (o.clip_partials is None) == (clip is None) and (o.grad_norm is None) == (clip is None)
        assert o.reconcile() == {"attempts": 0, "skipped": 0, "last_skipped": False, "run": 0} and o.step_count == 0


def test_guard_symbols_are_exported_and_bound():
    from adyolo_amd import _lib, ops
    lib = _lib.load()
    assert int(lib.adyolo_optim_guard_words()) == ops.OPTIM_GUARD_WORDS == 4
    for name in ("adyolo_adam_step_guard_dev", "adyolo_sgd_step_guard_dev"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert callable(ops.adam_step_guard_dev) and callable(ops.sgd_step_guard_dev)


# ------------------------------------------------------------------------------------------------ reconcile
def _attempts(opt, k):
    """what k optimizer attempts do to the host's mirror"""
    for _ in range(k):
        opt.replayed()


def test_reconcile_corrects_the_mirror_once():
    """7 attempts of which the record says 2 were skipped: ``step_count``, the device-value mirror, ``sched_step`` and
    ``ema_updates`` drop by 2, once -- the same record again changes nothing, a later record only by its new skips -- and
    ``sync_device_step`` then writes the corrected value."""
    from adyolo_amd.train import FusedAdam
    _, flat = _small_flat()
    opt = FusedAdam(flat, skip_nonfinite=True, **SCHED)
    _attempts(opt, 7)
    assert opt.step_count == 7 and opt.sched_step == 7 and opt.ema_updates == 7
    rec = _record(7, 2, 0, 0)
    assert opt.reconcile(rec) == {"attempts": 7, "skipped": 2, "last_skipped": False, "run": 0}
    assert (opt.step_count, opt._dev_step_value, opt.sched_step, opt.ema_updates) == (5, 5, 5, 5)
    assert opt.reconcile(rec)["skipped"] == 2 and opt.reconcile()["attempts"] == 7
    assert (opt.step_count, opt._dev_step_value, opt.sched_step, opt.ema_updates) == (5, 5, 5, 5)
    assert opt.lr_at(opt.step_count) == opt.lr_at(5) != opt.lr_at(7)
    _attempts(opt, 3)
    assert opt.reconcile(_record(10, 3, 1, 1)) == {"attempts": 10, "skipped": 3, "last_skipped": True, "run": 1}
    assert (opt.step_count, opt._dev_step_value) == (7, 7)
    opt.step_dev.fill_(-1)
    opt.sync_device_step()                                                      # mirror and device value agree: no write
    assert int(opt.step_dev) == -1
    _attempts(opt, 2)
    opt.guard_dev.copy_(_record(12, 4, 0, 0))
    opt._dev_step_value = 0                                                     # the device value is stale: the fill path ...
    opt.sync_device_step()                                                      # ... reads the record first
    assert int(opt.step_dev) == 8 and opt.step_count == 8


def test_reconcile_reads_the_record_itself_before_the_counter_is_saved_or_written():
    """Without a host copy the record is read from ``guard_dev`` -- only after an attempt -- by everything that saves the
    counter or writes the device counter from the mirror: ``state_dict``, ``sched_state_dict``, the ``step_count`` setter and
    the fill of ``sync_device_step``."""
    from adyolo_amd.train import FusedAdam, FusedSGD
    _, flat = _small_flat()

    def after_skips(cls=FusedAdam, **kw):
        opt = cls(flat, skip_nonfinite=True, **kw)
        _attempts(opt, 4)
        opt.guard_dev.copy_(_record(4, 1, 0, 0))
        return opt

    opt = after_skips(**SCHED)
    assert all(float(s["step"]) == 3.0 for s in opt.state_dict()["state"].values()) and opt.step_count == 3
    opt = after_skips(**SCHED)
    sd = opt.sched_state_dict()
    assert (sd["step"], sd["ema_updates"], opt.step_count) == (3, 3, 3)
    opt = after_skips()
    opt.step_count = 11                                                         # an absolute value: the old skips do not touch it
    assert opt.step_count == 11 and opt.reconcile()["skipped"] == 1 and opt.step_count == 11
    opt.sync_device_step()
    assert int(opt.step_dev) == 11
    opt = after_skips(FusedSGD, momentum=0.9)
    opt.guard_dev.copy_(_record(4, 4, 1, 4))                                     # every attempt skipped: the next is still the first
    assert opt.reconcile()["run"] == 4 and opt.step_count == 0 and opt.first_step
    opt.guard_dev.copy_(_record(9, 9, 1, 9))                                     # no attempt since: the record is not read again
    assert opt.reconcile()["attempts"] == 4


# ------------------------------------------------------------------------------------------------ checkpoint
def _guarded_pair(tmp_path, **tc):
    from adyolo_amd import checkpoint as ck
    from adyolo_amd.train import get_optimizers
    net, flat = _small_flat()
    opt = get_optimizers(_params(skip_nonfinite=True, **tc), flat)
    _attempts(opt, 6)
    opt.guard_dev.copy_(_record(6, 2, 1, 1))
    opt.exp_avg.fill_(0.25)
    opt.exp_avg_sq.fill_(0.5)
    path = str(tmp_path / "model_ckpt.h5")
    ck.save_checkpoint(path, net, opt, 3, 0.5, {}, [], "cpu")
    return ck, net, opt, path


def test_guard_state_dict_round_trips_through_a_checkpoint(tmp_path):
    """The file carries ``guard_state_dict`` and the number of APPLIED steps; a guarded optimizer resumes both, with flag and
    run clean; an unguarded optimizer loads the same file and ignores the entry."""
    from adyolo_amd.train import get_optimizers
    ck, net, opt, path = _guarded_pair(tmp_path, **SCHED)
    saved = torch.load(path, map_location="cpu", weights_only=False)
    assert saved["guard_state_dict"] == {"attempts": 6, "skipped": 2} == opt.guard_state_dict()
    assert all(float(s["step"]) == 4.0 for s in saved["optim_state_dict"]["state"].values())
    assert saved["sched_state_dict"]["step"] == 4 and saved["sched_state_dict"]["ema_updates"] == 4
    net2, flat2 = _small_flat(seed=6)
    fresh = get_optimizers(_params(skip_nonfinite=True, **SCHED), flat2)
    ck.load_checkpoint(path, net2, fresh, restore_rng=False)
    assert fresh.guard_dev.tolist() == [6, 2, 0, 0] and fresh.step_count == 4 and fresh.sched_step == 4
    assert fresh.reconcile() == {"attempts": 6, "skipped": 2, "last_skipped": False, "run": 0} and fresh.step_count == 4
    _attempts(fresh, 2)
    assert fresh.reconcile(_record(8, 3, 0, 0))["skipped"] == 3 and fresh.step_count == 5      # only the new skip counts
    net3, flat3 = _small_flat(seed=7)
    plain = get_optimizers(_params(**SCHED), flat3)
    ck.load_checkpoint(path, net3, plain, restore_rng=False)
    assert plain.guard_dev is None and plain.step_count == 4 and float(plain.exp_avg[0]) == 0.25


def test_checkpoints_without_the_entry_load_with_zeros_and_unguarded_files_are_unchanged(tmp_path):
    from adyolo_amd import checkpoint as ck
    from adyolo_amd.train import get_optimizers
    net, flat = _small_flat()
    old = get_optimizers(_params(), flat)
    _attempts(old, 3)
    path = str(tmp_path / "old.h5")
    ck.save_best(path, net, old, 1, 0.5)
    saved = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(saved) == ["confidence_thresh", "epoch_nb", "model_state_dict", "optim_state_dict"]
    net2, flat2 = _small_flat(seed=6)
    guarded = get_optimizers(_params(skip_nonfinite=True), flat2)
    guarded.guard_dev.copy_(_record(5, 5, 1, 5))
    ck.load_checkpoint(path, net2, guarded, restore_rng=False)
    assert guarded.guard_dev.tolist() == [0, 0, 0, 0] and guarded.step_count == 3
    assert guarded.guard_state_dict() == {"attempts": 0, "skipped": 0}


# ------------------------------------------------------------------------------------------------ epoch loops
class _StubTrainer:
    """``step`` returns the scripted loss (None in the script: a skipped step, whose loss is NaN) and leaves the guard record
    and the host's mirror as a guarded optimizer step does."""
    graphs = None

    def __init__(self, script, **tc):
        from adyolo_amd.train import get_optimizers
        _, self.flat = _small_flat()
        self.optimizer = get_optimizers(_params(**tc), self.flat)
        self.script, self.calls = list(script), 0

    def step(self, audio, target, spec=None):
        loss = self.script[self.calls]
        self.calls += 1
        g = self.optimizer.guard_dev
        if g is not None:
            skip = loss is None
            g[0] += 1
            g[1] += int(skip)
            g[2] = int(skip)
            g[3] = int(g[3]) + 1 if skip else 0
        self.optimizer.replayed()
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


def _audio_epoch(script, **tc):
    from adyolo_amd.train import train_one_epoch_audio
    tr = _StubTrainer(script, **tc)
    loader = [(torch.zeros(2, 8, 4, dtype=torch.int16), [0, 0], torch.zeros(1, 7)) for _ in script]
    return tr, lambda: train_one_epoch_audio(_params(**tc), loader, tr, stager=_StubStager(), rotate=False)


def _corpus_epoch(script, **tc):
    from adyolo_amd.train import train_one_epoch_corpus
    tr, corpus = _StubTrainer(script, **tc), _StubCorpus(2 * len(script))
    return tr, lambda: train_one_epoch_corpus(_params(**tc), corpus, tr)


@pytest.mark.parametrize("epoch", [_audio_epoch, _corpus_epoch])
def test_epoch_mean_is_over_the_applied_steps(epoch):
    """Losses 1, NaN (skipped), 2, NaN, NaN, 6: the mean is (1 + 2 + 6) / 3, not NaN and not / 6, and the optimizer leaves the
    epoch reconciled.  Without the guard the loop is the plain mean it always was."""
    script = [1.0, None, 2.0, None, None, 6.0]
    tr, run = epoch(script, skip_nonfinite=True)
    assert run() == 3.0 and tr.calls == 6
    assert tr.optimizer.step_count == 3 and tr.optimizer.reconcile() == {"attempts": 6, "skipped": 3, "last_skipped": False, "run": 0}
    tr, run = epoch([1.0, 2.0, 6.0, 7.0])
    assert run() == 4.0 and tr.optimizer.step_count == 4
    tr, run = epoch([None, None], skip_nonfinite=True)                          # nothing applied: 0 / max(0, 1)
    assert run() == 0.0 and tr.optimizer.step_count == 0


@pytest.mark.parametrize("epoch", [_audio_epoch, _corpus_epoch])
def test_patience_raises_at_a_run_of_ten_and_not_at_nine(epoch):
    tr, run = epoch([1.0, 3.0] + [None] * 9, skip_nonfinite=True)
    assert run() == 2.0 and tr.optimizer.reconcile()["run"] == 9
    tr, run = epoch([1.0] + [None] * 10, skip_nonfinite=True)
    with pytest.raises(FloatingPointError, match=r"10 consecutive.*1 of this epoch's 11 steps.*10 of 11 attempts"):
        run()
    assert tr.optimizer.step_count == 1                                         # reconciled before it raised
    tr, run = epoch([None] * 10 + [5.0], skip_nonfinite=True)                   # a run that ended inside the epoch is no alarm
    assert run() == 5.0
    tr, run = epoch([1.0] + [None] * 3, skip_nonfinite=True, skip_nonfinite_patience=3)
    with pytest.raises(FloatingPointError, match="3 consecutive"):
        run()
    tr, run = epoch([1.0] + [None] * 12, skip_nonfinite=True, skip_nonfinite_patience=None)
    assert run() == 1.0
