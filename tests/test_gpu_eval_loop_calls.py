"""GPU: the library calls the five device loops of ``adyolo_amd.test`` issue themselves, in order, and their host copies
(``test_epoch_corpus``, ``sweep_conf_thresh_corpus``, ``infer_epoch_corpus``, ``test_epoch_windows``,
``sweep_conf_thresh_windows``).

Every library call goes through ``ops._c(name, ...)``; the names are recorded there, with the recorder paused inside
``model(...)``, ``features(...)`` and ``forward(...)``, so what is kept is the loops' own sequence -- gather, labels, decode
(eager forward only: a recorded graph decodes inside ``forward``), loss, stitch, select, collect, merge, track, score -- whatever
convolution algorithm the model runs.  ``ops.to_host`` / ``ops.to_host_many`` are counted beside them.

The expected sequences are written as functions of the passes (or batches), the views and which passes emit frames, from the
loops' documented order; nothing here is read back from the code under test.  The host copies, per loop:
  test_epoch_*, output_pth=None     ONE ``to_host_many`` at the end, no ``to_host`` (exact)
  test_epoch_*, output_pth          per batch / pass one ``to_host`` (the last stage trims: it reads the row total) and one
                                    ``to_host_many`` (the rows; none for a tracked pass that emits no frame) more (exact)
  infer_epoch_corpus                the same per pass, one read at the end
  sweeps                            one read after the forward phase, two ``to_host`` per threshold (``scorer.scores()``), the last
                                    threshold's rows with ``output_pth``, and one read at the end if views or tracking are on
A one-word read may go through either function, so where a loop ends in one the two counts are asserted as their sum.

The split: four recordings of 12, 70, 30 and 30 label frames, 3 s windows with a 1 s margin, three windows per pass: eight
windows in three passes, the long recording cut by a pass boundary (a tracked pass holds its last frames back).  AD-YOLO head."""
import warnings

import pytest
import torch

from test_eval_corpus_cpu import eval_params, write_eval_split
from test_gpu_eval_windows import HOP, _reference_dir
from test_gpu_track_windows import OPTS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLIPS = (("c0_short", 12 * HOP + 77), ("c1_long", 70 * HOP), ("c2_one", 30 * HOP), ("c3_one", 30 * HOP))
BATCH = 3
VIEWS = [0, 5]
THRESHOLDS = (0.3, 0.6)

GATHER, GATHER_W, GATHER_WV = "adyolo_corpus_gather", "adyolo_corpus_gather_windows", "adyolo_corpus_gather_windows_view"
LABELS, DECODE, LOSS, STITCH = "adyolo_corpus_yolo_labels", "adyolo_yolo_decode", "adyolo_loss_per_clip", "adyolo_decode_stitch"
SELECT, COLLECT, MERGE = "adyolo_yolo_select", "adyolo_tta_collect", "adyolo_tta_merge"
TRACK, TRACK_RUN, SCORE, SCORE_RUNS = "adyolo_track_rows", "adyolo_track_run", "adyolo_seld_score", "adyolo_seld_score_runs"


# ------------------------------------------------------------------------------------------------------ the expected calls
def _forward(gather, eager, labelled, stitch):
    """launch (+ labels) -> forward [-> decode] (-> the loss) (-> stitch)."""
    return ([gather] + [LABELS] * labelled + [DECODE] * eager + [LOSS] * labelled + [STITCH] * stitch)


def _rows(views, link, further):
    """select [-> collect, then per further view: ``further`` (its forward, or nothing where it was kept), select, collect;
    merge] [-> link].  views: 0 without test-time augmentation, else their number."""
    names = [SELECT]
    if views:
        names += [COLLECT] + (further + [SELECT, COLLECT]) * (views - 1) + [MERGE]
    return names + ([link] if link else [])


def _clip_loop(n_batches, eager, views, tracked, sweep):
    plain, view = _forward(GATHER, eager, True, False), _forward(GATHER, eager, False, False)
    link = TRACK if tracked else None
    if not sweep:
        return (plain + _rows(views, link, view) + [SCORE]) * n_batches
    return (plain + view * max(0, views - 1)) * n_batches + (_rows(views, link, []) + [SCORE]) * n_batches * len(THRESHOLDS)


def _window_loop(emitted, eager, views, tracked, sweep, labelled=True):
    """emitted: per pass whether it emits a frame (a tracked pass may hold all of its frames back: nothing to score)."""
    plain, view = _forward(GATHER_W, eager, labelled, True), _forward(GATHER_WV, eager, False, True)
    link = TRACK_RUN if tracked else None
    names = []
    if not sweep:
        for emits in emitted:
            names += plain + _rows(views, link, view) + [SCORE_RUNS] * (emits and labelled)
        return names
    names = (plain + view * max(0, views - 1)) * len(emitted)
    for _ in THRESHOLDS:
        for emits in emitted:
            names += _rows(views, link, []) + [SCORE_RUNS] * emits
    return names


# ------------------------------------------------------------------------------------------------------------ the recorder
class _Outside:
    """``fn`` with the recorder paused while it runs; everything else is ``fn``'s own."""

    def __init__(self, fn, recorder):
        self._fn, self._recorder = fn, recorder

    def __call__(self, *args, **kwargs):
        self._recorder.paused += 1
        try:
            return self._fn(*args, **kwargs)
        finally:
            self._recorder.paused -= 1

    def __getattr__(self, name):
        return getattr(self._fn, name)


class _Recorder:
    def __init__(self, ops, monkeypatch):
        self.names, self.copies, self.paused = [], {"many": 0, "one": 0}, 0
        call, many, one = ops._c, ops.to_host_many, ops.to_host

        def record(name, *args):
            if not self.paused:
                self.names.append(name)
            return call(name, *args)

        def count_many(*ts):
            self.copies["many"] += 1
            return many(*ts)

        def count_one(t):
            self.copies["one"] += 1
            return one(t)
        monkeypatch.setattr(ops, "_c", record)
        monkeypatch.setattr(ops, "to_host_many", count_many)
        monkeypatch.setattr(ops, "to_host", count_one)

    def take(self):
        got = self.names, dict(self.copies)
        self.names, self.copies = [], {"many": 0, "one": 0}
        return got


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adyolo_amd  # noqa: F401
    from adyolo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def world(ops, tmp_path_factory):
    from adyolo_amd.augmentations import tta_options
    from adyolo_amd.corpus import (EvalDeviceCorpus, EvalWindowCorpus, InferDeviceCorpus, infer_split_from_arrays,
                                   load_eval_split)
    from adyolo_amd.features import FeatureExtractor
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.wrapper import WrapperCriterion, WrapperModel
    root = str(tmp_path_factory.mktemp("gpu_eval_loop_calls"))
    written = write_eval_split(root, clips=CLIPS, seed=9)
    prm = eval_params(root, device=DEV)
    # the untrained AD-YOLO head selects more than 64 rows in a frame: the pool of test_gpu_tta_windows.py
    prm["test_config"] = {"tta_views": VIEWS[1:], "tta_min_views": 1, "tta_max_rows_per_frame": 340}
    torch.manual_seed(8)
    model = WrapperModel((1, 7, 80, 64), (), prm).to(DEV).eval()
    hc = load_eval_split(prm, "test", rank=0, world=1, verify="all")
    post = LabelPostProcessor(prm)
    w = {"prm": prm, "model": model, "fx": FeatureExtractor(None, DEV), "crit": WrapperCriterion(prm), "post": post,
         "ref": _reference_dir(root), "tta": tta_options(prm, postprocessor=post)}
    assert w["tta"]["views"] == VIEWS
    w["clips"] = EvalDeviceCorpus(hc, prm, DEV)
    w["windows"] = EvalWindowCorpus(hc, prm, DEV, window_s=3, margin_s=1.0, batch_size=BATCH)
    names = w["windows"].get_filelist()
    w["infer"] = InferDeviceCorpus(infer_split_from_arrays(names, [written[n][0] for n in names], prm), prm, DEV, window_s=3,
                                   margin_s=1.0, batch_size=BATCH)
    w["batches"] = len(list(w["clips"].batches(2)))
    for key in ("windows", "infer"):
        corpus = w[key]
        assert (corpus.n_windows, corpus.n_passes) == (8, 3)                # 1 + 5 + 1 + 1 windows: the long one is cut
        held = [int(n) for n in corpus.track_plan(OPTS)["pass_frames"]]
        assert held != [int(n) for n in corpus.pass_frames] and sum(held) == sum(corpus.pass_frames)
        w[key + "_emitted"] = {False: [True] * corpus.n_passes, True: [n > 0 for n in held]}
    assert w["batches"] >= 2
    return w


CONFIGS = [(False, False), (True, False), (False, True), (True, True)]                  # (views, tracking)
LOOPS = ("test_epoch_corpus", "sweep_conf_thresh_corpus", "infer_epoch_corpus", "test_epoch_windows", "sweep_conf_thresh_windows")


@pytest.mark.parametrize("eager", [True, False], ids=["eager", "graph"])
@pytest.mark.parametrize("loop", LOOPS)
def test_the_loop_issues_these_calls_in_this_order(ops, world, tmp_path, monkeypatch, loop, eager):
    from adyolo_amd import test as atest
    from adyolo_amd.graph import ForwardGraphs
    from adyolo_amd.postprocess import LabelPostProcessor
    from adyolo_amd.seld_metrics import DeviceSELDScorer
    w = world
    rec = _Recorder(ops, monkeypatch)
    model, fx = _Outside(w["model"], rec), _Outside(w["fx"], rec)
    forward = None if eager else _Outside(ForwardGraphs(w["model"], w["fx"], w["post"], warm_calls=0), rec)
    windowed = loop != "test_epoch_corpus" and loop != "sweep_conf_thresh_corpus"
    sweep = loop.startswith("sweep")
    n_t = len(THRESHOLDS)
    for with_views, tracked in CONFIGS:
        views = len(VIEWS) if with_views else 0
        tta = w["tta"] if with_views else None
        track = OPTS if tracked else None
        for output in ([True] if loop == "infer_epoch_corpus" else [False, True]):
            out = str(tmp_path / ("%d%d%d" % (with_views, tracked, output))) if output else None
            scorer = DeviceSELDScorer(w["prm"], w["ref"], DEV)
            post = LabelPostProcessor(w["prm"])
            rec.take()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                             # (the caps of the tracking definition only warn)
                if loop == "test_epoch_corpus":
                    atest.test_epoch_corpus(w["clips"], model, fx, w["crit"], post, out, batch_size=2, forward=forward,
                                            device_scorer=scorer, tta=tta, track=track)
                elif loop == "sweep_conf_thresh_corpus":
                    atest.sweep_conf_thresh_corpus(w["clips"], model, fx, w["crit"], post, scorer, thresholds=THRESHOLDS,
                                                   output_pth=out, batch_size=2, forward=forward, tta=tta, track=track)
                elif loop == "infer_epoch_corpus":
                    atest.infer_epoch_corpus(w["infer"], model, fx, post, out, forward=forward, tracking=track, tta=tta)
                elif loop == "test_epoch_windows":
                    atest.test_epoch_windows(w["windows"], model, fx, w["crit"], post, out, forward=forward, device_scorer=scorer,
                                             tracking=track, tta=tta)
                else:
                    atest.sweep_conf_thresh_windows(w["windows"], model, fx, w["crit"], post, scorer, thresholds=THRESHOLDS,
                                                    output_pth=out, forward=forward, tracking=track, tta=tta)
            names, copies = rec.take()
            case = "%s, %s, views %d, tracking %s, output %s" % (loop, "eager" if eager else "graph", views, tracked, output)
            if windowed:
                emitted = w[("infer" if loop == "infer_epoch_corpus" else "windows") + "_emitted"][tracked]
                want = _window_loop(emitted, eager, views, tracked, sweep, labelled=loop != "infer_epoch_corpus")
                units, written = len(emitted), sum(emitted)
            else:
                want = _clip_loop(w["batches"], eager, views, tracked, sweep)
                units = written = w["batches"]
            print(case, copies, len(names), "calls")
            assert names == want, case
            if sweep:
                total = 1 + 2 * n_t + (units + written if output else 0) + (1 if views or tracked else 0)
                assert copies["many"] + copies["one"] == total, (case, copies)
            elif loop == "infer_epoch_corpus":
                assert copies["many"] + copies["one"] == units + written + 1, (case, copies)
            else:
                assert copies == {"many": 1 + (written if output else 0), "one": units if output else 0}, (case, copies)
