"""Training from an HBM-resident corpus: the chunked training split held on the device, batches made there.

The host path (``datasets.FoaDataset`` -> ``audio_collate_fn`` -> ``AudioStager``) reads one 20 s int16 WAV and one CSV per item,
rotates and encodes the labels on the host and stages every batch over PCIe.  Here the split is read once:

* ``load_chunked_split`` (host half, NumPy): the directory ``FoaDataset`` reads (``<data_pth>/<foa_dev|mic_dev>/dev-train-chunked_
  <w>s_<s>s`` + ``metadata_dev/...``), grouped by recording (``<rec>_chunkNNN``, parsed at the last ``_chunk``).  Each recording
  is rebuilt as ONE int16 stream -- chunk 001 whole, then the last ``stride`` samples of every later chunk -- so chunk k is
  ``stream[(k-1) stride : (k-1) stride + window]`` bit for bit, the zero padding of the last window included; and one event
  table -- chunk 001's rows, then the last ``stride / label_hop`` frames of every later chunk on the recording's frame axis.
  Every chunk CSV is checked against the table, and (``verify``) chunk audio against the stream.
* ``DeviceCorpus`` (device half, AD-YOLO): the streams as one int16 buffer and the events as one float64 table in HBM (0.69 GB
  per hour of 4-channel 24 kHz audio), ``FoaDataset``'s sampling surface (the same functions), and ``batch(indices)``: the same
  ``random`` draws as ``FoaDataset.__getitem__`` item by item, one small H2D copy of the item table, then ``adyolo_corpus_gather``
  (audio, rotated; with ``aug_config.channel_swap_augment`` its MIC form: the capsules permuted) and
  ``adyolo_corpus_yolo_labels`` (the AD-YOLO rows into a fixed-capacity target, padding b = -1).  No host sync.  With
  ``aug_config.time_mix_augment`` the draws of ``augmentations.draw_time_mix`` follow each item's, a second table of mates rides
  in the same copy and both calls take it: the mate's window summed in, the labels united (``augmentations.merge_labels``).  With
  ``aug_config.yaw_rotation_augment`` (FOA) every item and mate row carries its own yaw in word 7 (``augmentations.draw_yaw``,
  right after the combination draw) and the calls, given the yaw, turn the audio and move the azimuths after the combination.
* ``ClasswiseDeviceCorpus`` (device half, ``seddoa | masked-seddoa | accdoa | adpit``): the same split, sampling, draws and
  gather; the labels are ``adyolo_corpus_classwise_labels``, the dense ``ClasswiseLabelEncoder`` targets of the batch written
  whole, from a float32 table of every event's direction vector under no rotation and the 16 FOA combinations (``xyz_table``,
  built once on the host with the host's own functions: 204 bytes per event).  With the yaw rotation x and y come from two
  whole-degree tables instead (``ops.corpus_yaw_xyz_tables``), so the split's angles must then be whole degrees.

Parity: the same audio bit for bit and the same rows in the same order (or the same dense targets bit for bit) as the host
path iterated in the main process (``num_workers=0``); with DataLoader workers the host path's draws happen in per-worker streams.

Evaluation splits ('val' / 'valid' / 'test': whole recordings, static between epochs) have their own pair: ``load_eval_split``
reads the split ``FoaDataset(params, set_type, is_valid=True)`` reads into the same ``HostCorpus`` layout, one recording per
clip, and ``EvalDeviceCorpus`` uploads it once (audio, events, one item per clip) and makes each batch of
``test.test_epoch_corpus`` from a range of clips with no host data: the gather without rotation, then the AD-YOLO rows with the
clips' row starts or the dense class-wise target (all five losses in one class).

Inference on a folder of recordings of any length has the third pair: ``load_infer_split`` (or ``infer_split_from_arrays``)
lays the recordings out the same way, without events, and ``InferDeviceCorpus`` cuts them into overlapping windows of one shape
(``window_plan``) through a window table uploaded once; ``test.infer_epoch_corpus`` runs the windows in passes through one
recorded graph, keeps each window's frames that have context on both sides and stitches them back onto the recordings' axes.
With ``load_infer_split(..., resample=True)`` (``infer_split_from_arrays(..., rates=...)``) the recordings may be at any standard
rate and in int16, 24-bit or float32: those that are not int16 at ``data_config.sr`` stay in their native form on the host, and
the upload converts them on the device (``ops.resample_pcm``, resample.py) into the places the layout left for them.

Labelled evaluation of recordings of any length joins the two: ``EvalWindowCorpus`` takes the split of ``load_eval_split`` and
cuts it into the windows of ``InferDeviceCorpus`` (``plan_windows``, ``_WindowCorpus``), with one label item row per window
(``window_items``), for ``test.test_epoch_windows``; the device scorer then scores each pass's stitched run in segments
(``seld_metrics.run_segments``).

A live stream has no length to plan from: ``stream_plan`` is the window plan that does not need the recording's end, and
``StreamDeviceCorpus`` holds ONE such stream in a ring in HBM (``ops.stream_gather_windows`` reads the windows out of it) for
``test.StreamInference``, which returns each frame's detections once it is final.

One structure under all of it: every loader returns a ``HostCorpus``, whose constructor owns the stream layout (16-frame
alignment) and gives every field a value, with ``kind`` saying which split it is; the loaders share one WAV reader, one CSV
reader and one verify pick (``_read_wav``, ``_csv_rows``, ``_verify_picks``); the five device corpora share ``_CorpusBase``.
"""
import copy
import os
import random
import struct

import numpy as np
import torch

from . import ops
from .datasets import CLASSWISE_LABELS, FoaDataset, YoloLabelEncoder

# event table columns (host): recording frame, class, source, azimuth, elevation
_EV_COLS = 5


def _split_dirs(params, set_type):
    dc = params["data_config"]
    if set_type != "train":
        raise ValueError("load_chunked_split: only the chunked training split is supported (got set_type=%r)" % (set_type,))
    adir = {"foa": "foa_dev", "mic": "mic_dev"}[str(dc.get("audio_format", "foa")).lower()]     # FoaDataset's rule
    sub = "dev-train-chunked_{}s_{}s".format(dc["chunk_window_s"], dc["chunk_stride_s"])
    return os.path.join(dc["data_pth"], adir, sub), os.path.join(dc["data_pth"], "metadata_dev", sub)


def _parse_chunk(name):
    i = name.rfind("_chunk")
    if i < 0 or not name[i + 6:].isdigit():
        raise ValueError("load_chunked_split: %s is not named <recording>_chunkNNN" % name)
    return name[:i], int(name[i + 6:])


def _csv_rows(who, path, nb_classes=None):
    """A label CSV as ``FoaDataset`` sees it: ``load_csv2dict`` iterated -> [(frame, cls, src, az, el)] (polar rows only).
    nb_classes: also refuse a class outside [0, nb_classes).  who: the loader's name, for the messages."""
    if not os.path.exists(path):
        raise ValueError("%s: label file %s is missing" % (who, path))
    rows = []
    for frame, events in FoaDataset.load_csv2dict(path).items():
        for ev in events:
            if len(ev) != 4:
                raise ValueError("%s: %s has a row that is not [frame, class, source, azimuth, elevation]" % (who, path))
            if nb_classes is not None and not 0 <= ev[0] < nb_classes:
                raise ValueError("%s: %s has an event of class %d, outside [0, %d) (nb_classes)" % (who, path, ev[0], nb_classes))
            rows.append((frame, ev[0], ev[1], ev[2], ev[3]))
    return rows


def _read_wav(who, path, window=None, native=False):
    """One WAV file, memory-mapped -> (rate, data).  The file must hold int16 (n, 4) -- (window, 4) exactly with ``window`` --
    or, with ``native``, any sample format of ``resample.KINDS``; ``ValueError`` naming ``who`` (the loader) and the path
    otherwise.  Only ``native`` reads a 24-bit file, which scipy cannot map, into memory."""
    from scipy.io import wavfile
    try:
        rate, data = wavfile.read(path, mmap=True)
    except ValueError as e:
        if not native or "mmap" not in str(e):                   # only scipy's "mmap=True not compatible with 24-bit" is retried
            raise
        rate, data = wavfile.read(path, mmap=False)
    if native:
        from .resample import KINDS
        known = data.dtype in KINDS
    else:
        known = data.dtype == np.int16
    if not known or data.ndim != 2 or data.shape != (data.shape[0] if window is None else window, 4):
        raise ValueError("%s: %s holds %s %s, expected %s (%s, 4)"
                         % (who, path, data.dtype, tuple(data.shape), "int16, 24-bit or float32" if native else "int16",
                            "n" if window is None else "%d" % window))
    return int(rate), data


def _verify_picks(who, verify, n):
    """The indices of ``range(n)`` a loader reads a second time: all of them for "all", the first, middle (n // 2) and last for
    "sample", none for "none"; ``ValueError`` for any other value."""
    if verify not in ("sample", "all", "none"):
        raise ValueError("%s: verify must be 'sample', 'all' or 'none' (got %r)" % (who, verify))
    if verify == "all":
        return range(n)
    return sorted({0, n // 2, n - 1}) if verify == "sample" and n else ()


class HostCorpus:
    """A split in host memory (NumPy): what ``load_chunked_split`` (kind ``CHUNKED``), ``load_eval_split`` (``EVAL``) and
    ``load_infer_split`` / ``infer_split_from_arrays`` (``INFER``) return.  The constructor lays the recordings out and gives
    every field its empty value; the loader fills in the audio and, if the split has labels, the events.

    kind       CHUNKED | EVAL | INFER: what the device corpora ask instead of probing for fields
    rec_names  recording names; lengths int64 (R,): samples per recording (CHUNKED: of the rebuilt stream; a recording that is
               converted on the device: after conversion)
    rec_start  int64 (R + 1,): first frame of each stream in ``audio`` (end of the last at R), each a multiple of 16
    audio      int16 (max(S, 16), 4): the streams, zero between the end of one and the start of the next
    events     float64 (E, 5) [frame on the recording's axis, class, source, azimuth, elevation], recording after recording,
               frames ascending, file order within a frame; ev_start int64 (R + 1,).  INFER: (0, 5) and zeros
    max_events the largest event count of a window (CHUNKED) or of a recording (EVAL); INFER: 0
    chunks     name -> (recording, sample offset into ``audio``, frame offset on the recording's axis); chunk_events  name ->
               (first event, number of events) of its label window.  CHUNKED only, {} otherwise
    total_filelist, filelist  CHUNKED: the chunk names in ``os.listdir`` order, exactly as ``FoaDataset`` builds them (the
               device corpus draws its own ``filelist`` from them); otherwise this rank's recordings: == rec_names
    rank, world  the shard that was loaded (CHUNKED: 0, 1 -- the device corpus shards the draw)
    window, stride (samples; EVAL / INFER: the longest whole-hop length, a multiple of 600 samples, and 0), hop_label (samples
               per label frame), window_frames; wav_pth, csv_pth, set_type as ``FoaDataset`` has them (None without a folder)
    native, rates, kinds, native_lengths  None, except in an INFER split made with ``rates=`` / ``resample=True``: per
               recording the samples kept in their own rate and format (None where ``audio`` already holds them), the rate
               in Hz, the sample format (0 int16, 1 int32, 2 float32) and the length before conversion
    """

    CHUNKED, EVAL, INFER = "chunked", "eval", "infer"

    def __init__(self, kind, rec_names, lengths, hop_label, set_type, wav_pth=None, csv_pth=None, rank=0, world=1, window=None,
                 stride=0):
        self.kind, self.set_type, self.wav_pth, self.csv_pth = kind, set_type, wav_pth, csv_pth
        self.rank, self.world = rank, world
        self.rec_names = list(rec_names)
        self.filelist = self.total_filelist = list(rec_names)
        self.lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        self.rec_start = np.zeros(len(self.rec_names) + 1, dtype=np.int64)
        pos = 0
        for i, n in enumerate(self.lengths.tolist()):
            self.rec_start[i] = pos
            pos += (n + 15) // 16 * 16               # a contract with the gather kernels: their 16-byte loads are aligned
        self.rec_start[-1] = pos
        self.audio = np.zeros((max(pos, 16), 4), dtype=np.int16)
        self.set_events([np.zeros((0, _EV_COLS))] * len(self.rec_names))
        self.max_events = 0
        self.chunks, self.chunk_events = {}, {}
        if window is None:                                       # whole recordings: the longest whole-hop length
            window = int((self.lengths // 600).max() * 600) if len(self.rec_names) else 0
        self.window, self.stride, self.hop_label, self.window_frames = window, stride, hop_label, window // hop_label
        self.native = self.rates = self.kinds = self.native_lengths = None

    def set_events(self, per_recording):
        """The event table from one float64 (n, 5) array per recording."""
        self.events = np.concatenate(per_recording, 0) if per_recording else np.zeros((0, _EV_COLS))
        self.ev_start = np.concatenate([[0], np.cumsum([len(e) for e in per_recording])]).astype(np.int64)

    def stream(self, i):
        """Recording ``i``'s samples: a view of ``audio``, without the alignment tail."""
        s0 = int(self.rec_start[i])
        return self.audio[s0:s0 + int(self.lengths[i])]

    def nbytes(self):
        native = sum(a.nbytes for a in self.native or () if a is not None)
        return int(self.audio.nbytes + self.events.nbytes + native)


def load_chunked_split(params, set_type="train", verify="sample"):
    """The chunked training split -> ``HostCorpus`` (see the module docstring).  verify: "sample" (default) reads the first,
    middle and last chunk of every recording in full and compares them with their rebuilt windows, "all" every chunk, "none"
    nothing; every header is checked (int16, 4 channels, ``window`` samples) and every CSV is compared with the event table.
    Anything else raises ``ValueError`` naming the file."""
    who = "load_chunked_split"
    _verify_picks(who, verify, 0)                                # a bad value is refused before anything is read
    dc = params["data_config"]
    wav_pth, csv_pth = _split_dirs(params, set_type)
    sr = int(dc.get("sr", 24000))
    window, stride = int(round(sr * dc["chunk_window_s"])), int(round(sr * dc["chunk_stride_s"]))
    hop = int(sr * dc.get("label_hop_len_s", 0.1))                    # FoaDataset.hop_label
    if stride <= 0 or window < stride or stride % hop:
        raise ValueError("load_chunked_split: window %d / stride %d samples with a label hop of %d" % (window, stride, hop))
    window_frames, stride_frames = window // hop, stride // hop

    total_filelist = [i.replace(".wav", "") for i in os.listdir(wav_pth)]          # FoaDataset.total_filelist
    groups = {}
    for name in total_filelist:
        rec, k = _parse_chunk(name)
        groups.setdefault(rec, {})[k] = name
    rec_names = sorted(groups)
    for rec in rec_names:
        ks = sorted(groups[rec])
        if ks != list(range(1, len(ks) + 1)):
            raise ValueError("load_chunked_split: recording %s has chunks %s (expected 1..%d without gaps)" % (rec, ks, len(ks)))

    hc = HostCorpus(HostCorpus.CHUNKED, rec_names, [window + (len(groups[r]) - 1) * stride for r in rec_names], hop, set_type,
                    wav_pth, csv_pth, window=window, stride=stride)
    hc.filelist = hc.total_filelist = total_filelist
    ev_parts, ev_base = [], 0
    for r, rec in enumerate(rec_names):
        names = groups[rec]
        nk = len(names)
        paths = {k: os.path.join(wav_pth, names[k] + ".wav") for k in names}
        s0, stream = int(hc.rec_start[r]), hc.stream(r)
        # audio: chunk 1 whole, the last `stride` samples of every later chunk
        for k in range(1, nk + 1):
            data = _read_wav(who, paths[k], window)[1]
            if k == 1:
                stream[:window] = data
            else:
                lo = window + (k - 2) * stride
                stream[lo:lo + stride] = data[window - stride:]
            del data
        for k in sorted(nk - i for i in _verify_picks(who, verify, nk)):        # chunks 1, (nk + 1) // 2 and nk of "sample"
            lo = (k - 1) * stride
            if not np.array_equal(np.asarray(_read_wav(who, paths[k], window)[1]), stream[lo:lo + window]):
                raise ValueError("load_chunked_split: %s differs from the window rebuilt from its neighbours (overlapping chunks "
                                 "of %s disagree)" % (paths[k], rec))
        # labels: chunk 1's rows, then the last stride_frames frames of every later chunk, on the recording's frame axis
        csv = {k: _csv_rows(who, os.path.join(csv_pth, names[k] + ".csv")) for k in range(1, nk + 1)}
        rows = []
        for k in range(1, nk + 1):
            f_off = (k - 1) * stride_frames
            keep = [e for e in csv[k] if k == 1 or e[0] >= window_frames - stride_frames]
            keep.sort(key=lambda e: e[0])                                   # stable: file order within a frame
            rows += [(e[0] + f_off,) + tuple(e[1:]) for e in keep]
        ev = np.asarray(rows, dtype=np.float64).reshape(-1, _EV_COLS)
        frames = ev[:, 0]
        for k in range(1, nk + 1):
            f_off = (k - 1) * stride_frames
            lo, hi = np.searchsorted(frames, f_off, "left"), np.searchsorted(frames, f_off + window_frames, "left")
            want = [(float(e[0] - f_off),) + tuple(float(v) for v in e[1:]) for e in ev[lo:hi].tolist()]
            got = [tuple(float(v) for v in e) for e in csv[k]]
            if got != want:
                raise ValueError("load_chunked_split: %s disagrees with the event table of %s rebuilt from its chunks (rows "
                                 "outside [0, %d) frames, out of frame order, or overlaps that differ)"
                                 % (os.path.join(csv_pth, names[k] + ".csv"), rec, window_frames))
            hc.chunks[names[k]] = (r, s0 + (k - 1) * stride, f_off)
            hc.chunk_events[names[k]] = (ev_base + int(lo), int(hi - lo))
            hc.max_events = max(hc.max_events, int(hi - lo))
        ev_parts.append(ev)
        ev_base += ev.shape[0]
    hc.set_events(ev_parts)
    return hc


def max_cells_per_event(encoder):
    """The largest number of grid cells one event can occupy (``YoloLabelEncoder.encode_events``): the cells are the product
    of an azimuth and an elevation set, each piecewise constant between the cell bounds -- evaluated on every bound and every
    midpoint between neighbouring bounds."""
    def most(points, count):
        p = np.unique(np.asarray(points, dtype=np.float64))
        cand = np.concatenate([p, (p[1:] + p[:-1]) * 0.5])
        return max(int(count(c)) for c in cand)
    az_pts = [v for b in (encoder.az_lb, encoder.az_ub) for x in b for v in (x, x - 360.0, x + 360.0) if -180.0 <= v <= 180.0]
    el_pts = [v for b in (encoder.el_lb, encoder.el_ub) for v in b] + [-90.0, 90.0]

    def n_az(a):
        a = -180.0 if a == 180.0 else a
        return (((encoder.az_lb <= a) & (a < encoder.az_ub)) | (a + 360 < encoder.az_ub) | (encoder.az_lb < a - 360)).sum()

    def n_el(e):
        return ((encoder.el_lb <= e) & (e < encoder.el_ub)).sum()
    return most(az_pts + [-180.0, 180.0], n_az) * most(el_pts, n_el)


def _rank_world(rank, world):
    """FoaDataset's default: torch.distributed if initialised, else RANK / WORLD_SIZE, else 0 / 1."""
    if world is None:
        import torch.distributed as tdist
        if tdist.is_available() and tdist.is_initialized():
            rank, world = tdist.get_rank(), tdist.get_world_size()
        else:
            rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    return int(rank or 0), int(world)


def xyz_table(az, el):
    """float32 (E, 17, 3): the direction vector ``ClasswiseLabelEncoder`` writes for each event (azimuth / elevation in degrees)
    -- slot 0 without rotation (the host path does not call ``rotate_labels`` then), slot 1 + k after ``rotate_labels`` with
    combination k -- computed by the host's own functions on scalars and rounded to float32 as the encoder's output is.  Memoised
    on the bit patterns of the angles (``-0.0 == 0.0`` as a dict key, but ``sin(-0.0)`` is ``-0.0``)."""
    from .augmentations import COMBINATIONS, rotate_labels
    from .datasets import _polar_to_xyz
    az = np.asarray(az, dtype=np.float64).reshape(-1)
    el = np.asarray(el, dtype=np.float64).reshape(-1)
    n_slots = 1 + len(COMBINATIONS)
    if az.shape[0] == 0:
        return np.zeros((0, n_slots, 3), dtype=np.float32)
    keys, inv = np.unique(np.stack([az, el], 1).view(np.int64), axis=0, return_inverse=True)
    pairs = keys.view(np.float64).tolist()                       # Python floats, as load_csv2dict reads them
    memo = {}

    def xyz(a, e):
        k = struct.pack("<dd", a, e)
        v = memo.get(k)
        if v is None:
            v = memo[k] = _polar_to_xyz(a, e)
        return v
    uniq = np.empty((len(pairs), n_slots, 3), dtype=np.float64)
    for i, (a, e) in enumerate(pairs):
        uniq[i, 0] = xyz(a, e)
    rows = [[0, 0, a, e] for a, e in pairs]
    for k in range(len(COMBINATIONS)):
        for i, ev in enumerate(rotate_labels({0: rows}, k)[0]):
            uniq[i, 1 + k] = xyz(ev[2], ev[3])
    return uniq.astype(np.float32)[inv.reshape(-1)]


def xyz_unrotated(az, el):
    """float32 (E, 3): slot 0 of ``xyz_table`` alone (no rotation), for splits that are never rotated."""
    from .datasets import _polar_to_xyz
    pairs = np.stack([np.asarray(az, dtype=np.float64).reshape(-1), np.asarray(el, dtype=np.float64).reshape(-1)], 1)
    if pairs.shape[0] == 0:
        return np.zeros((0, 3), dtype=np.float32)
    keys, inv = np.unique(pairs.view(np.int64), axis=0, return_inverse=True)      # bit patterns: -0.0 and 0.0 differ
    uniq = np.asarray([_polar_to_xyz(a, e) for a, e in keys.view(np.float64).tolist()], dtype=np.float64)
    return uniq.astype(np.float32)[inv.reshape(-1)]


class _CorpusBase:
    """What the five device corpora share (the two windowed ones through ``_WindowCorpus``).  All of them: the adopted ``HostCorpus`` in HBM with the identity fields and methods
    of ``FoaDataset`` that the epoch loops read (``_adopt``), the status word and ``check``, and the small helpers of a
    ``launch`` (``_out``, ``_round_cap``, ``_yolo_tables``).  The two training corpora only (``DeviceCorpus``,
    ``ClasswiseDeviceCorpus``): the augmentation configuration and ``FoaDataset``'s sampling of files (``_train_setup``), the host
    draws of a batch, the upload of its item table and the audio gather (``draw`` .. ``_gather``).  Subclasses add the labels."""

    # the same functions as the host dataset: checkpoints (remaining_file) and the rank shards interchange with it
    sample_filelist_for_train_iter = FoaDataset.sample_filelist_for_train_iter
    init_remaining_file_from_list = FoaDataset.init_remaining_file_from_list
    get_remaining_file = FoaDataset.get_remaining_file
    get_filelist = FoaDataset.get_filelist
    __len__ = FoaDataset.__len__
    _copy, _random = copy, random                # the modules ``sample_filelist_for_train_iter`` and ``draw`` draw through

    def _adopt(self, hc, device, rank, world, is_valid, is_infer=False):
        """Every corpus: the host split, the device, what ``FoaDataset`` would answer for this split, the split in HBM."""
        self.host = hc
        self.device = torch.device(device)
        self.rank, self.world = rank, world
        self.is_valid, self.is_infer, self.set_type = is_valid, is_infer, "infer" if is_infer else hc.set_type
        self.wav_pth, self.csv_pth = hc.wav_pth, None if is_infer else hc.csv_pth
        self.hop_label = hc.hop_label
        self.rotate = False
        self.filelist = list(hc.filelist)
        self.max_events = int(hc.max_events)
        self._to_hbm(hc)

    def _train_setup(self, params):
        """The training corpora: the augmentations, the batch shape and the first draw of files (``FoaDataset.__init__``)."""
        from .augmentations import (MIC_SWAP_COMBS, SpecAug, channel_swap_enabled, feature_aug_config, mic_swap_source,
                                    time_mix_config, yaw_config)
        hc = self.host
        self.rotate = bool(params.get("aug_config", {}).get("rotation_augment", False))
        # yaw rotation (FOA only; ValueError: MIC audio or a bad yaw_step_deg): None or the step, and the gather's table
        self.yaw = yaw_config(params)
        self.yaw_tab = ops.corpus_yaw_table(self.device) if self.yaw is not None else None
        # MIC channel swap (ValueError: audio_format is not 'mic', or rotation_augment is on as well): the gather's table
        self.swap = channel_swap_enabled(params)
        self.mic_src = ops.corpus_mic_table({k: mic_swap_source(k) for k in MIC_SWAP_COMBS}) if self.swap else None
        self.specaug = SpecAug(params, False)
        self._mix_yaw = {} if self.yaw is None else {"yaw": self.yaw}     # what draw_time_mix is told of it: nothing when off
        self.mix = time_mix_config(params)    # time-domain mixing: None or (prob, gain lo, gain hi) (ValueError: a bad key)
        self.feat_aug = feature_aug_config(params)        # frequency shift / cutout: None or the parsed keys (ValueError: a bad key)
        self.batch_size = int(params["train_config"]["batch_size"])
        self.n_samples, self.n_label_frames = hc.window, hc.window // hc.hop_label
        self.total_filelist = list(hc.total_filelist)
        self.remaining_file = copy.deepcopy(self.total_filelist)
        self.nb_samples = self.batch_size * params["train_config"]["nb_iters"] * self.world
        self.sample_filelist_for_train_iter()

    def _yolo_tables(self, params):
        """The AD-YOLO label tables: the host encoder, the largest cell count of an event, the cell bounds in HBM, the grid."""
        self.encoder = enc = YoloLabelEncoder(params)
        self.cells = max_cells_per_event(enc)
        self.bounds = torch.from_numpy(np.concatenate([enc.az_lb, enc.az_ub, enc.el_lb, enc.el_ub]).astype(np.float64)).to(self.device)
        self.grid = (len(enc.az_lb), len(enc.el_lb))

    @staticmethod
    def _round_cap(rows):
        """At least one target row, rounded up to ``graph.TARGET_QUANTUM``: one input shape per recorded graph."""
        from . import graph
        q = graph.TARGET_QUANTUM
        return (max(1, int(rows)) + q - 1) // q * q

    def _out(self, given, shape, what="audio_out"):
        """An output of ``launch``: the caller's buffer, which must have this shape, or a new float32 tensor."""
        if given is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        if tuple(given.shape) != tuple(shape):
            raise ValueError("%s.launch: %s %s, expected %s" % (type(self).__name__, what, tuple(given.shape), tuple(shape)))
        return given

    def _to_hbm(self, hc):
        """The split in HBM: the int16 streams, the event table {frame, class, azimuth, elevation} in float64, the status word."""
        from .augmentations import COMBINATIONS
        self.pcm = torch.from_numpy(hc.audio).to(self.device)
        ev = hc.events[:, [0, 1, 3, 4]] if hc.events.shape[0] else np.zeros((1, 4))
        self.events = torch.from_numpy(np.ascontiguousarray(ev, dtype=np.float64)).to(self.device)
        self.n_events = int(hc.events.shape[0])
        self.rot = ops.corpus_rot_table(COMBINATIONS)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._pinned, self._copied, self._slot = {}, [None, None], 0

    def nbytes(self):
        return int(self.pcm.numel() * 2 + self.events.numel() * 8)

    # ---------------------------------------------------------------------------------------------------------- batches
    def draw(self, indices):
        """The host half of a batch: ``FoaDataset.__getitem__``'s ``random`` draws item by item (rotation or channel swap, then
        SpecAug) and the item table -> (items int64 (B, 8), spec int32 (B, 2, 4) or None), host arrays; with
        ``aug_config.yaw_rotation_augment`` each row's yaw (``augmentations.draw_yaw``, right after its combination draw) is word 7
        of the row, in whole degrees; with
        ``aug_config.freq_shift_augment`` / ``cutout_augment`` spec is int32 (B, 4, 4): the SpecAug rows (zeros with ``spec_augment``
        off), the cutout row, {shift, 0, 0, 0} (``augmentations.draw_feature_aug``, the last draws of every item).  With
        ``aug_config.time_mix_augment`` the item's mixing draws follow (``augmentations.draw_time_mix``) and a third element is
        returned: mates int64 (B, 8), the mate chunk as an item row with its own combination and the float32 bits of the gain in
        word 6, offset -1 where the item is unmixed."""
        from .augmentations import MIC_SWAP_COMBS, draw_feature_aug, draw_time_mix, draw_yaw
        from .features import HOP, N_MELS
        names = [self.filelist[i] for i in indices]
        b = len(names)
        items = np.zeros((b, ops.CORPUS_ITEM_WORDS), dtype=np.int64)
        spec = None
        if self.specaug.apply_augment or self.feat_aug is not None:
            spec = np.zeros((b, 2 if self.feat_aug is None else 4, 4), dtype=np.int32)
        mates = None
        if self.mix is not None:
            mates = np.zeros((b, ops.CORPUS_ITEM_WORDS), dtype=np.int64)
            mates[:, 0] = mates[:, 4] = -1
        for j, name in enumerate(names):
            rec, off, f_off = self.host.chunks[name]
            ev_lo, ev_n = self.host.chunk_events[name]
            comb = -1
            if self.rotate:
                comb = int(self._random.uniform(0, 16))                       # augmentations.py:76, as in __getitem__
            elif self.swap:
                comb = MIC_SWAP_COMBS[int(self._random.uniform(0, 8))]        # as in __getitem__: one draw
            phi = draw_yaw(self._random, self.yaw) if self.yaw is not None else 0
            if self.specaug.apply_augment:
                spec[j, :2] = self.specaug.draw_groups(1, self.n_samples // HOP, N_MELS, 2)[0].numpy()
            items[j] = (off, f_off, ev_lo, ev_n, comb, rec, 0, phi)
            if mates is not None:
                drawn = draw_time_mix(self._random, self.mix, self.total_filelist, name,
                                      "rotate" if self.rotate else "swap" if self.swap else None, **self._mix_yaw)
                if drawn is not None:
                    mate, m_comb, gain = drawn[:3]
                    m_rec, m_off, m_f_off = self.host.chunks[mate]
                    m_lo, m_n = self.host.chunk_events[mate]
                    mates[j] = (m_off, m_f_off, m_lo, m_n, -1 if m_comb is None else m_comb, m_rec,
                                int(np.float32(gain).view(np.uint32)), drawn[3] if self.yaw is not None else 0)
            if self.feat_aug is not None:
                spec[j, 2], spec[j, 3, 0] = draw_feature_aug(self._random, self.feat_aug, self.n_samples // HOP, N_MELS)
        if mates is not None:
            return items, spec, mates
        return items, spec

    def _upload(self, drawn):
        """One H2D copy of the item table (+ SpecAug tables) through a double-buffered page-locked buffer
        -> (items int64 (B, 8), spec int32 (B, rows, 4) or None; rows = 2, or 4 with the frequency-shift / cutout rows) on the
        device, and the mates int64 (B, 8) or None: with mates in ``drawn`` they travel in the same copy, behind the items."""
        items, spec = drawn[0], drawn[1]
        mates = drawn[2] if len(drawn) > 2 else None
        b = items.shape[0]
        n_i = b * ops.CORPUS_ITEM_WORDS
        n_m = n_i if mates is not None else 0
        # 8 int32 of SpecAug per item = 4 int64 words; 16 int32 = 8 words with the frequency-shift / cutout rows
        n_words = n_i + n_m + (spec.size // 2 if spec is not None else 0)
        slot = self._slot
        self._slot ^= 1
        key = (slot, n_words)
        host = self._pinned.get(key)
        if host is None:
            host = self._pinned[key] = torch.empty(n_words, dtype=torch.int64).pin_memory()
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()          # the copy out of this page-locked buffer two batches ago has landed
        hv = host.numpy()
        hv[:n_i] = items.reshape(-1)
        if mates is not None:
            hv[n_i:n_i + n_m] = mates.reshape(-1)
        if spec is not None:
            hv[n_i + n_m:].view(np.int32)[:] = spec.reshape(-1)
        dev = torch.empty(n_words, dtype=torch.int64, device=self.device)
        dev.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._copied[slot] = ev
        dev_items = dev[:n_i].view(b, ops.CORPUS_ITEM_WORDS)
        dev_spec = dev[n_i + n_m:].view(torch.int32).view(b, spec.shape[1], 4) if spec is not None else None
        dev_mates = dev[n_i:n_i + n_m].view(b, ops.CORPUS_ITEM_WORDS) if mates is not None else None
        return dev_items, dev_spec, dev_mates

    def batch(self, indices, audio_out=None, target_out=None):
        """Items ``indices`` of ``get_filelist()`` -> (audio (B, n, 4) f32, target, spec (B, 2 | 4, 4) int32 or None), on the device,
        with no host synchronisation.  audio_out / target_out: write into these buffers (a recorded step's)."""
        return self.launch(self.draw(indices), audio_out, target_out)

    def _begin(self, drawn, audio_out, target_out):
        """What every ``launch`` starts with: the H2D copy of the tables, then the output buffers (the caller's, checked against
        ``target_shape``, or new ones) -> (items, mates or None, spec or None, audio, target), all on the device."""
        dev_items, dev_spec, dev_mates = self._upload(drawn)
        b = dev_items.shape[0]
        audio = self._out(audio_out, (b, self.n_samples, 4))
        target = self._out(target_out, self.target_shape(b), "target_out")
        return dev_items, dev_mates, dev_spec, audio, target

    def _gather(self, dev_items, audio, dev_mates=None):
        """The audio of a batch: FOA-rotated (with ``aug_config.yaw_rotation_augment``: and yawed, each row by its word 7), or with
        ``aug_config.channel_swap_augment`` the MIC capsules permuted; with mates
        (``aug_config.time_mix_augment``) each mate's window, under its own combination, summed in by the same pass."""
        return ops.corpus_gather(self.pcm, dev_items, self.rot, audio, self.status, mates=dev_mates, mic_src=self.mic_src,
                                 yaw_tab=self.yaw_tab)

    def reset_status(self):
        self.status.zero_()

    def check(self, word=None):
        """Raise if a batch overflowed its capacity, had an item outside the corpus or an event class outside the model's (reads
        the status word: synchronises, unless the caller passes the word it already read)."""
        if word is None:
            word = int(ops.to_host(self.status)[0])
        ops.corpus_status_check(word)


class DeviceCorpus(_CorpusBase):
    """A ``HostCorpus`` in HBM with ``FoaDataset``'s sampling surface and a device-side ``batch``.

        corpus = DeviceCorpus(load_chunked_split(params), params, "cuda:0")
        audio, target, spec = corpus.batch(range(16))    # (16, n, 4) f32, (cap, 7) f32, (16, 2, 4) int32 or None: all on the device

    ``cap`` (the target rows) is fixed here: batch_size x (largest event count of a window; twice that with
    ``aug_config.time_mix_augment``, where an item holds two windows' events) x (largest cell count of an event), rounded up to
    ``graph.TARGET_QUANTUM`` -- one input shape, one recorded graph.  More rows than that in a batch (a smaller ``cap`` forced by
    the caller) set the status word; ``check()`` raises then.  AD-YOLO labels only: the class-wise losses train from
    ``ClasswiseDeviceCorpus``."""

    def __init__(self, host_corpus, params, device="cuda:0", rank=None, world=None, cap=None):
        self.loss_nm = params["args"]["loss"]
        if self.loss_nm != "adyolo":
            raise NotImplementedError("DeviceCorpus: loss %s -- AD-YOLO labels only; the class-wise losses train from "
                                      "ClasswiseDeviceCorpus" % self.loss_nm)
        self._adopt(host_corpus, device, *_rank_world(rank, world), is_valid=False)
        self._yolo_tables(params)
        self._train_setup(params)
        if cap is None:
            # a mixed item holds the events of two windows
            cap = self._round_cap(self.batch_size * (2 if self.mix is not None else 1) * self.max_events * self.cells)
        self.cap = int(cap)
        self.rows = None                 # int32 word on the device: the row count of the last batch

    def target_shape(self, batch):
        """The target of every batch: (cap, 7) rows, whatever the batch size."""
        return (self.cap, 7)

    def launch(self, drawn, audio_out=None, target_out=None):
        """The device half: one H2D copy of the item table (+ SpecAug tables), the gather and the label kernels.
        -> (audio (B, n, 4) f32, target (cap, 7) f32, spec (B, 2 | 4, 4) int32 or None) on the device; no host sync."""
        dev_items, dev_mates, dev_spec, audio, target = self._begin(drawn, audio_out, target_out)
        b = dev_items.shape[0]
        self.rows = torch.empty(1, dtype=torch.int32, device=self.device)
        self._gather(dev_items, audio, dev_mates)
        # with mates (time-domain mixing) both sources' rows in merged order; with the yaw rotation the azimuths moved by word 7
        ws_words = ops.corpus_labels_workspace_words(b, self.max_events, mix=dev_mates is not None)
        ws = torch.empty(max(1, ws_words), dtype=torch.int32, device=self.device)
        ops.corpus_yolo_labels(self.events, dev_items, self.max_events, self.n_label_frames, self.bounds, self.grid, self.rot, ws,
                               target, self.rows, self.status, mates=dev_mates, yaw=self.yaw is not None)
        return audio, target, dev_spec


class ClasswiseDeviceCorpus(_CorpusBase):
    """``DeviceCorpus`` for the class-wise losses (``seddoa | masked-seddoa | accdoa | adpit``): the same split in HBM, sampling
    surface, ``random`` draws and audio gather; the target is the dense tensor ``FoaDataset`` + ``audio_collate_fn`` make
    (``ClasswiseLabelEncoder`` on the rotated labels, stacked), written whole on the device by ``adyolo_corpus_classwise_labels``
    from ``xyz`` (``xyz_table`` of every event, float32 (E, 17, 3) in HBM).

        corpus = ClasswiseDeviceCorpus(load_chunked_split(params), params, "cuda:0")
        audio, target, spec = corpus.batch(range(64))    # target: corpus.target_shape(64), e.g. (64, T', 6, 4, C) for adpit

    Every event class must be in [0, nb_classes) (``ValueError`` naming the recording otherwise: the host encoders would fail on
    it).  No host sync in ``batch`` / ``launch``; ``check()`` reads the status word."""

    def __init__(self, host_corpus, params, device="cuda:0", rank=None, world=None):
        self.loss_nm = params["args"]["loss"]
        if self.loss_nm not in CLASSWISE_LABELS:
            raise ValueError("ClasswiseDeviceCorpus: loss %s -- the class-wise losses are %s (AD-YOLO trains from DeviceCorpus)"
                             % (self.loss_nm, ", ".join(sorted(CLASSWISE_LABELS))))
        self.nb_classes = c = int(params["data_config"]["nb_classes"])
        hc = host_corpus
        cls = hc.events[:, 1]
        bad = np.flatnonzero(~((cls >= 0) & (cls < c)))
        if bad.size:
            r = int(np.searchsorted(hc.ev_start, bad[0], "right")) - 1
            raise ValueError("ClasswiseDeviceCorpus: recording %s has an event of class %g, outside [0, %d) (nb_classes)"
                             % (hc.rec_names[r], cls[bad[0]], c))
        self._adopt(hc, device, *_rank_world(rank, world), is_valid=False)
        xyz = xyz_table(hc.events[:, 3], hc.events[:, 4]) if hc.events.shape[0] else \
            np.zeros((1, ops.CORPUS_XYZ_SLOTS, 3), dtype=np.float32)
        self.xyz = torch.from_numpy(xyz).to(self.device)
        self._train_setup(params)
        self.yaw_xyz = None
        if self.yaw is not None:         # x and y of a yawed event come from whole-degree tables: the split must have no other angle
            ang = hc.events[:, 3:5]
            frac = np.flatnonzero(~((ang == np.round(ang)).all(1) & (np.abs(ang[:, 0]) <= 180) & (np.abs(ang[:, 1]) <= 90)))
            if frac.size:
                r = int(np.searchsorted(hc.ev_start, frac[0], "right")) - 1
                raise ValueError("ClasswiseDeviceCorpus: aug_config.yaw_rotation_augment needs whole-degree labels, and recording "
                                 "%s has an event at azimuth %r, elevation %r (DeviceCorpus and FoaDataset take any angles)"
                                 % (hc.rec_names[r], float(ang[frac[0], 0]), float(ang[frac[0], 1])))
            self.yaw_xyz = ops.corpus_yaw_xyz_tables(self.device)

    def nbytes(self):
        return super().nbytes() + int(self.xyz.numel() * 4)

    def target_shape(self, batch):
        """(B, T', 4C) seddoa / masked-seddoa, (B, T', 3C) accdoa, (B, T', 6, 4, C) adpit."""
        return ops.corpus_classwise_shape(self.loss_nm, batch, self.n_label_frames, self.nb_classes)

    def launch(self, drawn, audio_out=None, target_out=None):
        """The device half: one H2D copy of the item table (+ SpecAug tables), the gather and the label kernel.
        -> (audio (B, n, 4) f32, target ``target_shape(B)`` f32, spec (B, 2 | 4, 4) int32 or None) on the device; no host sync."""
        dev_items, dev_mates, dev_spec, audio, target = self._begin(drawn, audio_out, target_out)
        self._gather(dev_items, audio, dev_mates)
        # with mates (time-domain mixing) the targets of the merged events; with the yaw rotation x and y from the whole-degree
        # tables, each row's yaw in word 7
        ops.corpus_classwise_labels(self.events, dev_items, self.xyz, self.max_events, self.n_label_frames, self.nb_classes,
                                    self.loss_nm, target, self.status, mates=dev_mates,
                                    rot=self.rot if self.yaw_xyz is not None else None, yaw_xyz=self.yaw_xyz)
        return audio, target, dev_spec


# ------------------------------------------------------------------------------------------------------- evaluation splits
def _eval_dirs(params, set_type):
    """The directories ``FoaDataset(params, set_type, is_valid=True)`` reads for a labelled evaluation split."""
    dc = params["data_config"]
    if set_type == "train":
        raise ValueError("load_eval_split: set_type='train' is the chunked training split (load_chunked_split)")
    if set_type == "infer":
        raise ValueError("load_eval_split: set_type='infer' has no labels; it is evaluated through test_epoch_audio")
    adir = {"foa": "foa_dev", "mic": "mic_dev"}[str(dc.get("audio_format", "foa")).lower()]     # FoaDataset's rule
    sub = "dev-{}".format(set_type)
    return os.path.join(dc["data_pth"], adir, sub), os.path.join(dc["data_pth"], "metadata_dev", sub)


def load_eval_split(params, set_type, rank=None, world=None, verify="sample"):
    """A labelled evaluation split ('val', 'valid', 'test': what ``FoaDataset(params, set_type, is_valid=True)`` accepts) read
    once -> ``HostCorpus`` of kind ``EVAL``: every recording whole in its stream and one event table.

    filelist    exactly ``FoaDataset``'s: ``os.listdir`` order on one rank, ``sorted(...)[rank::world]`` under data parallelism;
                only this rank's recordings are loaded.  rec_names == filelist: recording i is clip i.
    events      every CSV row, rows past ``len // hop_label`` label frames included (the label kernels drop them, as
                ``FoaDataset.__getitem__`` does), frames ascending, file order within a frame.

    ``ValueError`` naming the file: a file that is not int16 or not 4 channels wide, a missing CSV, a row that is not
    [frame, class, source, azimuth, elevation], a class outside [0, nb_classes), frames that do not ascend (the host's rows
    follow the file, the table the frames).  verify: "sample" reads the first, middle and last recording again and compares
    them with the stream, "all" every recording, "none" nothing."""
    who = "load_eval_split"
    _verify_picks(who, verify, 0)                                # a bad value is refused before anything is read
    dc = params["data_config"]
    wav_pth, csv_pth = _eval_dirs(params, set_type)
    if not os.path.isdir(wav_pth):
        raise ValueError("load_eval_split: %s is not a directory (set_type=%r)" % (wav_pth, set_type))
    nb_classes = int(dc["nb_classes"])
    hop = int(dc.get("sr", 24000) * dc.get("label_hop_len_s", 0.1))                 # FoaDataset.hop_label
    rank, world = _rank_world(rank, world)
    filelist = [i.replace(".wav", "") for i in os.listdir(wav_pth)]                  # FoaDataset.filelist
    if world > 1:
        filelist = sorted(filelist)[rank::world]
    paths = [os.path.join(wav_pth, name + ".wav") for name in filelist]
    # headers first: the stream is allocated once
    hc = HostCorpus(HostCorpus.EVAL, filelist, [_read_wav(who, p)[1].shape[0] for p in paths], hop, set_type, wav_pth, csv_pth,
                    rank, world)
    ev_parts = []
    for i, name in enumerate(filelist):
        hc.stream(i)[:] = _read_wav(who, paths[i])[1]
        path = os.path.join(csv_pth, name + ".csv")
        rows = _csv_rows(who, path, nb_classes)
        if any(rows[k][0] > rows[k + 1][0] for k in range(len(rows) - 1)):
            raise ValueError("load_eval_split: the frames of %s do not ascend" % path)
        ev_parts.append(np.asarray(rows, dtype=np.float64).reshape(-1, _EV_COLS))
        hc.max_events = max(hc.max_events, len(rows))
    hc.set_events(ev_parts)
    for i in _verify_picks(who, verify, len(filelist)):
        if not np.array_equal(np.asarray(_read_wav(who, paths[i])[1]), hc.stream(i)):
            raise ValueError("load_eval_split: %s changed while the split was read" % paths[i])
    return hc


class EvalDeviceCorpus(_CorpusBase):
    """A ``load_eval_split`` split in HBM: the audio, the events and the item table of every clip are uploaded once; a batch is
    made on the device from a range of clips with no host data at all.  All five losses: AD-YOLO rows or, for the class-wise
    heads, the dense targets.  No sampling, no rotation, no SpecAug.

        corpus = EvalDeviceCorpus(load_eval_split(params, "test"), params, "cuda:0")
        for idx in corpus.batches(8):
            audio, target, row_start = corpus.launch(idx)   # (B, t, 4) f32; (cap, 7) f32 + (B + 1,) int32, or dense + None

    ``cap`` (AD-YOLO target rows of a batch of B clips): B x (largest event count of a clip) x (largest cell count of an
    event), rounded up to ``graph.TARGET_QUANTUM``; ``cap_per_clip`` forces a smaller one (the status word then tells)."""

    def __init__(self, host_split, params, device="cuda:0", cap_per_clip=None):
        hc = host_split
        if hc.kind == HostCorpus.CHUNKED:
            raise ValueError("EvalDeviceCorpus: the split of load_eval_split is needed (got the chunked training split)")
        self.loss_nm = params["args"]["loss"]
        if self.loss_nm != "adyolo" and self.loss_nm not in CLASSWISE_LABELS:
            raise NotImplementedError("EvalDeviceCorpus: loss %s" % self.loss_nm)
        self.nb_classes = int(params["data_config"]["nb_classes"])
        self._adopt(hc, device, hc.rank, hc.world, is_valid=True)
        n = len(self.filelist)
        self.lengths = [int(v) for v in hc.lengths.tolist()]
        self.n_hops = [v // 600 * 600 for v in self.lengths]            # whole hops, as test_epoch_audio cuts a clip
        self.label_frames = [v // self.hop_label for v in self.lengths]
        items = np.zeros((max(n, 1), ops.CORPUS_ITEM_WORDS), dtype=np.int64)
        for i in range(n):
            items[i] = (hc.rec_start[i], 0, hc.ev_start[i], hc.ev_start[i + 1] - hc.ev_start[i], -1, i, 0, 0)
        self.items = torch.from_numpy(items).to(self.device)
        # rotation test-time augmentation (``launch_view``): the format, the item table of each view, the MIC source table
        self.audio_format = str(params["data_config"].get("audio_format", "foa")).lower()
        self._view_items, self.mic_src = {}, None
        if self.loss_nm == "adyolo":
            self._yolo_tables(params)
            self.cap_per_clip = int(cap_per_clip) if cap_per_clip is not None else max(1, self.max_events * self.cells)
            self.xyz = None
        else:
            full = np.zeros((max(1, hc.events.shape[0]), ops.CORPUS_XYZ_SLOTS, 3), dtype=np.float32)
            if hc.events.shape[0]:
                full[:, 0] = xyz_unrotated(hc.events[:, 3], hc.events[:, 4])     # only the unrotated slot is read
            self.xyz = torch.from_numpy(full).to(self.device)

    def nbytes(self):
        return super().nbytes() + int(self.items.numel() * 8) + (int(self.xyz.numel() * 4) if self.xyz is not None else 0)

    def batches(self, batch_size):
        """The index ranges ``test_epoch_audio(batch_size=...)`` forms on this file list: consecutive clips share a pass while
        their whole-hop length is equal (and with it, at the usual hops, their label frames)."""
        out, i, n, bs = [], 0, len(self.filelist), max(1, int(batch_size))
        while i < n:
            j = i + 1
            while j < min(i + bs, n) and self.n_hops[j] == self.n_hops[i] and self.label_frames[j] == self.label_frames[i]:
                j += 1
            out.append(range(i, j))
            i = j
        return out

    def cap(self, batch):
        """Target rows of a batch of ``batch`` clips (AD-YOLO)."""
        return self._round_cap(int(batch) * self.cap_per_clip)

    def _items_of(self, indices, table=None):
        table = self.items if table is None else table
        idx = list(indices)
        if not idx or min(idx) < 0 or max(idx) >= len(self.filelist):
            raise ValueError("EvalDeviceCorpus.launch: clips %s of a split of %d" % (idx, len(self.filelist)))
        if idx == list(range(idx[0], idx[0] + len(idx))):
            return idx, table[idx[0]:idx[0] + len(idx)]                          # a view: nothing crosses PCIe
        return idx, table.index_select(0, torch.tensor(idx, dtype=torch.int64).to(self.device, non_blocking=True))

    def _batch_shape(self, idx):
        """(B, samples, label frames) of the clips ``idx``, which must agree in both."""
        b, t, frames = len(idx), self.n_hops[idx[0]], self.label_frames[idx[0]]
        if any(self.n_hops[i] != t or self.label_frames[i] != frames for i in idx):
            raise ValueError("EvalDeviceCorpus.launch: clips %s differ in length (%s samples): one length per batch"
                             % (idx, [self.lengths[i] for i in idx]))
        if t <= 0 or frames <= 0:
            raise ValueError("EvalDeviceCorpus.launch: clip %s is shorter than one hop / label frame" % self.filelist[idx[0]])
        return b, t, frames

    def launch(self, indices, audio_out=None):
        """Clips ``indices`` of ``get_filelist()`` (equal whole-hop lengths, e.g. a range of ``batches``) -> (audio (B, t, 4) f32,
        target, row_start) on the device with no host synchronisation.  AD-YOLO: target (cap(B), 7) rows, b = -1 past the total,
        and row_start (B + 1,) int32, clip b's rows at [row_start[b], row_start[b + 1]); class-wise heads: the dense
        (B, T', ...) target and None.  audio_out: write the audio into this buffer (a recorded forward graph's input)."""
        idx, items = self._items_of(indices)
        b, t, frames = self._batch_shape(idx)
        audio = self._out(audio_out, (b, t, 4))
        ops.corpus_gather(self.pcm, items, self.rot, audio, self.status)
        if self.loss_nm != "adyolo":
            target = torch.empty(ops.corpus_classwise_shape(self.loss_nm, b, frames, self.nb_classes), dtype=torch.float32,
                                 device=self.device)
            ops.corpus_classwise_labels(self.events, items, self.xyz, self.max_events, frames, self.nb_classes, self.loss_nm,
                                        target, self.status)
            return audio, target, None
        me = self.max_events
        target = torch.empty((self.cap(b), 7), dtype=torch.float32, device=self.device)
        # the scan leaves lane (b, 0)'s exclusive offset at ws[b * me] and the total right behind the lanes: the row starts
        ws = torch.zeros(b * max(me, 1) + 1, dtype=torch.int32, device=self.device)
        ops.corpus_yolo_labels(self.events, items, me, frames, self.bounds, self.grid, self.rot, ws, target,
                               ws[b * max(me, 1):], self.status)
        row_start = ws[::max(me, 1)].contiguous()
        return audio, target, row_start

    def launch_view(self, indices, comb, audio_out=None):
        """The audio of ``launch`` for the same clips under combination ``comb`` (rotation test-time augmentation): FOA-rotated,
        or with ``data_config.audio_format: mic`` the capsules permuted (a combination that is no symmetry of the array:
        ``ValueError``).  Audio only -- a view has no labels -> audio (B, t, 4) f32.  The item table of a view is a copy of the
        split's with word 4 set, made once."""
        from .augmentations import COMBINATIONS, MIC_SWAP_COMBS, mic_swap_source
        comb = int(comb)
        if not 0 <= comb < len(COMBINATIONS):
            raise ValueError("EvalDeviceCorpus.launch_view: combination %r is not one of 0..%d" % (comb, len(COMBINATIONS) - 1))
        if self.audio_format == "mic":
            mic_swap_source(comb)                                # ValueError: no symmetry of the array
            if self.mic_src is None:
                self.mic_src = ops.corpus_mic_table({k: mic_swap_source(k) for k in MIC_SWAP_COMBS})
        if comb not in self._view_items:
            table = self.items.clone()
            table[:, 4] = comb
            self._view_items[comb] = table
        idx, items = self._items_of(indices, self._view_items[comb])
        b, t, _ = self._batch_shape(idx)
        audio = self._out(audio_out, (b, t, 4))
        return ops.corpus_gather(self.pcm, items, self.rot, audio, self.status, mic_src=self.mic_src)


# ------------------------------------------------------------------------------------------------------- windowed inference
def window_plan(n_frames, window_frames, margin_frames):
    """A recording of ``n_frames`` label frames cut into windows of ``window_frames`` that overlap so that every kept frame has
    ``margin_frames`` of context on both sides -> [(start_frame, src_lo, dst_lo, n)] per window: the window starts at label frame
    start_frame of the recording, and its frames [src_lo, src_lo + n) (window-local) are the recording's [dst_lo, dst_lo + n).

    F <= Wf: one window (0, 0, 0, F).  Otherwise, with the stride S = Wf - 2 Mf, ceil((F - Wf) / S) + 1 windows: window k
    starts at k S, the last one at F - Wf (tail-aligned: it ends with the recording and holds no padding); window 0 keeps
    [0, Wf - Mf), a middle one [Mf, Wf - Mf), the last one from where the one before stopped up to F.  The kept ranges tile
    [0, F) exactly once, in order.  ``ValueError`` unless Wf > 2 Mf >= 0."""
    f, wf, mf = int(n_frames), int(window_frames), int(margin_frames)
    if mf < 0 or wf <= 2 * mf:
        raise ValueError("window_plan: a window of %d frames with a margin of %d (window_frames > 2 * margin_frames >= 0)" % (wf, mf))
    if f < 0:
        raise ValueError("window_plan: %d frames" % f)
    if f <= wf:
        return [(0, 0, 0, f)]
    s = wf - 2 * mf
    k_n = -(-(f - wf) // s) + 1
    out = [(0, 0, 0, wf - mf)]
    for k in range(1, k_n - 1):
        out.append((k * s, mf, k * s + mf, s))
    done = (k_n - 2) * s + wf - mf                       # where window K - 2 stopped (K = 2: window 0, at Wf - Mf)
    start = f - wf
    out.append((start, done - start, done, f - done))
    return out


def split_pass_rows(rows, counts, base_frame, frame_start):
    """The host half of a windowed pass: rows (N, 5) [frame of the run, class, x, y, z] in frame order and counts (frames of the
    run,) rows per frame (``select_device_rows`` on the stitched run), the run starting at ``base_frame`` on the axis of all
    recordings laid end to end, frame_start (R + 1,) the first frame of each recording on that axis -> {recording: {frame of the
    recording: [[class, x, y, z], ...]}}, frames ascending: ``group_rows`` split at the recording boundaries."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 5)
    frame_start = np.asarray(frame_start, dtype=np.int64).reshape(-1)
    if int(counts.sum()) != len(rows) or base_frame < 0 or base_frame + len(counts) > int(frame_start[-1]):
        raise ValueError("split_pass_rows: %d rows, %d frame counts summing to %d, frames [%d, %d) of %d"
                         % (len(rows), len(counts), int(counts.sum()), base_frame, base_frame + len(counts), int(frame_start[-1])))
    ends = np.cumsum(counts)
    frames = np.flatnonzero(counts)
    glob = frames + int(base_frame)
    rec = np.searchsorted(frame_start, glob, "right") - 1
    local = glob - frame_start[rec]
    vals = rows[:, 1:].tolist()
    out = {}
    for r, f, s, e in zip(rec.tolist(), local.tolist(), (ends[frames] - counts[frames]).tolist(), ends[frames].tolist()):
        out.setdefault(r, {})[f] = vals[s:e]
    return out


def infer_split_from_arrays(names, arrays, params, rates=None):
    """Recordings held in memory (int16 (n, 4) each) -> the ``HostCorpus`` ``load_infer_split`` returns: every recording whole in
    one int16 stream, each on a 16-frame boundary, ``lengths``, no events.  ``ValueError`` naming the recording for anything
    that is not int16 (n, 4).

    rates: one sample rate (Hz) per recording; each array may then be int16, int32 (24-bit PCM left-justified, as scipy reads
    it) or float32 (n, 4).  An int16 recording at ``data_config.sr`` is laid out as above.  Every other one keeps its samples on
    the host (``native``) and has its converted length, ceil(n L / M) (``resample.n_out``), in ``lengths`` and a zeroed place
    of that length in ``audio``, which ``InferDeviceCorpus`` fills on the device: ``rec_start``, the window plan and the frame
    axis are those of the converted recordings.  The split then also holds ``rates``, ``kinds`` (0 int16, 1 int32, 2 float32)
    and ``native_lengths``.  ``ValueError`` naming the recording and both rates for a ratio ``resample.plan`` refuses."""
    names = [str(n) for n in names]
    arrays = list(arrays)
    if len(names) != len(arrays):
        raise ValueError("infer_split_from_arrays: %d names for %d arrays" % (len(names), len(arrays)))
    dc = params["data_config"]
    hop = int(dc.get("sr", 24000) * dc.get("label_hop_len_s", 0.1))                 # FoaDataset.hop_label
    native = None
    if rates is None:
        for name, a in zip(names, arrays):
            if getattr(a, "dtype", None) != np.int16 or a.ndim != 2 or a.shape[1] != 4:
                raise ValueError("infer_split_from_arrays: %s holds %s %s, expected int16 (n, 4)"
                                 % (name, getattr(a, "dtype", type(a).__name__), tuple(getattr(a, "shape", ()))))
        lengths = np.asarray([a.shape[0] for a in arrays], dtype=np.int64).reshape(-1)
    else:
        from . import resample
        sr = int(dc.get("sr", 24000))
        rates = [int(r) for r in rates]
        if len(rates) != len(names):
            raise ValueError("infer_split_from_arrays: %d rates for %d arrays" % (len(rates), len(arrays)))
        kinds, native, lengths = [], [], []
        for name, a, rate in zip(names, arrays, rates):
            dtype = getattr(a, "dtype", None)
            kind = resample.KINDS.get(dtype) if isinstance(dtype, np.dtype) else None
            if kind is None or a.ndim != 2 or a.shape[1] != 4:
                raise ValueError("infer_split_from_arrays: %s holds %s %s, expected int16, int32 or float32 (n, 4)"
                                 % (name, getattr(a, "dtype", type(a).__name__), tuple(getattr(a, "shape", ()))))
            try:
                l, m = resample.ratio(rate, sr)
            except ValueError as e:
                raise ValueError("infer_split_from_arrays: %s: %s" % (name, e))
            if max(l, m) > resample.MAX_P:                        # what resample.plan refuses, before anything is uploaded
                raise ValueError("infer_split_from_arrays: %s: %d -> %d Hz is the ratio %d / %d, beyond resample.plan (%d)"
                                 % (name, rate, sr, l, m, resample.MAX_P))
            kinds.append(kind)
            native.append(None if (l == m and kind == 0) else a)
            lengths.append(resample.n_out(a.shape[0], l, m))
        native_lengths = np.asarray([a.shape[0] for a in arrays], dtype=np.int64).reshape(-1)
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    hc = HostCorpus(HostCorpus.INFER, names, lengths, hop, "infer")
    for i, a in enumerate(arrays):
        if native is None or native[i] is None:
            hc.stream(i)[:] = a
    if native is not None:
        hc.native, hc.rates, hc.native_lengths = native, np.asarray(rates, dtype=np.int64).reshape(-1), native_lengths
        hc.kinds = np.asarray(kinds, dtype=np.int64).reshape(-1)
    return hc


def load_infer_split(params, rank=None, world=None, verify="sample", files=None, resample=False):
    """The int16 4-channel WAV files under ``params['args']['infer_pth']`` read once -> ``HostCorpus`` (the layout of
    ``load_eval_split`` without events).  The file list is ``FoaDataset(params, 'infer')``'s: ``os.listdir`` order on one rank,
    ``sorted(...)[rank::world]`` under data parallelism.  files: names (without ``.wav``) of the recordings to load, in the
    order of that list -- a folder that does not fit HBM is taken in parts; a name the list does not hold raises.
    ``ValueError`` naming the file for anything that is not int16 (n, 4).  verify: as in ``load_eval_split``.

    resample=True: every file's rate and sample format are read.  int16, 24-bit (scipy: int32, left-justified) and float32 files
    of four channels at any rate ``resample.plan`` takes against ``data_config.sr`` are accepted, anything else is refused by
    path; an int16 file at ``data_config.sr`` is laid out as above and every other one keeps its samples on the host for
    ``InferDeviceCorpus`` to convert on the device (``infer_split_from_arrays`` with ``rates``).  Without it the rate of a file
    is not looked at: a 48 kHz recording is run as if it were at ``data_config.sr``."""
    who = "load_infer_split"
    _verify_picks(who, verify, 0)                                # a bad value is refused before anything is read
    wav_pth = str(params["args"]["infer_pth"])
    if not os.path.isdir(wav_pth):
        raise ValueError("load_infer_split: %s is not a directory (args.infer_pth)" % wav_pth)
    rank, world = _rank_world(rank, world)
    filelist = [i.replace(".wav", "") for i in os.listdir(wav_pth)]                  # FoaDataset.filelist
    if world > 1:
        filelist = sorted(filelist)[rank::world]
    if files is not None:
        want = set(str(f) for f in files)
        missing = sorted(want - set(filelist))
        if missing:
            raise ValueError("load_infer_split: %s is not among this rank's files of %s" % (", ".join(missing), wav_pth))
        filelist = [f for f in filelist if f in want]

    paths = [os.path.join(wav_pth, name + ".wav") for name in filelist]

    def read(path):
        rate, data = _read_wav(who, path, native=resample)
        if resample:                                             # what resample.plan refuses, by path
            from .resample import MAX_P, ratio
            sr = int(params["data_config"].get("sr", 24000))
            if max(ratio(rate, sr)) > MAX_P:
                raise ValueError("load_infer_split: %s is at %d Hz; %d -> %d Hz is the ratio %d / %d, beyond resample.plan (%d)"
                                 % ((path, rate, rate, sr) + ratio(rate, sr) + (MAX_P,)))
        return rate, data

    files_read = [read(p) for p in paths]
    hc = infer_split_from_arrays(filelist, [data for _, data in files_read], params,
                                 rates=[rate for rate, _ in files_read] if resample else None)
    for i in _verify_picks(who, verify, len(filelist)):
        rate, data = read(paths[i])
        if hc.native is not None and hc.native[i] is not None:
            kept = np.asarray(hc.native[i])
            same = rate == int(hc.rates[i]) and data.dtype == kept.dtype and data.shape == kept.shape and \
                np.array_equal(np.ascontiguousarray(data).view(np.uint8), np.ascontiguousarray(kept).view(np.uint8))
        else:
            same = np.array_equal(np.asarray(data), hc.stream(i))
        if not same:
            raise ValueError("load_infer_split: %s changed while the split was read" % paths[i])
    hc.wav_pth, hc.rank, hc.world = wav_pth, rank, world
    return hc


def plan_windows(label_frames, lengths, rec_start, hop, n_samples, window_frames, margin_frames, batch_size):
    """The window table of a split cut into windows of one shape (pure NumPy; ``InferDeviceCorpus`` and ``EvalWindowCorpus``):
    every recording's ``window_plan`` (no window for a recording without a label frame), all windows in file order, cut into
    passes of ``batch_size`` windows, the last pass filled up with empty windows -> dict of
      table        int64 (passes * batch_size, ``ops.WINDOW_WORDS``): {stream offset, valid samples, src_lo, destination frame on
                   the axis of all recordings laid end to end, n, recording (-1: an empty window), 0, 0}
      starts       int64 (n_windows,): each window's first label frame on its own recording's axis
      frame_start  int64 (R + 1,): the first frame of each recording on the common axis
      n_windows, n_passes, pass_base (the first frame of each pass's run on the common axis), pass_frames (its length)."""
    label_frames = [int(v) for v in label_frames]
    frame_start = np.concatenate([[0], np.cumsum(label_frames)]).astype(np.int64)
    rows, starts = [], []
    for r, frames in enumerate(label_frames):
        if frames == 0:
            continue
        for start, src_lo, dst_lo, cnt in window_plan(frames, window_frames, margin_frames):
            off = int(rec_start[r]) + start * hop
            rows.append((off, min(n_samples, int(lengths[r]) - start * hop), src_lo, int(frame_start[r]) + dst_lo, cnt, r, 0, 0))
            starts.append(start)
    n_windows = len(rows)
    n_passes = (n_windows + batch_size - 1) // batch_size
    total = int(frame_start[-1])
    rows += [(0, 0, 0, total, 0, -1, 0, 0)] * (n_passes * batch_size - n_windows)                     # empty windows
    table = np.asarray(rows, dtype=np.int64).reshape(-1, ops.WINDOW_WORDS)
    per = table.reshape(n_passes, batch_size, ops.WINDOW_WORDS)
    return {"table": table, "starts": np.asarray(starts, dtype=np.int64), "frame_start": frame_start, "n_windows": n_windows,
            "n_passes": n_passes, "pass_base": [int(v) for v in per[:, 0, 3].tolist()],
            "pass_frames": [int(v) for v in per[:, :, 4].sum(1).tolist()]}


def plan_track(frame_start, pass_bounds, hold):
    """``_WindowCorpus.track_plan`` in NumPy: frame_start (R + 1,) the recordings' first frames on the common axis,
    pass_bounds (passes + 1,) the passes' bounds on it, hold D -> {'hold', 'bounds', 'pass_base', 'pass_frames',
    'segments_host'}."""
    start = np.asarray(frame_start, dtype=np.int64).reshape(-1)
    b = np.asarray(pass_bounds, dtype=np.int64).reshape(-1)
    hold = int(hold)
    if hold < 0 or len(b) < 2 or b[0] != 0 or b[-1] != start[-1] or (np.diff(b) <= 0).any():
        raise ValueError("plan_track: hold %d, pass bounds %s on %d frames" % (hold, b.tolist(), int(start[-1])))
    rec = np.searchsorted(start, b, "right") - 1                     # the recording a bound lies in (the last one starting there)
    rec = np.minimum(rec, len(start) - 2)
    inside = (b != start[rec]) & (b != start[-1])
    e = np.where(inside, np.maximum(b - hold, start[rec]), b)
    tables = []
    for p in range(len(b) - 1):
        lo, hi = int(b[p]), int(b[p + 1])
        rows = []
        for r in range(int(np.searchsorted(start[1:], lo, "right")), len(start) - 1):
            s, t = int(start[r]), int(start[r + 1])
            if s >= hi:
                break
            if t > s:
                a, z = max(s, lo), min(t, hi)
                rows.append((a - lo, z - a, int(a > s), int(z < t)))
        tables.append(np.asarray(rows, dtype=np.int32).reshape(-1, 4))
    return {"hold": hold, "bounds": e, "pass_base": [int(v) for v in e[:-1].tolist()],
            "pass_frames": [int(v) for v in np.diff(e).tolist()], "segments_host": tables}


class _WindowCorpus(_CorpusBase):
    """What the two windowed corpora share: the window and margin arguments (``_window_setup``, before anything is uploaded),
    the window table (``plan_windows``) and its upload, ``pass_table`` and the gather of a pass."""

    def _window_setup(self, hc, params, window_s, margin_s, batch_size):
        """window_s / margin_s / batch_size checked and kept as samples and label frames -> the sample rate."""
        from .features import HOP
        who = type(self).__name__
        dc = params["data_config"]
        sr = int(dc.get("sr", 24000))
        hop = int(hc.hop_label)
        window_s = dc["chunk_window_s"] if window_s is None else window_s
        margin_s = 2.0 if margin_s is None else margin_s
        n, m = int(round(sr * float(window_s))), int(round(sr * float(margin_s)))
        if n <= 0 or m < 0 or abs(n - sr * float(window_s)) > 1e-6 or abs(m - sr * float(margin_s)) > 1e-6 or n % hop or m % hop:
            raise ValueError("%s: window %r s / margin %r s are not whole multiples of the label hop (%d samples at "
                             "%d Hz)" % (who, window_s, margin_s, hop, sr))
        if n % HOP:
            raise ValueError("%s: a window of %d samples is not a whole number of feature hops (%d)" % (who, n, HOP))
        self.window_frames, self.margin_frames = n // hop, m // hop
        if self.window_frames <= 2 * self.margin_frames:
            raise ValueError("%s: a window of %r s keeps nothing between two margins of %r s" % (who, window_s, margin_s))
        self.batch_size = int(batch_size)
        if not 1 <= self.batch_size < 65536:
            raise ValueError("%s: batch_size %r" % (who, batch_size))
        self.n_samples = n
        # rotation test-time augmentation (``launch_view``): the format, the MIC source table (made by the first MIC view)
        self.audio_format = str(dc.get("audio_format", "foa")).lower()
        self.mic_src = None
        return sr

    def _window_tables(self, hc):
        """The split's window plan on the host (``plan_windows``)."""
        hop = int(hc.hop_label)
        self.lengths = [int(v) for v in hc.lengths.tolist()]
        self.label_frames = [v // hop for v in self.lengths]
        plan = plan_windows(self.label_frames, self.lengths, hc.rec_start, hop, self.n_samples, self.window_frames,
                            self.margin_frames, self.batch_size)
        self.frame_start, self.table_host, self.window_starts = plan["frame_start"], plan["table"], plan["starts"]
        self.n_windows, self.n_passes = plan["n_windows"], plan["n_passes"]
        self.pass_base, self.pass_frames = plan["pass_base"], plan["pass_frames"]

    def _upload_table(self):
        table = self.table_host
        self.table = torch.from_numpy(table if len(table) else np.zeros((1, ops.WINDOW_WORDS), dtype=np.int64)).to(self.device)

    def pass_table(self, p):
        """The window rows of pass ``p``: a view of the table in HBM."""
        if not 0 <= p < self.n_passes:
            raise ValueError("%s: pass %r of %d" % (type(self).__name__, p, self.n_passes))
        return self.table[p * self.batch_size:(p + 1) * self.batch_size]

    def _gather_pass(self, p, audio_out):
        audio = self._out(audio_out, (self.batch_size, self.n_samples, 4))
        return ops.corpus_gather_windows(self.pcm, self.pass_table(p), audio, self.status)

    def launch_view(self, p, comb, audio_out=None):
        """The audio of ``launch`` for pass ``p`` under combination ``comb`` (rotation test-time augmentation): FOA-rotated, or
        with ``data_config.audio_format: mic`` the capsules permuted (a combination that is no symmetry of the array:
        ``ValueError``), the padding of a short window turned with the rest.  Audio only -- a view has no labels -> audio
        (batch_size, n_samples, 4) f32.  The combination travels by value: nothing is uploaded, no host synchronisation.  A
        ``resample=True`` split is read as every pass reads it: the converted int16 stream."""
        from .augmentations import COMBINATIONS, MIC_SWAP_COMBS, mic_swap_source
        who = type(self).__name__
        comb = int(comb)
        if not 0 <= comb < len(COMBINATIONS):
            raise ValueError("%s.launch_view: combination %r is not one of 0..%d" % (who, comb, len(COMBINATIONS) - 1))
        if self.audio_format == "mic":
            mic_swap_source(comb)                                # ValueError: no symmetry of the array
            if self.mic_src is None:
                self.mic_src = ops.corpus_mic_table({k: mic_swap_source(k) for k in MIC_SWAP_COMBS})
        audio = self._out(audio_out, (self.batch_size, self.n_samples, 4))
        return ops.corpus_gather_windows_view(self.pcm, self.pass_table(p), comb, self.rot, audio, self.status,
                                              mic_src=self.mic_src)

    hold_block = 1                                      # the hold of ``track_plan`` is a whole multiple of this many frames

    def track_plan(self, opts):
        """Tracking through the passes (``postprocess.track_run``; ``test.test_epoch_windows(tracking=opts)``): built once per
        (max_gap, min_len), its tables uploaded once; a pass uploads nothing.  The hold D is ``track_hold(max_gap, min_len)``
        rounded up to ``hold_block`` frames.  Pass p walks the frames [b[p], b[p + 1]) of the common axis and EMITS [e[p], e[p
        + 1]): a bound that is a recording's start or end stays, one inside a recording moves back by D, not past that
        recording's start.  -> dict of
          hold         D
          bounds       e, int64 (passes + 1,), ascending (repeats: a pass that emits nothing)
          pass_base, pass_frames   e[p] and e[p + 1] - e[p] per pass
          segments_host            per pass the int32 (S, 4) table of ``track_run``: one row per recording with frames in the pass
          segments                 the same tables on the device."""
        from .postprocess import track_hold
        key = (int(opts["max_gap"]), int(opts["min_len"]))
        cache = self.__dict__.setdefault("_track_plans", {})
        if key not in cache:
            plan = plan_track(self.frame_start, self.pass_base + [int(self.frame_start[-1])],
                              -(-track_hold(*key) // self.hold_block) * self.hold_block)
            plan["segments"] = [torch.from_numpy(s).to(self.device) for s in plan["segments_host"]]
            cache[key] = plan
        return cache[key]


class InferDeviceCorpus(_WindowCorpus):
    """A ``load_infer_split`` / ``infer_split_from_arrays`` split in HBM, cut into windows of ONE shape for
    ``test.infer_epoch_corpus``: every recording's ``window_plan`` (F = length // hop_label label frames; F = 0: no window), all
    windows in file order, cut into passes of ``batch_size`` windows, the last pass filled up with empty windows.  The window
    table (``ops.WINDOW_WORDS`` int64 per window: stream offset, valid samples, src_lo, destination frame on the axis of all
    recordings laid end to end, n, recording) is built here once and uploaded once: no pass copies anything to the device.

        corpus = InferDeviceCorpus(load_infer_split(params), params, "cuda:0", window_s=20, margin_s=2.0, batch_size=8)
        audio = corpus.launch(p)                 # pass p: (batch_size, n_samples, 4) f32 on the device, no host sync

    window_s defaults to ``data_config.chunk_window_s`` (what the model was trained on), margin_s to 2.0 (a configuration
    default, not a tuned value); both must be whole multiples of the label hop, the window also of the feature hop.

    A split that carries native recordings (``load_infer_split(..., resample=True)``) is converted on the device during the
    upload (``_convert_native``); everything after the upload is the same."""

    def __init__(self, host_split, params, device="cuda:0", window_s=None, margin_s=None, batch_size=8):
        hc = host_split
        if hc.kind == HostCorpus.CHUNKED:
            raise ValueError("InferDeviceCorpus: the split of load_infer_split is needed (got the chunked training split)")
        sr = self._window_setup(hc, params, window_s, margin_s, batch_size)
        self._adopt(hc, device, hc.rank, hc.world, is_valid=True, is_infer=True)
        self._window_tables(hc)
        self._convert_native(hc, sr)
        self._upload_table()

    def _convert_native(self, hc, sr):
        """The recordings a ``resample=True`` / ``rates=`` split kept in their native rate or format: per (rate, kind) group the
        native samples uploaded as one stream, one ``ops.resample_pcm`` launch into ``self.pcm`` at the recordings' places, the
        native buffer dropped before the next group's upload (the allocator hands the block on in stream order: no sync).  The
        alignment tails stay int16 zero.  The status word is read after each group (one host synchronisation per group, beside
        uploads that block the host anyway): a non-finite float sample or a bad row raises ``AdyoloHipError`` naming the group,
        here and not in a later ``check()``, because ``infer_epoch_corpus`` clears the word when a pass begins."""
        native = hc.native
        if native is None:
            return
        from . import resample
        groups = {}
        for i, a in enumerate(native):
            if a is not None and a.shape[0]:
                groups.setdefault((int(hc.rates[i]), int(hc.kinds[i])), []).append(i)
        for (rate, kind), members in sorted(groups.items()):
            pl = resample.plan_for(rate, sr)
            recs, pos = [], 0
            for i in members:
                recs.append((pos, int(hc.native_lengths[i]), int(hc.rec_start[i]), int(hc.lengths[i])))
                pos += int(hc.native_lengths[i])
            stream = np.concatenate([native[i] for i in members], 0) if len(members) > 1 else np.ascontiguousarray(native[members[0]])
            src = torch.from_numpy(stream).to(self.device)
            del stream
            taps = torch.from_numpy(pl["taps"]).to(self.device)
            for r0 in range(0, len(recs), 32768):                           # rows per launch: the grid's second dimension
                rows = torch.tensor(recs[r0:r0 + 32768], dtype=torch.int64, device=self.device)
                ops.resample_pcm(src, rows, taps, pl["M"], pl["centre"], self.pcm, self.status)
            del src, taps
            # read here, once per group: a pass begins with reset_status(), so a bit left in the word would be lost unseen
            word = int(ops.to_host(self.status)[0])
            if word:
                self.status.zero_()
                shown = ", ".join(hc.rec_names[i] for i in members[:8]) + (", ..." if len(members) > 8 else "")
                why = "; ".join(msg for bit, msg in ops.CORPUS_STATUS if word & bit)
                raise ops._lib.AdyoloHipError("InferDeviceCorpus: converting the %d Hz %s recordings (%s) failed (status 0x%x): %s"
                                              % (rate, ("int16", "24-bit", "float32")[kind], shown, word, why))

    def nbytes(self):
        return int(self.pcm.numel() * 2 + self.table.numel() * 8)

    def launch(self, p, audio_out=None):
        """Pass ``p`` -> audio (batch_size, n_samples, 4) f32 on the device; no host data, no host synchronisation.  audio_out:
        write into this buffer (a recorded forward graph's input)."""
        return self._gather_pass(p, audio_out)


# ------------------------------------------------------------------------------------------- labelled windowed evaluation
def window_items(plan, label_frames, window_frames, ev_start, event_frames):
    """The label item row of every window of ``plan`` (``plan_windows``; pure NumPy) -> int64 (passes * batch_size,
    ``ops.CORPUS_ITEM_WORDS``): {stream offset, the window's first label frame on its recording's axis, first event, events, -1
    (no rotation), recording, 0, 0}.  The events of a window are the recording's frame-sorted events (``event_frames``: the
    frame column of the split's event table, ``ev_start`` its recordings) whose frame lies in [start, min(start + window_frames,
    the recording's label frames)), found by binary search; an empty window's row holds no events."""
    table = plan["table"]
    items = np.zeros((len(table), ops.CORPUS_ITEM_WORDS), dtype=np.int64)
    items[:, 4] = -1
    event_frames = np.asarray(event_frames, dtype=np.float64).reshape(-1)
    for w in range(plan["n_windows"]):
        r, start = int(table[w, 5]), int(plan["starts"][w])
        end = min(start + int(window_frames), int(label_frames[r]))
        e0, e1 = int(ev_start[r]), int(ev_start[r + 1])
        lo, hi = (int(v) for v in np.searchsorted(event_frames[e0:e1], [start, end], "left"))
        items[w] = (table[w, 0], start, e0 + lo, hi - lo, -1, r, 0, 0)
    return items


class EvalWindowCorpus(_WindowCorpus):
    """A ``load_eval_split`` split in HBM, cut into windows of ONE shape like ``InferDeviceCorpus``, with labels: labelled
    evaluation of recordings of any length for ``test.test_epoch_windows`` / ``test.sweep_conf_thresh_windows``.  The window
    table, one label item row per window and (per scorer, ``segments``) the scorer's segment tables are built once and uploaded
    once; a pass uploads nothing.

        corpus = EvalWindowCorpus(load_eval_split(params, "test"), params, "cuda:0", window_s=20, margin_s=2.0, batch_size=8)
        audio, target, row_start = corpus.launch(p)         # as EvalDeviceCorpus.launch, for the windows of pass p

    window_s / margin_s: ``InferDeviceCorpus``'s rules, and both must be whole multiples of the scorer's block (``fpb = int(sr
    / int(sr * label_hop_len_s))`` label frames, 10 at the usual rates; ``ValueError`` otherwise): kept ranges start at Wf - Mf
    and advance by Wf - 2 Mf, the tail-aligned last window starts where its predecessor stopped, so every pass boundary inside
    a recording falls on a block boundary (``adyolo_seld_score_runs``).  A recording without a label frame has no window; its
    zero-frame segment rides in the pass of the next recording (``seld_metrics.run_segments``).  A split without any window:
    ``ValueError``.  ``launch_view`` gives a pass's audio under a combination (rotation test-time augmentation).
    ``resample=True`` splits are not supported here."""

    def __init__(self, host_split, params, device="cuda:0", window_s=None, margin_s=None, batch_size=8, cap_per_window=None):
        hc = host_split
        if hc.kind != HostCorpus.EVAL:
            raise ValueError("EvalWindowCorpus: the split of load_eval_split is needed (got the %s split)" % hc.kind)
        self.loss_nm = params["args"]["loss"]
        if self.loss_nm != "adyolo" and self.loss_nm not in CLASSWISE_LABELS:
            raise NotImplementedError("EvalWindowCorpus: loss %s" % self.loss_nm)
        self.nb_classes = int(params["data_config"]["nb_classes"])
        dc = params["data_config"]
        sr = self._window_setup(hc, params, window_s, margin_s, batch_size)
        self.frames_per_block = fpb = int(sr / int(sr * dc.get("label_hop_len_s", 0.1)))     # DeviceSELDScorer's block
        self.hold_block = fpb                                        # emitted run bounds stay on block boundaries
        if self.window_frames % fpb or self.margin_frames % fpb:
            raise ValueError("EvalWindowCorpus: a window of %d label frames with a margin of %d: both must be whole multiples of "
                             "the scorer's block (%d frames)" % (self.window_frames, self.margin_frames, fpb))
        if not any(int(v) // int(hc.hop_label) for v in hc.lengths.tolist()):
            raise ValueError("EvalWindowCorpus: no recording of the split holds a label frame: there is no window to run")
        self._adopt(hc, device, hc.rank, hc.world, is_valid=True)
        self._window_tables(hc)
        plan = {"table": self.table_host, "starts": self.window_starts, "n_windows": self.n_windows}
        items = window_items(plan, self.label_frames, self.window_frames, hc.ev_start, hc.events[:, 0])
        self.items_host = items
        self.max_events = int(items[:, 3].max())                     # the largest event count of a WINDOW
        self.pass_bounds = self.pass_base + [int(self.frame_start[-1])]
        self._upload_table()
        self.items = torch.from_numpy(items).to(self.device)
        self._segments = {}
        if self.loss_nm == "adyolo":
            self._yolo_tables(params)
            self.cap_per_window = int(cap_per_window) if cap_per_window is not None else max(1, self.max_events * self.cells)
            self.xyz = None
        else:
            full = np.zeros((max(1, hc.events.shape[0]), ops.CORPUS_XYZ_SLOTS, 3), dtype=np.float32)
            if hc.events.shape[0]:
                full[:, 0] = xyz_unrotated(hc.events[:, 3], hc.events[:, 4])     # only the unrotated slot is read
            self.xyz = torch.from_numpy(full).to(self.device)

    def nbytes(self):
        return super().nbytes() + int((self.table.numel() + self.items.numel()) * 8) + \
            (int(self.xyz.numel() * 4) if self.xyz is not None else 0)

    def cap(self):
        """Target rows of a pass (AD-YOLO)."""
        return self._round_cap(self.batch_size * self.cap_per_window)

    def windows_in_pass(self, p):
        """The windows of pass ``p`` that belong to a recording (the others, at the end of the last pass, are empty)."""
        return max(0, min(self.batch_size, self.n_windows - p * self.batch_size))

    def segments(self, scorer, bounds=None):
        """``scorer.segment_tables`` for this corpus's passes: built and uploaded on the first call, cached per scorer.
        bounds: other run bounds than the passes' (the emitted bounds of ``track_plan``; repeated ones, runs without a frame,
        are dropped) -> one entry per pass, None for a pass whose run is empty."""
        if bounds is None:
            hit = self._segments.get(id(scorer))
            if hit is None or hit[0] is not scorer:
                hit = self._segments[id(scorer)] = (scorer, scorer.segment_tables(self.get_filelist(), self.label_frames,
                                                                                  self.pass_bounds))
            return hit[1]
        bounds = [int(v) for v in np.asarray(bounds).reshape(-1).tolist()]
        key = (id(scorer), tuple(bounds))
        hit = self._segments.get(key)
        if hit is None or hit[0] is not scorer:
            tables = iter(scorer.segment_tables(self.get_filelist(), self.label_frames, sorted(set(bounds))))
            hit = self._segments[key] = (scorer, [next(tables) if hi > lo else None for lo, hi in zip(bounds, bounds[1:])])
        return hit[1]

    def launch(self, p, audio_out=None):
        """Pass ``p`` -> (audio (batch_size, n_samples, 4) f32, target, row_start) on the device, as ``EvalDeviceCorpus.launch``
        with a window for a clip: the AD-YOLO rows (cap(), 7) and row_start (batch_size + 1,) int32, or the dense class-wise
        target (batch_size, window_frames, ...) and None; an empty window has no rows / an all-zero target.  No host data, no
        host synchronisation.  audio_out: write the audio into this buffer (a recorded forward graph's input)."""
        b, frames = self.batch_size, self.window_frames
        audio = self._gather_pass(p, audio_out)
        items = self.items[p * b:(p + 1) * b]
        if self.loss_nm != "adyolo":
            target = torch.empty(ops.corpus_classwise_shape(self.loss_nm, b, frames, self.nb_classes), dtype=torch.float32,
                                 device=self.device)
            ops.corpus_classwise_labels(self.events, items, self.xyz, self.max_events, frames, self.nb_classes, self.loss_nm,
                                        target, self.status)
            return audio, target, None
        me = self.max_events
        target = torch.empty((self.cap(), 7), dtype=torch.float32, device=self.device)
        ws = torch.zeros(b * max(me, 1) + 1, dtype=torch.int32, device=self.device)
        ops.corpus_yolo_labels(self.events, items, me, frames, self.bounds, self.grid, self.rot, ws, target,
                               ws[b * max(me, 1):], self.status)
        row_start = ws[::max(me, 1)].contiguous()
        return audio, target, row_start


# ----------------------------------------------------------------------------------------------------- streaming inference
def stream_plan(window_frames, margin_frames, hop_frames, hop_label, planned, pushed, closing=False):
    """The window plan of a LIVE stream, whose end is not known: the definition (pure Python) of what
    ``StreamDeviceCorpus`` runs.  Wf = window_frames, Mf = margin_frames, Hf = hop_frames, all in label frames of ``hop_label``
    samples; ``ValueError`` unless Mf >= 1 and 1 <= Hf <= Wf - 2 Mf.  F = pushed // hop_label label frames are there.

    While the stream is open, step k = 0, 1, ... is runnable as soon as k Hf + Wf <= F.  Its window starts at frame k Hf; step 0
    keeps the window-local frames [0, Wf - Mf), step k >= 1 keeps [Wf - Mf - Hf, Wf - Mf): the stream's frames [k Hf + Wf - Mf
    - Hf, k Hf + Wf - Mf).  On close at F frames: F == 0 nothing; F <= Wf and no step ran: one window (0, 0, 0, F) whose valid
    samples are all pushed samples, capped at the window (the rule of ``plan_windows``: the sub-frame remainder is fed);
    otherwise one tail-aligned window starting at F - Wf that keeps from where the last step stopped up to F.  Mf >= 1 makes
    that closing window keep at least one frame, so an open tracker carry can always be flushed by a call that has frames.

    The kept ranges tile [0, F) exactly once, in order; every kept frame of a window that is not the first has at least Mf
    frames of context on its left, every kept frame of a window that is not the closing one Mf on its right.  With Hf = Wf - 2
    Mf every frame is kept from a window that starts where the window keeping it in ``window_plan(F, Wf, Mf)`` starts: the two
    plans are the same unless (F - Wf) % Hf == 0, when the stream has already run the last start as a step and runs it once
    more as the closing window.

    The form is incremental: ``planned`` is the number of frames the rows returned so far keep (0 at the start; each call's
    rows end at its own new value, the dst + n of the last row), ``pushed`` the samples pushed so far, ``closing`` whether the
    stream ends here -> the NEW rows, in the layout of ``ops.WINDOW_WORDS`` that ``adyolo_decode_stitch`` takes unchanged:
    (absolute sample offset since the stream began, valid samples, src_lo, dst frame on the stream's axis, n, 0, 0, 0).  The
    calls over any partition of a stream, concatenated, are the one call (0, total, closing=True).

    Latency: frame f is final once a window that ends at or after f + Mf has run, at most Mf + Hf frames after f was pushed
    (the frames of step 0 wait for the first whole window, Wf frames; the closing window makes the rest final at once).  With tracking a frame is held back a further ``hold`` frames
    (``postprocess.track_hold``)."""
    wf, mf, hf, hop = int(window_frames), int(margin_frames), int(hop_frames), int(hop_label)
    planned, pushed = int(planned), int(pushed)
    if mf < 1 or hf < 1 or hf > wf - 2 * mf:
        raise ValueError("stream_plan: a window of %d frames, a margin of %d, a hop of %d (margin >= 1, 1 <= hop <= window - "
                         "2 * margin)" % (wf, mf, hf))
    if hop < 1 or pushed < 0:
        raise ValueError("stream_plan: %d samples pushed, a label hop of %d" % (pushed, hop))
    f = pushed // hop
    # ``planned`` is 0 or where a step stopped, k Hf + Wf - Mf (or F of a closed stream: nothing is left to plan)
    if planned < 0 or planned > f or (planned and planned != f and (planned < wf - mf or (planned - (wf - mf)) % hf)):
        raise ValueError("stream_plan: %d frames planned of %d (not where a step stops)" % (planned, f))
    if planned == f:
        return []
    n, rows = wf * hop, []
    k = 0 if planned == 0 else (planned - (wf - mf)) // hf + 1
    while k * hf + wf <= f:
        lo = 0 if k == 0 else wf - mf - hf
        rows.append((k * hf * hop, n, lo, k * hf + lo, wf - mf - lo, 0, 0, 0))
        planned = k * hf + wf - mf
        k += 1
    if closing:
        if planned == 0:                                              # F <= Wf and no step ran
            rows.append((0, min(pushed, n), 0, 0, f, 0, 0, 0))
        else:
            start = f - wf
            rows.append((start * hop, n, planned - start, planned, f - planned, 0, 0, 0))
    return rows


class StreamDeviceCorpus(_WindowCorpus):
    """ONE live stream of int16 4-channel audio at ``data_config.sr`` on the device, for ``test.StreamInference``: a ring in HBM
    that takes samples as they come (absolute sample s at ``ring[s % capacity]``), the windows of ``stream_plan`` gathered out
    of it (``ops.stream_gather_windows``) in passes of ONE shape, (batch_size, n_samples, 4), so one recorded graph serves the
    whole stream.

        corpus = StreamDeviceCorpus(params, "cuda:0", window_s=20, margin_s=2.0, hop_s=1.0)
        taken = corpus.append(pcm)               # int16 (n, 4), any n: -> how many samples the ring took
        for _ in range(corpus.runnable()):
            audio = corpus.launch()              # (batch_size, n_samples, 4) f32, no host sync

    window_s / margin_s: as ``InferDeviceCorpus``, the margin at least one label frame.  hop_s: the step from window to window,
    a whole number of label hops between 1 and window - 2 margin (the default: the plan of ``window_plan``).  A pass is up to
    batch_size consecutive runnable windows of the stream (catch-up after a large push), then empty filler windows.

    capacity_s: the ring.  A sample must stay until no later window reads it.  The last launched step starts at k Hf; the
    closing window starts at F - Wf >= k' Hf for the last runnable step k' >= k, and every later step starts later still: so
    everything from the start of the last launched window (0 before the first) is kept, and nothing older is needed.  Step k +
    1 ends Hf + Wf frames after that point, so the smallest ring that always lets the next step become runnable holds (Wf +
    Hf) label frames = n_samples + hop samples; less is refused.  The default, n_samples + batch_size hops, lets a catch-up
    pass fill its batch.  ``append`` takes what fits (never overwriting a kept sample) and returns the count; the rest is
    appended after the runnable passes have been launched -- ``StreamInference.push`` does that, so any push size works.

    Per push: one copy into a page-locked staging buffer (two of them, alternating: a buffer is written again only when the
    copy out of it has landed) and at most two asynchronous copies into the ring (two when the piece crosses the seam); per
    pass one asynchronous copy of the pass's window table from page-locked memory.  No kernel, no blocking copy.  The views of
    a pass (``launch_view``) are gathered before the next ``append``: a window that has been overwritten is a bad item."""

    def __init__(self, params, device="cuda:0", window_s=None, margin_s=None, hop_s=None, batch_size=1, capacity_s=None):
        from types import SimpleNamespace
        from .augmentations import COMBINATIONS
        who = "StreamDeviceCorpus"
        dc = params["data_config"]
        hop = int(dc.get("sr", 24000) * dc.get("label_hop_len_s", 0.1))                 # FoaDataset.hop_label
        sr = self._window_setup(SimpleNamespace(hop_label=hop), params, window_s, margin_s, batch_size)
        wf, mf = self.window_frames, self.margin_frames
        if mf < 1:
            raise ValueError("%s: a margin of at least one label frame is needed (the closing window must keep a frame)" % who)
        if hop_s is None:
            h = (wf - 2 * mf) * hop
        else:
            h = int(round(sr * float(hop_s)))
            if h <= 0 or abs(h - sr * float(hop_s)) > 1e-6 or h % hop:
                raise ValueError("%s: hop %r s is not a whole multiple of the label hop (%d samples at %d Hz)" % (who, hop_s, hop, sr))
        self.hop_frames = h // hop
        if not 1 <= self.hop_frames <= wf - 2 * mf:
            raise ValueError("%s: a hop of %d label frames with a window of %d and a margin of %d (1 <= hop <= window - 2 * "
                             "margin)" % (who, self.hop_frames, wf, mf))
        self.hop_label = hop
        self.min_capacity = self.n_samples + h
        if capacity_s is None:
            cap = self.n_samples + self.batch_size * h
        else:
            cap = int(round(sr * float(capacity_s)))
            if abs(cap - sr * float(capacity_s)) > 1e-6:
                raise ValueError("%s: capacity %r s is not a whole number of samples at %d Hz" % (who, capacity_s, sr))
        if cap < self.min_capacity or cap & 1:
            raise ValueError("%s: a ring of %d samples; it must be even and hold a window and a hop, %d samples (%g s)"
                             % (who, cap, self.min_capacity, self.min_capacity / sr))
        self.capacity = cap
        self.device = torch.device(device)
        self.ring = torch.zeros((cap, 4), dtype=torch.int16, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.rot = ops.corpus_rot_table(COMBINATIONS)
        self._stage = [torch.empty((cap, 4), dtype=torch.int16).pin_memory() for _ in range(2)]
        self._table_host = [torch.empty((self.batch_size, ops.WINDOW_WORDS), dtype=torch.int64).pin_memory() for _ in range(2)]
        self._table = torch.zeros((self.batch_size, ops.WINDOW_WORDS), dtype=torch.int64, device=self.device)
        self._stage_ev, self._table_ev, self._stage_slot, self._table_slot = [None, None], [None, None], 0, 0
        self.reset()

    def reset(self):
        """A new stream in the same buffers: nothing pushed, nothing planned, the status word cleared.  No allocation."""
        self.head, self.planned, self.closed = 0, 0, False
        self._pending, self._low = [], 0
        self.n_windows = self.n_passes = 0
        # the CURRENT pass (a stream has no pass p to ask for: ``pass_table`` is the table itself, not ``_WindowCorpus``'s lookup)
        self.pass_table, self.pass_base, self.pass_frames, self.pass_windows, self.pass_closing = None, 0, 0, 0, False
        self.pass_rows = []
        self.status.zero_()

    def nbytes(self):
        return int(self.ring.numel() * 2 + self._table.numel() * 8)

    @property
    def frames(self):
        """Label frames pushed so far."""
        return self.head // self.hop_label

    @property
    def free(self):
        """Samples ``append`` can take now."""
        return self._low + self.capacity - self.head

    def append(self, pcm):
        """pcm int16 (n, 4), any n >= 0 -> the number of samples taken, min(n, ``free``): the rest does not fit until the
        runnable passes have been launched.  No host synchronisation beyond the staging buffer's own event."""
        if self.closed:
            raise ValueError("StreamDeviceCorpus.append: the stream is closed (reset() starts a new one)")
        if torch.is_tensor(pcm):
            pcm = pcm.numpy()
        if getattr(pcm, "dtype", None) != np.int16 or pcm.ndim != 2 or pcm.shape[1] != 4:
            raise ValueError("StreamDeviceCorpus.append: %s %s, expected int16 (n, 4)"
                             % (getattr(pcm, "dtype", type(pcm).__name__), tuple(getattr(pcm, "shape", ()))))
        take = min(int(pcm.shape[0]), self.free)
        if take <= 0:
            return 0
        slot = self._stage_slot
        self._stage_slot ^= 1
        if self._stage_ev[slot] is not None:
            self._stage_ev[slot].synchronize()            # the copies out of this buffer two pushes ago have landed
        stage = self._stage[slot]
        stage.numpy()[:take] = pcm[:take]
        at = self.head % self.capacity
        first = min(take, self.capacity - at)
        self.ring[at:at + first].copy_(stage[:first], non_blocking=True)
        if first < take:                                  # across the seam
            self.ring[:take - first].copy_(stage[first:take], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._stage_ev[slot] = ev
        self.head += take
        return take

    def runnable(self, closing=False):
        """The number of passes that can be launched now.  closing: the stream ends here -- the closing window is planned with
        the steps still runnable, and ``append`` is refused from now on."""
        if not self.closed:
            rows = stream_plan(self.window_frames, self.margin_frames, self.hop_frames, self.hop_label, self.planned, self.head,
                               closing)
            if rows:
                self._pending += rows
                self.planned = rows[-1][3] + rows[-1][4]
            self.closed = bool(closing)
        return -(-len(self._pending) // self.batch_size)

    def _next_pass(self):
        rows = self._pending[:self.batch_size]
        if not rows:
            raise ValueError("StreamDeviceCorpus.launch: no window is runnable (runnable() says how many passes are)")
        del self._pending[:len(rows)]
        end = rows[-1][3] + rows[-1][4]
        self.pass_rows = rows + [(0, 0, 0, end, 0, -1, 0, 0)] * (self.batch_size - len(rows))       # empty windows
        self.pass_base, self.pass_frames, self.pass_windows = rows[0][3], end - rows[0][3], len(rows)
        self.pass_closing = self.closed and not self._pending
        self._low = rows[-1][0]
        self.n_windows += len(rows)
        self.n_passes += 1
        slot = self._table_slot
        self._table_slot ^= 1
        if self._table_ev[slot] is not None:
            self._table_ev[slot].synchronize()            # the copy out of this page-locked table two passes ago has landed
        host = self._table_host[slot]
        host.numpy()[:] = np.asarray(self.pass_rows, dtype=np.int64)
        self._table.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._table_ev[slot] = ev
        self.pass_table = self._table

    def launch(self, audio_out=None):
        """The next pass -> audio (batch_size, n_samples, 4) f32 on the device; ``pass_table`` (the rows in HBM), ``pass_rows``
        (on the host), ``pass_base``, ``pass_frames``, ``pass_windows`` and ``pass_closing`` (the pass holds the closing
        window) then describe it.  The table goes up from page-locked memory; no host synchronisation.  audio_out: write into
        this buffer (a recorded forward graph's input)."""
        audio = self._out(audio_out, (self.batch_size, self.n_samples, 4))
        self._next_pass()
        return ops.stream_gather_windows(self.ring, self.head, self.pass_table, audio, self.status)

    def launch_view(self, comb, audio_out=None):
        """The audio of the CURRENT pass (the last ``launch``) under combination ``comb``: as ``_WindowCorpus.launch_view``."""
        from .augmentations import COMBINATIONS, MIC_SWAP_COMBS, mic_swap_source
        who = "StreamDeviceCorpus"
        comb = int(comb)
        if self.pass_table is None:
            raise ValueError("%s.launch_view: no pass has been launched" % who)
        if not 0 <= comb < len(COMBINATIONS):
            raise ValueError("%s.launch_view: combination %r is not one of 0..%d" % (who, comb, len(COMBINATIONS) - 1))
        if self.audio_format == "mic":
            mic_swap_source(comb)                                # ValueError: no symmetry of the array
            if self.mic_src is None:
                self.mic_src = ops.corpus_mic_table({k: mic_swap_source(k) for k in MIC_SWAP_COMBS})
        audio = self._out(audio_out, (self.batch_size, self.n_samples, 4))
        return ops.stream_gather_windows(self.ring, self.head, self.pass_table, audio, self.status, comb=comb, rot=self.rot,
                                         mic_src=self.mic_src)
