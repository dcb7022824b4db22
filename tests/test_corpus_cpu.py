"""CPU: the host half of the HBM-resident corpus (ad-yolo_amd/corpus.py).  A synthetic DCASE-layout split is chunked here by a
restatement of the reference's ``chunk_instance`` (20 s window, 1 s stride, zero-padded last window, chunk CSVs with frames
relative to the window); ``load_chunked_split`` must rebuild every chunk bit for bit from its recording's stream and every CSV
from its event table, catch a chunk that disagrees with its neighbours, and ``DeviceCorpus`` must draw the files, rotations and
SpecAug tables that ``FoaDataset`` draws from the same ``random`` state (the sampling surface is built without a GPU)."""
import csv
import os
import random

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import adyolo_amd  # noqa: F401
from adyolo_amd.corpus import DeviceCorpus, load_chunked_split, max_cells_per_event
from adyolo_amd.datasets import FoaDataset, YoloLabelEncoder

SR = 2400                      # a low rate keeps the split small; every length below is in seconds as in the reference
RECORDINGS = (("fold1_room1_mix001", 60.0), ("fold1_room2_mix002", 37.4), ("fold2_room1_mix003", 20.0),
              ("fold3_take_chunk7_mix", 24.0))                                 # 41 + 19 + 1 + 5 = 66 chunks


def chunk_instance(audio, label, sr, window_s, stride_s, hop_s):
    """The reference's preprocess.chunk_instance, restated: (audio slice, {relative frame: events}) per window."""
    win, st = int(sr * window_s), int(sr * stride_s)
    cw, cs = int(window_s / hop_s), int(stride_s / hop_s)
    pad = st - (len(audio) - win) % st if (len(audio) - win) % st != 0 else 0
    audio = np.pad(audio, [(0, pad), (0, 0)], "constant")
    windows = list(sliding_window_view(audio, win, axis=0)[::st].transpose(0, 2, 1))
    idx = np.arange(0, int(len(audio) / float(int(sr * hop_s))))
    lab = list(sliding_window_view(idx, cw, axis=0)[::cs])
    assert len(windows) == len(lab)
    out = []
    for a, fi in zip(windows, lab):
        sl = {}
        for f in range(cw):
            if label.get(fi[f]) is not None and f not in sl:
                sl[f] = label.get(fi[f])
        out.append((np.ascontiguousarray(a), sl))
    return out, audio


def _events(rs, n_frames, window_f=200, stride_f=10):
    """{frame: [[cls, src, az, el], ...]} frames ascending; az = 180 / -180, el = +-90, first and last frames of windows."""
    special = [(180.0, 0.0), (-180.0, 12.5), (0.0, 90.0), (45.0, -90.0), (179.999, 89.9), (-0.25, -45.0), (90.0, 22.5)]
    label = {}
    forced = {0, n_frames - 1, window_f - 1, stride_f, stride_f + window_f - 1}
    for f in range(n_frames):
        k = rs.choice(4, p=[0.55, 0.3, 0.1, 0.05])
        if f in forced:
            k = max(k, 1)
        evs = []
        for s in range(k):
            if rs.rand() < 0.3:
                az, el = special[rs.randint(len(special))]
            else:
                az, el = float(rs.uniform(-180, 180)), float(rs.uniform(-90, 90))
            evs.append([int(rs.randint(13)), s, az, el])
        if evs:
            label[f] = evs
    return label


def write_split(root, recordings=RECORDINGS, sr=SR, window_s=20, stride_s=1, hop_s=0.1, seed=0):
    """The chunked training split of ``recordings`` under root (foa_dev / metadata_dev, dev-train-chunked_<w>s_<s>s), written as
    the reference's chunker writes it.  -> {recording: padded int16 stream}."""
    rs = np.random.RandomState(seed)
    sub = "dev-train-chunked_{}s_{}s".format(window_s, stride_s)
    wdir, cdir = os.path.join(root, "foa_dev", sub), os.path.join(root, "metadata_dev", sub)
    os.makedirs(wdir, exist_ok=True)
    os.makedirs(cdir, exist_ok=True)
    from scipy.io import wavfile
    streams = {}
    for rec, secs in recordings:
        n = int(round(secs * sr))
        audio = rs.randint(-32768, 32768, size=(n, 4)).astype(np.int16)
        label = _events(rs, int(n / int(sr * hop_s)), int(window_s / hop_s), int(stride_s / hop_s))
        chunks, padded = chunk_instance(audio, label, sr, window_s, stride_s, hop_s)
        streams[rec] = padded
        for i, (a, sl) in enumerate(chunks):
            name = "%s_chunk%03d" % (rec, i + 1)
            wavfile.write(os.path.join(wdir, name + ".wav"), sr, a)
            with open(os.path.join(cdir, name + ".csv"), "w", newline="") as fid:
                w = csv.writer(fid, delimiter=",", quoting=csv.QUOTE_NONE)
                for frame, events in sl.items():
                    for ev in events:
                        w.writerow([int(frame), int(ev[0]), int(ev[1]), ev[2], ev[3]])
    return streams


def params_for(root, batch_size=4, nb_iters=11, rotation=True, spec=True, window_s=20, stride_s=1, sr=SR):
    return {"args": {"device": "cpu", "encoder": "se-resnet34", "loss": "adyolo"},
            "data_config": {"nb_classes": 13, "data_pth": str(root), "chunk_window_s": window_s, "chunk_stride_s": stride_s,
                            "sr": sr, "label_hop_len_s": 0.1},
            "train_config": {"grid_size": [45, 45], "nb_anchors": 5, "train_unify": [45.0, 25.0, 10.0], "g_overlap": 0.5,
                             "batch_size": batch_size, "nb_iters": nb_iters},
            "aug_config": {"rotation_augment": rotation, "spec_augment": spec, "spec_augment_thresh": 0.6,
                           "spec_augment_time_mask_param": 20, "spec_augment_freq_mask_param": 16}}


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    root = tmp_path_factory.mktemp("corpus")
    streams = write_split(root)
    return root, streams


def _flat(label):
    return [(float(f), float(e[0]), float(e[1]), float(e[2]), float(e[3])) for f, evs in label.items() for e in evs]


def test_every_chunk_is_its_rebuilt_window_and_every_csv_its_table_slice(split):
    from scipy.io import wavfile
    root, streams = split
    hc = load_chunked_split(params_for(root), verify="all")
    assert sorted(hc.total_filelist) == sorted(n.replace(".wav", "") for n in os.listdir(hc.wav_pth))
    assert hc.total_filelist == [n.replace(".wav", "") for n in os.listdir(hc.wav_pth)]     # listdir order, as FoaDataset
    assert len(hc.total_filelist) == 66 and hc.rec_names == sorted(r for r, _ in RECORDINGS)
    assert hc.window == 20 * SR and hc.stride == SR and hc.window_frames == 200
    for r, rec in enumerate(hc.rec_names):                       # each stream is the padded recording, chunk suffix parsed last
        s0 = int(hc.rec_start[r])
        assert np.array_equal(hc.audio[s0:s0 + len(streams[rec])], streams[rec])
    assert int(hc.rec_start[-1]) % 16 == 0 and all(int(s) % 16 == 0 for s in hc.rec_start)
    max_ev = 0
    for name in hc.total_filelist:
        rec, off, f_off = hc.chunks[name]
        _, data = wavfile.read(os.path.join(hc.wav_pth, name + ".wav"))
        assert np.array_equal(data, hc.audio[off:off + hc.window]), name
        lo, n = hc.chunk_events[name]
        ev = hc.events[lo:lo + n]
        got = [(e[0] - f_off,) + tuple(e[1:]) for e in ev.tolist()]
        assert got == _flat(FoaDataset.load_csv2dict(os.path.join(hc.csv_pth, name + ".csv"))), name
        assert hc.rec_names[rec] == name[:name.rfind("_chunk")]
        max_ev = max(max_ev, n)
    assert hc.max_events == max_ev > 0
    # the last window of the 37.4 s recording ends in the chunker's zero padding
    r = hc.rec_names.index("fold1_room2_mix002")
    tail = hc.audio[int(hc.rec_start[r]) + int(round(37.4 * SR)):int(hc.rec_start[r]) + len(streams["fold1_room2_mix002"])]
    assert tail.shape[0] > 0 and not tail.any()


def test_a_changed_overlap_sample_is_caught_and_named(split, tmp_path):
    import shutil
    from scipy.io import wavfile
    root, _ = split
    for d in ("foa_dev", "metadata_dev"):
        shutil.copytree(os.path.join(root, d), os.path.join(tmp_path, d))
    prm = params_for(tmp_path)
    name = "fold1_room1_mix001_chunk007"                         # not first, middle or last: only verify="all" reads it whole
    path = os.path.join(load_chunked_split(prm, verify="none").wav_pth, name + ".wav")
    sr, data = wavfile.read(path)
    data = data.copy()
    data[100, 2] ^= 1                                            # inside the overlap with chunk 006 (not the new last second)
    wavfile.write(path, sr, data)
    load_chunked_split(prm, verify="sample")                     # the sampled chunks are intact
    with pytest.raises(ValueError, match=name):
        load_chunked_split(prm, verify="all")


def test_bad_headers_and_csvs_are_named(split, tmp_path):
    import shutil
    from scipy.io import wavfile
    root, _ = split
    for d in ("foa_dev", "metadata_dev"):
        shutil.copytree(os.path.join(root, d), os.path.join(tmp_path, d))
    prm = params_for(tmp_path)
    wav_pth = load_chunked_split(prm, verify="none").wav_pth
    name = "fold2_room1_mix003_chunk001"
    wavfile.write(os.path.join(wav_pth, name + ".wav"), SR, np.zeros((20 * SR, 2), dtype=np.int16))
    with pytest.raises(ValueError, match=name):
        load_chunked_split(prm, verify="none")
    wavfile.write(os.path.join(wav_pth, name + ".wav"), SR, np.zeros((20 * SR, 4), dtype=np.int16))
    csv_pth = os.path.join(tmp_path, "metadata_dev", os.path.basename(wav_pth))
    bad = "fold1_room1_mix001_chunk012"
    with open(os.path.join(csv_pth, bad + ".csv"), "a") as f:
        f.write("5,3,0,10.0,20.0\n")                             # a row no neighbouring chunk has
    with pytest.raises(ValueError, match=bad):
        load_chunked_split(prm, verify="none")


def _host_epoch(ds):
    """FoaDataset iterated in the main process: per item (file, comb, spec table)."""
    out = []
    for i in range(len(ds)):
        item = ds[i]
        out.append((ds.filelist[i], item[1], item[3].tolist() if len(item) == 4 else None))
    return out


def _corpus_epoch(corpus, bs):
    out = []
    files = corpus.get_filelist()
    for b0 in range(0, len(files), bs):
        idx = range(b0, min(len(files), b0 + bs))
        items, spec = corpus.draw(idx)
        for j, i in enumerate(idx):
            rec, off, f_off = corpus.host.chunks[files[i]]
            assert (items[j, 0], items[j, 1], items[j, 5]) == (off, f_off, rec)
            out.append((files[i], int(items[j, 4]), spec[j].tolist() if spec is not None else None))
    return out


def _branch(ds):
    return "sample" if len(ds.remaining_file) >= ds.nb_samples else ("refill" if len(ds.remaining_file) <= 0 else "wrap")


@pytest.mark.parametrize("spec", [True, False], ids=["specaug", "rotation_only"])
def test_three_epochs_draw_what_foadataset_draws(split, spec):
    root, _ = split
    prm = params_for(root, batch_size=4, nb_iters=11, spec=spec)       # 44 of 66 files per epoch
    hc = load_chunked_split(prm)

    def run(make, epoch):
        random.seed(1234)
        ds = make()
        seq, branches = [epoch(ds)], []
        for _ in range(3):
            branches.append(_branch(ds))
            ds.sample_filelist_for_train_iter()
            seq.append(epoch(ds))
        return seq, branches, random.getstate(), ds

    host, hb, hstate, _ = run(lambda: FoaDataset(prm, "train", rank=0, world=1), _host_epoch)
    dev, db, dstate, corpus = run(lambda: DeviceCorpus(hc, prm, "cpu", rank=0, world=1), lambda c: _corpus_epoch(c, 4))
    assert hb == db == ["wrap", "sample", "refill"]                  # after the constructor's draw (66 -> 22)
    assert host == dev and hstate == dstate
    assert len(corpus) == 44 and corpus.nb_samples == 44
    combs = {c for ep in dev for _, c, _ in ep}
    assert combs <= set(range(16)) and len(combs) > 8
    if spec:
        assert any(s != [[0, 0, 0, 0], [0, 0, 0, 0]] for ep in dev for _, _, s in ep)


def test_all_three_sampling_branches_are_reached(split):
    """66 files, 44 per epoch: sample (66 -> 22), wrap-around (22 -> 44), sample (44 -> 0), refill (0 -> 22)."""
    root, _ = split
    prm = params_for(root, batch_size=4, nb_iters=11)
    hc = load_chunked_split(prm)
    random.seed(7)
    c = DeviceCorpus(hc, prm, "cpu", rank=0, world=1)
    seen = []
    for _ in range(3):
        seen.append(_branch(c))
        c.sample_filelist_for_train_iter()
    assert seen == ["wrap", "sample", "refill"]
    random.seed(7)
    ds = FoaDataset(prm, "train", rank=0, world=1)
    for _ in range(3):
        ds.sample_filelist_for_train_iter()
    assert ds.get_filelist() == c.get_filelist() and ds.get_remaining_file() == c.get_remaining_file()


def test_resume_from_remaining_file_is_identical(split):
    root, _ = split
    prm = params_for(root, batch_size=4, nb_iters=11)
    hc = load_chunked_split(prm)
    random.seed(99)
    c = DeviceCorpus(hc, prm, "cpu", rank=0, world=1)
    saved = list(c.get_remaining_file())                     # what a checkpoint stores
    state = random.getstate()
    c.sample_filelist_for_train_iter()
    want = (list(c.get_filelist()), _corpus_epoch(c, 4))
    for make in (lambda: DeviceCorpus(hc, prm, "cpu", rank=0, world=1), lambda: FoaDataset(prm, "train", rank=0, world=1)):
        random.seed(5)
        other = make()
        other.init_remaining_file_from_list(list(saved))
        random.setstate(state)
        other.sample_filelist_for_train_iter()
        got = _corpus_epoch(other, 4) if isinstance(other, DeviceCorpus) else _host_epoch(other)
        assert (list(other.get_filelist()), got) == want


def test_rank_shards_are_disjoint_and_cover_the_single_process_draw(split):
    root, _ = split
    prm2 = params_for(root, batch_size=4, nb_iters=5)               # 4 x 5 x 2 = 40 files per global draw
    prm1 = params_for(root, batch_size=4, nb_iters=10)              # the same global draw on one process
    hc = load_chunked_split(prm2)
    shards, hosts = [], []
    for rank in (0, 1):
        random.seed(3)
        shards.append(DeviceCorpus(hc, prm2, "cpu", rank=rank, world=2))
        random.seed(3)
        hosts.append(FoaDataset(prm2, "train", rank=rank, world=2))
    random.seed(3)
    single = DeviceCorpus(hc, prm1, "cpu", rank=0, world=1)
    for _ in range(2):
        a, b, full = shards[0].get_filelist(), shards[1].get_filelist(), single.get_filelist()
        assert sorted(a + b) == sorted(full)
        if len(set(full)) == len(full):                          # (a wrap-around draw may repeat a file, as upstream)
            assert not set(a) & set(b)
        assert a == single.get_filelist()[0::2] and b == single.get_filelist()[1::2]
        assert a == hosts[0].get_filelist() and b == hosts[1].get_filelist()
        st = random.getstate()
        for s in shards + hosts:
            random.setstate(st)
            s.sample_filelist_for_train_iter()
        random.setstate(st)
        single.sample_filelist_for_train_iter()


def test_capacity_bound_and_refusals(split):
    root, _ = split
    enc = YoloLabelEncoder(grid_size=(45, 45), g_overlap=0.5)
    cells = max_cells_per_event(enc)
    az = np.linspace(-180, 180, 7201)
    el = np.linspace(-90, 90, 3601)
    n_az = max(int((((enc.az_lb <= (-180.0 if a == 180 else a)) & ((-180.0 if a == 180 else a) < enc.az_ub))
                     | ((-180.0 if a == 180 else a) + 360 < enc.az_ub) | (enc.az_lb < (-180.0 if a == 180 else a) - 360)).sum())
               for a in az)
    n_el = max(int(((enc.el_lb <= e) & (e < enc.el_ub)).sum()) for e in el)
    assert cells == n_az * n_el
    rows = enc.encode_events([0] * 3, [1] * 3, [0.0, 22.5, -45.0], [0.0, 45.0, 0.0])
    assert rows.shape[0] <= 3 * cells
    prm = params_for(root)
    prm["args"]["loss"] = "accdoa"
    with pytest.raises(NotImplementedError, match="accdoa"):
        DeviceCorpus(load_chunked_split(params_for(root)), prm, "cpu")
    with pytest.raises(ValueError):
        load_chunked_split(params_for(root), set_type="valid")
