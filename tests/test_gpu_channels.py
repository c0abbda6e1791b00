"""Per-channel detection on a real MI355X: ss_add_pcm_channels* (no mixdown: a recording of C channels becomes C signals), the merged
table ss_get_regions_union ("speech on any channel"), ss_get_region_peaks, and the drop-in's settings.hip_channel_mode = 'each'.

The oracle is inside the project: channel c of a recording run alone must equal the same samples given as a one-channel file, bit for
bit -- the stored signal (decode + resampler arithmetic) and, because the network's passes are position- and batch-invariant, every
logit, average and region.  All comparisons below are device against device and exact; nothing here has a tolerance."""
import os

import numpy as np
import pytest

from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

RATES = (8000, 16000, 22050, 44100, 48000, 96000)        # plain decode (22 050), the fused resampler, the unfused pair (44 100, 96 000)
CHANNELS = (1, 2, 3, 6)                                   # 3 and 6: more than one pass over the PCM in the fused form
FRAMES = 20011                                            # odd; a few items of the fused form, one per block, a ragged last one


def _formats(native):
    return (native.PCM_U8, native.PCM_S16, native.PCM_S24, native.PCM_S32, native.PCM_F32, native.PCM_F64, native.PCM_S16BE)


def _pcm(native, rng, fmt, frames, ch):
    """Random interleaved PCM of one encoding as bytes [frames, ch, bytes per sample] (full range, so every bit of a sample matters)."""
    n = frames * ch
    if fmt == native.PCM_U8:
        a = rng.integers(0, 256, n, dtype=np.uint8)
    elif fmt in (native.PCM_S16, native.PCM_S16BE):
        a = rng.integers(-32768, 32768, n).astype("<i2" if fmt == native.PCM_S16 else ">i2")
    elif fmt == native.PCM_S24:
        a = rng.integers(0, 256, n * 3, dtype=np.uint8)
    elif fmt == native.PCM_S32:
        a = rng.integers(-2 ** 31, 2 ** 31, n).astype("<i4")
    elif fmt == native.PCM_F32:
        a = rng.uniform(-1, 1, n).astype("<f4")
    else:
        a = rng.uniform(-1, 1, n).astype("<f8")
    return np.ascontiguousarray(a).view(np.uint8).reshape(frames, ch, native._BPS[fmt])


def _channel(raw, c):
    return np.ascontiguousarray(raw[:, c, :]).reshape(-1)


@pytest.fixture(scope="session")
def native(build_all):
    from softspoken_amd import native
    return native


@pytest.fixture(scope="session")
def contexts(native, blob):
    """One context per precision for the whole session."""
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = native.Context(blob, 0, precision=precision)
        return made[precision]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="session", params=["fp32", "f16x2"])
def ctx(request, contexts):
    return contexts(request.param)


def _ingest_equal(native, ctx, raw, fmt, sr, frames, ch, tag):
    ctx.reset()
    first = ctx.add_pcm_channels(raw.reshape(-1), fmt, sr, ch, frames)
    got = [ctx.read_signal(first + c, padded=True) for c in range(ch)]
    durs = [ctx.signal_length(first + c) for c in range(ch)]
    for c in range(ch):
        ctx.reset()
        fid = ctx.add_pcm(_channel(raw, c), fmt, sr, 1, frames)
        want = ctx.read_signal(fid, padded=True)
        assert ctx.signal_length(fid) == durs[c], tag
        assert got[c].shape == want.shape and np.array_equal(got[c].view(np.uint32), want.view(np.uint32)), (tag, c)
        assert frames < 100 or np.any(want != 0), tag


def test_ingest_is_bit_identical_to_the_channel_alone(native, ctx):
    """Every rate x format x channel count: read_signal (padding included) of channel c after add_pcm_channels == after add_pcm of
    channel c's samples as mono PCM, compared as bit patterns."""
    rng = np.random.default_rng(7)
    for sr in RATES:
        for fmt in _formats(native):
            for ch in CHANNELS:
                _ingest_equal(native, ctx, _pcm(native, rng, fmt, FRAMES, ch), fmt, sr, FRAMES, ch, (sr, fmt, ch))


def test_ingest_short_odd_and_empty_files(native, ctx):
    rng = np.random.default_rng(8)
    for sr in RATES:
        for frames in (0, 1, 7, 333, 7681):               # 7681 frames at 48 kHz: one item of the fused form and one sample
            for fmt, ch in ((native.PCM_S16, 2), (native.PCM_S24, 3), (native.PCM_F32, 2), (native.PCM_S16, 6)):
                _ingest_equal(native, ctx, _pcm(native, rng, fmt, frames, ch), fmt, sr, frames, ch, (sr, fmt, ch, frames))


def test_ingest_batch_of_recordings(native, ctx):
    """add_pcm_channels_batch_device: recordings of different lengths back to back in one device buffer; recording r, channel c is file
    first + r * channels + c."""
    rng = np.random.default_rng(9)
    frames = [20011, 0, 4099, 12345]
    for sr, fmt, ch in ((48000, native.PCM_S16, 2), (44100, native.PCM_S24, 3), (22050, native.PCM_F32, 2), (16000, native.PCM_S16, 6),
                        (48000, native.PCM_F64, 3)):
        raws = [_pcm(native, rng, fmt, n, ch) for n in frames]
        blob_ = np.concatenate([r.reshape(-1) for r in raws])
        ctx.reset()
        dev = ctx.device_alloc(blob_.nbytes + 64)
        try:
            ctx.device_upload(dev, blob_)
            ctx.add_f32_22k(np.ones(10, np.float32))      # the batch does not start at file 0
            first = ctx.add_pcm_channels_batch_device(dev, fmt, sr, ch, frames, host_copy=blob_)
            assert first == 1
            got = [[ctx.read_signal(first + r * ch + c, padded=True) for c in range(ch)] for r in range(len(frames))]
            one = ctx.add_pcm_channels_device(dev, fmt, sr, ch, frames[0])           # the single-recording form, from device memory
            for c in range(ch):
                assert np.array_equal(ctx.read_signal(one + c, padded=True).view(np.uint32), got[0][c].view(np.uint32))
        finally:
            ctx.device_free(dev)
        for r, raw in enumerate(raws):
            for c in range(ch):
                ctx.reset()
                want = ctx.read_signal(ctx.add_pcm(_channel(raw, c), fmt, sr, 1, frames[r]), padded=True)
                assert np.array_equal(got[r][c].view(np.uint32), want.view(np.uint32)), (sr, fmt, ch, r, c)


# The fused form is persistent: one block per CU (256) walks items of 4 groups x L outputs -- 7680 input frames at 48 kHz, 2560 at
# 16 kHz -- and only from its SECOND item on does a block run the part that is new against the mixdown kernel: the next item's request
# issued behind the last channel's staging while the current item's descriptors are still in use, the hand-over between items, further
# passes over several items.  The recordings above give every block one item; these give each block 2 to 4, an uneven number of them.
LONG = (  # rate, format, channels, frames (odd: a ragged last item)
    (48000, "PCM_S16", 2, 6240007),      # FAST: 813 items
    (48000, "PCM_F32", 2, 4800011),      # the decoding template: 626 items
    (48000, "PCM_S24", 3, 4320005),      # two passes (2 + 1 channels) over 563 items
    (16000, "PCM_S16", 6, 1920003),      # three passes over 751 items, interpolating pair (phases in lane order)
)


@pytest.mark.parametrize("sr,fmt,ch,frames", LONG)
def test_ingest_of_long_recordings_walks_several_items_per_block(native, ctx, sr, fmt, ch, frames):
    fmt = getattr(native, fmt)
    items = -(-int(native.lib().ss_resampled_length(frames, sr)) // 3528)
    assert items > 2 * 256 and items % 256 != 0
    _ingest_equal(native, ctx, _pcm(native, np.random.default_rng(frames), fmt, frames, ch), fmt, sr, frames, ch, (sr, fmt, ch, frames))


@pytest.mark.parametrize("sr,fmt,ch,frames", [(48000, "PCM_S16", 2, [3000001, 100003, 1500007, 7, 0, 2999999]),
                                              (48000, "PCM_F32", 3, [2000003, 50001, 900001, 1]),
                                              (16000, "PCM_S24", 3, [700001, 5, 1000003, 30001])])
def test_ingest_of_a_long_batch_skips_items_past_short_files(native, ctx, sr, fmt, ch, frames):
    """A batch has (items of its longest file) x files items; those past a shorter file's end are skipped, so a block's walk meets
    invalid items between valid ones, also while it looks for the item to request next."""
    fmt = getattr(native, fmt)
    per_file = -(-int(native.lib().ss_resampled_length(max(frames), sr)) // 3528)
    assert per_file * len(frames) > 3 * 256 and per_file % 256 != 0
    rng = np.random.default_rng(sum(frames))
    raws = [_pcm(native, rng, fmt, n, ch) for n in frames]
    blob_ = np.concatenate([r.reshape(-1) for r in raws])
    ctx.reset()
    dev = ctx.device_alloc(blob_.nbytes + 64)
    try:
        ctx.device_upload(dev, blob_)
        first = ctx.add_pcm_channels_batch_device(dev, fmt, sr, ch, frames, host_copy=blob_)
        got = [[ctx.read_signal(first + r * ch + c, padded=True) for c in range(ch)] for r in range(len(frames))]
    finally:
        ctx.device_free(dev)
    for r, raw in enumerate(raws):
        for c in range(ch):
            ctx.reset()
            want = ctx.read_signal(ctx.add_pcm(_channel(raw, c), fmt, sr, 1, frames[r]), padded=True)
            assert np.array_equal(got[r][c].view(np.uint32), want.view(np.uint32)), (sr, fmt, ch, r, c)


def test_ingest_arguments_and_kernel_statistics(native):
    """Argument limits of add_pcm; channels == 1 is add_pcm; the launches appear under their own names with the algorithmic bytes."""
    c = native.Context(None, 0, profile=True)
    try:
        rng = np.random.default_rng(10)
        raw = _pcm(native, rng, native.PCM_S16, 9000, 2)
        for bad in (dict(ch=0), dict(ch=65), dict(sr=0), dict(fmt=99)):
            with pytest.raises((native.NativeError, ValueError)):
                c.add_pcm_channels(raw.reshape(-1), bad.get("fmt", native.PCM_S16), bad.get("sr", 48000), bad.get("ch", 2), 9000)
        with pytest.raises(ValueError):
            c.add_pcm_channels(raw.reshape(-1), native.PCM_S16, 48000, 2, 9001)      # the buffer is shorter than that
        n_out = int(native.lib().ss_resampled_length(9000, 48000))
        for sr, names in ((48000, {"resample_fused_channels": 9000 * 4 + 4 * 2 * n_out}),
                          (22050, {"decode_channels_batch": 9000 * 4 + 4 * 2 * 9000}),
                          (44100, {"decode_channels_batch": 9000 * 4 + 4 * 2 * 9000, "resample_batch": None})):
            c.reset()
            c.reset_stats()
            c.add_pcm_channels(raw.reshape(-1), native.PCM_S16, sr, 2, 9000)
            st = {s["name"]: s for s in c.kernel_stats()}
            assert set(st) == set(names), (sr, sorted(st))
            for k, nbytes in names.items():
                assert st[k]["launches"] == 1 and (nbytes is None or st[k]["bytes"] == nbytes), (sr, k, st[k])
        c.reset()
        c.reset_stats()
        mono = _channel(raw, 0)
        a = c.add_pcm_channels(mono, native.PCM_S16, 48000, 1, 9000)
        b = c.add_pcm(mono, native.PCM_S16, 48000, 1, 9000)
        assert (a, b) == (0, 1) and np.array_equal(c.read_signal(a), c.read_signal(b))
        assert {s["name"] for s in c.kernel_stats()} == {"resample_fused"}          # one channel: the existing path, twice
    finally:
        c.close()


# ---- runs --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def stereo():
    """40 s / 48 kHz 16-bit stereo, seed 3004: with the synthetic checkpoint the float64 oracle finds 5 regions on the mixdown, 4 on
    each channel and 2 on "any channel", with hundreds of bins above on one channel only."""
    from softspoken_amd import synth
    pcm = synth.to_pcm16(synth.synth_audio(3004, 40.0, 48000, 2))                  # [frames, 2] interleaved
    assert pcm.shape == (40 * 48000, 2)
    return np.ascontiguousarray(pcm)


def _results(ctx, fid):
    a, idx = ctx.avg(fid)
    return ctx.window_logits(fid), a, idx, ctx.regions(fid)


def _host_table(native, avgs, idx, threshold=0.1, break_s=0.5):
    """Merged regions and their first / last bin numbers, restated on the host: runs of the fmax series, gaps merged on the "%.4f"
    bin times (NNDetector.py:103-143), -3 s."""
    m = np.fmax.reduce(np.asarray(avgs), axis=0)
    runs, first, last = [], None, None
    for v, i in zip(m.tolist(), idx.tolist()):
        if v > threshold:
            first = i if first is None else first
            last = i
        elif first is not None:
            runs.append([first, last])
            first = None
    if first is not None:
        runs.append([first, last])
    merged = []
    for r in runs:
        if merged and float(O.time_str(r[0])) - float(O.time_str(merged[-1][1])) <= break_s:
            merged[-1][1] = r[1]
        else:
            merged.append(list(r))
    return [(float(O.time_str(a)) - 3, float(O.time_str(b)) - 3) for a, b in merged], merged


def test_channels_run_alone_equal_the_one_channel_files_and_merge(native, ctx, stereo):
    frames = len(stereo)
    ctx.reset()
    first = ctx.add_pcm_channels(stereo.reshape(-1), native.PCM_S16, 48000, 2, frames)
    assert ctx.run()
    each = [_results(ctx, first + c) for c in range(2)]
    merged = ctx.regions_union(first, 2)
    peaks = ctx.region_peaks(first, 2)
    assert ctx.num_windows(first) == ctx.num_windows(first + 1) > 60
    # (a) every channel of the job == that channel alone as a mono file, on the same context
    for c in range(2):
        ctx.reset()
        fid = ctx.add_pcm(np.ascontiguousarray(stereo[:, c]), native.PCM_S16, 48000, 1, frames)
        assert ctx.run()
        lg, a, idx, reg = _results(ctx, fid)
        assert np.array_equal(lg.view(np.uint32), each[c][0].view(np.uint32)), c
        assert np.array_equal(a.view(np.uint64), each[c][1].view(np.uint64)) and np.array_equal(idx, each[c][2]), c
        assert reg == each[c][3] and len(reg) > 0, c
        assert ctx.regions_union(fid, 1) == reg                                    # one channel: the file's own table
    # (b) the merged table == find_regions on the NaN-ignoring maximum of the channels' averages; the peaks == host maxima (doubles)
    idx = each[0][2]
    assert np.array_equal(idx, each[1][2])
    avgs = [each[0][1], each[1][1]]
    assert merged == native.find_regions(np.fmax(avgs[0], avgs[1]), idx) == native.find_regions_union(np.stack(avgs), idx)
    table, bins = _host_table(native, avgs, idx)
    assert merged == table and len(merged) >= 1
    want = np.array([[np.fmax.reduce(a[(idx >= lo) & (idx <= hi)], initial=-np.inf) for a in avgs] for lo, hi in bins])
    assert peaks.shape == want.shape and np.array_equal(peaks, want)
    assert np.all(peaks.max(axis=1) > 0.1)                                         # at least one channel heard every region
    # (c) and it is not any table that could be had before: each channel's, or the mixdown's
    ctx.reset()
    mix = ctx.add_pcm(stereo.reshape(-1), native.PCM_S16, 48000, 2, frames)
    assert ctx.run()
    mixed = ctx.regions(mix)
    assert merged != each[0][3] and merged != each[1][3] and merged != mixed
    only0 = int(np.sum((avgs[0] > 0.1) & ~(avgs[1] > 0.1))); only1 = int(np.sum((avgs[1] > 0.1) & ~(avgs[0] > 0.1)))
    assert only0 > 100 and only1 > 100, (only0, only1)
    print(f"regions: mixdown {len(mixed)}, channel 0 {len(each[0][3])}, channel 1 {len(each[1][3])}, merged {len(merged)}; "
          f"bins above on channel 0 only {only0}, on channel 1 only {only1}")


def test_union_getters_refuse_what_is_not_there(native, ctx, stereo):
    n = 48000 * 8
    ctx.reset()
    first = ctx.add_pcm_channels(stereo[:n].reshape(-1), native.PCM_S16, 48000, 2, n)
    short = ctx.add_pcm(np.ascontiguousarray(stereo[:n // 2, 0]), native.PCM_S16, 48000, 1, n // 2)
    assert ctx.run()
    ctx.regions_union(first, 2)
    for a, k in ((first, 4), (-1, 2), (first + 3, 1), (first, 0)):
        with pytest.raises(native.NativeError) as e:
            ctx.regions_union(a, k)
        assert e.value.code == native.SS_ERR_ARG
    with pytest.raises(native.NativeError) as e:              # files of different bin counts are not the channels of one recording
        ctx.regions_union(first + 1, 2)
    assert e.value.code == native.SS_ERR_ARG and short == first + 2
    with pytest.raises(native.NativeError) as e:
        ctx.region_peaks(first + 1, 2)
    assert e.value.code == native.SS_ERR_ARG
    # the regions stay readable while the next job is added; the peaks read device buffers, as ss_get_avg does
    table = ctx.regions_union(first, 2)
    ctx.reset()
    ctx.add_pcm(np.ascontiguousarray(stereo[:n, 0]), native.PCM_S16, 48000, 1, n)
    assert ctx.regions_union(first, 2) == table
    with pytest.raises(native.NativeError) as e:
        ctx.region_peaks(first, 2)
    assert e.value.code == native.SS_ERR_STATE


# ---- drop-in -----------------------------------------------------------------------------------------------------------------------
class _PM:
    def __init__(self, files, detections_file):
        self.files = files
        self.current_project = {'detections_file': detections_file}

    def get_unprocessed_list(self):
        return list(self.files)


@pytest.fixture(scope="module")
def project(tmp_path_factory, build_all):
    from softspoken_amd import synth
    d = tmp_path_factory.mktemp("chan") / "site b"
    d.mkdir()
    files = {}
    for name, seed, secs, sr, ch in (("mono.wav", 1001, 20.0, 16000, 1), ("st_a.wav", 3004, 40.0, 48000, 2), ("st_b.wav", 3002, 40.0, 48000, 2)):
        x = synth.synth_audio(seed, secs, sr, ch)
        pcm = synth.to_pcm16(x if ch > 1 else x[0])
        (d / name).write_bytes(synth.wav_bytes(pcm, sr))
        files[name] = str(d / name)
    ck = d / "model_checkpoint.pth"
    synth.save_checkpoint(str(ck), 0, epoch=0)
    return dict(dir=str(d), files=files, ck=str(ck))


def _run_worker(files, csv, ck, precision=None):
    from root.code.frontend.NNDetector import NNDetector
    from root.code.backend.worker import ProcessWorker
    from softspoken_amd.detections import DetectionProject
    side = os.path.splitext(csv)[0] + "_channels.csv"
    for p in (csv, side):
        if os.path.exists(p):
            os.remove(p)
    pm = _PM(files, csv)
    det = NNDetector(pm, checkpoint_path=ck)
    if precision:
        det.model.precision = precision
    w = ProcessWorker(det, DetectionProject(pm), det.plan_detection_job())
    msgs = []
    w.signals.message.connect(msgs.append)
    w.run()
    assert not msgs, msgs
    return open(csv).read(), (open(side).read() if os.path.exists(side) else None), det


def test_worker_in_each_mode_files_the_merged_tables_and_the_side_file(native, contexts, project, tmp_path, monkeypatch):
    from root.code.backend import settings
    from root.code.backend.voice_activity import add_file_to_context
    from softspoken_amd.detections import CSV_HEADER
    names = ["mono.wav", "st_a.wav", "st_b.wav"]
    files = [project["files"][n] for n in names]
    monkeypatch.setattr(settings, "hip_channel_mode", "each")
    got, side, det = _run_worker(files, str(tmp_path / "each.csv"), project["ck"])
    assert det.model.effective_precision() == "f16x2"
    # what the library gives for the same files on a context of that precision
    ctx = contexts("f16x2")
    want, want_side, next_id = CSV_HEADER + "\n", "ID,file_name,n_channels,heard,peaks\n", 1
    tables = {}
    for f, name in zip(files, names):
        ctx.reset()
        fid, info = add_file_to_context(ctx, f)
        assert ctx.run()
        reg = ctx.regions_union(fid, info.channels)
        pk = ctx.region_peaks(fid, info.channels)
        tables[name] = reg
        assert len(reg) > 0 and det.channel_detail[f] == (info.channels, pk.tolist())
        want += native.format_csv_rows(project["dir"], name, reg, next_id)
        for k, row in enumerate(pk.tolist()):
            heard = ";".join(str(c) for c, v in enumerate(row) if v > settings.threshold)
            want_side += f"{next_id + k},{name},{info.channels},{heard},{';'.join('%.6f' % v for v in row)}\n"
        next_id += len(reg)
    assert got == want and side == want_side
    assert det.detect_files(files) == {f: [(float(s), float(e)) for s, e in tables[n]] for f, n in zip(files, names)}
    # 'mix': byte-identical to a run with the setting absent, no side file; a mono file's rows are the same in both modes
    monkeypatch.setattr(settings, "hip_channel_mode", "mix")
    mix, mix_side, det_mix = _run_worker(files, str(tmp_path / "mix.csv"), project["ck"])
    monkeypatch.delattr(settings, "hip_channel_mode")
    absent, absent_side, _ = _run_worker(files, str(tmp_path / "mix.csv"), project["ck"])
    assert mix == absent and mix_side is None and absent_side is None and det_mix.channel_detail == {}
    assert mix != got
    rows = lambda text: [ln.split(",", 1)[1] for ln in text.splitlines() if ",mono.wav," in ln]
    assert rows(mix) == rows(got) and len(rows(got)) > 0


def test_each_mode_carries_through_the_f16x2_range_fallback(native, project, tmp_path, monkeypatch, caplog):
    """A float32 stereo WAV with one NaN sample on channel 0: the f16x2 mode refuses it (SS_ERR_RANGE), the file is run again on the
    fp32 side context -- in the same channel mode -- and the job equals the one of a detector that ran in fp32 from the start."""
    import logging
    from root.code.backend import settings
    from softspoken_amd import synth
    x = np.ascontiguousarray(synth.synth_audio(3004, 40.0, 48000, 2).T.astype(np.float32))
    x[48000 * 20, 0] = np.float32("nan")
    nanwav = tmp_path / "st_nan.wav"
    nanwav.write_bytes(synth.wav_bytes(x, 48000, "f32"))
    files = [str(nanwav), project["files"]["mono.wav"]]
    monkeypatch.setattr(settings, "hip_channel_mode", "each")
    with caplog.at_level(logging.WARNING):
        got, side, det = _run_worker(files, str(tmp_path / "a.csv"), project["ck"])
    assert det.model.effective_precision() == "f16x2" and det.model._fp32_tmp is not None
    assert sum("cannot represent an input" in r.getMessage() for r in caplog.records) == 1
    want, want_side, det32 = _run_worker(files, str(tmp_path / "a.csv"), project["ck"], precision="fp32")
    # the refused file's rows are the fp32 job's in both files; the mono file stayed in f16x2 (same regions, peaks of that precision)
    of = lambda text, name: [ln for ln in text.splitlines() if "," + name + "," in ln]
    assert got == want and side is not None and of(side, "st_nan.wav") == of(want_side, "st_nan.wav") and len(of(side, "st_nan.wav")) >= 1
    assert [ln.split(",")[:4] for ln in side.splitlines()] == [ln.split(",")[:4] for ln in want_side.splitlines()]
    assert got.count("st_nan.wav") >= 1 and det.channel_detail[str(nanwav)][0] == 2
    assert det.channel_detail[str(nanwav)] == det32.channel_detail[str(nanwav)]
    assert det.detect_files(files) == det32.detect_files(files)                     # with_range_fallback: the job path, same mode
