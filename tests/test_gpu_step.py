"""settings.step_size on a real MI355X (ss_set_window_step): whole-file runs, streams, window-range sharding and the drop-in at window
steps other than 0.6 s, held to the reference restated in tests/step_ref.py -- plans equal, per-window logits equal to ss_infer_windows
at the reference's starts bit for bit, averages equal to the reference's float64 averaging of those logits as int64 views, regions equal
to the reference's -- and, at the default step, to a context whose step was never set.

Small on purpose: passes of 16 windows (ss_set_chunk_windows(16)) so that every run crosses pass and file boundaries, one 12 s stereo
recording (at most 150 windows, at 0.1 s), a 0.05 s and a 0-frame recording, and a 44.1 kHz file with an odd frame count (the resampled
length is ceil(frames / 2), the plan's comes from round(): the plan and the signal disagree by a sample)."""
import math
import os

import numpy as np
import pytest

import step_ref as R
from oracle import oracle_np as O
from softspoken_amd import synth

pytestmark = pytest.mark.gpu
STEPS = (0.1, 99 / 512, 0.3, 1.5, 3.0)
BREAK = 0.5
CHUNK = 16


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native as N
    return N


@pytest.fixture(scope="module")
def recs(native):
    """(pcm, format, rate, channels, frames) of the recordings every whole-file case runs as one job; [0] is the 12 s one."""
    main = synth.to_pcm16(synth.synth_audio(1201, 12.0, 16000, 2, bursts=4))                  # (frames, 2) interleaved
    short = synth.to_pcm16(synth.synth_audio(1202, 0.05, 16000, 1, with_silence=False))
    odd = synth.to_pcm16(synth.synth_audio(1203, 132301 / 44100, 44100, 1, with_silence=False))
    assert main.shape == (192000, 2) and len(short) == 800 and len(odd) == 132301
    return [(main, native.PCM_S16, 16000, 2, 192000), (short, native.PCM_S16, 16000, 1, 800),
            (np.zeros(0, np.int16), native.PCM_S16, 16000, 1, 0), (odd, native.PCM_S16, 44100, 1, 132301)]


@pytest.fixture(scope="module")
def ctxs(native, blob):
    made = {}

    def get(prec, key=0):
        if (prec, key) not in made:
            made[(prec, key)] = native.Context(blob, 0, precision=prec, chunk=CHUNK)
        return made[(prec, key)]
    yield get
    for c in made.values():
        c.close()


def _job(ctx, recs, thr, brk=BREAK):
    """One job over `recs` with the context's step -> per file dict(fid, W, n_padded, logits, avg, idx, regions)."""
    ctx.reset()
    fids = [ctx.add_pcm(p, f, sr, ch, n) for p, f, sr, ch, n in recs]
    assert ctx.run(thr, brk)
    out = []
    for fid in fids:
        avg, idx = ctx.avg(fid)
        out.append(dict(fid=fid, W=ctx.num_windows(fid), n_padded=ctx.signal_length(fid, padded=True), logits=ctx.window_logits(fid),
                        avg=avg, idx=idx, regions=ctx.regions(fid)))
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["W"] == y["W"] and x["regions"] == y["regions"] and np.array_equal(x["idx"], y["idx"])
        assert np.array_equal(_bits(x["logits"]), _bits(y["logits"])) and np.array_equal(_bits(x["avg"]), _bits(y["avg"]))


@pytest.fixture(scope="module")
def base(native, ctxs, recs):
    """The job at the default step on a context whose step was never set, and the threshold of every case: the median of the 12 s
    recording's averages there, so that bins fall on both sides of it."""
    c = ctxs("f16x2", "never set")
    assert c.window_step == 0.6
    res = _job(c, recs, 0.1)
    thr = float(np.median(res[0]["avg"]))
    return dict(thr=thr, res=_job(c, recs, thr))


def _check_against_reference(native, ctx, recs, step, thr):
    ctx.set_window_step(step)
    assert ctx.window_step == step
    res = _job(ctx, recs, thr)
    for (pcm, fmt, sr, ch, frames), r in zip(recs, res):
        starts = R.clamp_plan(R.plan(frames / sr, step), r["n_padded"])
        assert r["W"] == len(starts) and r["logits"].shape == (len(starts), 1, 256)
        want_avg, want_idx = R.average(r["logits"], r["n_padded"], step)
        assert np.array_equal(r["idx"], want_idx)
        assert np.array_equal(_bits(r["avg"]), _bits(want_avg))
        want_regions = R.find_regions(want_avg, want_idx, thr, BREAK)
        assert r["regions"] == native.find_regions(r["avg"], r["idx"], thr, BREAK) == want_regions
        r["starts"] = starts
    assert len(R.find_regions(*R.average(res[0]["logits"], res[0]["n_padded"], step), thr, BREAK)) >= 2, "the input gives the reference < 2 regions"
    # the run's per-window logits are ss_infer_windows' at the reference's starts (read after the getters: it reuses their buffer)
    for r in res:
        if len(r["starts"]):
            assert np.array_equal(_bits(ctx.infer_windows(r["fid"], r["starts"])[1]), _bits(r["logits"]))
    return res


@pytest.mark.parametrize("step", STEPS)
def test_whole_file_run_equals_the_reference(native, ctxs, recs, base, step):
    res = _check_against_reference(native, ctxs("f16x2"), recs, step, base["thr"])
    assert res[0]["W"] == len(R.plan(12.0, step)) > CHUNK or step >= 1.5                      # (several passes wherever the plan allows)


def test_whole_file_run_equals_the_reference_fp32(native, ctxs, recs, base):
    _check_against_reference(native, ctxs("fp32"), recs, 99 / 512, base["thr"])


def test_default_step_set_equals_never_set(native, ctxs, recs, base):
    c = ctxs("f16x2")
    c.set_window_step(1.5)
    _job(c, recs[:1], base["thr"])
    c.set_window_step(0.6)
    _same_results(_job(c, recs, base["thr"]), base["res"])
    assert len(base["res"][0]["regions"]) >= 2
    for (pcm, fmt, sr, ch, frames), r in zip(recs, base["res"]):                              # ... and both are the reference at 0.6
        assert r["W"] == len(R.clamp_plan(R.plan(frames / sr, 0.6), r["n_padded"]))
        want_avg, want_idx = R.average(r["logits"], r["n_padded"], 0.6)
        assert np.array_equal(r["idx"], want_idx) and np.array_equal(_bits(r["avg"]), _bits(want_avg))
        assert r["regions"] == R.find_regions(want_avg, want_idx, base["thr"], BREAK)


def test_run_from_logits_follows_the_step(native, ctxs, recs, base):
    c = ctxs("f16x2")
    c.set_window_step(1.5)
    want = _job(c, recs, base["thr"])
    logits = np.concatenate([r["logits"].reshape(-1, 256) for r in want])
    for ctx2 in (c, native.Context(None, 0)):
        ctx2.set_window_step(1.5)
        ctx2.reset()
        fids = [ctx2.add_pcm(p, f, sr, ch, n) for p, f, sr, ch, n in recs]
        ctx2.run_from_logits(logits, base["thr"], BREAK)
        for fid, r in zip(fids, want):
            a, i = ctx2.avg(fid)
            assert ctx2.num_windows(fid) == r["W"] and np.array_equal(i, r["idx"]) and np.array_equal(_bits(a), _bits(r["avg"]))
            assert ctx2.regions(fid) == r["regions"]
        ctx2.set_window_step(0.6)                                                              # another step: another plan
        with pytest.raises(native.NativeError) as e:
            ctx2.run_from_logits(logits, base["thr"], BREAK)
        assert e.value.code == native.SS_ERR_ARG
        if ctx2 is not c:
            ctx2.close()


def test_channels_run_alone_follow_the_step(native, ctxs, recs, base):
    c = ctxs("f16x2")
    c.set_window_step(1.5)
    pcm, fmt, sr, ch, frames = recs[0]
    c.reset()
    fid = c.add_pcm_channels(pcm, fmt, sr, ch, frames)
    assert c.run(base["thr"], BREAK)
    avgs, idxs = zip(*(c.avg(fid + k) for k in range(ch)))
    assert np.array_equal(idxs[0], idxs[1]) and c.num_windows(fid) == c.num_windows(fid + 1) == len(R.plan(12.0, 1.5))
    for k in range(ch):                                                                        # each channel alone: the mono job at 1.5
        want_avg, want_idx = R.average(c.window_logits(fid + k), c.signal_length(fid + k, padded=True), 1.5)
        assert np.array_equal(idxs[k], want_idx) and np.array_equal(_bits(avgs[k]), _bits(want_avg))
    merged = c.regions_union(fid, ch)
    assert merged == native.find_regions_union(np.stack(avgs), idxs[0], base["thr"], BREAK)
    assert merged == R.find_regions(np.fmax(avgs[0], avgs[1]), idxs[0], base["thr"], BREAK) and len(merged) >= 1


def test_set_window_step_in_flight_and_refusals(native, ctxs, recs, base):
    c = ctxs("f16x2")
    c.set_window_step(0.3)
    c.reset()
    fid = c.add_pcm(*recs[0])
    c.run_begin(base["thr"], BREAK)
    with pytest.raises(native.NativeError) as e:
        c.set_window_step(1.5)
    assert e.value.code == native.SS_ERR_STATE and c.window_step == 0.3
    c.run_end()
    before = (c.num_windows(fid), c.regions(fid), c.avg(fid), c.window_logits(fid))
    c.set_window_step(1.5)                                                                     # the ended run's getters stay valid
    after = (c.num_windows(fid), c.regions(fid), c.avg(fid), c.window_logits(fid))
    assert before[:2] == after[:2] and before[0] == len(R.plan(12.0, 0.3))
    assert np.array_equal(_bits(before[2][0]), _bits(after[2][0])) and np.array_equal(before[2][1], after[2][1])
    assert np.array_equal(_bits(before[3]), _bits(after[3]))
    for bad in (0, -1, 0.0999, 3.0001, float("nan"), float("inf")):
        assert native.lib().ss_set_window_step(c._h, float(bad)) == native.SS_ERR_ARG and c.window_step == 1.5
        with pytest.raises(ValueError):
            c.set_window_step(bad)
    for ok in (0.1, 3.0):
        c.set_window_step(ok)
        assert c.window_step == ok


def test_separation_silencer_stays_on_the_default_step(native, ctxs, recs):
    pcm, fmt, sr, ch, frames = recs[0]
    never, c = ctxs("f16x2", "never set"), ctxs("f16x2")
    regions = [(2.0, 4.5), (9.0, 9.4)]
    want = never.separate_pcm(pcm, fmt, sr, ch, frames, regions)
    want_maps = never.separation_maps(0, 300, 200)
    for step in (1.5, 0.1):
        c.set_window_step(step)
        assert np.array_equal(c.separate_pcm(pcm, fmt, sr, ch, frames, regions), want)
        assert np.array_equal(c.separation_maps(0, 300, 200).view(np.int32), want_maps.view(np.int32))
        assert c.window_step == step


# ---- streams ------------------------------------------------------------------------------------------------------------------
def _bound_B(sr):
    """B of include/softspoken.h."""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "softspoken.h")).read()
    assert "B = 3 s + 2 x (3 / 256) s + half / sample_rate" in hdr
    half = 0 if sr == 22050 else math.ceil(32.0 / min(1.0, 22050.0 / sr))
    return 3.0 + 2 * 3.0 / 256 + half / sr, half


def _state_bound(step, half):
    """include/softspoken.h "State": samples below 3 s + step, the resampler's history below 2 half + 1 frames, the logits of at most
    ceil(256 / s_b) + 1 windows, and the host record (its size is not part of the interface: 4 KiB allowed for it)."""
    s_b = step * 256 / 3
    return 4 * (math.ceil((3.0 + step) * 22050) + 2 * half + 1 + (math.ceil(256 / s_b) + 1) * 256) + 4096


def _stream_steps(ctx, steps, rec, pieces, thr):
    """Streams of the given window steps on one context, fed the same pieces and stepped together -> per stream
    (regions, avg, idx) concatenated; after every step: the latency bound and the state bound of each stream."""
    pcm, fmt, sr, ch, frames = rec
    B, half = _bound_B(sr)
    sids = []
    for step in steps:
        ctx.set_window_step(step)
        sids.append(ctx.stream_open(fmt, sr, ch, thr, BREAK))
    ctx.set_window_step(0.45)                                       # the streams keep the step they were opened with
    got = [([], [], []) for _ in sids]

    def step_all(held_s, closing=False):
        ctx.stream_step()
        for k, sid in enumerate(sids):
            a, i = ctx.stream_avg(sid)
            got[k][0].extend(ctx.stream_regions(sid)); got[k][1].append(a); got[k][2].append(i)
            info = ctx.stream_info(sid)
            assert info["state_bytes"] <= _state_bound(steps[k], half), (steps[k], info)
            if not closing:
                # every bin at audio time t with t + B < the audio held is out: final_until_s covers it, and the bins returned so
                # far reach it (bins are returned in ascending order without gaps in the covered ones)
                assert info["final_until_s"] >= held_s - B - 1e-9, (steps[k], held_s, info)
                done = np.concatenate(got[k][2])
                j_need = math.ceil((held_s - B + 3.0) * 256 / 3) - 1                       # last bin with j 3 / 256 - 3 + B < held
                assert j_need < 0 or (len(done) and done[-1] >= j_need), (steps[k], held_s, j_need)
    at = 0
    for n in list(pieces) + [frames]:
        n = min(n, frames - at)
        if n <= 0:
            break
        for sid in sids:
            ctx.stream_push(sid, pcm[at:at + n], frames=n)
        at += n
        step_all(at / sr)
    for sid in sids:
        ctx.stream_close(sid)
    step_all(frames / sr, closing=True)
    for sid in sids:
        assert ctx.stream_info(sid)["finished"] == 1
        ctx.stream_free(sid)
    return [(r, np.concatenate(a), np.concatenate(i)) for r, a, i in got]


@pytest.mark.parametrize("pieces", [(1, 777, 20001), tuple([4800] * 39)], ids=["1-777-20001-rest", "0.3s-pieces"])
def test_streams_of_three_steps_share_passes_and_equal_the_whole_file_runs(native, ctxs, recs, base, pieces):
    steps = (99 / 512, 1.5, 3.0)
    c, ref = ctxs("f16x2"), ctxs("f16x2", "whole file")
    got = _stream_steps(c, steps, recs[0], pieces, base["thr"])
    for step, (regions, avg, idx) in zip(steps, got):
        ref.set_window_step(step)
        want = _job(ref, recs[:1], base["thr"])[0]
        assert regions == want["regions"] and np.array_equal(idx, want["idx"]) and np.array_equal(_bits(avg), _bits(want["avg"]))
        assert len(regions) >= 2


def test_stream_of_the_odd_44k_file_and_the_empty_one(native, ctxs, recs, base):
    c, ref = ctxs("f16x2"), ctxs("f16x2", "whole file")
    for rec in (recs[3], recs[2], recs[1]):
        got = _stream_steps(c, (99 / 512, 3.0), rec, (1, 777, 20001), base["thr"])
        for step, (regions, avg, idx) in zip((99 / 512, 3.0), got):
            ref.set_window_step(step)
            want = _job(ref, [rec], base["thr"])[0]
            assert regions == want["regions"] and np.array_equal(idx, want["idx"]) and np.array_equal(_bits(avg), _bits(want["avg"]))


def test_stream_image_carries_the_step_into_an_fp32_context(native, ctxs, recs, base):
    pcm, fmt, sr, ch, frames = recs[0]
    thr, step = base["thr"], 1.5
    src, dst = ctxs("f16x2"), ctxs("fp32")
    dst.set_window_step(1.5)
    want = _job(dst, recs[:1], thr)[0]                                                       # the fp32 whole-file run at 1.5
    dst.set_window_step(0.3)                                                                 # the image's step counts, not the context's
    src.set_window_step(step)
    sid = src.stream_open(fmt, sr, ch, thr, BREAK)
    avg, idx, regions = [], [], []

    def step_on(c, s):
        c.stream_step()
        a, i = c.stream_avg(s)
        avg.append(a); idx.append(i); regions.extend(c.stream_regions(s))
    cut = 16000 * 7
    src.stream_push(sid, pcm[:cut - 3000], frames=cut - 3000)
    step_on(src, sid)
    src.stream_push(sid, pcm[cut - 3000:cut], frames=3000)                                   # staged input travels in the image
    image = src.stream_export(sid)
    n_f16 = src.stream_info(sid)["windows_run"]
    src.stream_free(sid)
    assert image[:8] == b"SSSTRM02" and n_f16 >= 2
    sid = dst.stream_import(image)
    assert dst.stream_export(sid) == image                                                   # (round trip: the step is in it)
    dst.stream_push(sid, pcm[cut:], frames=frames - cut)
    step_on(dst, sid)
    dst.stream_close(sid)
    step_on(dst, sid)
    dst.stream_free(sid)
    avg, idx = np.concatenate(avg), np.concatenate(idx)
    assert np.array_equal(idx, want["idx"])
    # the windows run before the export are f16x2's (scores within 1e-4 of fp32: include/softspoken.h, SS_FLAG_F16X2); every bin
    # that only later windows cover is the fp32 run's bit for bit
    assert np.abs(avg - want["avg"]).max() < 1e-4
    pure = idx >= R.start_bin(n_f16 - 1, step) + 256
    assert pure.any() and np.array_equal(_bits(avg[pure]), _bits(want["avg"][pure]))
    if regions != want["regions"]:                                                           # only bins within 1e-4 of the threshold may decide differently
        assert np.all(np.abs(want["avg"][(avg > thr) != (want["avg"] > thr)] - thr) < 1e-4)
    with pytest.raises(native.NativeError) as e:                                             # a step outside the range in an image: refused
        at = image.index(np.float64(step).tobytes())                                         # (behind the header of a default-step image)
        dst.stream_import(image[:at] + np.float64(3.5).tobytes() + image[at + 8:])
    assert e.value.code == native.SS_ERR_FORMAT


def test_default_step_image_is_the_one_always_written(native, ctxs, recs):
    pcm, fmt, sr, ch, frames = recs[0]
    never, was_set = ctxs("f16x2", "never set"), ctxs("f16x2")
    was_set.set_window_step(3.0)
    was_set.set_window_step(0.6)
    images = []
    for c in (never, was_set):
        sid = c.stream_open(fmt, sr, ch, 0.1, BREAK)
        c.stream_push(sid, pcm[:100000], frames=100000)
        c.stream_step()
        c.stream_push(sid, pcm[100000:100777], frames=777)
        images.append(c.stream_export(sid))
        c.stream_free(sid)
    assert images[0][:8] == images[1][:8] == b"SSSTRM01" and len(images[0]) == len(images[1])
    assert images[0] == images[1]
    was_set.set_window_step(1.5)
    sid = was_set.stream_import(images[0])                                                   # an image without a step: the default one
    assert was_set.stream_export(sid) == images[0]
    was_set.stream_free(sid)


def test_stream_detector_takes_a_step(native, blob, ctxs, recs, base):
    from softspoken_amd.stream import StreamDetector
    pcm, fmt, sr, ch, frames = recs[0]
    ref = ctxs("f16x2", "whole file")
    ref.set_window_step(1.5)
    want = _job(ref, recs[:1], base["thr"])[0]
    det = StreamDetector(blob, precision="f16x2", chunk=CHUNK, step=1.5)
    s = det.open(fmt, sr, ch, base["thr"], BREAK)
    regions, avg, idx = [], [], []
    for k in range(0, frames, 48000):
        s.push(pcm[k:k + 48000])
        out = det.step()[s]
        regions += out[0]; avg.append(out[1]); idx.append(out[2])
    s.close()
    out = det.step()[s]
    regions += out[0]; avg.append(out[1]); idx.append(out[2])
    det.close()
    assert regions == want["regions"] and np.array_equal(np.concatenate(idx), want["idx"])
    assert np.array_equal(_bits(np.concatenate(avg)), _bits(want["avg"]))
    with pytest.raises(ValueError):
        StreamDetector(blob, step=3.5)


# ---- sharding and the drop-in --------------------------------------------------------------------------------------------------
def test_recording_sharded_by_window_ranges_follows_the_step(native, ctxs, recs, base, tmp_path):
    import torch.distributed as dist
    from softspoken_amd import parallel
    c = ctxs("f16x2")
    c.set_window_step(1.5)
    want = _job(c, recs[:1], base["thr"])[0]
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "rendezvous"), rank=0, world_size=1)
    try:
        got = parallel.detect_recording_sharded(c, *recs[0], threshold=base["thr"], break_s=BREAK)
    finally:
        if own:
            dist.destroy_process_group()
    assert got == want["regions"] and c.num_windows(0) == want["W"] == len(R.plan(12.0, 1.5))
    odd = _job(c, [recs[3]], base["thr"])[0]                                                  # the clamp, with the context's step
    assert odd["W"] == len(R.clamp_plan(R.plan(132301 / 44100, 1.5), odd["n_padded"]))


class _PM:
    def __init__(self, files, detections_file):
        self.files = files
        self.current_project = {'detections_file': detections_file}

    def get_unprocessed_list(self):
        return list(self.files)


def test_dropin_worker_follows_settings_step_size(native, recs, base, tmp_path, monkeypatch):
    from root.code.backend import settings
    from root.code.backend.worker import ProcessWorker
    from root.code.frontend.NNDetector import NNDetector
    from softspoken_amd.detections import DetectionProject
    monkeypatch.setattr(settings, "step_size", 1.5)
    monkeypatch.setattr(settings, "threshold", base["thr"])
    monkeypatch.setattr(settings, "hip_chunk_windows", CHUNK)
    d = tmp_path / "site b"
    d.mkdir()
    wav, ck, csv = str(d / "rec12.wav"), str(d / "model_checkpoint.pth"), str(d / "p_detections.csv")
    synth.write_wav(wav, recs[0][0], 16000)
    synth.save_checkpoint(ck, 0, epoch=0)
    pm = _PM([wav], csv)
    det = NNDetector(pm, checkpoint_path=ck)
    plan = det.plan_detection_job()
    assert np.array_equal(plan[wav], R.plan(12.0, 1.5))
    totals = []
    poll = det.file_poll
    monkeypatch.setattr(det, "file_poll", lambda token, progress=None, block=True:
                        poll(token, lambda done, total: (totals.append((done, total)), progress(done, total)), block))
    msgs = []
    w = ProcessWorker(det, DetectionProject(pm), plan)
    w.signals.message.connect(msgs.append)
    w.run()
    assert not msgs
    ctx = det.model.hip_context()
    assert ctx.window_step == 1.5 and ctx.num_windows(0) == len(plan[wav])
    assert totals and totals[-1] == (len(plan[wav]), len(plan[wav])) and all(t == len(plan[wav]) for _, t in totals)
    avg, idx = ctx.avg(0)                                                                     # the device's averages of that run
    want_avg, want_idx = R.average(ctx.window_logits(0), ctx.signal_length(0, padded=True), 1.5)
    assert np.array_equal(idx, want_idx) and np.array_equal(_bits(avg), _bits(want_avg))
    regions = R.find_regions(avg, idx, base["thr"], 0.5)
    assert len(regions) >= 2
    assert open(csv).read() == O.csv_text([(k + 1, str(d), "rec12.wav", s, e) for k, (s, e) in enumerate(regions)])
    # a value edited between two jobs reaches the reused context; one outside the range raises and names the limits
    monkeypatch.setattr(settings, "step_size", 0.3)
    assert det.model.hip_context().window_step == 0.3 and len(det.plan_detection_job()[wav]) == len(R.plan(12.0, 0.3))
    monkeypatch.setattr(settings, "step_size", 3.5)
    with pytest.raises(ValueError) as e:
        det.plan_detection_job()
    assert "0.1" in str(e.value) and "3.0" in str(e.value)
