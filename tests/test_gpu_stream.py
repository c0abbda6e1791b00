"""Streaming detection (ss_stream_*, softspoken_amd.stream) against the whole-file run on the same frames, which the C3 and parity
tests pin to the reference: regions equal as ss_region values, averages and bin numbers equal bit for bit, for any split of the input,
any cadence of steps and whatever shares the passes."""
import logging
import math
import os

import numpy as np
import pytest

from softspoken_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native as N
    return N


@pytest.fixture(scope="module")
def c1_pcm():
    return synth.to_pcm16(synth.synth_audio(1001, 60.0, 16000, 1))


@pytest.fixture(scope="module")
def c3_pcm():
    return synth.to_pcm16(synth.synth_audio(3000, 600.0, 16000, 1))


@pytest.fixture(scope="module")
def ctxs(native, blob):
    made = {}

    def get(prec, key=0):
        if (prec, key) not in made:
            made[(prec, key)] = native.Context(blob, 0, precision=prec)
        return made[(prec, key)]
    yield get
    for c in made.values():
        c.close()


def offline(ctx, pcm, fmt, sr, ch, thr=0.1, brk=0.5):
    return offline_frames(ctx, pcm, fmt, sr, ch, len(pcm), thr, brk)


def _bytes(pcm):
    return np.frombuffer(np.ascontiguousarray(pcm).tobytes(), dtype=np.uint8)


def streamed(ctx, pcm, fmt, sr, ch, pieces, step_every=1, thr=0.1, brk=0.5, on_step=None):
    """pieces: frame counts (the rest of the recording is pushed in one last piece)."""
    from softspoken_amd.native import _BPS
    b = _bytes(pcm)
    fb = ch * _BPS[fmt]
    total = b.size // fb
    sid = ctx.stream_open(fmt, sr, ch, thr, brk)
    regs, avg, idx = [], [], []

    def step():
        ctx.stream_step()
        r = ctx.stream_regions(sid)
        a, i = ctx.stream_avg(sid)
        regs.extend(r); avg.append(a); idx.append(i)
        if on_step:
            on_step(sid, r, a, i)
    at, k = 0, 0
    for n in list(pieces) + [total]:
        n = min(n, total - at)
        if n <= 0:
            break
        ctx.stream_push(sid, b[at * fb:(at + n) * fb], frames=n)
        at += n
        k += 1
        if k % step_every == 0:
            step()
    ctx.stream_close(sid)
    step()
    assert ctx.stream_info(sid)["finished"] == 1
    ctx.stream_free(sid)
    return regs, np.concatenate(avg), np.concatenate(idx)


def assert_same(got, want):
    assert got[0] == want[0]
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64))      # bit for bit (NaN included)


def _random_pieces(seed, total, lo=1, hi=40000):
    rng = np.random.default_rng(seed)
    out, s = [], 0
    while s < total:
        n = int(rng.integers(lo, hi))
        out.append(n)
        s += n
    return out


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_c1_streamed_equals_offline(native, ctxs, c1_pcm, precision):
    c = ctxs(precision)
    want = offline(c, c1_pcm, native.PCM_S16, 16000, 1)
    assert want[0], "C1 has regions"
    splits = [
        ([1] * 400 + [997] * 2000, 1),                    # one frame at a time first, then 997
        ([1] * 400 + [997] * 2000, 7),
        ([16000] * 100, 1),
        (_random_pieces(5, len(c1_pcm)), 1),
        (_random_pieces(6, len(c1_pcm)), 4),
        ([], 1),                                          # the whole file in one push
    ]
    for pieces, every in splits:
        assert_same(streamed(c, c1_pcm, native.PCM_S16, 16000, 1, pieces, every), want)


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_c3_streamed_equals_offline(native, ctxs, c3_pcm, precision):
    c = ctxs(precision)
    want = offline(c, c3_pcm, native.PCM_S16, 16000, 1)
    for pieces, every in (([16000] * 600, 1), (_random_pieces(7, len(c3_pcm), 1, 400000), 3), ([], 1)):
        assert_same(streamed(c, c3_pcm, native.PCM_S16, 16000, 1, pieces, every), want)


def _encode(x, fmt):
    """float mono/interleaved x in [-1, 1] -> samples of the encoding (uint8 bytes for 24-bit)."""
    if fmt == 1:
        return np.clip(np.round(x * 127 + 128), 0, 255).astype(np.uint8)
    if fmt == 2:
        return np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    if fmt == 5:
        return x.astype(np.float32)
    if fmt == 8:
        return np.clip(np.round(x * 32767), -32768, 32767).astype(">i2")
    if fmt == 3:
        v = np.clip(np.round(x * 8388607), -8388608, 8388607).astype(np.int32).reshape(-1)
        b = v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]
        return np.ascontiguousarray(b).reshape(-1)
    raise ValueError(fmt)


@pytest.mark.parametrize("fmt,sr,ch", [(2, 48000, 2), (5, 44100, 1), (1, 8000, 1), (3, 22050, 1), (8, 16000, 1)])
def test_rates_and_formats(native, ctxs, fmt, sr, ch):
    c = ctxs("f16x2")
    x = np.ascontiguousarray(synth.synth_audio(77 + sr + fmt, 20.0, sr, ch).T)     # (frames, channels), interleaved
    if ch == 1:
        x = x[:, 0]
    pcm = _encode(x, fmt)
    frames = len(x)
    want = offline_frames(c, pcm, fmt, sr, ch, frames)
    got = streamed(c, pcm, fmt, sr, ch, _random_pieces(sr + fmt, frames, 1, 9000), 2)
    assert_same(got, want)


def offline_frames(ctx, pcm, fmt, sr, ch, frames, thr=0.1, brk=0.5):
    ctx.reset()
    fid = ctx.add_pcm(np.ascontiguousarray(pcm), fmt, sr, ch, frames)
    ctx.run(thr, brk)
    avg, idx = ctx.avg(fid)
    return ctx.regions(fid), avg, idx


def test_64_staggered_streams_share_passes(native, blob):
    c = native.Context(blob, 0, precision="f16x2", chunk=16)
    ref = native.Context(blob, 0, precision="f16x2")
    rates = (8000, 16000, 22050, 44100, 48000)
    recs = []
    for k in range(64):
        sr = rates[k % len(rates)]
        pcm = synth.to_pcm16(synth.synth_audio(9000 + k, 4.0 + (k % 9), sr, 1))
        recs.append((sr, pcm, offline_frames(ref, pcm, native.PCM_S16, sr, 1, len(pcm))))
    state = {}
    rng = np.random.default_rng(3)
    for rnd in range(200):
        for k, (sr, pcm, _) in enumerate(recs):
            if k not in state and rnd >= k % 16:
                state[k] = dict(sid=c.stream_open(native.PCM_S16, sr, 1, 0.1, 0.5), at=0, r=[], a=[], i=[], done=False)
            st = state.get(k)
            if st is None or st["done"]:
                continue
            if st["at"] < len(pcm):
                n = int(rng.integers(sr // 10, sr))
                c.stream_push(st["sid"], pcm[st["at"]:st["at"] + n], frames=min(n, len(pcm) - st["at"]))
                st["at"] += n
            elif not c.stream_info(st["sid"])["closed"]:
                c.stream_close(st["sid"])
        c.stream_step()
        for k, st in state.items():
            if st["done"]:
                continue
            st["r"] += c.stream_regions(st["sid"])
            a, i = c.stream_avg(st["sid"])
            st["a"].append(a); st["i"].append(i)
            if c.stream_info(st["sid"])["finished"]:
                st["done"] = True
        if len(state) == 64 and all(st["done"] for st in state.values()):
            break
    for k, (sr, pcm, want) in enumerate(recs):
        st = state[k]
        assert st["done"]
        assert_same((st["r"], np.concatenate(st["a"]), np.concatenate(st["i"])), want)
    c.close(); ref.close()


def test_empty_and_short_streams(native, ctxs):
    c = ctxs("fp32")
    for pcm in (np.zeros(0, np.int16), synth.to_pcm16(synth.synth_audio(42, 2.0, 16000, 1, with_silence=False))):
        want = offline_frames(c, pcm, native.PCM_S16, 16000, 1, len(pcm))
        assert_same(streamed(c, pcm, native.PCM_S16, 16000, 1, [len(pcm) // 3 + 1] * 3 if len(pcm) else []), want)


def test_step_boundary_inside_a_merged_gap(native, ctxs, c1_pcm):
    """A threshold at which the offline run merges two above-threshold runs across a short gap; the stream is stepped with a
    boundary inside that gap."""
    c = ctxs("fp32")
    _, avg, idx = offline(c, c1_pcm, native.PCM_S16, 16000, 1)
    brk = 0.5
    found = None
    for thr in np.quantile(avg, [0.5, 0.6, 0.7, 0.8, 0.9]):
        above = avg > thr
        for k in range(1, len(avg) - 1):
            if above[k - 1] and not above[k]:
                e = k - 1
                j = k
                while j < len(avg) and not above[j]:
                    j += 1
                if j < len(avg) and (idx[j] - idx[e]) * 3 / 256 <= brk - 0.05 and j - e >= 3:
                    found = (float(thr), idx[e], idx[j])
                    break
        if found:
            break
    assert found, "no merged gap in C1's averages"
    thr, b_end, b_next = found
    want = offline(c, c1_pcm, native.PCM_S16, 16000, 1, thr, brk)
    # the bins of the gap become final when the audio reaches their time + 3 s: split the pushes there
    t_gap = ((b_end + b_next) / 2) * 3 / 256 - 3.0 + 3.0 + 0.02
    first = int(t_gap * 16000)
    got = streamed(c, c1_pcm, native.PCM_S16, 16000, 1, [first, 1600, 1600], 1, thr, brk)
    assert_same(got, want)


def _bound_B(sr):
    """B of include/softspoken.h."""
    hdr = open(os.path.join(ROOT, "include", "softspoken.h")).read()
    assert "B = 3 s + 2 x (3 / 256) s + half / sample_rate" in hdr
    half = 0 if sr == 22050 else math.ceil(32.0 / min(1.0, 22050.0 / sr))
    return 3.0 + 2 * 3.0 / 256 + half / sr


def test_latency_bound(native, ctxs, c1_pcm):
    c = ctxs("fp32")
    brk = 0.5
    want = offline(c, c1_pcm, native.PCM_S16, 16000, 1, 0.1, brk)
    B = _bound_B(16000)
    final_r = set(want[0])
    arrivals = []                                          # (region, audio held when it was returned)
    sid = c.stream_open(native.PCM_S16, 16000, 1, 0.1, brk)
    for k in range(0, len(c1_pcm), 1600):                 # 0.1 s pieces, a step after each
        c.stream_push(sid, c1_pcm[k:k + 1600])
        held = min(k + 1600, len(c1_pcm)) / 16000.0
        c.stream_step()
        for reg in c.stream_regions(sid):
            assert reg in final_r                          # never contradicted by the final table
            arrivals.append((reg, held))
        a, i = c.stream_avg(sid)
        assert c.stream_info(sid)["final_until_s"] >= held - B - 0.1 - 1e-9
    c.stream_close(sid)
    c.stream_step()
    tail = c.stream_regions(sid)
    assert [r for r, _ in arrivals] + tail == want[0]
    total = len(c1_pcm) / 16000.0
    for reg, t in arrivals:
        # returned by the first step after the audio held passes t_end + break + B (one 0.1 s piece of slack)
        assert t <= reg[1] + brk + B + 0.1 + 1e-9, (reg, t)
    for reg in tail:
        assert reg[1] + brk + B > total - 0.1             # only what the bound lets wait for the close
    c.stream_free(sid)


def test_state_does_not_grow(native, ctxs, c3_pcm):
    c = ctxs("f16x2")
    sid = c.stream_open(native.PCM_S16, 16000, 1, 0.1, 0.5)
    sizes = {}
    for k in range(600):
        c.stream_push(sid, c3_pcm[k * 16000:(k + 1) * 16000])
        c.stream_step()
        if k + 1 in (60, 600):
            sizes[k + 1] = c.stream_info(sid)["state_bytes"]
    assert abs(sizes[600] - sizes[60]) <= 4096, sizes
    assert sizes[600] < 400_000, sizes
    c.stream_free(sid)


@pytest.mark.parametrize("route", [("f16x2", "f16x2"), ("f16x2", "fp32", "f16x2")])
def test_export_import(native, ctxs, c1_pcm, route):
    ref = ctxs(route[0])
    want = streamed(ref, c1_pcm, native.PCM_S16, 16000, 1, [16000] * 60)
    ctxs_ = [ctxs(p, key=1 + k) for k, p in enumerate(route)]
    c = ctxs_[0]
    sid = c.stream_open(native.PCM_S16, 16000, 1, 0.1, 0.5)
    regs, avg, idx = [], [], []
    hop = [20, 40] if len(route) == 3 else [30]
    for k in range(60):
        if hop and k == hop[0]:
            hop.pop(0)
            nxt = ctxs_[ctxs_.index(c) + 1]
            image = c.stream_export(sid)
            c.stream_push(sid, c1_pcm[:5])                   # the source is left alone by the export
            c.stream_free(sid)
            sid, c = nxt.stream_import(image), nxt
        c.stream_push(sid, c1_pcm[k * 16000:(k + 1) * 16000])
        if k % 2:
            c.stream_step()
            regs += c.stream_regions(sid); a, i = c.stream_avg(sid); avg.append(a); idx.append(i)
    c.stream_close(sid)
    c.stream_step()
    regs += c.stream_regions(sid); a, i = c.stream_avg(sid); avg.append(a); idx.append(i)
    c.stream_free(sid)
    got = (regs, np.concatenate(avg), np.concatenate(idx))
    if len(route) == 2:
        assert_same(got, want)
    else:                                                  # the fp32 leg: the f16x2 contract of 1e-4
        assert np.array_equal(got[2], want[2])
        assert np.abs(got[1] - want[1]).max() < 1e-4


def test_range_fallback_of_the_stream_detector(native, blob, caplog):
    from softspoken_amd.stream import StreamDetector
    x = synth.synth_audio(4242, 20.0, 16000, 1)[0].astype(np.float32)
    x[16000 * 7 + 123] = np.nan
    fp = native.Context(blob, 0, precision="fp32")
    want = offline_frames(fp, x, native.PCM_F32, 16000, 1, len(x))
    fp.close()
    det = StreamDetector(blob, precision="f16x2")
    s = det.open(native.PCM_F32, 16000, 1, 0.1, 0.5)
    clean = det.open(native.PCM_S16, 16000, 1, 0.1, 0.5)
    cpcm = synth.to_pcm16(synth.synth_audio(4243, 20.0, 16000, 1))
    regs, avg, idx = [], [], []
    with caplog.at_level(logging.WARNING):
        for k in range(0, len(x), 8000):
            s.push(x[k:k + 8000]); clean.push(cpcm[k:k + 8000])
            out = det.step()
            regs += out[s][0]; avg.append(out[s][1]); idx.append(out[s][2])
        s.close(); clean.close()
        out = det.step()
        regs += out[s][0]; avg.append(out[s][1]); idx.append(out[s][2])
    assert s.precision == "fp32"
    avg, idx = np.concatenate(avg), np.concatenate(idx)
    assert np.array_equal(idx, want[2])
    nan = np.isnan(want[1])
    assert np.array_equal(np.isnan(avg), nan)
    assert np.abs(avg[~nan] - want[1][~nan]).max() < 1e-4
    if regs != want[0]:                                    # only bins within 1e-4 of the threshold may decide differently
        assert np.all(np.abs(want[1][~nan][(avg[~nan] > 0.1) != (want[1][~nan] > 0.1)] - 0.1) < 1e-4)
    det.close()


def test_streams_and_jobs_share_a_context(native, blob, c1_pcm):
    clip = synth.to_pcm16(synth.synth_audio(31, 25.0, 16000, 1))
    alone = native.Context(blob, 0, precision="f16x2")
    want_s = streamed(alone, c1_pcm, native.PCM_S16, 16000, 1, [8000] * 120)
    want_j = offline_frames(alone, clip, native.PCM_S16, 16000, 1, len(clip))
    c = native.Context(blob, 0, precision="f16x2")
    c.reset()
    fid = c.add_pcm(clip, native.PCM_S16, 16000, 1, len(clip))
    sid = c.stream_open(native.PCM_S16, 16000, 1, 0.1, 0.5)
    regs, avg, idx = [], [], []
    for k in range(120):
        c.stream_push(sid, c1_pcm[k * 8000:(k + 1) * 8000])
        if k == 50:
            c.run(0.1, 0.5)
        if k == 80:
            c.run_begin(0.1, 0.5)
            with pytest.raises(native.NativeError) as e:
                c.stream_step()
            assert e.value.code == 4
            c.run_end()
            c.reset()
            fid = c.add_pcm(clip, native.PCM_S16, 16000, 1, len(clip))
        c.stream_step()
        regs += c.stream_regions(sid); a, i = c.stream_avg(sid); avg.append(a); idx.append(i)
        if k == 60:
            a_j, i_j = c.avg(fid)
            assert c.regions(fid) == want_j[0]
            assert np.array_equal(a_j.view(np.int64), want_j[1].view(np.int64))
    c.stream_close(sid)
    c.stream_step()
    regs += c.stream_regions(sid); a, i = c.stream_avg(sid); avg.append(a); idx.append(i)
    assert_same((regs, np.concatenate(avg), np.concatenate(idx)), want_s)
    c.run(0.1, 0.5)
    assert c.regions(fid) == want_j[0]
    a_j, _ = c.avg(fid)
    assert np.array_equal(a_j.view(np.int64), want_j[1].view(np.int64))
    c.close(); alone.close()
