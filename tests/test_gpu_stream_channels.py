"""Each-channel streams (ss_stream_open_channels) on a real MI355X, against the whole-file per-channel run
(ss_add_pcm_channels + ss_run, ss_get_regions_union, ss_get_region_peaks) on the same context and ss_silence_pcm for the bytes.
Everything is exact unless a comment says why not: per-channel averages bit for bit, bin numbers, the merged regions as values, the
peaks bit for bit, the output byte for byte -- for any split into pieces, any cadence of steps, whatever shares the steps, and across
export / import."""
import math
import os

import numpy as np
import pytest

from softspoken_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR, BRK = 0.1, 0.5
SR, CH = 48000, 2


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native as N
    return N


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


@pytest.fixture(scope="module")
def stereo():
    """The main input: 40 s / 48 kHz 16-bit stereo, seed 3004 (5 regions on the mixdown, 4 on each channel, 2
    merged, hundreds of bins above the threshold on one channel only)."""
    pcm = np.ascontiguousarray(synth.to_pcm16(synth.synth_audio(3004, 40.0, SR, CH)))
    assert pcm.shape == (40 * SR, CH)
    return pcm


def _bytes(pcm):
    return np.frombuffer(np.ascontiguousarray(pcm).tobytes(), dtype=np.uint8)


def whole_file(ctx, pcm, fmt, sr, ch, frames, thr=THR, brk=BRK):
    """The reference: every channel run alone in one job, the merged table and the peaks."""
    ctx.reset()
    first = ctx.add_pcm_channels(_bytes(pcm), fmt, sr, ch, frames)
    ctx.run(thr, brk)
    lanes = [ctx.avg(first + c) for c in range(ch)]
    for a, i in lanes:
        assert np.array_equal(i, lanes[0][1])
    return dict(lane=[a for a, _ in lanes], idx=lanes[0][1], own=[ctx.regions(first + c) for c in range(ch)],
                merged=ctx.regions_union(first, ch), peaks=ctx.region_peaks(first, ch))


def whole_mix(ctx, pcm, fmt, sr, ch, frames, thr=THR, brk=BRK):
    ctx.reset()
    fid = ctx.add_pcm(_bytes(pcm), fmt, sr, ch, frames)
    ctx.run(thr, brk)
    a, i = ctx.avg(fid)
    return ctx.regions(fid), a, i


@pytest.fixture(scope="module")
def whole(native, ctxs, stereo):
    """Whole-file results of the main input per precision, computed once; never changed by a test."""
    made = {}

    def get(prec):
        if prec not in made:
            w = whole_file(ctxs(prec), stereo, native.PCM_S16, SR, CH, len(stereo))
            w["mix"] = whole_mix(ctxs(prec), stereo, native.PCM_S16, SR, CH, len(stereo))
            made[prec] = w
        w = made[prec]
        # the equalities below would pass on a recording whose channels agree: this one's do not
        assert len(w["merged"]) >= 2
        a0, a1 = w["lane"][0] > THR, w["lane"][1] > THR
        assert np.sum(a0 & ~a1) > 0 and np.sum(a1 & ~a0) > 0
        assert w["merged"] != w["mix"][0] and w["merged"] != w["own"][0] and w["merged"] != w["own"][1]
        return w
    return get


class Got:
    """What a stream returned, step by step."""

    def __init__(self, ch, lanes, out_on=False):
        self.ch, self.lanes, self.out_on = ch, lanes, out_on
        self.regs, self.avg, self.idx, self.peaks, self.out, self.at = [], [], [], [], [], 0
        self.lane = [[] for _ in range(lanes)]

    def take(self, ctx, sid):
        r = ctx.stream_regions(sid)
        a, i = ctx.stream_avg(sid)
        self.regs += r; self.avg.append(a); self.idx.append(i)
        if self.lanes > 1:
            for c in range(self.lanes):
                la, li = ctx.stream_avg_channel(sid, c)
                assert np.array_equal(li, i)
                self.lane[c].append(la)
            pk = ctx.stream_region_peaks(sid, self.lanes)
            assert pk.shape == (len(r), self.lanes)
            self.peaks.append(pk)
        if self.out_on:
            first, o = ctx.stream_output(sid, self.ch)
            assert first == self.at and o.shape[1] == self.ch          # contiguous from step to step
            self.at += len(o)
            self.out.append(o)
        return r, i

    def merged(self):
        return np.concatenate(self.avg)

    def bins(self):
        return np.concatenate(self.idx)

    def channel(self, c):
        return np.concatenate(self.lane[c])

    def all_peaks(self):
        return np.concatenate(self.peaks) if self.peaks else np.zeros((0, self.lanes))

    def pcm(self):
        return np.concatenate(self.out)


def feed(ctx, sid, pcm, fb, pieces, step_every, got, on_step=None, finish=True):
    """pieces: frame counts (the rest of the recording goes in one last piece)."""
    b = _bytes(pcm)
    total = b.size // fb
    at, k = 0, 0
    for n in list(pieces) + [total]:
        n = min(n, total - at)
        if n <= 0:
            break
        ctx.stream_push(sid, b[at * fb:(at + n) * fb], frames=n)
        at += n
        k += 1
        if k % step_every == 0:
            ctx.stream_step()
            r, i = got.take(ctx, sid)
            if on_step:
                on_step(at, r, i)
    if finish:
        ctx.stream_close(sid)
        ctx.stream_step()
        got.take(ctx, sid)
        assert ctx.stream_info(sid)["finished"] == 1
        ctx.stream_free(sid)
    return got


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_each(got, w):
    """A finished each-channel stream against the whole-file per-channel run."""
    assert np.array_equal(got.bins(), w["idx"])
    for c in range(got.lanes):
        assert np.array_equal(bits(got.channel(c)), bits(w["lane"][c])), c                  # bit for bit, NaN included
    assert np.array_equal(got.merged(), np.fmax.reduce(np.asarray(w["lane"]), axis=0), equal_nan=True)
    assert got.regs == w["merged"]
    assert got.all_peaks().shape == w["peaks"].shape and np.array_equal(bits(got.all_peaks()), bits(w["peaks"]))


def _random_pieces(seed, total, lo=1, hi=40000):
    rng = np.random.default_rng(seed)
    out, s = [], 0
    while s < total:
        n = int(rng.integers(lo, hi))
        out.append(n)
        s += n
    return out


# the last three cut inside regions and inside merged gaps: where the carried peaks can go wrong
SPLITS = {
    "whole": lambda n: ([], 1),
    "ones-then-997": lambda n: ([1] * 400 + [997] * (n // 997 + 1), 1),
    "ones-then-997-every-7": lambda n: ([1] * 400 + [997] * (n // 997 + 1), 7),
    "random-a": lambda n: (_random_pieces(11, n), 1),
    "random-b": lambda n: (_random_pieces(12, n), 3),
    "tenths": lambda n: ([SR // 10] * (n // (SR // 10) + 1), 1),
}


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_streamed_equals_whole_file(native, ctxs, stereo, whole, precision, split):
    w = whole(precision)
    c = ctxs(precision)
    pieces, every = SPLITS[split](len(stereo))
    sid = c.stream_open_channels(native.PCM_S16, SR, CH, THR, BRK)
    assert_each(feed(c, sid, stereo, 4, pieces, every, Got(CH, CH)), w)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def _encode(native, x, fmt):
    """float [frames, ch] in [-1, 1] -> interleaved bytes of the encoding."""
    x = np.ascontiguousarray(x).reshape(-1)
    if fmt == native.PCM_U8:
        a = np.clip(np.round(x * 127 + 128), 0, 255).astype(np.uint8)
    elif fmt == native.PCM_S16:
        a = np.clip(np.round(x * 32767), -32768, 32767).astype("<i2")
    elif fmt == native.PCM_S16BE:
        a = np.clip(np.round(x * 32767), -32768, 32767).astype(">i2")
    elif fmt == native.PCM_S24:
        v = np.clip(np.round(x * 8388607), -8388608, 8388607).astype("<i4")
        a = np.ascontiguousarray(v.view(np.uint8).reshape(-1, 4)[:, :3])
    elif fmt == native.PCM_S32:
        a = np.clip(np.round(x.astype(np.float64) * 2147483647), -2 ** 31, 2 ** 31 - 1).astype("<i4")
    elif fmt == native.PCM_F32:
        a = x.astype("<f4")
    elif fmt == native.PCM_F64:
        a = x.astype("<f8")
    else:
        raise ValueError(fmt)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


FORMATS = ("PCM_U8", "PCM_S16", "PCM_S24", "PCM_S32", "PCM_F32", "PCM_F64", "PCM_S16BE")
RATES = (16000, 22050, 48000)                         # 22 050 Hz: the planes are the lanes' signals
# every format at every channel count; the rate walks along, so every (format, rate) and (channels, rate) pair occurs too
SHAPES = [(f, ch, RATES[(k + j) % 3]) for k, f in enumerate(FORMATS) for j, ch in enumerate((2, 3, 6))]


def _stream_equals_whole(native, c, raw, fmt, sr, ch, frames, pieces):
    w = whole_file(c, raw, fmt, sr, ch, frames)
    sid = c.stream_open_channels(fmt, sr, ch, THR, BRK)
    got = feed(c, sid, raw, ch * native._BPS[fmt], pieces, 1, Got(ch, ch))
    assert_each(got, w)
    return w


@pytest.mark.parametrize("fmt,ch,sr", SHAPES)
@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_formats_and_shapes_through_the_decode_kernel(native, ctxs, precision, fmt, ch, sr):
    """4 s, an odd frame count, one frame at a time for the first 64 frames (every alignment of a frame in the upload: 24-bit with three
    channels puts frame boundaries at 9 bytes), then 997-frame pieces."""
    fmt = getattr(native, fmt)
    frames = 4 * sr - 3
    x = synth.synth_audio(500 + sr + 7 * fmt + ch, 4.0, sr, ch).T[:frames]
    w = _stream_equals_whole(native, ctxs(precision), _encode(native, x, fmt), fmt, sr, ch, frames, [1] * 64 + [997] * (frames // 997 + 1))
    assert len(w["idx"]) > 256 and all(np.isfinite(a).all() for a in w["lane"])
    assert any(not np.array_equal(w["lane"][0], a) for a in w["lane"][1:])                      # the channels differ


@pytest.mark.parametrize("frames", [1, 7])
@pytest.mark.parametrize("fmt,ch,sr", [("PCM_S16", 2, 48000), ("PCM_S24", 3, 16000), ("PCM_F64", 6, 22050)])
def test_recordings_of_a_few_frames(native, ctxs, fmt, ch, sr, frames):
    fmt = getattr(native, fmt)
    x = synth.synth_audio(77, 1.0, sr, ch, with_silence=False).T[1000:1000 + frames]
    for precision in ("fp32", "f16x2"):
        _stream_equals_whole(native, ctxs(precision), _encode(native, x, fmt), fmt, sr, ch, frames, [1] * 3)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def _mix_loop(native, c, stereo, piece, company=None):
    """A mix stream of the main input in 0.5 s pieces; company(round) may open, push and close other streams before each step."""
    sid = c.stream_open(native.PCM_S16, SR, CH, THR, BRK)
    got = Got(CH, 1)
    n_rounds = len(stereo) // piece
    for k in range(n_rounds + 1):
        if k < n_rounds:
            c.stream_push(sid, stereo[k * piece:(k + 1) * piece], frames=piece)
        else:
            c.stream_close(sid)
        if company:
            company(k)
        c.stream_step()
        got.take(c, sid)
        if company:
            company(-1 - k)
    assert c.stream_info(sid)["finished"] == 1
    c.stream_free(sid)
    return got


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_company(native, ctxs, stereo, whole, precision):
    w = whole(precision)
    c = ctxs(precision)
    piece = SR // 2
    n_rounds = len(stereo) // piece
    alone = _mix_loop(native, c, stereo, piece)
    left = np.ascontiguousarray(stereo[:, 0])
    short = np.ascontiguousarray(synth.to_pcm16(synth.synth_audio(3002, 8.0, 16000, 2)))
    w_short = whole_file(c, short, native.PCM_S16, 16000, 2, len(short))
    w_short_mix = whole_mix(c, short, native.PCM_S16, 16000, 2, len(short))
    st = {}

    def company(k):
        if k < 0:                                                  # after the step: collect
            for s in st.values():
                if not s["done"]:
                    s["got"].take(c, s["sid"])
                    s["done"] = bool(c.stream_info(s["sid"])["finished"])
            return
        if k == 0:
            st["each"] = dict(sid=c.stream_open_channels(native.PCM_S16, SR, CH, THR, BRK), got=Got(CH, CH), done=False)
            st["left"] = dict(sid=c.stream_open(native.PCM_S16, SR, 1, THR, BRK), got=Got(1, 1), done=False)
        if k == 11:                                                # others open midway and finish midway
            st["short_each"] = dict(sid=c.stream_open_channels(native.PCM_S16, 16000, 2, THR, BRK), got=Got(2, 2), done=False)
            st["short_mix"] = dict(sid=c.stream_open(native.PCM_S16, 16000, 2, THR, BRK), got=Got(2, 1), done=False)
        if k < n_rounds:
            c.stream_push(st["each"]["sid"], stereo[k * piece:(k + 1) * piece], frames=piece)
            c.stream_push(st["left"]["sid"], left[k * piece:(k + 1) * piece], frames=piece)
        else:
            c.stream_close(st["each"]["sid"]); c.stream_close(st["left"]["sid"])
        if 11 <= k < 11 + 9:
            lo, hi = (k - 11) * 16000, (k - 10) * 16000
            for name in ("short_each", "short_mix"):
                if lo < len(short):
                    c.stream_push(st[name]["sid"], short[lo:hi], frames=len(short[lo:hi]))
                else:
                    c.stream_close(st[name]["sid"])

    mixed = _mix_loop(native, c, stereo, piece, company)
    assert all(s["done"] for s in st.values())
    for s in st.values():
        c.stream_free(s["sid"])
    # each equals its own whole-file result
    assert_each(st["each"]["got"], w)
    assert_each(st["short_each"]["got"], w_short)
    for g, ref in ((mixed, w["mix"]), (st["short_mix"]["got"], w_short_mix)):
        assert g.regs == ref[0] and np.array_equal(g.bins(), ref[2]) and np.array_equal(bits(g.merged()), bits(ref[1]))
    # the mix stream is what it is without the others
    assert mixed.regs == alone.regs and np.array_equal(bits(mixed.merged()), bits(alone.merged())) and np.array_equal(mixed.bins(), alone.bins())
    # the mono stream of channel 0 is lane 0, bit for bit
    lg = st["left"]["got"]
    assert np.array_equal(bits(lg.merged()), bits(st["each"]["got"].channel(0))) and np.array_equal(lg.bins(), st["each"]["got"].bins())
    assert lg.regs == w["own"][0]


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def test_one_channel_is_a_plain_stream_and_the_launch_names(native, blob, stereo, whole):
    whole("f16x2")
    c = native.Context(blob, 0, precision="f16x2", profile=True)
    new = {"stream_decode_channels", "stream_union"}
    try:
        mono = np.ascontiguousarray(stereo[:10 * SR, 0])
        pieces = [1, 4999, SR, 3 * SR]
        c.reset_stats()
        a = feed(c, c.stream_open_channels(native.PCM_S16, SR, 1, THR, BRK), mono, 2, pieces, 1, Got(1, 1))
        b = feed(c, c.stream_open(native.PCM_S16, SR, 1, THR, BRK), mono, 2, pieces, 1, Got(1, 1))
        assert a.regs == b.regs and np.array_equal(bits(a.merged()), bits(b.merged())) and np.array_equal(a.bins(), b.bins()) and len(a.bins()) > 500
        sid = c.stream_open_channels(native.PCM_S16, SR, 1, THR, BRK)
        c.stream_push(sid, mono[:5 * SR]); c.stream_step()
        assert c.stream_export(sid)[:8] == b"SSSTRM01"
        with pytest.raises(native.NativeError) as e:
            c.stream_region_peaks(sid, 1)
        assert e.value.code == native.SS_ERR_STATE
        c.stream_free(sid)
        names = {s["name"] for s in c.kernel_stats()}
        assert "stream_decode" in names and "stream_average" in names and not (names & new), names
        # a step over mix streams only
        c.reset_stats()
        m = c.stream_open(native.PCM_S16, SR, CH, THR, BRK)
        c.stream_push(m, stereo[:5 * SR]); c.stream_step()
        names = {s["name"] for s in c.kernel_stats()}
        assert "stream_decode" in names and not (names & new), names
        with pytest.raises(native.NativeError) as e:
            c.stream_region_peaks(m, CH)
        assert e.value.code == native.SS_ERR_STATE
        with pytest.raises(native.NativeError) as e:
            c.stream_avg_channel(m, 1)
        assert e.value.code == native.SS_ERR_ARG
        a0, i0 = c.stream_avg_channel(m, 0)
        assert len(a0) > 0 and np.array_equal(bits(a0), bits(c.stream_avg(m)[0])) and np.array_equal(i0, c.stream_avg(m)[1])
        # ... and one with an each-channel stereo stream
        c.reset_stats()
        s = c.stream_open_channels(native.PCM_S16, SR, CH, THR, BRK)
        c.stream_push(s, stereo[:5 * SR]); c.stream_push(m, stereo[5 * SR:6 * SR]); c.stream_step()
        stats = {k["name"]: k for k in c.kernel_stats()}
        assert new <= set(stats) and "stream_decode" in stats
        assert stats["stream_decode_channels"]["launches"] == 1 and stats["stream_decode_channels"]["bytes"] == 5 * SR * 4 + 4 * 2 * 5 * SR
        nb = len(c.stream_avg(s)[1])
        assert stats["stream_union"]["launches"] == 1 and nb > 0
        for ch in (-1, 2):
            with pytest.raises(native.NativeError) as e:
                c.stream_avg_channel(s, ch)
            assert e.value.code == native.SS_ERR_ARG
        assert c.stream_export(s)[:8] == b"SSSTRM04"
    finally:
        c.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
ERASES = {"default": None, "padded": dict(pad_s=0.05, min_len_s=0.1)}


@pytest.fixture(scope="module")
def silenced(native, ctxs, stereo, whole):
    """Per (precision, erase): the whole-file silencer over E(merged table), and a mix stream's output of the same recording."""
    made = {}

    def get(prec, key):
        if (prec, key) not in made:
            c, w = ctxs(prec), whole(prec)
            e = {"pad_s": 0.0, "min_len_s": 0.0, **(ERASES[key] or {})}
            want = c.silence_pcm(stereo, native.PCM_S16, SR, CH, len(stereo), native.erase_table(w["merged"], e["pad_s"], e["min_len_s"]))
            mix = feed(c, c.stream_open_output(native.PCM_S16, SR, CH, THR, BRK, e), stereo, 4, [], 1, Got(CH, 1, True)).pcm()
            made[(prec, key)] = (want, mix)
        return made[(prec, key)]
    return get


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("erase", list(ERASES))
@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_output_is_the_whole_file_silencer_over_the_merged_table(native, ctxs, stereo, whole, silenced, precision, erase, split):
    w = whole(precision)
    c = ctxs(precision)
    want, mix = silenced(precision, erase)
    pieces, every = SPLITS[split](len(stereo))
    sid = c.stream_open_channels(native.PCM_S16, SR, CH, THR, BRK, ERASES[erase] or dict())
    got = Got(CH, CH, True)
    b = _bytes(stereo)
    at, k = 0, 0
    for n in list(pieces) + [len(stereo)]:
        n = min(n, len(stereo) - at)
        if n <= 0:
            break
        c.stream_push(sid, b[at * 4:(at + n) * 4], frames=n)
        at += n; k += 1
        if k % every == 0:
            c.stream_step(); got.take(c, sid)
            assert got.at <= at
    c.stream_close(sid); c.stream_step(); got.take(c, sid)
    info = c.stream_output_info(sid)
    assert c.stream_info(sid)["finished"] == 1 and info["frames_out"] == len(stereo) == got.at and info["frames_held"] == 0
    c.stream_free(sid)
    assert got.regs == w["merged"]
    out = got.pcm()
    assert out.shape == want.shape and out.dtype == want.dtype and np.array_equal(out, want)
    assert 0 < info["frames_erased"] < len(stereo)
    zeroed = np.flatnonzero(~want.any(axis=1) & stereo.any(axis=1))
    assert info["frames_erased"] >= len(zeroed) > 0
    assert not np.array_equal(out, mix)                                # the merged table mattered


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def _bounds(sr, brk, erase):
    """B and D of include/softspoken.h."""
    hdr = open(os.path.join(ROOT, "include", "softspoken.h")).read()
    assert "B = 3 s + 2 x (3 / 256) s + half / sample_rate" in hdr
    assert "D = B + break_s + pad_s + min_len_s" in hdr
    half = 0 if sr == 22050 else math.ceil(32.0 / min(1.0, 22050.0 / sr))
    B = 3.0 + 2 * 3.0 / 256 + half / sr
    return B, B + brk + erase["pad_s"] + erase["min_len_s"]


@pytest.mark.parametrize("sr", [48000, 16000])
def test_latency_bounds(native, ctxs, stereo, whole, sr):
    """0.1 s pieces, a step after each.  With H the audio held at a step: every bin with t + B < H, every merged region with
    t_end + break_s + B < H and every frame with t + D < H has been returned by then.  Bin times are the reference's 4-decimal strings
    (within 5e-5 s of idx x 3 / 256): the bins are tested on them; the frame limit is nearbyint(L x sample_rate), so one frame."""
    whole("fp32")
    c = ctxs("fp32")
    erase = dict(pad_s=0.05, min_len_s=0.1)
    pcm = stereo if sr == SR else np.ascontiguousarray(synth.to_pcm16(synth.synth_audio(3004, 40.0, sr, CH)))
    w = whole("fp32") if sr == SR else whole_file(c, pcm, native.PCM_S16, sr, CH, len(pcm))
    assert len(w["merged"]) >= 1
    B, D = _bounds(sr, BRK, erase)
    t_bin = np.array([float("%.4f" % (i * 3.0 / 256.0)) - 3.0 for i in w["idx"].tolist()])
    n = len(pcm)
    sid = c.stream_open_channels(native.PCM_S16, sr, CH, THR, BRK, erase)
    got = Got(CH, CH, True)
    seen = dict(bins=0, regs=0)

    def on_step(at, r, i):
        H = at / sr
        seen["bins"] += len(i)
        assert seen["bins"] >= int(np.sum(t_bin + B < H)), H
        assert len(got.regs) >= sum(1 for _, e in w["merged"] if e + BRK + B < H), H
        assert got.regs == w["merged"][:len(got.regs)]
        assert got.at >= min(n, (H - D) * sr - 1), (H, got.at)
    feed(c, sid, pcm, 4, [sr // 10] * (n // (sr // 10)), 1, got, on_step)
    assert_each(got, w)
    assert np.array_equal(got.pcm(), c.silence_pcm(pcm, native.PCM_S16, sr, CH, n, native.erase_table(w["merged"], 0.05, 0.1)))


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
LANES_AT = 8 + 8 * 4 + 4 * 8 + 14 * 8 + 8                 # magic, ints, doubles, counters, step: the lane count of "SSSTRM04"


def _move_case(native, src, dst, stereo, w_src, with_output):
    """Feed the main input in 0.25 s pieces on src, export inside the longest merged region, finish on dst.
    -> (got, bins returned before the move, windows run before it, the image)"""
    piece = SR // 4
    s0, e0 = max(w_src["merged"], key=lambda r: r[1] - r[0])
    assert e0 - s0 > 1.0
    move_at = int(((s0 + e0) / 2 + 3.2) * SR) // piece * piece          # the bins up to the middle of the region are final by then
    erase = dict(pad_s=0.05, min_len_s=0.1)
    sid = src.stream_open_channels(native.PCM_S16, SR, CH, THR, BRK, erase if with_output else None)
    got = Got(CH, CH, with_output)
    c, before, image, win_run = src, None, None, None
    for at in range(0, len(stereo), piece):
        if at == move_at:
            # an open merged region: the walk is inside it -- final bins of it are above the threshold, it is not returned yet (and
            # cannot be: its end is not final)
            t = got.bins() * 3.0 / 256.0 - 3.0
            assert (s0, e0) not in got.regs and np.any((got.merged() > THR) & (t > s0 - 0.001)) and t[-1] < e0 - 0.1
            before, win_run = len(got.bins()), src.stream_info(sid)["windows_run"]
            image = src.stream_export(sid)
            assert image[:8] == b"SSSTRM04"
            src.stream_free(sid)
            sid, c = dst.stream_import(image), dst
        c.stream_push(sid, stereo[at:at + piece], frames=len(stereo[at:at + piece]))
        c.stream_step()
        got.take(c, sid)
    c.stream_close(sid); c.stream_step(); got.take(c, sid)
    assert c.stream_info(sid)["finished"] == 1 and image is not None
    if with_output:
        assert c.stream_output_info(sid)["frames_out"] == len(stereo) == got.at
    c.stream_free(sid)
    return got, before, win_run, image


@pytest.mark.parametrize("with_output", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_image_into_a_second_context(native, ctxs, stereo, whole, precision, with_output):
    w = whole(precision)
    got, before, _, _ = _move_case(native, ctxs(precision), ctxs(precision, key=1), stereo, w, with_output)
    assert before > 0
    assert_each(got, w)                                    # everything, peaks included
    if with_output:
        want = ctxs(precision).silence_pcm(stereo, native.PCM_S16, SR, CH, len(stereo), native.erase_table(w["merged"], 0.05, 0.1))
        assert np.array_equal(got.pcm(), want)


@pytest.mark.parametrize("with_output", [False, True])
def test_image_from_f16x2_into_fp32(native, ctxs, stereo, whole, with_output):
    """Before the move: the f16x2 whole-file run's, bit for bit.  After it the windows run in fp32: a bin that only such windows cover
    is the fp32 run's bit for bit; the bins in between also average carried f16x2 logits and lie within the f16x2 mode's 1e-4 of it."""
    w16, w32 = whole("f16x2"), whole("fp32")
    got, before, win_run, _ = _move_case(native, ctxs("f16x2"), ctxs("fp32", key=1), stereo, w16, with_output)
    assert np.array_equal(got.bins(), w32["idx"]) and np.array_equal(w16["idx"], w32["idx"]) and 0 < before < len(w32["idx"])
    pure = got.bins() >= native.window_start_bin(win_run - 1) + 256
    assert 0 < np.sum(pure) < len(pure) - before
    for ch in range(CH):
        a = got.channel(ch)
        assert np.array_equal(bits(a[:before]), bits(w16["lane"][ch][:before]))
        assert np.array_equal(bits(a[pure]), bits(w32["lane"][ch][pure]))
        assert np.abs(a[before:] - w32["lane"][ch][before:]).max() < 1e-4
    assert np.array_equal(got.merged(), np.fmax(got.channel(0), got.channel(1)))
    assert got.all_peaks().shape == (len(got.regs), CH)
    assert got.regs == native.find_regions(got.merged(), got.bins(), THR, BRK)


def test_broken_images_are_refused_and_open_nothing(native, ctxs, stereo, whole):
    c = ctxs("f16x2")
    for erase in (None, dict(pad_s=0.05, min_len_s=0.1)):
        sid = c.stream_open_channels(native.PCM_S16, SR, CH, THR, BRK, erase)
        c.stream_push(sid, stereo[:6 * SR]); c.stream_step()
        c.stream_push(sid, stereo[6 * SR:6 * SR + 777])                        # staged frames travel too
        image = c.stream_export(sid)
        c.stream_free(sid)
        assert image[:8] == b"SSSTRM04" and int.from_bytes(image[LANES_AT:LANES_AT + 4], "little") == CH
        three = bytearray(image); three[LANES_AT:LANES_AT + 4] = (3).to_bytes(4, "little")
        nxt = c.stream_import(image)
        c.stream_free(nxt)
        for img in (image[:-1], image[:len(image) // 2], image[:LANES_AT + 2], image + b"\0", bytes(three)):
            with pytest.raises(native.NativeError) as e:
                c.stream_import(img)
            assert e.value.code == native.SS_ERR_ARG
        again = c.stream_import(image)
        assert again == nxt + 1                                                 # the refused ones opened nothing
        c.stream_free(again)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nan_case(native, ctxs):
    x = np.ascontiguousarray(synth.synth_audio(3004, 40.0, SR, CH).T.astype(np.float32))
    x[SR * 20, 0] = np.float32("nan")
    return x, whole_file(ctxs("fp32"), x, native.PCM_F32, SR, CH, len(x))


def test_a_nan_on_one_channel_does_not_hide_the_other(native, ctxs, whole, nan_case):
    """fp32 takes the NaN sample without a refusal.  The merged series is the NaN-passing maximum (assert_each compares it with
    np.fmax of the whole-file lanes), so wherever channel 0's average is NaN the merged value is channel 1's, and channel 1's regions
    stand in the merged table.  (Measured on the MI355X: the fp32 run's averages of channel 0 hold no NaN at all for this input -- 0
    of 3891 bins --, so the table is decided by finite values on both channels here; the count is printed.)"""
    whole("fp32")
    x, w = nan_case
    c = ctxs("fp32")
    got = feed(c, c.stream_open_channels(native.PCM_F32, SR, CH, THR, BRK), x, 8, [SR // 2] * 80, 1, Got(CH, CH))
    assert_each(got, w)
    nan0 = np.isnan(got.channel(0))
    print("bins whose average is NaN on channel 0:", int(nan0.sum()), "of", len(nan0))
    assert not np.isnan(got.channel(1)).any() and not np.isnan(got.merged()).any()
    assert np.array_equal(got.merged()[nan0], got.channel(1)[nan0])
    assert len(w["own"][1]) > 0                                                 # channel 1 opens regions, and each lies inside a merged one
    for s1, e1 in w["own"][1]:
        assert any(s <= s1 and e1 <= e for s, e in got.regs), (s1, e1)


def test_f16x2_refuses_the_step_and_commits_nothing(native, ctxs, whole, nan_case):
    whole("f16x2")
    x, _ = nan_case
    c = ctxs("f16x2")
    sid = c.stream_open_channels(native.PCM_F32, SR, CH, THR, BRK, dict(pad_s=0.05, min_len_s=0.1))
    c.stream_push(sid, x[:SR * 19]); c.stream_step()
    info, oinfo, image = c.stream_info(sid), c.stream_output_info(sid), c.stream_export(sid)
    last = (c.stream_regions(sid), c.stream_avg_channel(sid, 1), c.stream_region_peaks(sid, CH), c.stream_output(sid, CH))
    assert info["windows_run"] > 0 and oinfo["frames_out"] > 0
    c.stream_push(sid, x[SR * 19:SR * 22])
    with pytest.raises(native.NativeError) as e:
        c.stream_step()
    assert e.value.code == native.SS_ERR_RANGE
    after, oafter = c.stream_info(sid), c.stream_output_info(sid)
    staged = dict(frames_pushed=info["frames_pushed"] + 3 * SR, frames_staged=3 * SR)       # the staged frames are kept
    assert {k: v for k, v in after.items() if k not in staged and k != "windows_ready"} == \
           {k: v for k, v in info.items() if k not in staged and k != "windows_ready"}
    assert {k: after[k] for k in staged} == staged and after["windows_ready"] > 0
    assert oafter == dict(oinfo, frames_held=oinfo["frames_held"] + 3 * SR)
    again = (c.stream_regions(sid), c.stream_avg_channel(sid, 1), c.stream_region_peaks(sid, CH), c.stream_output(sid, CH))
    assert again[0] == last[0] and np.array_equal(again[1][0], last[1][0]) and np.array_equal(again[2], last[2])
    assert again[3][0] == last[3][0] and np.array_equal(again[3][1], last[3][1])
    # the carried state is as it was: the image differs from the earlier one by the staged bytes alone
    image2 = c.stream_export(sid)
    assert len(image2) == len(image) + 3 * SR * 8
    c.stream_free(sid)


def test_the_detector_finishes_an_each_channel_stream_in_fp32(native, blob, whole, nan_case, caplog):
    """One refusal; the stream moves with its mode.  What became final before the refusal was computed in f16x2, so against the fp32
    run the averages carry the f16x2 mode's 1e-4, as StreamDetector's mix streams do (tests/test_gpu_stream.py)."""
    import logging
    from softspoken_amd.stream import StreamDetector
    whole("fp32")
    x, w = nan_case
    det = StreamDetector(blob, precision="f16x2")
    s = det.open(native.PCM_F32, SR, CH, THR, BRK, channel_mode="each")
    regs, avg, idx, lane1, peaks = [], [], [], [], []
    with caplog.at_level(logging.WARNING):
        for k in list(range(0, len(x), SR // 2)) + [None]:
            if k is None:
                s.close()
            else:
                s.push(x[k:k + SR // 2])
            r, a, i = det.step()[s]
            regs += r; avg.append(a); idx.append(i); lane1.append(s.avg(1)[0]); peaks.append(s.peaks())
    assert s.precision == "fp32" and s.channel_mode == "each" and det._refused_steps == 1
    avg, idx, lane1, peaks = np.concatenate(avg), np.concatenate(idx), np.concatenate(lane1), np.concatenate(peaks)
    want = np.fmax(w["lane"][0], w["lane"][1])
    assert np.array_equal(idx, w["idx"]) and not np.isnan(avg).any()
    assert np.abs(avg - want).max() < 1e-4 and np.abs(lane1 - w["lane"][1]).max() < 1e-4
    if regs != w["merged"]:                                # only bins within 1e-4 of the threshold may decide differently
        assert np.all(np.abs(want[(avg > THR) != (want > THR)] - THR) < 1e-4)
    else:
        assert peaks.shape == w["peaks"].shape and np.abs(peaks - w["peaks"]).max() < 1e-4
    det.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
def test_state_does_not_grow_and_counts_the_raw_pcm_once(native, ctxs, stereo, whole):
    whole("f16x2")
    c = ctxs("f16x2")
    erase = dict(pad_s=0.05, min_len_s=0.1)
    piece = SR // 2
    e = c.stream_open_channels(native.PCM_S16, SR, CH, THR, BRK)
    eo = c.stream_open_channels(native.PCM_S16, SR, CH, THR, BRK, erase)
    mo = c.stream_open_output(native.PCM_S16, SR, CH, THR, BRK, erase)
    sizes = []
    for k in range(len(stereo) // piece):
        for sid in (e, eo, mo):
            c.stream_push(sid, stereo[k * piece:(k + 1) * piece], frames=piece)
        c.stream_step()
        sizes.append(c.stream_info(e)["state_bytes"])
        if k >= 10:
            raw_e = c.stream_output_info(eo)["frames_held"] * 4
            raw_m = c.stream_output_info(mo)["frames_held"] * 4
            lane_part = c.stream_info(mo)["state_bytes"] - raw_m
            assert c.stream_info(eo)["state_bytes"] <= CH * lane_part + raw_e, k
            assert c.stream_info(eo)["state_bytes"] >= c.stream_info(e)["state_bytes"] + raw_e
    mid = np.abs(np.diff(sizes[10:])).max()
    assert mid > 0 and abs(sizes[79] - sizes[39]) <= mid, (sizes[39], sizes[79], mid)        # 20 s and 40 s of the stream
    assert sizes[79] < 2 * 400_000
    for sid in (e, eo, mo):
        c.stream_free(sid)
