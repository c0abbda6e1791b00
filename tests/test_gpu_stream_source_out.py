"""Source-output streams on a real MI355X (ss_stream_open_source / ss_stream_output_bytes, include/softspoken.h "source output"): the
concatenation of what such a stream returns equals ss_silence_pcm_source(the whole recording, E(R)) byte for byte, R being the regions
the same stream returned -- for odd piece sizes down to one frame, steps that return nothing, 9-byte frames, every word alignment of
the two source segments, each-channel lanes, a move to an fp32 context through the image, and a step shared with the older kinds of
stream, which must return exactly what they return alone."""
import signal

import numpy as np
import pytest

import source_out_ref as S
import stream_output_ref as R
from softspoken_amd import synth

pytestmark = pytest.mark.gpu
SR, SECONDS = 16000, 10.0
ERASE = dict(pad_s=0.05, min_len_s=0.0)


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file runs once under its own limit: a step that hangs ends the test, not the session."""
    def on_alarm(signum, frame):
        raise TimeoutError("the stream test passed its 120 s limit")
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native as N
    return N


@pytest.fixture(scope="module")
def ctxs(native, blob):
    made = {}

    def get(prec):
        if prec not in made:
            made[prec] = native.Context(blob, 0, precision=prec)
        return made[prec]
    yield get
    for c in made.values():
        c.close()


_RECS = {}


def _rec(fmt, ch, seed=71):
    """(bytes uint8, frames) of a 10 s recording at 16 kHz in the encoding fmt."""
    if (fmt, ch, seed) not in _RECS:
        x = synth.synth_audio(seed, SECONDS, SR, ch).T.reshape(-1, ch).astype(np.float32)
        if fmt == 5:
            x = x * np.float32(1.3)                                  # beyond +-1: the 16-bit path would wrap these
        _RECS[(fmt, ch, seed)] = (S.encode(x.reshape(-1), fmt), len(x))
    return _RECS[(fmt, ch, seed)]


def _threshold(native, ctx, data, fmt, ch, frames, brk=0.5):
    """A quantile of the recording's own averages at which E(regions) erases some frames and keeps some."""
    def offline(thr):
        ctx.reset()
        fid = ctx.add_pcm(data, fmt, SR, ch, frames)
        ctx.run(thr, brk)
        return ctx.regions(fid), ctx.avg(fid)[0]
    avg = offline(0.1)[1]
    for q in (0.5, 0.4, 0.6, 0.3, 0.7):
        thr = float(np.nanquantile(avg, q))
        table = native.erase_table(offline(thr)[0], ERASE["pad_s"], ERASE["min_len_s"])
        erased = sum(b - a for a, b in R.silence_ranges(table, SR, frames))
        if 0.05 * frames < erased < 0.95 * frames:
            return thr
    raise AssertionError("no quantile of the averages gives something to erase and something to keep")


def _pieces(seed, total, head=()):
    rng = np.random.default_rng(seed)
    out = list(head)
    while sum(out) < total:
        out.append(int(rng.integers(1, 9000)) | 1)                   # odd sizes
    return out


def _drive(ctx, streams, data, fb, frames, pieces, on_mid=None):
    """Push the recording into every stream of `streams` ({name: [sid, kind]}; kind "source" / "pcm16" / "plain") piece by piece, one
    step per piece -> {name: dict(regions, out, avg, steps)}; checks that every step continues where the last one ended.  on_mid(k):
    called once half the pieces are in, may replace the stream ids (an export / import)."""
    res = {k: dict(regions=[], out=[], avg=[], idx=[], at=0, counts=[]) for k in streams}

    def step():
        for name, (c, sid, kind, _) in streams.items():
            r = res[name]
            r["regions"].extend(c.stream_regions(sid))
            a, idx = c.stream_avg(sid)
            r["avg"].append(a)
            r["idx"].append(idx)
            if kind == "plain":
                continue
            first, o = c.stream_output_bytes(sid, fb) if kind == "source" else c.stream_output(sid, fb // S.BPS[streams[name][3]])
            assert first == r["at"]
            r["at"] += len(o)
            r["counts"].append(len(o))
            r["out"].append(o)
    at = 0
    for k, n in enumerate(pieces):
        n = min(n, frames - at)
        if n <= 0:
            break
        for c, sid, *_ in streams.values():
            c.stream_push(sid, data[at * fb:(at + n) * fb], frames=n)
        at += n
        for c in {id(v[0]): v[0] for v in streams.values()}.values():
            c.stream_step()
        step()
        if on_mid and k == len(pieces) // 2:
            on_mid()
            on_mid = None
    for c, sid, *_ in streams.values():
        c.stream_close(sid)
    for c in {id(v[0]): v[0] for v in streams.values()}.values():
        c.stream_step()
    step()
    for name, (c, sid, kind, *_) in streams.items():
        assert c.stream_info(sid)["finished"] == 1
        if kind != "plain":
            assert res[name]["at"] == frames and c.stream_output_info(sid)["frames_held"] == 0
            res[name]["out"] = np.concatenate(res[name]["out"])
        res[name]["avg"] = np.concatenate(res[name]["avg"])
        res[name]["idx"] = np.concatenate(res[name]["idx"])
        c.stream_free(sid)
    return res


def _expect(native, ctx, data, fmt, ch, frames, regions):
    table = native.erase_table(regions, ERASE["pad_s"], ERASE["min_len_s"])
    want = ctx.silence_pcm_source(data, fmt, SR, ch, frames, table)
    assert np.array_equal(want, S.silence_source(data, fmt, SR, ch, frames, table))
    erased = int(S.frame_mask(frames, SR, table).sum())
    assert 0 < erased < frames
    return want


def _assert_bytes(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        raise AssertionError(f"{len(bad)} frames differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


CASES = {"s16 stereo": (2, 2), "s24 x 3": (3, 3), "u8 mono": (1, 1), "f32 stereo": (5, 2)}


@pytest.mark.parametrize("name", list(CASES))
def test_stream_equals_the_whole_file_call(native, ctxs, name):
    fmt, ch = CASES[name]
    ctx = ctxs("fp32")
    data, frames = _rec(fmt, ch)
    fb = ch * S.BPS[fmt]
    thr = _threshold(native, ctx, data, fmt, ch, frames)
    sid = ctx.stream_open_source(fmt, SR, ch, thr, 0.5, ERASE)
    pieces = _pieces(3 + fmt, frames, head=[1] * 40 + [3, 5, 7, 997])
    r = _drive(ctx, {"s": [ctx, sid, "source", fmt]}, data, fb, frames, pieces)["s"]
    assert r["counts"][0] == 0 and 0 in r["counts"][:40] and max(r["counts"]) > 0          # steps that return nothing, and steps that do
    _assert_bytes(r["out"], _expect(native, ctx, data, fmt, ch, frames, r["regions"]))


def test_each_channel_stream(native, ctxs):
    fmt, ch = 2, 2
    ctx = ctxs("fp32")
    data, frames = _rec(fmt, ch)
    thr = _threshold(native, ctx, data, fmt, ch, frames)
    sid = ctx.stream_open_source(fmt, SR, ch, thr, 0.5, ERASE, each_channel=True)
    r = _drive(ctx, {"s": [ctx, sid, "source", fmt]}, data, 4, frames, _pieces(11, frames))["s"]
    _assert_bytes(r["out"], _expect(native, ctx, data, fmt, ch, frames, r["regions"]))


def test_export_import_mid_stream_into_an_fp32_context(native, ctxs):
    fmt, ch = 3, 3
    a, b = ctxs("f16x2"), ctxs("fp32")
    data, frames = _rec(fmt, ch)
    thr = _threshold(native, b, data, fmt, ch, frames)
    streams = {"s": [a, a.stream_open_source(fmt, SR, ch, thr, 0.5, ERASE), "source", fmt]}
    seen = {}

    def move():
        c, sid = streams["s"][0], streams["s"][1]
        image = c.stream_export(sid)
        seen["magic"] = (image[:8], image[8:16])
        streams["s"][0], streams["s"][1] = b, b.stream_import(image)
        c.stream_free(sid)
    r = _drive(a, streams, data, 9, frames, _pieces(12, frames), on_mid=move)["s"]
    assert seen["magic"] == (b"SSSTRM06", b"SSSTRM03")
    _assert_bytes(r["out"], _expect(native, b, data, fmt, ch, frames, r["regions"]))


def test_a_shared_step_leaves_the_older_streams_as_they_were(native, ctxs):
    fmt, ch = 2, 2
    ctx = ctxs("fp32")
    data, frames = _rec(fmt, ch)
    thr = _threshold(native, ctx, data, fmt, ch, frames)
    pieces = _pieces(13, frames, head=[1, 1, 4001])

    def run(kinds):
        streams = {}
        for kind in kinds:
            sid = (ctx.stream_open_source(fmt, SR, ch, thr, 0.5, ERASE) if kind == "source" else
                   ctx.stream_open_output(fmt, SR, ch, thr, 0.5, ERASE) if kind == "pcm16" else ctx.stream_open(fmt, SR, ch, thr, 0.5))
            streams[kind] = [ctx, sid, kind, fmt]
        return _drive(ctx, streams, data, 4, frames, pieces)
    shared = run(("source", "pcm16", "plain"))
    for kind in ("pcm16", "plain"):
        alone = run((kind,))[kind]
        assert alone["regions"] == shared[kind]["regions"]
        assert alone["avg"].tobytes() == shared[kind]["avg"].tobytes() and np.array_equal(alone["idx"], shared[kind]["idx"])
        if kind == "pcm16":
            assert alone["counts"] == shared[kind]["counts"] and alone["out"].tobytes() == shared[kind]["out"].tobytes()
    table = native.erase_table(shared["pcm16"]["regions"], ERASE["pad_s"], ERASE["min_len_s"])
    assert np.array_equal(shared["pcm16"]["out"], ctx.silence_pcm(data, fmt, SR, ch, frames, table))
    _assert_bytes(shared["source"]["out"], _expect(native, ctx, data, fmt, ch, frames, shared["source"]["regions"]))
    assert shared["source"]["regions"] == shared["pcm16"]["regions"] and shared["source"]["counts"] == shared["pcm16"]["counts"]


def test_the_wrong_getter_is_a_state_error(native, ctxs):
    ctx = ctxs("fp32")
    src = ctx.stream_open_source(2, SR, 1, 0.1, 0.5, None)
    old = ctx.stream_open_output(2, SR, 1, 0.1, 0.5, ERASE)
    plain = ctx.stream_open(2, SR, 1, 0.1, 0.5)
    try:
        for fn, sid in ((ctx.stream_output, src), (ctx.stream_output_bytes, old), (ctx.stream_output_bytes, plain)):
            with pytest.raises(native.NativeError) as e:
                fn(sid, 2)
            assert e.value.code == native.SS_ERR_STATE
        assert ctx.stream_output_bytes(src, 2)[1].shape == (0, 2) and ctx.stream_output_info(src)["pad_s"] == 0.0
        assert ctx.stream_export(old)[:8] == b"SSSTRM03" and ctx.stream_export(plain)[:8] == b"SSSTRM01"
        with pytest.raises(native.NativeError):
            ctx.stream_import(b"SSSTRM06" + ctx.stream_export(plain))
    finally:
        for sid in (src, old, plain):
            ctx.stream_free(sid)


def test_stream_detector_and_wav_writer(tmp_path, native, ctxs):
    from softspoken_amd.stream import StreamDetector, StreamWavWriter
    fmt, ch = 1, 1
    ctx = ctxs("fp32")
    data, frames = _rec(fmt, ch)
    thr = _threshold(native, ctx, data, fmt, ch, frames)
    det = StreamDetector(precision="fp32", context_factory=lambda p: ctx)
    s = det.open(fmt, SR, ch, threshold=thr, erase=ERASE, encoding="source")
    regions = []
    with StreamWavWriter(tmp_path / "feed.wav", SR, ch, fmt=fmt) as w:
        for at in range(0, frames, 12345):
            s.push(data[at:at + 12345])
            regions += det.step()[s][0]
            w.write(s.output())
        s.close()
        regions += det.step()[s][0]
        w.write(s.output())
    det.free(s)
    want = _expect(native, ctx, data, fmt, ch, frames, regions)
    assert (tmp_path / "feed.wav").read_bytes() == native.wav_header(fmt, SR, ch, frames) + want.tobytes()
    with pytest.raises(ValueError):
        StreamWavWriter(tmp_path / "x.wav", SR, 2, fmt=native.PCM_S16BE)
    with pytest.raises(ValueError):
        det.open(fmt, SR, ch, encoding="flac")
