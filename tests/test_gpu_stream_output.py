"""The streaming silencer (ss_stream_open_output / ss_stream_output, softspoken_amd.stream) against the whole-file silencer over the
whole-file detection: the concatenation of a stream's output equals ss_silence_pcm(recording, E(regions)) byte for byte, for any split
of the input, any cadence of steps, every encoding and whatever shares the step; the frames arrive contiguous, final and within the
latency bound D of include/softspoken.h, and the carried state does not grow with the stream."""
import logging
import math
import os

import numpy as np
import pytest

import stream_output_ref as R
from softspoken_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADS = (0.0, 0.05, 0.7)
MIN_LENS = (0.0, 0.3, 2.0)
BREAKS = (0.0, 0.5)


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native as N
    return N


@pytest.fixture(scope="module")
def c1_pcm():
    return synth.to_pcm16(synth.synth_audio(1001, 60.0, 16000, 1))


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


def _bytes(pcm):
    return np.frombuffer(np.ascontiguousarray(pcm).tobytes(), dtype=np.uint8)


def offline(ctx, pcm, fmt, sr, ch, frames, thr, brk):
    ctx.reset()
    fid = ctx.add_pcm(np.ascontiguousarray(pcm), fmt, sr, ch, frames)
    ctx.run(thr, brk)
    avg, idx = ctx.avg(fid)
    return ctx.regions(fid), avg, idx


def expected(native, ctx, pcm, fmt, sr, ch, frames, regions, erase):
    """(the whole-file silencer's output over E(regions), erased frames)"""
    table = native.erase_table(regions, erase["pad_s"], erase["min_len_s"])
    erased = sum(b - a for a, b in R.silence_ranges(table, sr, frames))
    return ctx.silence_pcm(np.ascontiguousarray(pcm), fmt, sr, ch, frames, table), erased


def streamed(ctx, pcm, fmt, sr, ch, pieces, step_every=1, thr=0.1, brk=0.5, erase=None, on_step=None):
    """pieces: frame counts (the rest of the recording is pushed in one last piece) -> (regions, int16 [frames, ch], info at the end).
    Checks on the way that every step continues where the last one ended and that the finished stream has returned every frame."""
    from softspoken_amd.native import _BPS
    b = _bytes(pcm)
    fb = ch * _BPS[fmt]
    total = b.size // fb
    sid = ctx.stream_open_output(fmt, sr, ch, thr, brk, erase)
    regs, out, state = [], [], dict(at=0)

    def step(pushed):
        ctx.stream_step()
        regs.extend(ctx.stream_regions(sid))
        first, a = ctx.stream_output(sid, ch)
        assert first == state["at"] and a.shape[1] == ch
        state["at"] += len(a)
        assert state["at"] <= pushed
        out.append(a)
        if on_step:
            on_step(sid, pushed, state["at"])
    at, k = 0, 0
    for n in list(pieces) + [total]:
        n = min(n, total - at)
        if n <= 0:
            break
        ctx.stream_push(sid, b[at * fb:(at + n) * fb], frames=n)
        at += n
        k += 1
        if k % step_every == 0:
            step(at)
    ctx.stream_close(sid)
    step(total)
    assert ctx.stream_info(sid)["finished"] == 1
    info = ctx.stream_output_info(sid)
    assert info["frames_out"] == total == state["at"] and info["frames_held"] == 0
    ctx.stream_free(sid)
    return regs, np.concatenate(out), info


def assert_bytes(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        raise AssertionError(f"{len(bad)} frames differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def _random_pieces(seed, total, lo=1, hi=40000):
    rng = np.random.default_rng(seed)
    out, s = [], 0
    while s < total:
        n = int(rng.integers(lo, hi))
        out.append(n)
        s += n
    return out


def _grid():
    return [dict(pad_s=p, min_len_s=m, brk=b) for p in PADS for m in MIN_LENS for b in BREAKS]


def working_threshold(native, ctx, pcm, fmt, sr, ch, frames, combos):
    """A quantile of the recording's own averages at which every combination erases some frames and keeps some: work for the kernel
    on both sides of a range.  -> (threshold, {break_s: whole-file regions})"""
    _, avg, _ = offline(ctx, pcm, fmt, sr, ch, frames, 0.1, 0.5)
    for q in (0.5, 0.4, 0.6, 0.3, 0.7, 0.2, 0.8):
        thr = float(np.nanquantile(avg, q))
        regs = {b: offline(ctx, pcm, fmt, sr, ch, frames, thr, b)[0] for b in sorted({c["brk"] for c in combos})}
        n = [sum(hi - lo for lo, hi in R.silence_ranges(native.erase_table(regs[c["brk"]], c["pad_s"], c["min_len_s"]), sr, frames)) for c in combos]
        if all(0 < e < frames for e in n):
            return thr, regs
    raise AssertionError("no quantile of the averages gives every combination something to erase and something to keep")


@pytest.fixture(scope="module")
def c1_case(native, ctxs, c1_pcm):
    made = {}

    def get(prec):
        if prec not in made:
            made[prec] = working_threshold(native, ctxs(prec), c1_pcm, native.PCM_S16, 16000, 1, len(c1_pcm), _grid())
        return made[prec]
    return get


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_c1_output_equals_the_whole_file_silencer(native, ctxs, c1_pcm, c1_case, precision):
    c = ctxs(precision)
    thr, regs = c1_case(precision)
    n = len(c1_pcm)
    splits = [
        ([1] * 400 + [997] * 2000, 1, dict(pad_s=0.05, min_len_s=0.3, brk=0.5)),     # one frame at a time first, then 997
        ([1] * 400 + [997] * 2000, 7, dict(pad_s=0.7, min_len_s=0.0, brk=0.0)),
        (_random_pieces(5, n), 1, dict(pad_s=0.0, min_len_s=0.0, brk=0.5)),
        (_random_pieces(6, n), 4, dict(pad_s=0.7, min_len_s=2.0, brk=0.5)),           # pad_s > break_s: padded regions merge
        ([16000] * 100, 1, dict(pad_s=0.05, min_len_s=2.0, brk=0.0)),
        ([16000] * 100, 4, dict(pad_s=0.0, min_len_s=0.3, brk=0.5)),
        ([], 1, dict(pad_s=0.05, min_len_s=0.0, brk=0.5)),                            # the whole file in one push
    ]
    for pieces, every, g in splits:
        erase = dict(pad_s=g["pad_s"], min_len_s=g["min_len_s"])
        want, erased = expected(native, c, c1_pcm, native.PCM_S16, 16000, 1, n, regs[g["brk"]], erase)
        assert 0 < erased < n
        r, got, info = streamed(c, c1_pcm, native.PCM_S16, 16000, 1, pieces, every, thr, g["brk"], erase)
        assert r == regs[g["brk"]]
        assert info["frames_erased"] == erased and (info["pad_s"], info["min_len_s"]) == (g["pad_s"], g["min_len_s"])
        assert_bytes(got, want)


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_c1_parameter_grid(native, ctxs, c1_pcm, c1_case, precision):
    c = ctxs(precision)
    thr, regs = c1_case(precision)
    n = len(c1_pcm)
    for k, g in enumerate(_grid()):
        erase = dict(pad_s=g["pad_s"], min_len_s=g["min_len_s"])
        want, erased = expected(native, c, c1_pcm, native.PCM_S16, 16000, 1, n, regs[g["brk"]], erase)
        assert 0 < erased < n
        pieces = [16000] * 100 if k % 2 else _random_pieces(100 + k, n, 1, 30000)
        r, got, info = streamed(c, c1_pcm, native.PCM_S16, 16000, 1, pieces, 1 + k % 3, thr, g["brk"], erase)
        assert r == regs[g["brk"]] and info["frames_erased"] == erased
        assert_bytes(got, want)


def _encode(x, fmt):
    """float interleaved x in [-1, 1] -> the bytes of the encoding"""
    if fmt == 1:
        return np.clip(np.round(x * 127 + 128), 0, 255).astype(np.uint8).reshape(-1)
    if fmt in (2, 8):
        return _bytes(np.clip(np.round(x * 32767), -32768, 32767).astype("<i2" if fmt == 2 else ">i2"))
    if fmt in (3, 9):
        v = np.clip(np.round(x * 8388607), -8388608, 8388607).astype("<i4").reshape(-1)
        b = v.view(np.uint8).reshape(-1, 4)[:, :3]
        return np.ascontiguousarray(b if fmt == 3 else b[:, ::-1]).reshape(-1)
    if fmt == 6:
        return _bytes(x.astype("<f8"))
    raise ValueError(fmt)


# S24 with 1 and 3 channels (frames of 3 and 9 bytes), U8 mono, F64 stereo, S16BE, S24BE, S16 stereo; every rate but C1's
@pytest.mark.parametrize("fmt,sr,ch,every", [(3, 8000, 1, 1), (3, 22050, 3, 2), (1, 44100, 1, 3), (6, 48000, 2, 1), (8, 22050, 1, 2),
                                             (9, 44100, 1, 1), (2, 48000, 2, 3), (3, 48000, 3, 1), (2, 8000, 2, 2)])
def test_encodings_and_alignment(native, ctxs, fmt, sr, ch, every):
    c = ctxs("f16x2")
    x = np.ascontiguousarray(synth.synth_audio(500 + sr + 10 * fmt + ch, 8.0, sr, ch).T)     # (frames, channels)
    frames = len(x)
    pcm = _encode(x, fmt)
    erase = dict(pad_s=0.05, min_len_s=0.0)
    thr, regs = working_threshold(native, c, pcm, fmt, sr, ch, frames, [dict(erase, brk=0.5)])
    want, erased = expected(native, c, pcm, fmt, sr, ch, frames, regs[0.5], erase)
    assert 0 < erased < frames
    pieces = [1] * 40 + [7] * 40 + [997] * (frames // 997 + 1)            # prime frame counts: every piece boundary at another alignment
    r, got, info = streamed(c, pcm, fmt, sr, ch, pieces, every, thr, 0.5, erase)
    assert r == regs[0.5] and info["frames_erased"] == erased
    assert_bytes(got, want)


def _bound_D(sr, brk, erase):
    """D of include/softspoken.h, with B read as tests/test_gpu_stream.py reads it."""
    hdr = open(os.path.join(ROOT, "include", "softspoken.h")).read()
    assert "B = 3 s + 2 x (3 / 256) s + half / sample_rate" in hdr
    assert "D = B + break_s + pad_s + min_len_s" in hdr
    half = 0 if sr == 22050 else math.ceil(32.0 / min(1.0, 22050.0 / sr))
    return 3.0 + 2 * 3.0 / 256 + half / sr + brk + erase["pad_s"] + erase["min_len_s"]


def test_latency_bound(native, ctxs, c1_pcm, c1_case):
    c = ctxs("fp32")
    thr, regs = c1_case("fp32")
    n = len(c1_pcm)
    for g in (dict(pad_s=0.05, min_len_s=0.3, brk=0.5), dict(pad_s=0.7, min_len_s=2.0, brk=0.0)):
        erase = dict(pad_s=g["pad_s"], min_len_s=g["min_len_s"])
        D = _bound_D(16000, g["brk"], erase)
        seen = []

        def on_step(sid, pushed, out_frames):
            held = pushed / 16000.0
            seen.append(out_frames / 16000.0 - (held - D - 0.1))
            assert out_frames / 16000.0 >= held - D - 0.1, (held, out_frames)
        want, _ = expected(native, c, c1_pcm, native.PCM_S16, 16000, 1, n, regs[g["brk"]], erase)
        _, got, _ = streamed(c, c1_pcm, native.PCM_S16, 16000, 1, [1600] * 700, 1, thr, g["brk"], erase, on_step)    # 0.1 s pieces
        assert_bytes(got, want)
        print("latency slack, seconds (min over the steps):", g, min(seen))


def test_open_region_flows_as_zeros_and_state_is_bounded(native, ctxs, c1_pcm):
    """threshold -inf: one region, open for the whole stream."""
    c = ctxs("f16x2")
    pcm = np.tile(c1_pcm, 4)                                               # 240 s
    n, piece = len(pcm), 16000
    erase = dict(pad_s=0.05, min_len_s=0.3)
    D = _bound_D(16000, 0.5, erase)
    sizes = {}

    def on_step(sid, pushed, out_frames):
        if pushed < n:
            assert out_frames / 16000.0 >= pushed / 16000.0 - D - 1.0      # it flows while the region is open
        if pushed in (60 * piece, 240 * piece) and pushed not in sizes:
            sizes[pushed] = c.stream_info(sid)["state_bytes"]
    regs, got, info = streamed(c, pcm, native.PCM_S16, 16000, 1, [piece] * 240, 1, -math.inf, 0.5, erase, on_step)
    assert len(regs) == 1
    want, erased = expected(native, c, pcm, native.PCM_S16, 16000, 1, n, regs, erase)
    assert erased > n // 2 and info["frames_erased"] == erased
    assert_bytes(got, want)
    assert not got[16000:-16000].any()
    assert abs(sizes[240 * piece] - sizes[60 * piece]) <= piece * 2 + 4096, sizes


def test_no_regions_is_the_plain_transcode(native, ctxs, c1_pcm):
    c = ctxs("f16x2")
    pcm = c1_pcm[:8 * 16000]
    regs, got, info = streamed(c, pcm, native.PCM_S16, 16000, 1, _random_pieces(9, len(pcm), 1, 9000), 2, math.inf, 0.5, dict(pad_s=0.7, min_len_s=0.0))
    assert regs == [] and info["frames_erased"] == 0
    assert_bytes(got, c.silence_pcm(pcm, native.PCM_S16, 16000, 1, len(pcm), []))


def test_16_staggered_streams_with_and_without_output(native, blob):
    c = native.Context(blob, 0, precision="f16x2", chunk=16)
    ref = native.Context(blob, 0, precision="f16x2")
    kinds = [(2, 16000, 1), (3, 48000, 3), (1, 8000, 1), (6, 44100, 2), (8, 22050, 1), (2, 48000, 2), (9, 16000, 1), (3, 22050, 1)]
    recs = []
    for k in range(16):
        fmt, sr, ch = kinds[k % 8]
        x = np.ascontiguousarray(synth.synth_audio(7000 + k, 5.0 + (k % 5), sr, ch).T)
        pcm, frames = _encode(x, fmt), len(x)
        with_out = (k < 8) == (k % 2 == 0)                   # half and half; every kind once with output and once without
        erase = dict(pad_s=(0.0, 0.05, 0.7)[k % 3], min_len_s=(0.0, 0.3)[k % 2])
        thr, regs = working_threshold(native, ref, pcm, fmt, sr, ch, frames, [dict(erase, brk=0.5)])
        recs.append(dict(fmt=fmt, sr=sr, ch=ch, pcm=pcm, frames=frames, fb=ch * native._BPS[fmt], out=with_out, erase=erase, thr=thr,
                         want=offline(ref, pcm, fmt, sr, ch, frames, thr, 0.5)))
    rng = np.random.default_rng(11)
    state = {}
    for rnd in range(300):
        for k, r in enumerate(recs):
            if k not in state and rnd >= k % 8:
                sid = (c.stream_open_output(r["fmt"], r["sr"], r["ch"], r["thr"], 0.5, r["erase"]) if r["out"]
                       else c.stream_open(r["fmt"], r["sr"], r["ch"], r["thr"], 0.5))
                state[k] = dict(sid=sid, at=0, r=[], a=[], i=[], o=[], oat=0, done=False)
            st = state.get(k)
            if st is None or st["done"]:
                continue
            if st["at"] < r["frames"]:
                n = min(int(rng.integers(r["sr"] // 10, r["sr"])), r["frames"] - st["at"])
                c.stream_push(st["sid"], r["pcm"][st["at"] * r["fb"]:(st["at"] + n) * r["fb"]], frames=n)
                st["at"] += n
            elif not c.stream_info(st["sid"])["closed"]:
                c.stream_close(st["sid"])
        c.stream_step()
        for k, st in state.items():
            if st["done"]:
                continue
            r = recs[k]
            st["r"] += c.stream_regions(st["sid"])
            a, i = c.stream_avg(st["sid"])
            st["a"].append(a); st["i"].append(i)
            if r["out"]:
                first, o = c.stream_output(st["sid"], r["ch"])
                assert first == st["oat"]
                st["oat"] += len(o); st["o"].append(o)
            else:
                with pytest.raises(native.NativeError) as e:
                    c.stream_output(st["sid"], r["ch"])
                assert e.value.code == native.SS_ERR_STATE
            if c.stream_info(st["sid"])["finished"]:
                st["done"] = True
        if len(state) == 16 and all(st["done"] for st in state.values()):
            break
    for k, r in enumerate(recs):
        st = state[k]
        assert st["done"]
        regs, avg, idx = r["want"]
        assert st["r"] == regs                               # every stream, with output or without: the whole-file table and averages
        assert np.array_equal(np.concatenate(st["i"]), idx)
        assert np.array_equal(np.concatenate(st["a"]).view(np.int64), avg.view(np.int64))
        if r["out"]:
            want, erased = expected(native, ref, r["pcm"], r["fmt"], r["sr"], r["ch"], r["frames"], regs, r["erase"])
            assert 0 < erased < r["frames"]
            assert_bytes(np.concatenate(st["o"]), want)
    c.close(); ref.close()


@pytest.mark.parametrize("route", [("f16x2", "f16x2"), ("f16x2", "fp32", "f16x2")])
def test_export_import(native, ctxs, c1_pcm, c1_case, route):
    thr, regs_f16 = c1_case("f16x2")
    erase = dict(pad_s=0.7, min_len_s=0.3)
    cs = [ctxs(p, key=1 + k) for k, p in enumerate(route)]
    c = cs[0]
    sid = c.stream_open_output(native.PCM_S16, 16000, 1, thr, 0.5, erase)
    regs, out, at = [], [], 0
    hop = [20, 40] if len(route) == 3 else [30]
    for k in range(60):
        if hop and k == hop[0]:
            hop.pop(0)
            nxt = cs[cs.index(c) + 1]
            image = c.stream_export(sid)
            assert image[:8] == b"SSSTRM03"
            held = c.stream_output_info(sid)
            c.stream_push(sid, c1_pcm[:5])                   # the source is left alone by the export
            c.stream_free(sid)
            sid, c = nxt.stream_import(image), nxt
            assert c.stream_output_info(sid) == held
            assert c.stream_export(sid) == image             # an image read back before any step is the same image
        c.stream_push(sid, c1_pcm[k * 16000:(k + 1) * 16000])
        if k % 2:
            c.stream_step()
            regs += c.stream_regions(sid)
            first, a = c.stream_output(sid, 1)
            assert first == at
            at += len(a); out.append(a)
    c.stream_close(sid)
    c.stream_step()
    regs += c.stream_regions(sid)
    first, a = c.stream_output(sid, 1)
    assert first == at and at + len(a) == len(c1_pcm)
    out.append(a)
    c.stream_free(sid)
    if len(route) == 2:
        assert regs == regs_f16[0.5]
    want, erased = expected(native, c, c1_pcm, native.PCM_S16, 16000, 1, len(c1_pcm), regs, erase)     # the regions THIS stream returned
    assert 0 < erased < len(c1_pcm)
    assert_bytes(np.concatenate(out), want)


def test_plain_streams_write_the_images_they_wrote(native, ctxs, c1_pcm):
    c = ctxs("f16x2")
    sid = c.stream_open(native.PCM_S16, 16000, 1, 0.1, 0.5)
    c.stream_push(sid, c1_pcm[:80000])
    c.stream_step()
    assert c.stream_export(sid)[:8] == b"SSSTRM01"
    with pytest.raises(native.NativeError) as e:
        c.stream_output_info(sid)
    assert e.value.code == native.SS_ERR_STATE
    c.stream_free(sid)


def test_output_arguments_and_broken_images(native, ctxs, c1_pcm):
    import ctypes as C
    c = ctxs("f16x2")
    for bad in (dict(pad_s=-0.1), dict(min_len_s=float("nan")), dict(pad_s=float("inf"))):
        with pytest.raises(native.NativeError) as e:
            c.stream_open_output(native.PCM_S16, 16000, 1, 0.1, 0.5, bad)
        assert e.value.code == native.SS_ERR_ARG
    sid = c.stream_open_output(native.PCM_S16, 16000, 1, math.inf, 0.5, None)          # NULL: 0, 0
    assert (c.stream_output_info(sid)["pad_s"], c.stream_output_info(sid)["min_len_s"]) == (0.0, 0.0)
    assert c.stream_output(sid, 1)[1].shape == (0, 1)                                 # before any step: nothing, at frame 0
    c.stream_push(sid, c1_pcm[:6 * 16000])
    c.stream_step()
    first, a = c.stream_output(sid, 1)
    assert first == 0 and 0 < len(a) < 6 * 16000
    f, n = C.c_int64(0), C.c_int64(0)
    small = np.zeros(len(a) - 1, dtype=np.int16)
    assert native.lib().ss_stream_output(c._h, sid, native._ptr(small), len(small), C.byref(f), C.byref(n)) == native.SS_ERR_CAPACITY
    assert n.value == len(a)
    image = c.stream_export(sid)
    c.stream_free(sid)
    frames_out_at = 8 + 8 * 4 + 4 * 8 + 14 * 8 + 8 + 16                                # magic, ints, doubles, counters, step, erase: frames_out
    broken = bytearray(image); broken[frames_out_at:frames_out_at + 8] = (10 ** 9).to_bytes(8, "little")
    for img in (image[:-1], image + b"\0", bytes(broken), image[:200]):
        with pytest.raises(native.NativeError) as e:
            c.stream_import(img)
        assert e.value.code == native.SS_ERR_FORMAT
    c.stream_free(c.stream_import(image))


def test_a_refused_step_advances_no_output(native, blob, caplog):
    from softspoken_amd.stream import StreamDetector
    x = synth.synth_audio(4242, 20.0, 16000, 1)[0].astype(np.float32)
    x[16000 * 7 + 123] = np.nan
    erase = dict(pad_s=0.05, min_len_s=0.3)
    fp = native.Context(blob, 0, precision="fp32")
    thr = float(np.nanquantile(offline(fp, x, native.PCM_F32, 16000, 1, len(x), 0.1, 0.5)[1], 0.5))
    # on the context itself: the refused step leaves the output where it was, its last frames still readable
    c = native.Context(blob, 0, precision="f16x2")
    sid = c.stream_open_output(native.PCM_F32, 16000, 1, thr, 0.5, erase)
    c.stream_push(sid, x[:16000 * 6])
    c.stream_step()
    before, last = c.stream_output_info(sid), c.stream_output(sid, 1)
    assert before["frames_out"] > 0
    c.stream_push(sid, x[16000 * 6:16000 * 12])
    with pytest.raises(native.NativeError) as e:
        c.stream_step()
    assert e.value.code == native.SS_ERR_RANGE
    after = c.stream_output_info(sid)
    assert after["frames_out"] == before["frames_out"] and after["frames_erased"] == before["frames_erased"]
    assert after["frames_held"] == before["frames_held"] + 16000 * 6
    again = c.stream_output(sid, 1)
    assert again[0] == last[0] and np.array_equal(again[1], last[1])
    c.close()
    # through the detector: the stream finishes in fp32, and its output is the silencer's over the regions it returned
    det = StreamDetector(blob, precision="f16x2")
    s = det.open(native.PCM_F32, 16000, 1, thr, 0.5, erase=erase)
    regs, out, at = [], [], 0
    with caplog.at_level(logging.WARNING):
        for k in list(range(0, len(x), 8000)) + [None]:
            if k is None:
                s.close()
            else:
                s.push(x[k:k + 8000])
            regs += det.step()[s][0]
            first, a = s.output()
            assert first == at
            at += len(a); out.append(a)
    assert s.precision == "fp32" and at == len(x)
    assert s.output_info()["pad_s"] == 0.05 and s.output_info()["min_len_s"] == 0.3
    want, erased = expected(native, fp, x, native.PCM_F32, 16000, 1, len(x), regs, erase)
    assert 0 < erased < len(x)
    assert_bytes(np.concatenate(out), want)
    det.close(); fp.close()


def test_stream_wav_writer(native, ctxs, c1_pcm, tmp_path):
    from softspoken_amd.stream import StreamDetector, StreamWavWriter
    pcm = np.ascontiguousarray(np.stack([c1_pcm[:20 * 16000], c1_pcm[20 * 16000:40 * 16000]], axis=1))          # stereo
    erase = dict(pad_s=0.05, min_len_s=0.3)
    thr, _ = working_threshold(native, ctxs("f16x2"), pcm, native.PCM_S16, 16000, 2, len(pcm), [dict(erase, brk=0.5)])
    det = StreamDetector(context_factory=lambda p: ctxs(p, key=5))
    s = det.open(native.PCM_S16, 16000, 2, thr, 0.5, erase=erase)
    got = []
    path = tmp_path / "feed.wav"
    with StreamWavWriter(path, 16000, 2) as w:
        for k in list(range(0, len(pcm), 12345)) + [None]:
            if k is None:
                s.close()
            else:
                s.push(pcm[k:k + 12345])
            got += det.step()[s][0]
            w.write(s.output())
    det.free(s)
    want, erased = expected(native, ctxs("f16x2"), pcm, native.PCM_S16, 16000, 2, len(pcm), got, erase)
    assert 0 < erased < len(pcm)
    assert path.read_bytes() == native.wav_header_pcm16(16000, 2, len(pcm)) + want.astype("<i2").tobytes()
