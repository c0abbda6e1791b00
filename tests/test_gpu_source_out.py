"""Source output on a real MI355X (include/softspoken.h "source output"): ss_silence_pcm_source's bytes equal to
the reference of tests/source_out_ref.py for every encoding; ss_separate_pcm_source and ss_separate_pcm_channels_source equal to the
input's bytes outside the merged intervals and, inside them, held to the float64 reference of tests/separation_ref.py:

    |got - y64 u| <= r + 4 e32 u,   u = S / 32767,   r = max(0.5, 0.5 ulp_float32(y) S)      (integer formats, in codes)
    |got - y64 / 32767| <= 0.5 ulp_float32(y) + 4 e32 / 32767                                (F32 / F64, unit scale)

e32 being the case's max |separate_f32 - y64| (LSB of the 16-bit path), computed here on the CPU; the device's own error never sets the
tolerance (source_out_ref.separation_bound; tests/test_source_out_host.py shows the reference itself inside it)."""
import numpy as np
import pytest

import separation_ref as R
import source_out_cases as K
import source_out_ref as S
import test_gpu_separation as T

pytestmark = pytest.mark.gpu

ALL_FORMATS = sorted(K.FMT.items(), key=lambda kv: kv[1])


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


@pytest.fixture(scope="module")
def audio(native):
    c = native.Context(None, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def heads(sd_np):
    return dict(spread=R.spread_head(sd_np))


@pytest.fixture(scope="module")
def ctx_spread(native, heads):
    c = T._head_ctx(native, heads["spread"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_gain0(native, sd_np):
    c = native.Context(T._crafted_blob(sd_np, 4.0), 0, precision="fp32")
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_gain1(native, sd_np):
    c = native.Context(T._crafted_blob(sd_np, -1.0), 0, precision="fp32")
    yield c
    c.close()


def _random_bytes(fmt, ch, frames, seed):
    """Any bytes are a recording of an integer format; the float formats get finite values, so that no test depends on NaN payloads
    by accident (test_float_specials does on purpose)."""
    rng = np.random.default_rng(seed)
    n = frames * ch
    if fmt in S.BITS:
        return rng.integers(0, 256, size=n * S.BPS[fmt], dtype=np.uint8)
    return S.encode(rng.uniform(-1.5, 1.5, size=n).astype(np.float32), fmt)


# ---- zeroing: bytes equal to the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fmt", ALL_FORMATS)
def test_zeroing_equals_the_reference(audio, name, fmt):
    sr = 8000
    for ch in (1, 2, 3):
        for frames in (0, 1, 5, 1001):
            data = _random_bytes(fmt, ch, frames, 100 * fmt + 10 * ch + frames % 7)
            for regions in (T.REGIONS, [], [(0.0, 1.0)]):
                got = audio.silence_pcm_source(data, fmt, sr, ch, frames, regions)
                want = S.silence_source(data, fmt, sr, ch, frames, regions)
                assert got.dtype == np.uint8 and got.shape == (frames, ch * S.BPS[fmt])
                assert np.array_equal(got, want), (name, ch, frames, len(regions))
            if frames:
                assert np.array_equal(audio.silence_pcm_source(data, fmt, sr, ch, frames, []).reshape(-1), data)
    assert (1001 * 9) % 16 != 0


@pytest.mark.parametrize("fmt,ch", [(3, 3), (1, 1)])
def test_range_edges_inside_one_word(audio, fmt, ch):
    """Frame ranges that begin and end inside the same 16-byte word (and in neighbouring words), at every phase of the word."""
    sr, frames = 8000, 400
    fb = ch * S.BPS[fmt]
    data = _random_bytes(fmt, ch, frames, 9)
    for first in range(0, 40):
        regions = [(first / sr, (first + 1) / sr), ((first + 50) / sr, (first + 50 + (16 // fb) + 1) / sr),
                   ((first + 100) / sr, (first + 101) / sr), ((first + 102) / sr, (first + 103) / sr)]
        iv = R.merged_intervals(regions, sr, frames)
        assert len(iv) == 4 and iv[0] == (first, first + 1)
        got = audio.silence_pcm_source(data, fmt, sr, ch, frames, regions)
        assert np.array_equal(got, S.silence_source(data, fmt, sr, ch, frames, regions)), first


def test_float_specials_pass_bit_for_bit(audio):
    sr, ch = 8000, 2
    bits = np.array([0x7FC12345, 0xFFA00001, 0x80000000, 0x3FA66666, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000], dtype=np.uint32)
    words = np.tile(bits, 50)
    frames = words.size // ch
    regions = [(0.01, 0.02)]
    for fmt, data in ((5, words.astype("<u4").view(np.uint8)), (11, words.astype(">u4").view(np.uint8))):
        got = audio.silence_pcm_source(data, fmt, sr, ch, frames, regions)
        m = S.frame_mask(frames, sr, regions)
        assert m.sum() == 80 and np.array_equal(got[~m], data.reshape(frames, -1)[~m]) and not got[m].any()
    d64 = np.tile(np.array([0x7FF8000000012345, 0x8000000000000000, 0x0000000000000001, 0x7FF0000000000000], dtype=np.uint64), 100)
    got = audio.silence_pcm_source(d64.view(np.uint8), 6, sr, ch, d64.size // ch, regions)
    assert np.array_equal(got, S.silence_source(d64.view(np.uint8), 6, sr, ch, d64.size // ch, regions))


def test_zeroing_refusals(native, audio):
    data = _random_bytes(2, 2, 100, 1)
    out = np.empty(399, dtype=np.uint8)
    rc = native.lib().ss_silence_pcm_source(audio._h, native._ptr(data), 2, 8000, 2, 100, native._regions([]), 0, native._ptr(out), out.nbytes)
    assert rc == native.SS_ERR_CAPACITY
    rc = native.lib().ss_silence_pcm_source(audio._h, native._ptr(data), 13, 8000, 2, 100, native._regions([]), 0, native._ptr(out), 400)
    assert rc == native.SS_ERR_ARG


# ---- separation ----------------------------------------------------------------------------------------------------------------
def _maps(native, ctx, data, fmt, sr, ch, frames, regions, each=False, **params):
    plan = native.separation_plan(sr, frames, regions, **params)
    wins = sorted({i for r in plan["ranges"] for i in range(r["win_first"], r["win_last"] + 1)})
    ctx.reset()
    idx = np.array(wins, dtype=np.int64) * 13230
    if each:
        first = ctx.add_pcm_channels(data, fmt, sr, ch, frames)
        out = []
        for c in range(ch):
            spec, _ = ctx.infer_windows(first + c, idx, want_spec=True)
            out.append({w: spec[t] for t, w in enumerate(wins)})
        return plan, out
    fid = ctx.add_pcm(data, fmt, sr, ch, frames)
    spec, _ = ctx.infer_windows(fid, idx, want_spec=True)
    return plan, {w: spec[t] for t, w in enumerate(wins)}


def _bound_case(native, ctx, label, rec, sr, regions, **params):
    data, fmt, x = rec
    frames, ch = x.shape
    plan, by_win = _maps(native, ctx, data, fmt, sr, ch, frames, regions, **params)
    _, y64 = R.separate(x, sr, regions, by_win, unrounded=True, **params)
    e32 = float(np.abs(R.separate_f32(x, sr, regions, by_win, **params).astype(np.float64) - y64).max())
    got = ctx.separate_pcm_source(data, fmt, sr, ch, frames, regions, **params)
    assert got.dtype == np.uint8 and got.shape == (frames, ch * S.BPS[fmt])
    m = S.frame_mask(frames, sr, regions)
    K.check_bound(label, got, data, fmt, ch, m, y64, e32, plan["n_fft"])
    assert not np.array_equal(got[m], data.reshape(frames, -1)[m])            # the spread head's gains move the audio
    return got


@pytest.mark.parametrize("name,sr,ch", K.SEP_CASES)
def test_separation_bound(native, ctx_spread, name, sr, ch):
    _bound_case(native, ctx_spread, f"{name}/{sr}/{ch}", K.rec(name, sr, ch), sr, T.B1_REGIONS)


def test_separation_bound_f16x2_context(native, heads):
    name, sr, ch = K.F16_CASE
    ctx = T._head_ctx(native, heads["spread"], "f16x2")
    try:
        _bound_case(native, ctx, f"{name}/{sr}/{ch} f16x2", K.rec(name, sr, ch), sr, T.B1_REGIONS)
    finally:
        ctx.close()


@pytest.mark.parametrize("name,sr,ch", K.LINK_CASES)
def test_float_sources_link_exactly_to_the_16_bit_path(ctx_spread, name, sr, ch):
    """Both paths encode the same float32 y: rint(float32(got) x 32767) in float32 is separate_pcm's sample, mix and each-channel."""
    data, fmt, x = K.rec(name, sr, ch)
    frames = len(x)
    for src_fn, pcm_fn in ((ctx_spread.separate_pcm_source, ctx_spread.separate_pcm),
                           (ctx_spread.separate_pcm_channels_source, ctx_spread.separate_pcm_channels)):
        got = S.decode(src_fn(data, fmt, sr, ch, frames, T.B1_REGIONS).reshape(-1), fmt).reshape(frames, ch)
        want = pcm_fn(data, fmt, sr, ch, frames, T.B1_REGIONS)
        q = np.rint(got.astype(np.float32) * np.float32(32767.0)).astype(np.int64)
        assert np.abs(q).max() < 32768 and np.array_equal(q, want.astype(np.int64))


def test_saturation_in_place_of_the_wrap(native, ctx_spread):
    """A full-scale pcm16 recording with min_gain = 1 (every gain 1: the output is the input up to the resynthesis' rounding): inside
    the bound of its own case.  A wrapped sample would miss by 65 535."""
    sr, ch = 16000, 2
    rng = np.random.default_rng(3)
    x = np.where(rng.random((int(2.5 * sr), ch)) < 0.5, -1.0, 32767.0 / 32768.0).astype(np.float32)
    x[::7] = (0.9 * rng.standard_normal((len(x[::7]), ch))).clip(-1.0, 32767.0 / 32768.0).astype(np.float32)
    rec = K.pack(x, "pcm16", sr)
    data, fmt, dec = rec
    assert (S.codes(data, fmt) == 32767).mean() > 0.3 and (S.codes(data, fmt) == -32768).mean() > 0.3
    plan, by_win = _maps(native, ctx_spread, data, fmt, sr, ch, len(dec), T.B1_REGIONS, min_gain=1.0)
    _, y64 = R.separate(dec, sr, T.B1_REGIONS, by_win, unrounded=True, min_gain=1.0)
    e32 = float(np.abs(R.separate_f32(dec, sr, T.B1_REGIONS, by_win, min_gain=1.0).astype(np.float64) - y64).max())
    got = ctx_spread.separate_pcm_source(data, fmt, sr, ch, len(dec), T.B1_REGIONS, min_gain=1.0)
    m = S.frame_mask(len(dec), sr, T.B1_REGIONS)
    K.check_bound("saturation pcm16 full scale", got, data, fmt, ch, m, y64, e32, plan["n_fft"])
    _, tol = S.separation_bound(y64[m], e32, fmt)
    d = np.abs(S.codes(got.reshape(-1), fmt) - S.codes(data, fmt)).reshape(len(dec), ch)[m]
    print(f"SRCBOUND saturation: largest |out - source| = {int(d.max())} codes, bound {float(tol.max()):.4f}")
    assert d.max() <= float(tol.max()) + 1e-6                   # every gain 1: y64 u is the source's code; a wrap would miss by 65 535
    # the same recording under the spread head's own gains: the filtered full-scale signal overshoots the codes by thousands of samples
    # (CPU oracle: 2400 of them), and every one of them must sit on the rail it left through
    plan, by_win = _maps(native, ctx_spread, data, fmt, sr, ch, len(dec), T.B1_REGIONS)
    _, y64 = R.separate(dec, sr, T.B1_REGIONS, by_win, unrounded=True)
    e32 = float(np.abs(R.separate_f32(dec, sr, T.B1_REGIONS, by_win).astype(np.float64) - y64).max())
    got = ctx_spread.separate_pcm_source(data, fmt, sr, ch, len(dec), T.B1_REGIONS)
    K.check_bound("saturation pcm16 overshoot", got, data, fmt, ch, m, y64, e32, plan["n_fft"])
    q = y64[m] / 32767.0 * 32768.0
    codes = S.codes(np.ascontiguousarray(got[m]).reshape(-1), fmt).reshape(-1, ch)
    hi, lo = q > 32768.0, q < -32769.0
    print(f"SRCBOUND saturation: {int(hi.sum())} samples above the top code, {int(lo.sum())} below the bottom one")
    assert hi.sum() > 100 and lo.sum() > 100 and (codes[hi] == 32767).all() and (codes[lo] == -32768).all()


@pytest.mark.parametrize("name,sr,ch", [("pcm16", 48000, 2), ("u8", 8000, 1), ("pcm24", 96000, 3), ("s24be", 22050, 2), ("f32", 16000, 1)])
def test_gain_zero_is_the_zeroing_silencer(ctx_gain0, name, sr, ch):
    data, fmt, x = K.rec(name, sr, ch, seconds=2.0, seed=12, scale=1.6)
    got = ctx_gain0.separate_pcm_source(data, fmt, sr, ch, len(x), T.REGIONS, fade_s=0.0, min_gain=0.0, above_fmax="mute")
    want = ctx_gain0.silence_pcm_source(data, fmt, sr, ch, len(x), T.REGIONS)
    assert np.array_equal(want, S.silence_source(data, fmt, sr, ch, len(x), T.REGIONS))
    assert np.array_equal(got, want)                                 # (x + (0 - x) is +0.0: the float formats' zero bytes too)


@pytest.mark.parametrize("name,sr,ch", [("pcm16", 48000, 2), ("pcm24", 192000, 2)])
def test_gain_one_returns_the_source_within_one_code(ctx_gain1, name, sr, ch):
    """Every gain 1 (above_fmax keep): the resynthesis is the input up to float32 rounding, which an encode at the decode's own scale
    turns back into the source's codes -- within one code, where the 16-bit path moves half of all codes."""
    data, fmt, x = K.rec(name, sr, ch, seconds=1.5, seed=13, scale=0.5)
    got = ctx_gain1.separate_pcm_source(data, fmt, sr, ch, len(x), T.REGIONS, above_fmax="keep")
    d = np.abs(S.codes(got.reshape(-1), fmt) - S.codes(data, fmt))
    assert d.max() <= 1


def test_each_channel_bound_and_the_one_channel_form(native, ctx_spread):
    name, sr, ch = K.F16_CASE
    data, fmt, x = K.rec(name, sr, ch)
    frames = len(x)
    plan, by_win = _maps(native, ctx_spread, data, fmt, sr, ch, frames, T.B1_REGIONS, each=True)
    got = ctx_spread.separate_pcm_channels_source(data, fmt, sr, ch, frames, T.B1_REGIONS)
    m = S.frame_mask(frames, sr, T.B1_REGIONS)
    bps = S.BPS[fmt]
    for c in range(ch):
        xc = x[:, c:c + 1]
        _, y64 = R.separate(xc, sr, T.B1_REGIONS, by_win[c], unrounded=True)
        e32 = float(np.abs(R.separate_f32(xc, sr, T.B1_REGIONS, by_win[c]).astype(np.float64) - y64).max())
        src_c = np.ascontiguousarray(data.reshape(frames, ch, bps)[:, c]).reshape(-1)
        K.check_bound(f"each {name}/{sr} channel {c}", np.ascontiguousarray(got.reshape(frames, ch, bps)[:, c]), src_c, fmt, 1, m, y64, e32,
                      plan["n_fft"])
    mix = ctx_spread.separate_pcm_source(data, fmt, sr, ch, frames, T.B1_REGIONS)
    assert not np.array_equal(mix, got)
    mono = K.rec("pcm24", 44100, 1)
    a = ctx_spread.separate_pcm_channels_source(mono[0], mono[1], 44100, 1, len(mono[2]), T.B1_REGIONS)
    b = ctx_spread.separate_pcm_source(mono[0], mono[1], 44100, 1, len(mono[2]), T.B1_REGIONS)
    assert a.tobytes() == b.tobytes()


def test_two_calls_identical_reset_counting_and_refusals(native, ctx_spread):
    data, fmt, x = K.rec("pcm24", 44100, 1)
    args = (data, fmt, 44100, 1, len(x), [(0.5, 1.0), (1.5, 1.7)])
    for fn in (ctx_spread.separate_pcm_source, ctx_spread.separate_pcm_channels_source):
        g0 = ctx_spread.reset_generation()
        a = fn(*args, fade_s=0.02, min_gain=0.1)
        b = fn(*args, fade_s=0.02, min_gain=0.1)
        assert a.tobytes() == b.tobytes() and ctx_spread.reset_generation() == g0 + 2
        with pytest.raises(native.NativeError) as e:
            fn(*args, min_gain=2.0)
        assert e.value.code == native.SS_ERR_ARG
    z = ctx_spread.silence_pcm_source(*args)
    assert z.tobytes() == ctx_spread.silence_pcm_source(*args).tobytes()
    audio = native.Context(None, 0)
    try:
        for fn in (audio.separate_pcm_source, audio.separate_pcm_channels_source):
            with pytest.raises(native.NativeError) as e:
                fn(*args)
            assert e.value.code == native.SS_ERR_STATE                # audio-only
    finally:
        audio.close()
    out = np.empty(data.size - 1, dtype=np.uint8)
    p = native.separation_params(0.01, 0.0, "mute", 1)
    import ctypes as C
    rc = native.lib().ss_separate_pcm_source(ctx_spread._h, native._ptr(data), fmt, 44100, 1, len(x), native._regions(args[5]), 2, C.byref(p),
                                             native._ptr(out), out.nbytes)
    assert rc == native.SS_ERR_CAPACITY


def test_silence_job_source_on_the_device(tmp_path, native, audio):
    """The headless job end to end with the real context: a 24-bit WAV with a LIST chunk, and an AIFF."""
    import pandas as pd
    import struct
    from softspoken_amd import silence, synth
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    out.mkdir()
    data, fmt, x = K.rec("pcm24", 44100, 1, seconds=1.0)
    hdr = native.wav_header(fmt, 44100, 1, len(x))
    lst = b"LIST" + struct.pack("<I", 12) + b"INFOICMT" + struct.pack("<I", 0)
    body = hdr[12:36] + lst + hdr[36:44] + data.tobytes() + b"\x00" * (data.size & 1) + b"bext" + struct.pack("<I", 4) + b"\x01\x02\x03\x04"
    wav = b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WAVE" + body
    (src / "a.wav").write_bytes(wav)
    aif = synth.aiff_bytes(S.codes(K.rec("pcm16", 16000, 3)[0], 2).reshape(-1, 3), 16000, 16)
    (src / "b.aiff").write_bytes(aif)
    df = pd.DataFrame({"ID": [1, 2], "file_path": [str(src)] * 2, "file_name": ["a.wav", "b.aiff"], "start_time": [0.2, 0.5],
                       "end_time": [0.4, 0.9], "erase": [1, 1]})
    job = silence.SilenceJob(df, str(out), ctx=audio, encoding="source")
    paths = job.run()
    assert not job.errors and sorted(p.name for p in out.iterdir()) == ["a_silenced.wav", "b_silenced.aiff"] and len(paths) == 2
    for name, image, reg in (("a_silenced.wav", wav, (0.2, 0.4)), ("b_silenced.aiff", aif, (0.5, 0.9))):
        got = (out / name).read_bytes()
        info = native.wav_parse(image)
        fb = info.channels * info.bits // 8
        a, b = info.data_offset, info.data_offset + info.frames * fb
        want = S.silence_source(np.frombuffer(image, dtype=np.uint8)[a:b], info.format, info.sample_rate, info.channels, info.frames, [reg])
        assert got == image[:a] + want.tobytes() + image[b:]
        assert got != image
