"""Source output (include/softspoken.h "source output") without a GPU: the reference's encode, ss_wav_header,
SilenceJob's "source" encoding with a fake context, the setting, the exports, and the separation bound applied to the reference itself
on the GPU test's cases (the spec maps from the fp32 CPU oracle)."""
import os
import struct

import numpy as np
import pandas as pd
import pytest

import separation_ref as R
import source_out_cases as K
import source_out_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


# ---- the reference's encode ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [1, 2, 3, 7, 8, 9])
def test_decode_encode_is_the_identity_on_every_code(fmt):
    bits = S.BITS[fmt]
    k = np.arange(-(1 << (bits - 1)), 1 << (bits - 1), dtype=np.int64)
    stored = k + 128 if fmt == 1 else k
    le = np.stack([(stored >> (8 * i)) & 255 for i in range(bits // 8)], axis=1).astype(np.uint8)
    data = np.ascontiguousarray(le[:, ::-1] if fmt in S.BIG_ENDIAN else le).reshape(-1)
    assert np.array_equal(S.codes(data, fmt), k)
    x = S.decode(data, fmt)
    back = S.encode(x, fmt)
    assert np.array_equal(back, data)
    assert np.array_equal(S.decode(back, fmt), x)


@pytest.mark.parametrize("fmt", sorted(S.BITS))
def test_encode_saturates_and_a_nan_gives_zero(fmt):
    bits = S.BITS[fmt]
    top, low = (1 << (bits - 1)) - 1, -(1 << (bits - 1))
    y = np.array([1.0, -1.0, 1.3, -1.3, np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    assert S.codes(S.encode(y, fmt), fmt).tolist() == [top, low, top, low, 0, top, low, 0, 0]
    assert S.encode(np.zeros(3, np.float32), fmt).tolist() == [S.ZERO_BYTE[fmt]] * (3 * S.BPS[fmt])


def test_encode_rounds_the_float32_product_to_nearest_even():
    y = np.array([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768], dtype=np.float32)
    assert S.codes(S.encode(y, 2), 2).tolist() == [0, 2, 2, 0, -2]


def test_float_formats_keep_the_value():
    y = np.array([1.3, -0.0, 1e-40, np.inf, 0.1], dtype=np.float32)
    for fmt in (5, 6, 11, 12):
        assert S.decode(S.encode(y, fmt), fmt).tobytes() == y.tobytes()
    assert S.encode(y, 11).reshape(-1, 4)[:, ::-1].tobytes() == S.encode(y, 5).tobytes()
    assert S.encode(y, 6).view("<f8").tolist() == y.astype(np.float64).tolist()


# ---- ss_wav_header -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("ch", [1, 2, 5])
def test_wav_header_round_trips_through_both_parsers(native, fmt, ch):
    from oracle import oracle_np as O
    sr, frames = 44100, 37
    hdr = native.wav_header(fmt, sr, ch, frames)
    assert len(hdr) == 44
    img = hdr + bytes(frames * ch * S.BPS[fmt])
    info = native.wav_parse(img)
    assert (info.format, info.sample_rate, info.channels, info.frames, info.data_offset, info.data_bytes) == \
        (fmt, sr, ch, frames, 44, frames * ch * S.BPS[fmt])
    assert struct.unpack("<H", hdr[20:22])[0] == (3 if fmt >= 5 else 1)
    o = O.parse_wav(img)
    assert o == dict(fmt_tag=3 if fmt >= 5 else 1, channels=ch, sr=sr, bits=8 * S.BPS[fmt], data_off=44,
                     data_len=frames * ch * S.BPS[fmt], frames=frames)


def test_wav_header_is_the_pcm16_header_for_s16_and_refuses_the_rest(native):
    for sr, ch, frames in ((8000, 1, 0), (48000, 2, 123457), (96000, 5, 9)):
        assert native.wav_header(2, sr, ch, frames) == native.wav_header_pcm16(sr, ch, frames)
    for fmt in range(7, 13):
        with pytest.raises(native.NativeError) as e:
            native.wav_header(fmt, 48000, 2, 10)
        assert e.value.code == native.SS_ERR_ARG
    for fmt, ch, frames in ((2, 2, 1 << 30), (5, 1, 1 << 30), (6, 1, 1 << 29), (1, 1, 1 << 32), (3, 2, 715827883)):
        assert frames * ch * S.BPS[fmt] >= (1 << 32)
        with pytest.raises(native.NativeError) as e:
            native.wav_header(fmt, 48000, ch, frames)
        assert e.value.code == native.SS_ERR_ARG
    assert len(native.wav_header(5, 48000, 1, (1 << 30) - 16)) == 44
    with pytest.raises(native.NativeError):
        native.wav_header(0, 48000, 1, 10)


# ---- exports -------------------------------------------------------------------------------------------------------------------
def test_the_exports_are_declared_and_bound(native):
    hdr = open(os.path.join(ROOT, "include", "softspoken.h")).read()
    for name in ("ss_silence_pcm_source", "ss_separate_pcm_source", "ss_separate_pcm_channels_source", "ss_wav_header"):
        assert name in native.EXPORTS and name + "(" in hdr and getattr(native.lib(), name) is not None
    assert native.lib().ss_abi_version() == 3 == native.ABI_VERSION
    for name in ("silence_pcm_source", "separate_pcm_source", "separate_pcm_channels_source"):
        assert callable(getattr(native.Context, name))


# ---- SilenceJob ----------------------------------------------------------------------------------------------------------------
class _Ctx:
    """Every entry point answers with a recognisable fill; the *_source ones in bytes."""
    def __init__(self, log):
        self.log = log

    def _out16(self, name, channels, frames):
        self.log.append(name)
        return np.full((frames, channels), 0x0101 * len(self.log), dtype=np.int16)

    def _out8(self, name, fmt, channels, frames):
        self.log.append(name)
        return np.full((frames, channels * S.BPS[fmt]), 0xA0 + len(self.log), dtype=np.uint8)

    def silence_pcm(self, pcm, fmt, sr, channels, frames, regions):
        return self._out16("silence_pcm", channels, frames)

    def separate_pcm(self, pcm, fmt, sr, channels, frames, regions, **kw):
        return self._out16("separate_pcm", channels, frames)

    def separate_pcm_channels(self, pcm, fmt, sr, channels, frames, regions, **kw):
        return self._out16("separate_pcm_channels", channels, frames)

    def silence_pcm_source(self, pcm, fmt, sr, channels, frames, regions):
        return self._out8("silence_pcm_source", fmt, channels, frames)

    def separate_pcm_source(self, pcm, fmt, sr, channels, frames, regions, **kw):
        return self._out8("separate_pcm_source", fmt, channels, frames)

    def separate_pcm_channels_source(self, pcm, fmt, sr, channels, frames, regions, **kw):
        return self._out8("separate_pcm_channels_source", fmt, channels, frames)


class _Model:
    def __init__(self):
        self.log = []

    def with_range_fallback(self, fn, key=None):
        return fn(_Ctx(self.log))


def _chunk(tag: bytes, body: bytes) -> bytes:
    return tag + struct.pack("<I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")


@pytest.fixture()
def review(tmp_path):
    """meta.wav: 24-bit mono, 7 frames (an odd data size and its pad byte), a LIST chunk before `data` and a bext chunk after it;
    take.aif: 16-bit stereo AIFF."""
    from softspoken_amd import synth
    src = tmp_path / "in"
    src.mkdir()
    (tmp_path / "out").mkdir()
    rng = np.random.default_rng(7)
    body = rng.integers(1, 255, size=21, dtype=np.uint8).tobytes()
    fmt_ = _chunk(b"fmt ", struct.pack("<HHIIHH", 1, 1, 8000, 24000, 3, 24))
    lst = _chunk(b"LIST", b"INFOINAM" + struct.pack("<I", 5) + b"dawn\x00\x00")
    bext = _chunk(b"bext", bytes(range(1, 200)) + b"\x07")
    chunks = b"WAVE" + fmt_ + lst + _chunk(b"data", body) + bext
    wav = b"RIFF" + struct.pack("<I", len(chunks)) + chunks
    (src / "meta.wav").write_bytes(wav)
    aif = synth.aiff_bytes(rng.integers(-3000, 3000, size=(500, 2)), 8000, 16)
    (src / "take.aif").write_bytes(aif)
    df = pd.DataFrame({"ID": [1, 2], "file_path": [str(src)] * 2, "file_name": ["meta.wav", "take.aif"], "start_time": [0.0, 0.01],
                       "end_time": [0.0005, 0.03], "erase": [1, 1]})
    return df, str(tmp_path / "out"), dict(wav=wav, aif=aif, body=body)


@pytest.mark.parametrize("method,mode,calls", [("zero", None, ["silence_pcm_source"] * 2),
                                               ("separate", "mix", ["separate_pcm_source"] * 2),
                                               ("separate", "each", ["separate_pcm_source", "separate_pcm_channels_source"])])
def test_silence_job_source_keeps_the_file_image(native, review, method, mode, calls):
    from softspoken_amd import silence
    df, out, src = review
    m = _Model()
    job = silence.SilenceJob(df, out, ctx=_Ctx(m.log), model=m, method=method, channel_mode=mode, encoding="source")
    paths = job.run()
    assert not job.errors and sorted(os.path.basename(p) for p in paths) == ["meta_silenced.wav", "take_silenced.aif"]
    assert m.log == calls
    for k, (name, image) in enumerate((("meta_silenced.wav", src["wav"]), ("take_silenced.aif", src["aif"]))):
        got = open(os.path.join(out, name), "rb").read()
        info = native.wav_parse(image)
        a, b = info.data_offset, info.data_offset + info.frames * info.channels * (info.bits // 8)
        assert len(got) == len(image)
        assert got[:a] == image[:a] and got[b:] == image[b:]                    # header, LIST, bext, pad byte; FORM, COMM, SSND header
        assert got[a:b] == bytes([0xA0 + k + 1]) * (b - a)                      # the sample bytes are the call's output
        back = native.wav_parse(got)
        assert (back.format, back.frames, back.data_offset) == (info.format, info.frames, info.data_offset)
    wav = open(os.path.join(out, "meta_silenced.wav"), "rb").read()
    assert b"LIST" in wav[:60] and wav.index(b"bext") > wav.index(b"data") and len(src["body"]) == 21


def test_silence_job_pcm16_writes_what_it_wrote(native, review, monkeypatch):
    from root.code.backend import settings
    from softspoken_amd import silence
    df, out, src = review
    monkeypatch.delattr(settings, "hip_silence_encoding", raising=False)          # unset: the default
    for kw in (dict(), dict(encoding="pcm16")):
        for method, mode, calls in (("zero", None, ["silence_pcm"] * 2), ("separate", "each", ["separate_pcm", "separate_pcm_channels"])):
            m = _Model()
            paths = silence.SilenceJob(df, out, ctx=_Ctx(m.log), model=m, method=method, channel_mode=mode, **kw).run()
            assert sorted(os.path.basename(p) for p in paths) == ["meta_silenced.wav", "take_silenced.wav"] and m.log == calls
            got = open(os.path.join(out, "meta_silenced.wav"), "rb").read()
            assert got == native.wav_header_pcm16(8000, 1, 7) + np.full(7, 0x0101, dtype=np.int16).tobytes()
            got = open(os.path.join(out, "take_silenced.wav"), "rb").read()
            assert got == native.wav_header_pcm16(8000, 2, 500) + np.full(1000, 0x0202, dtype=np.int16).tobytes()
    monkeypatch.setattr(settings, "hip_silence_encoding", "source", raising=False)  # None follows the setting
    m = _Model()
    paths = silence.silence_files(df, out, ctx=_Ctx(m.log), model=m)
    assert m.log == ["silence_pcm_source"] * 2 and sorted(os.path.basename(p) for p in paths) == ["meta_silenced.wav", "take_silenced.aif"]


def test_the_setting_is_checked_where_it_is_read(review, monkeypatch):
    import importlib
    from root.code.backend import settings, voice_activity
    from softspoken_amd import silence
    df, out, _ = review
    try:
        monkeypatch.delenv("SOFTSPOKEN_SILENCE_ENCODING", raising=False)
        assert importlib.reload(settings).hip_silence_encoding == "pcm16"
        monkeypatch.setenv("SOFTSPOKEN_SILENCE_ENCODING", "source")
        assert importlib.reload(settings).hip_silence_encoding == "source"
    finally:
        monkeypatch.undo()
        importlib.reload(settings)
    monkeypatch.setattr(settings, "hip_silence_encoding", "pcm24", raising=False)
    with pytest.raises(ValueError):
        voice_activity.silence_encoding()
    with pytest.raises(ValueError):
        silence.SilenceJob(df, out, ctx=_Ctx([])).run()
    for bad in ("wav", "", "SOURCE", 16):
        with pytest.raises(ValueError):
            silence.SilenceJob(df, out, encoding=bad)
    monkeypatch.setattr(settings, "hip_silence_encoding", "source", raising=False)
    assert voice_activity.silence_encoding() == "source"


# ---- the reference passes its own bound ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spread(sd_np):
    return R.spread_head(sd_np)


@pytest.mark.parametrize("name,sr,ch", K.SEP_CASES + [K.F16_CASE])
def test_the_reference_lies_inside_the_separation_bound(native, spread, name, sr, ch):
    """encode(separate_f32) of every GPU case, with the oracle network's maps, held to separation_bound: the bound is one that plain
    float32 arithmetic of the definition meets, with the margin of 4 unused."""
    import test_gpu_separation as T
    from oracle import oracle_np as O
    data, fmt, x = K.rec(name, sr, ch)
    frames = len(x)
    plan = native.separation_plan(sr, frames, T.B1_REGIONS)
    wins = sorted({i for r in plan["ranges"] for i in range(r["win_first"], r["win_last"] + 1)})
    spec = R._oracle_spec(spread, O.pad_3s(O.resample(O.to_mono(x), sr)), wins)
    by_win = {w: spec[t] for t, w in enumerate(wins)}
    _, y64 = R.separate(x, sr, T.B1_REGIONS, by_win, unrounded=True)
    y32 = R.separate_f32(x, sr, T.B1_REGIONS, by_win)
    e32 = float(np.abs(y32.astype(np.float64) - y64).max())
    m = S.frame_mask(frames, sr, T.B1_REGIONS)
    assert 0 < m.sum() < frames
    y = (y32.astype(np.float64) / 32767.0).astype(np.float32)                     # the float32 blend in unit scale
    got = S.separate_source(data, fmt, sr, ch, frames, T.B1_REGIONS, y)
    K.check_bound(f"reference {name}/{sr}/{ch}", got, data, fmt, ch, m, y64, e32, plan["n_fft"])
