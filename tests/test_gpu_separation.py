"""The separation silencer on a real MI355X (include/softspoken.h "separation silencer"): averaged maps bit for bit, the transcode
outside the intervals bit for bit, the two limits of the gain (ss_silence_pcm's zeros, the plain transcode), the orientation of the
spectrum, parity with the float64 reference of tests/separation_ref.py, determinism, and the headless SilenceJob."""
import os

import numpy as np
import pandas as pd
import pytest

import separation_ref as R

pytestmark = pytest.mark.gpu

REGIONS = [(0.25, 0.5), (0.4, 0.75), (1.9, 99.0), (-2.0, 0.0105), (1.2, 1.1), (1.00005, 1.00015), (0.3, 0.35)]


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


def _crafted_blob(sd_np, speech_bias):
    """The session checkpoint with a constant spec head: Conv2d(32, 2, 1) weights 0, env bias 0, speech bias as given -> maps
    y_env = 0 and y_speech = relu(speech_bias): gain 0 (speech_bias > 0) or 1 (both powers 0)."""
    from softspoken_amd import checkpoint
    sd = dict(sd_np)
    sd["spec_output_conv.1.weight"] = np.zeros_like(sd_np["spec_output_conv.1.weight"])
    sd["spec_output_conv.1.bias"] = np.array([0.0, speech_bias], dtype=np.float32)
    return checkpoint.pack_state_dict(sd)


@pytest.fixture(scope="module")
def ctxs(native, blob):
    c = {p: native.Context(blob, 0, precision=p) for p in ("fp32", "f16x2")}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def ctx_gain0(native, sd_np):
    c = native.Context(_crafted_blob(sd_np, 4.0), 0, precision="fp32")
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_gain1(native, sd_np):
    c = native.Context(_crafted_blob(sd_np, -1.0), 0, precision="fp32")
    yield c
    c.close()


def _make(fmt, sr, ch, seconds, seed, scale=1.6):
    """(data chunk bytes, WavInfo, decoded float32 (frames, ch), WAV image) of a seeded recording.  scale 1.6 reaches full scale (the
    silencer tests' recordings); comparisons with a tolerance use quieter ones, whose resynthesis cannot cross the int16 wrap."""
    from softspoken_amd import synth
    from oracle import oracle_np as O
    x = synth.synth_audio(seed, seconds, sr, ch, with_silence=False).T.reshape(-1, ch)
    x = (x * scale).astype(np.float32)
    if fmt == "pcm16":
        pcm = np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16)
    elif fmt == "pcm24":
        pcm = np.clip(np.rint(x * 8388608), -8388608, 8388607).astype(np.int32)
    elif fmt == "pcm32":
        pcm = np.clip(np.rint(x.astype(np.float64) * 2147483648), -2147483648, 2147483647).astype(np.int64).astype(np.int32)
    elif fmt == "u8":
        pcm = np.clip(np.rint(x * 128 + 128), 0, 255).astype(np.uint8)
    else:
        pcm = (x * 1.3).astype(np.float32)
    wav = synth.wav_bytes(pcm.squeeze(), sr, fmt)
    from softspoken_amd import native
    info = native.wav_parse(wav)
    data = np.frombuffer(wav, dtype=np.uint8, count=info.data_bytes, offset=info.data_offset)
    return data, info, O.decode_pcm(wav, O.parse_wav(wav)), wav


def _mask(frames, sr, regions):
    m = np.zeros(frames, dtype=bool)
    for a, b in R.merged_intervals(regions, sr, frames):
        m[a:b] = True
    return m


@pytest.mark.parametrize("prec", ["fp32", "f16x2"])
def test_maps_equal_whole_file_average(ctxs, c1, prec):
    ctx = ctxs[prec]
    ctx.reset()
    fid = ctx.add_f32_22k(c1["sig"])
    spec, _ = ctx.infer_windows(fid, c1["starts"], want_spec=True)
    W = len(c1["starts"])
    n_bins = min(round(len(c1["padded"]) / 22050 * 256 / 3), R.win_start(W - 1) + 256)
    by_win = {i: spec[i] for i in range(W)}
    for first, n in ((0, 40), (2731, 77), (n_bins - 60, 60)):
        got = ctx.separation_maps(fid, first, n)
        want = R.average_maps(by_win, range(first, first + n))
        assert got.dtype == np.float32 and np.array_equal(got, want), (first, n)
    from softspoken_amd import native
    for first, n in ((n_bins - 1, 2), (-1, 3), (5, 0)):
        with pytest.raises(native.NativeError) as e:
            ctx.separation_maps(fid, first, n)
        assert e.value.code == 1


@pytest.mark.parametrize("fmt,sr,ch", [("pcm16", 48000, 2), ("pcm24", 44100, 1), ("pcm32", 96000, 4), ("u8", 8000, 1), ("f32", 22050, 2)])
def test_outside_intervals_is_the_transcode(ctxs, fmt, sr, ch):
    ctx = ctxs["fp32"]
    data, info, x, _ = _make(fmt, sr, ch, 2.0, 11)
    got = ctx.separate_pcm(data, info.format, sr, ch, info.frames, REGIONS)
    plain = ctx.silence_pcm(data, info.format, sr, ch, info.frames, [])
    m = _mask(info.frames, sr, REGIONS)
    assert got.shape == plain.shape and got.dtype == np.int16
    assert np.array_equal(got[~m], plain[~m])
    assert not np.array_equal(got[m], plain[m])                     # the session checkpoint's gains are neither 0 nor 1


@pytest.mark.parametrize("fmt,sr,ch", [("pcm16", 48000, 2), ("u8", 8000, 1), ("pcm24", 96000, 3)])
def test_gain_zero_is_the_zeroing_silencer(ctx_gain0, fmt, sr, ch):
    data, info, _, _ = _make(fmt, sr, ch, 2.0, 12)
    got = ctx_gain0.separate_pcm(data, info.format, sr, ch, info.frames, REGIONS, fade_s=0.0, min_gain=0.0, above_fmax="mute")
    want = ctx_gain0.silence_pcm(data, info.format, sr, ch, info.frames, REGIONS)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("fmt,sr,ch", [("pcm16", 48000, 2), ("f32", 16000, 1), ("pcm24", 192000, 2)])
def test_gain_one_is_the_transcode(ctx_gain1, fmt, sr, ch):
    data, info, _, _ = _make(fmt, sr, ch, 1.5, 13, scale=0.5)
    got = ctx_gain1.separate_pcm(data, info.format, sr, ch, info.frames, REGIONS, above_fmax="keep")
    plain = ctx_gain1.silence_pcm(data, info.format, sr, ch, info.frames, [])
    assert np.abs(got.astype(np.int32) - plain.astype(np.int32)).max() <= 1


def _tone_amplitude(y, sr, f):
    t = np.arange(len(y)) / sr
    A = np.stack([np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)], 1)
    c, *_ = np.linalg.lstsq(A, y, rcond=None)
    return float(np.hypot(*c))


def test_orientation_low_band_removed_high_band_kept(ctx_gain0):
    sr, secs = 48000, 4.0
    t = np.arange(int(sr * secs)) / sr
    x = 0.3 * np.sin(2 * np.pi * 1000 * t) + 0.3 * np.sin(2 * np.pi * 12000 * t)
    pcm = np.rint(x * 32767).astype(np.int16)
    got = ctx_gain0.separate_pcm(pcm, 2, sr, 1, len(pcm), [(1.0, 3.0)], above_fmax="keep")[:, 0].astype(np.float64) / 32767
    inner = slice(int(1.1 * sr), int(2.9 * sr))
    ref = pcm.astype(np.float64)[inner] / 32767
    a1, a1_in = _tone_amplitude(got[inner], sr, 1000), _tone_amplitude(ref, sr, 1000)
    a12, a12_in = _tone_amplitude(got[inner], sr, 12000), _tone_amplitude(ref, sr, 12000)
    assert 20 * np.log10(a1 / a1_in) <= -60.0
    assert abs(20 * np.log10(a12 / a12_in)) <= 0.1


@pytest.mark.parametrize("prec", ["fp32", "f16x2"])
def test_parity_with_float64_reference(native, ctxs, prec):
    ctx = ctxs[prec]
    sr, ch = 48000, 2
    data, info, x, _ = _make("pcm16", sr, ch, 60.0, 21, scale=0.5)
    regions = [(-1.0, 2.5), (20.0, 27.3), (57.0, 70.0)]
    plan = native.separation_plan(sr, info.frames, regions)
    wins = sorted({i for r in plan["ranges"] for i in range(r["win_first"], r["win_last"] + 1)})
    assert len(wins) == plan["windows_run"]
    ctx.reset()
    fid = ctx.add_pcm(data, info.format, sr, ch, info.frames)
    spec, _ = ctx.infer_windows(fid, np.array(wins, dtype=np.int64) * 13230, want_spec=True)
    want = R.separate(x, sr, regions, {w: spec[t] for t, w in enumerate(wins)})
    got = ctx.separate_pcm(data, info.format, sr, ch, info.frames, regions)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1, (prec, int(d.max()), int((d > 1).sum()))
    m = _mask(info.frames, sr, regions)
    assert not d[~m].any()


def test_two_calls_identical_and_counted_as_reset(native, ctxs):
    ctx = ctxs["fp32"]
    data, info, _, _ = _make("pcm16", 44100, 2, 8.0, 31)
    regions = [(0.5, 3.0), (5.0, 5.4)]
    g0 = ctx.reset_generation()
    a = ctx.separate_pcm(data, info.format, 44100, 2, info.frames, regions, fade_s=0.02, min_gain=0.1)
    b = ctx.separate_pcm(data, info.format, 44100, 2, info.frames, regions, fade_s=0.02, min_gain=0.1)
    assert a.tobytes() == b.tobytes()
    assert ctx.reset_generation() == g0 + 2
    audio = native.Context(None, 0)
    with pytest.raises(native.NativeError) as e:
        audio.separate_pcm(data, info.format, 44100, 2, info.frames, regions)
    assert e.value.code == 4                                          # SS_ERR_STATE: audio-only
    audio.close()
    with pytest.raises(native.NativeError) as e:
        ctx.separate_pcm(data, info.format, 44100, 2, info.frames, regions, min_gain=2.0)
    assert e.value.code == 1


def test_silence_job_separate(tmp_path, c1, sd_torch, ctxs, native):
    import torch
    from root.code.backend.pytorch_neural_nets import SpecUNet_2D
    from softspoken_amd import silence, synth
    src = tmp_path / "in"
    src.mkdir()
    out = tmp_path / "out"
    out.mkdir()
    a_data, a_info, _, a_wav = _make("pcm16", 48000, 2, 6.0, 41)
    (src / "a.wav").write_bytes(a_wav)
    x = c1["pcm"][: 16000 * 12].astype(np.float32) / np.float32(32768.0)
    x[16000 * 5] = np.float32("nan")                                  # inside an interval: the f16x2 mode refuses this file
    nan_wav = synth.wav_bytes(x, 16000, "f32")
    (src / "nan.wav").write_bytes(nan_wav)
    df = pd.DataFrame({"ID": [1, 2, 3, 4], "file_path": [str(src)] * 4, "file_name": ["a.wav", "a.wav", "nan.wav", "a.wav"],
                       "start_time": [0.5, 3.0, 4.0, 5.0], "end_time": [1.5, 3.2, 6.0, 5.5], "erase": [1, 1, 1, 0]})
    m = SpecUNet_2D(precision="f16x2")
    with torch.no_grad():
        m.load_state_dict(sd_torch)
    m.eval()
    seen = []
    job = silence.SilenceJob(df, str(out), method="separate", model=m, min_gain=0.05, file_complete=lambda p: seen.append(p))
    paths = job.run()
    assert sorted(os.listdir(out)) == ["a_silenced.wav", "nan_silenced.wav"] and not job.errors and len(seen) == 2 == len(paths)
    want_a = ctxs["f16x2"].separate_pcm(a_data, a_info.format, 48000, 2, a_info.frames, [(0.5, 1.5), (3.0, 3.2)], min_gain=0.05)
    assert (out / "a_silenced.wav").read_bytes() == native.wav_header_pcm16(48000, 2, a_info.frames) + want_a.tobytes()
    n_info = native.wav_parse(nan_wav)
    n_data = np.frombuffer(nan_wav, dtype=np.uint8, count=n_info.data_bytes, offset=n_info.data_offset)
    with pytest.raises(native.NativeError) as e:
        ctxs["f16x2"].separate_pcm(n_data, n_info.format, 16000, 1, n_info.frames, [(4.0, 6.0)], min_gain=0.05)
    assert e.value.code == native.SS_ERR_RANGE
    want_n = ctxs["fp32"].separate_pcm(n_data, n_info.format, 16000, 1, n_info.frames, [(4.0, 6.0)], min_gain=0.05)
    assert (out / "nan_silenced.wav").read_bytes() == native.wav_header_pcm16(16000, 1, n_info.frames) + want_n.tobytes()
    assert m.effective_precision() == "f16x2"
    with pytest.raises(ValueError):
        silence.SilenceJob(df, str(out), method="separate")
