"""The separation silencer on a real MI355X (include/softspoken.h "separation silencer"): averaged maps bit for bit, the transcode
outside the intervals bit for bit, the two limits of the gain (ss_silence_pcm's zeros, the plain transcode), the orientation of the
spectrum, parity with the float64 reference of tests/separation_ref.py, determinism, and the headless SilenceJob.

The parity cases hold every output sample to the reference's unrounded float64 output y64 (in LSB): |got - y64| <= 0.5 + tau, 0.5 being
the output rounding and tau = 4 e32, e32 the largest |separate_f32 - y64| of the same case (the float32 CPU restatement of steps 3 and 4,
computed inside the test).  The margin of 4 covers the device's different order of roundings (Stockham radix-16 against the CPU
library's factorisation) and its float32 alpha, band weights and fade weight; the device's own error never sets tau.  The gains come from
two crafted heads (separation_ref.spread_head / mixed_head): the session checkpoint's gain is exactly 1 on almost every cell."""
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
    x = synth.synth_audio(seed, seconds, sr, ch, with_silence=False).T.reshape(-1, ch)
    return _pack((x * scale).astype(np.float32), fmt, sr)


def _pack(x, fmt, sr):
    """_make's tuple for samples x float32 (frames, ch)."""
    from softspoken_amd import synth
    from oracle import oracle_np as O
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
    wav = synth.wav_bytes(pcm.squeeze(axis=1) if pcm.shape[1] == 1 else pcm, sr, fmt)
    from softspoken_amd import native
    info = native.wav_parse(wav)
    data = np.frombuffer(wav, dtype=np.uint8, count=info.data_bytes, offset=info.data_offset)
    return data, info, O.decode_pcm(wav, O.parse_wav(wav)).reshape(-1, x.shape[1]), wav


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
    by_win = {w: spec[t] for t, w in enumerate(wins)}
    want, y64 = R.separate(x, sr, regions, by_win, unrounded=True)
    got = ctx.separate_pcm(data, info.format, sr, ch, info.frames, regions)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1, (prec, int(d.max()), int((d > 1).sum()))
    m = _mask(info.frames, sr, regions)
    assert not d[~m].any()
    e32 = float(np.abs(R.separate_f32(x, sr, regions, by_win).astype(np.float64) - y64).max())      # the bound of the cases below
    excess = float(np.maximum(np.abs(got.astype(np.float64) - y64)[m] - 0.5, 0.0).max())
    print(f"SEPBOUND session checkpoint {prec}: N=1024 ch={ch} e32={e32:.5f} tau={4 * e32:.5f} excess={excess:.5f} samples={int(m.sum()) * ch}")
    assert excess <= 4.0 * e32, (prec, excess, 4.0 * e32)


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


# ---- the bound: every FFT size, channel count, format, parameter and cut against the unrounded float64 reference ---------------
B1_REGIONS = [(-1.0, 0.3), (0.9, 1.4), (1.35, 1.6), (1.8, 1.8004), (2.2, 99.0)]     # file start, a merged pair, < one hop at any rate, file end
B1_CASES = [(8000, 256, 1, "u8"), (16000, 512, 3, "pcm16"), (22050, 512, 2, "f32"), (44100, 1024, 1, "pcm24"), (96000, 2048, 5, "pcm32"),
            (192000, 4096, 2, "pcm16"), (384000, 8192, 1, "pcm16"), (384000, 8192, 3, "pcm24")]
B1_SECONDS, B1_SEED = 2.5, 51


def _bound_case(native, ctx, label, rec, sr, regions, **params):
    """One parity case on the recording rec (_make's tuple): spec maps from the device on exactly the plan's windows -> the float64
    reference (unrounded) and its float32 restatement on the CPU -> the device's output held to 0.5 + 4 e32 inside the merged
    intervals and to the transcode's bits outside.  Prints the case's line; returns what the callers assert further things on."""
    data, info, x, _ = rec
    ch, frames = x.shape[1], info.frames
    plan = native.separation_plan(sr, frames, regions, **params)
    wins = sorted({i for r in plan["ranges"] for i in range(r["win_first"], r["win_last"] + 1)})
    ctx.reset()
    by_win = {}
    if wins:
        fid = ctx.add_pcm(data, info.format, sr, ch, frames)
        spec, _ = ctx.infer_windows(fid, np.array(wins, dtype=np.int64) * 13230, want_spec=True)
        by_win = {w: spec[t] for t, w in enumerate(wins)}
    ivs = []
    want, y64 = R.separate(x, sr, regions, by_win, unrounded=True, info=ivs, **params)
    y32 = R.separate_f32(x, sr, regions, by_win, **params)
    got = ctx.separate_pcm(data, info.format, sr, ch, frames, regions, **params)
    plain = ctx.silence_pcm(data, info.format, sr, ch, frames, [])
    m = _mask(frames, sr, regions)
    assert got.shape == (frames, ch) and got.dtype == np.int16
    assert np.array_equal(got[~m], plain[~m]), label
    e32 = float(np.abs(y32.astype(np.float64) - y64).max()) if frames else 0.0
    tau = 4.0 * e32
    err = np.abs(got.astype(np.float64) - y64)[m]
    excess = float(np.maximum(err - 0.5, 0.0).max()) if err.size else 0.0
    print(f"SEPBOUND {label}: N={plan['n_fft']} ch={ch} e32={e32:.5f} tau={tau:.5f} excess={excess:.5f} samples={err.size}")
    assert excess <= tau, (label, excess, tau, int((err - 0.5 > tau).sum()))
    return dict(got=got, want=want, y64=y64, ivs=ivs, plan=plan, e32=e32, tau=tau, excess=excess)


def _head_ctx(native, sd, prec="fp32", **kw):
    from softspoken_amd import checkpoint
    return native.Context(checkpoint.pack_state_dict(sd), 0, precision=prec, **kw)


@pytest.fixture(scope="module")
def heads(sd_np):
    return dict(spread=R.spread_head(sd_np), mixed=R.mixed_head(sd_np))


@pytest.fixture(scope="module")
def ctx_spread(native, heads):
    c = _head_ctx(native, heads["spread"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_mixed(native, heads):
    c = _head_ctx(native, heads["mixed"])
    yield c
    c.close()


@pytest.mark.parametrize("sr,n_fft,ch,fmt", B1_CASES)
def test_bound_fft_sizes_channels_formats(native, ctx_spread, sr, n_fft, ch, fmt):
    """Every sep_stft_kernel<N> instantiation under a gain that moves with band and time, odd channel counts (the last complex FFT
    carries an empty imaginary half), every PCM format; 22050 Hz has no resampler, 44100 Hz the unfused one."""
    r = _bound_case(native, ctx_spread, f"{sr}/{ch}/{fmt}", _make(fmt, sr, ch, B1_SECONDS, B1_SEED, scale=0.5), sr, B1_REGIONS)
    assert r["plan"]["n_fft"] == n_fft and len(r["ivs"]) == 4
    R.assert_spread(R.gain_stats([iv["G"] for iv in r["ivs"]]))


def _sil_args(rec, sr):
    data, info, x, _ = rec
    return data, info.format, sr, x.shape[1], info.frames


def test_bound_f16x2_context(native, heads):
    ctx = _head_ctx(native, heads["spread"], "f16x2")
    try:
        r = _bound_case(native, ctx, "48000/2/pcm16 f16x2", _make("pcm16", 48000, 2, B1_SECONDS, B1_SEED, scale=0.5), 48000, B1_REGIONS)
        R.assert_spread(R.gain_stats([iv["G"] for iv in r["ivs"]]))
    finally:
        ctx.close()


@pytest.mark.parametrize("sr,ch,fmt", [(48000, 2, "pcm16"), (8000, 1, "pcm16")])
def test_bound_mixed_head(native, ctx_mixed, sr, ch, fmt):
    """Cells whose gain is exactly 0 (env 0: sep_log_power's -inf on one side), exactly 1 (speech 0, or both) and ordinary, side by side."""
    r = _bound_case(native, ctx_mixed, f"mixed {sr}/{ch}", _make(fmt, sr, ch, B1_SECONDS, B1_SEED, scale=0.5), sr, B1_REGIONS)
    R.assert_mixed(R.gain_stats([iv["G"] for iv in r["ivs"]]))


PARAM_CASES = [
    (48000, 2, dict(fade_s=0.0, min_gain=0.1, above_fmax="mute", speech_channel=1)),
    (48000, 2, dict(fade_s=0.5, min_gain=0.45, above_fmax="keep", speech_channel=1)),
    (48000, 2, dict(fade_s=0.02, min_gain=1.0, above_fmax="mute", speech_channel=1)),
    (48000, 2, dict(fade_s=0.02, min_gain=0.0, above_fmax="keep", speech_channel=0)),
    (16000, 1, dict(fade_s=0.5, min_gain=0.1, above_fmax="keep", speech_channel=1)),      # the Nyquist bin sits at exactly 8000 Hz
    (16000, 1, dict(fade_s=0.0, min_gain=0.45, above_fmax="mute", speech_channel=0)),
    (16000, 1, dict(fade_s=0.02, min_gain=1.0, above_fmax="keep", speech_channel=1)),
    (16000, 1, dict(fade_s=0.02, min_gain=0.1, above_fmax="mute", speech_channel=1)),
]


@pytest.mark.parametrize("sr,ch,params", PARAM_CASES, ids=lambda v: "-".join(str(x) for x in v.values()) if isinstance(v, dict) else str(v))
def test_bound_parameters(native, ctx_spread, sr, ch, params):
    rec = _make("pcm16", sr, ch, B1_SECONDS, B1_SEED, scale=0.5)
    r = _bound_case(native, ctx_spread, f"{sr}/{ch} {params}", rec, sr, B1_REGIONS, **params)
    G = np.concatenate([iv["G"].ravel() for iv in r["ivs"]])
    if params["fade_s"] == 0.5:                                         # the two ramps meet: no sample of any interval has weight 1
        assert all(R.fade_weights(iv["a"], iv["b"], round(0.5 * sr)).max() < 1.0 for iv in r["ivs"])
    if params["min_gain"] == 0.45:                                      # the floor clips a part of the spread gains, not all of them
        assert 0.05 < (G == 0.45).mean() < 0.95 and G.min() == 0.45
    if params["min_gain"] == 1.0:                                       # every gain 1: the reference is the transcode
        m = _mask(rec[1].frames, sr, B1_REGIONS)
        x64 = rec[2].astype(np.float64)[m] * 32767.0
        assert np.abs(r["y64"][m] - x64).max() <= 1e-6
        assert np.abs(r["got"].astype(np.float64)[m] - x64).max() <= 0.5 + r["tau"] + 1e-6
    other = dict(params, speech_channel=1 - params["speech_channel"])
    if params["min_gain"] < 1.0:                                        # the two orientations of the head give different audio
        got2 = ctx_spread.separate_pcm(*_sil_args(rec, sr), B1_REGIONS, **other)
        assert not np.array_equal(got2, r["got"])
    keep2 = dict(params, above_fmax="mute" if params["above_fmax"] == "keep" else "keep")
    if params["min_gain"] < 1.0 and sr == 48000:                        # a third of the STFT bins lie at or above 8000 Hz
        assert not np.array_equal(ctx_spread.separate_pcm(*_sil_args(rec, sr), B1_REGIONS, **keep2), r["got"])


@pytest.fixture(scope="module")
def after_edges(ctx_spread):
    """A call whose bytes say that the context still works."""
    rec = _make("pcm16", 8000, 1, 1.0, 52, scale=0.5)
    return rec, ctx_spread.separate_pcm(*_sil_args(rec, 8000), [(0.2, 0.7)])


EDGE_CASES = {
    "100 frames": (48000, 2, 100, [(0.0, 1.0)]),                       # shorter than one FFT
    "1 frame": (48000, 1, 1, [(0.0, 1.0)]),
    "0.05 s": (48000, 2, 2400, [(0.004, 0.031), (0.0449, 0.05)]),
    "one sample": (48000, 2, 2400, [(0.02, 0.02 + 1.0 / 48000)]),
    "both clamps": (20, 1, 30, [(-1.0, 99.0)]),                         # 20 Hz: a hop of 64 samples is 3.2 s, frame -1 lies before bin 0's centre
}


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_bound_edges(native, ctx_spread, after_edges, name):
    """Inputs the header promises to take, at the edges of the plan: recordings shorter than one FFT, an interval of one sample, and a
    recording whose frames lie before the first and behind the last bin that has a window."""
    sr, ch, frames, regions = EDGE_CASES[name]
    rng = np.random.default_rng(53)
    x = (0.25 * rng.standard_normal((frames, ch))).clip(-0.9, 0.9).astype(np.float32)
    rec = _pack(x, "pcm16", sr)
    r = _bound_case(native, ctx_spread, f"edge {name}", rec, sr, regions)
    assert len(r["ivs"]) == len(R.merged_intervals(regions, sr, frames)) >= 1
    if name == "one sample":
        assert [(iv["a"], iv["b"]) for iv in r["ivs"]] == [(960, 961)]
    if name == "both clamps":
        assert any(iv["clamp_lo"] for iv in r["ivs"]) and any(iv["clamp_hi"] for iv in r["ivs"])
    rec0, want0 = after_edges
    assert np.array_equal(ctx_spread.separate_pcm(*_sil_args(rec0, 8000), [(0.2, 0.7)]), want0)


def test_maps_and_output_across_passes(native, heads, ctx_spread, c1):
    """sep_accumulate_kernel's carry: with 7 windows per pass the float64 sums of a bin travel through memory from pass to pass; the
    maps equal the one-pass context's and the reference's average bit for bit, and the separated bytes do not depend on the passes."""
    small = _head_ctx(native, heads["spread"], chunk=7)
    try:
        first, n = 100, 1500
        fid = small.add_f32_22k(c1["sig"])
        got = small.separation_maps(fid, first, n)
        ctx_spread.reset()
        fid1 = ctx_spread.add_f32_22k(c1["sig"])
        one = ctx_spread.separation_maps(fid1, first, n)
        wins = [i for i in range(len(c1["starts"])) if R.win_start(i) + 255 >= first and R.win_start(i) <= first + n - 1]
        assert len(wins) >= 30
        spec, _ = ctx_spread.infer_windows(fid1, np.array(wins, dtype=np.int64) * 13230, want_spec=True)
        want = R.average_maps({w: spec[t] for t, w in enumerate(wins)}, range(first, first + n))
        assert np.array_equal(got, one) and np.array_equal(got, want) and want.any()
        rec = _make("pcm16", 16000, 3, B1_SECONDS, B1_SEED, scale=0.5)                 # 10 windows: two passes of the small context
        assert native.separation_plan(16000, rec[1].frames, B1_REGIONS)["windows_run"] > 7
        a = small.separate_pcm(*_sil_args(rec, 16000), B1_REGIONS)
        b = ctx_spread.separate_pcm(*_sil_args(rec, 16000), B1_REGIONS)
        assert a.tobytes() == b.tobytes()
    finally:
        small.close()


def test_bound_across_the_piece_cut(native, heads):
    """The product library's own cut: an interval longer than one piece of the 256 MB frame buffer.  192 kHz, 6 channels: 3 channel
    pairs x 4096 x 8 bytes per frame -> 2730 frames, a piece of 2722 hops = 14.5 s; the interval of 15 s takes two pieces, and the
    second does not fit the first's chunk."""
    sr, ch, N = 192000, 6, 4096
    budget = (256 << 20) // (((ch + 1) // 2) * N * 8)                  # kSepFrameBytes / (npairs N sizeof(float2)) of separate_pcm
    piece = (budget - 8) * (N // 4)
    regions = [(0.5, 15.5)]
    assert piece < 15 * sr < 2 * piece                                 # two pieces; a later change of the budget must not make it one
    ctx = _head_ctx(native, heads["spread"], profile=True)
    try:
        rec = _make("pcm16", sr, ch, 16.0, 54, scale=0.5)
        ctx.reset_stats()
        r = _bound_case(native, ctx, "192000/6 two pieces", rec, sr, regions)
        st = {k["name"]: k["launches"] for k in ctx.kernel_stats()}
        assert st.get(f"sep_stft_kernel<{N}>") == 2 and st.get("sep_blend_kernel") == 2, st
        R.assert_spread(R.gain_stats([iv["G"] for iv in r["ivs"]]))
    finally:
        ctx.close()


_CUT_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from softspoken_amd import synth, native
import separation_ref as R
import test_gpu_separation as T
ctx = T._head_ctx(native, R.spread_head(synth.make_state_dict(0)))
for sr, ch in ((48000, 2), (16000, 3)):
    regions = [(0.013, 1.2), (1.7, 2.95), (1.5, 1.5 + 1.0 / sr)]
    rec = T._make("pcm16", sr, ch, 3.0, 55, scale=0.5)
    assert [b - a for a, b in R.merged_intervals(regions, sr, rec[1].frames)][1] == 1
    ctx.debug_set_separation_budget(0)
    r = T._bound_case(native, ctx, "cuts %d/%d default budget" % (sr, ch), rec, sr, regions)
    hop = r["plan"]["hop"]
    for budget in (16, 17, 23, 64):
        ctx.debug_set_separation_budget(budget)
        got = ctx.separate_pcm(*T._sil_args(rec, sr), regions)
        bad = np.flatnonzero((got != r["got"]).any(axis=1))
        assert bad.size == 0, (sr, ch, budget, bad[:8], (bad[:8] - round(0.013 * sr)) / ((budget - 8) * hop))
        assert (1.2 - 0.013) * sr > 2 * (budget - 8) * hop          # the first interval takes more than two pieces
print("CUTS_OK")
"""


def test_every_cut_alignment_gives_the_same_bytes(build_all):
    """ss_debug_set_separation_budget (development build only) moves the piece and chunk cuts through 3 s recordings: pieces of 8, 9,
    15 and 56 hops, several chunks per call.  The blend adds the same four frames in ascending order wherever the cuts fall, and a
    recomputed shared frame is the same frame, so every budget must give the default budget's bytes -- which pass the bound."""
    import subprocess, sys
    from softspoken_amd import build as hip_build
    tests = os.path.dirname(os.path.abspath(__file__))
    e = dict(os.environ); e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
    r = subprocess.run([sys.executable, "-c", _CUT_SCRIPT.format(root=os.path.dirname(tests), tests=tests)], env=e, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "CUTS_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
