"""Per-channel separation on a real MI355X (ss_separate_pcm_channels, include/softspoken.h "Per-channel separation", DESIGN.md
section 17): every channel held to the float64 reference of tests/separation_ref.py run on that channel alone with the maps of that
channel's own passes -- the bound of test_gpu_separation.py, 0.5 + 4 e32 --, the exact equalities with ss_separate_pcm that any wrong
split or recombination of the two spectra breaks, the cuts (passes, pieces, chunks), the call's behaviour and the headless SilenceJob.

The conditions on these inputs (every channel a good parity case on its own, no two channels with the same gains, the gain a channel
gets moving its output by tens of LSB) are test_separation_channels_host.py's, with the CPU oracle."""
import os

import numpy as np
import pandas as pd
import pytest

import separation_channels_cases as K
import separation_ref as R
import test_gpu_separation as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


@pytest.fixture(scope="module")
def heads(sd_np):
    return dict(spread=R.spread_head(sd_np), mixed=R.mixed_head(sd_np))


@pytest.fixture(scope="module")
def ctx_spread(native, heads):
    c = T._head_ctx(native, heads["spread"], profile=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_mixed(native, heads):
    c = T._head_ctx(native, heads["mixed"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_f16(native, heads):
    c = T._head_ctx(native, heads["spread"], "f16x2")
    yield c
    c.close()


_RECS = {}


def _rec(sr, ch, fmt):
    if (sr, ch, fmt) not in _RECS:
        _RECS[(sr, ch, fmt)] = T._make(fmt, sr, ch, T.B1_SECONDS, T.B1_SEED, scale=0.5)
    return _RECS[(sr, ch, fmt)]


def _channel_maps(native, ctx, rec, sr, regions, **params):
    """reset + add_pcm_channels + the device's spec maps of the plan's windows, per channel: (plan, first file id, [by_win of channel c])."""
    data, info, x, _ = rec
    ch = x.shape[1]
    plan = native.separation_plan(sr, info.frames, regions, **params)
    wins = K.plan_windows(plan)
    ctx.reset()
    first = ctx.add_pcm_channels(data, info.format, sr, ch, info.frames)
    by_win = []
    for c in range(ch):
        spec, _ = ctx.infer_windows(first + c, np.array(wins, dtype=np.int64) * 13230, want_spec=True)
        by_win.append({w: spec[t] for t, w in enumerate(wins)})
    return plan, first, by_win


def _bound_case(native, ctx, label, rec, sr, regions, **params):
    """test_gpu_separation._bound_case per channel: channel c of the device's output against R.separate of channel c alone with the
    maps of the device's own passes over file first + c, |got - y64| <= 0.5 + 4 e32 inside the merged intervals (e32 from that
    channel's float32 restatement), the transcode's bytes outside.  Prints the case's line."""
    data, info, x, _ = rec
    ch, frames = x.shape[1], info.frames
    plan, first, by_win = _channel_maps(native, ctx, rec, sr, regions, **params)
    got = ctx.separate_pcm_channels(data, info.format, sr, ch, frames, regions, **params)
    plain = ctx.silence_pcm(data, info.format, sr, ch, frames, [])
    m = T._mask(frames, sr, regions)
    assert got.shape == (frames, ch) and got.dtype == np.int16
    assert np.array_equal(got[~m], plain[~m]), label
    rows, ivs_all = [], []
    for c in range(ch):
        xc = x[:, c:c + 1]
        ivs = []
        _, y64 = R.separate(xc, sr, regions, by_win[c], unrounded=True, info=ivs, **params)
        y32 = R.separate_f32(xc, sr, regions, by_win[c], **params)
        e32 = float(np.abs(y32.astype(np.float64) - y64).max())
        err = np.abs(got[:, c].astype(np.float64) - y64[:, 0])[m]
        rows.append((e32, float(np.maximum(err - 0.5, 0.0).max()), int((err - 0.5 > 4.0 * e32).sum())))
        ivs_all.append(ivs)
    worst = max(rows, key=lambda r: r[1] - 4.0 * r[0])
    print(f"SEPBOUND each {label}: N={plan['n_fft']} ch={ch} e32={worst[0]:.5f} tau={4 * worst[0]:.5f} excess={worst[1]:.5f} "
          f"samples={int(m.sum())} per channel; e32 of the channels {min(r[0] for r in rows):.5f}-{max(r[0] for r in rows):.5f}, "
          f"largest excess {max(r[1] for r in rows):.5f}")
    for c, (e32, excess, n_bad) in enumerate(rows):
        assert excess <= 4.0 * e32, (label, c, excess, 4.0 * e32, n_bad)
    return dict(got=got, plan=plan, ivs=ivs_all, by_win=by_win, first=first)


def _args(rec, sr):
    data, info, x, _ = rec
    return data, info.format, sr, x.shape[1], info.frames


# ---- the bound, per channel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,ch,fmt", K.BOUND_CASES)
def test_bound_per_channel_fft_sizes_channels_formats(native, ctx_spread, sr, ch, fmt):
    """Every sep_stft_each_kernel<N>, channel pairs with two different gains, odd counts (the last channel alone in its FFT), every
    format."""
    r = _bound_case(native, ctx_spread, f"{sr}/{ch}/{fmt}", _rec(sr, ch, fmt), sr, T.B1_REGIONS)
    assert r["plan"]["n_fft"] == K.N_FFT[sr]
    Gs = [[iv["G"] for iv in ivs] for ivs in r["ivs"]]
    for c in range(ch):
        assert len(Gs[c]) == 4
        R.assert_spread(R.gain_stats(Gs[c]))
    for a in range(ch):
        for b in range(a + 1, ch):
            assert K.pair_distance(Gs[a], Gs[b]) >= K.PAIR_DISTANCE, (a, b)
    mix = ctx_spread.separate_pcm(*_args(_rec(sr, ch, fmt), sr), T.B1_REGIONS)
    assert not np.array_equal(mix, r["got"])                                  # the mix's gains give other audio


@pytest.mark.parametrize("sr,ch,fmt", K.MIXED_CASES)
def test_bound_per_channel_mixed_head(native, ctx_mixed, sr, ch, fmt):
    r = _bound_case(native, ctx_mixed, f"mixed {sr}/{ch}", _rec(sr, ch, fmt), sr, T.B1_REGIONS)
    for ivs in r["ivs"]:
        R.assert_mixed(R.gain_stats([iv["G"] for iv in ivs]))


def test_bound_per_channel_f16x2_context(native, ctx_f16):
    sr, ch, fmt = K.MAIN_CASE
    r = _bound_case(native, ctx_f16, f"{sr}/{ch}/{fmt} f16x2", _rec(sr, ch, fmt), sr, T.B1_REGIONS)
    for ivs in r["ivs"]:
        R.assert_spread(R.gain_stats([iv["G"] for iv in ivs]))


def test_bound_per_channel_parameters(native, ctx_spread):
    sr, ch, fmt = K.MAIN_CASE
    rec = _rec(sr, ch, fmt)
    r = _bound_case(native, ctx_spread, f"{sr}/{ch} {K.PARAMS}", rec, sr, T.B1_REGIONS, **K.PARAMS)
    G = np.concatenate([iv["G"].ravel() for ivs in r["ivs"] for iv in ivs])
    assert G.min() >= 0.1 and (G == 0.1).mean() < 0.5                         # the floor holds, and not on most cells
    for other in (dict(K.PARAMS, speech_channel=1), dict(K.PARAMS, above_fmax="mute")):
        assert not np.array_equal(ctx_spread.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS, **other), r["got"]), other


# ---- exact equalities with ss_separate_pcm -------------------------------------------------------------------------------------
def test_one_channel_is_separate_pcm(ctx_spread):
    sr, ch, fmt = K.MONO_CASE
    rec = _rec(sr, ch, fmt)
    a = ctx_spread.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS)
    b = ctx_spread.separate_pcm(*_args(rec, sr), T.B1_REGIONS)
    plain = ctx_spread.silence_pcm(*_args(rec, sr), [])
    assert a.tobytes() == b.tobytes() and not np.array_equal(a, plain)


def test_the_unpaired_channel_is_separate_pcm_of_it_as_a_mono_file(ctx_spread):
    """Channel 2 of three rides alone in its complex FFT, with Gb := Ga: S = Ga and D = 0, the mix kernel's arithmetic."""
    sr, ch, fmt = 16000, 3, "pcm16"
    rec = _rec(sr, ch, fmt)
    got = ctx_spread.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS)
    mono = T._pack(np.ascontiguousarray(rec[2][:, 2:3]), fmt, sr)
    assert np.array_equal(mono[2][:, 0], rec[2][:, 2])                         # the same samples (pcm16 survives the round trip)
    want = ctx_spread.separate_pcm(*_args(mono, sr), T.B1_REGIONS)
    assert got[:, 2].tobytes() == want[:, 0].tobytes()
    for c in (0, 1):                                                          # the paired channels do not: another rounding order
        monoc = T._pack(np.ascontiguousarray(rec[2][:, c:c + 1]), fmt, sr)
        d = np.abs(got[:, c].astype(np.int32) - ctx_spread.separate_pcm(*_args(monoc, sr), T.B1_REGIONS)[:, 0].astype(np.int32))
        assert d.max() <= 1


def test_equal_channels_are_separate_pcm(ctx_spread):
    """Two channels with the same samples: the mix is the channel (the mean of x and x is x), every table is the same table, and
    S Z + 0 conj(Z[N - q]) must be the mix kernel's g Z byte for byte."""
    sr, ch, fmt = K.MAIN_CASE
    x0 = _rec(sr, ch, fmt)[2][:, 0:1]
    rec = T._pack(np.ascontiguousarray(np.repeat(x0, 2, axis=1)), fmt, sr)
    data, info, x, _ = rec
    assert np.array_equal(x[:, 0], x[:, 1]) and np.array_equal(x[:, 0], x0[:, 0])
    ctx_spread.reset()
    fid = ctx_spread.add_pcm(*_args(rec, sr))
    mix_sig = ctx_spread.read_signal(fid)
    ctx_spread.reset()
    first = ctx_spread.add_pcm_channels(*_args(rec, sr))
    assert np.array_equal(mix_sig, ctx_spread.read_signal(first)) and np.array_equal(mix_sig, ctx_spread.read_signal(first + 1))
    a = ctx_spread.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS)
    b = ctx_spread.separate_pcm(*_args(rec, sr), T.B1_REGIONS)
    plain = ctx_spread.silence_pcm(*_args(rec, sr), [])
    assert a.tobytes() == b.tobytes() and not np.array_equal(a, plain)


# ---- cuts ----------------------------------------------------------------------------------------------------------------------
def test_passes_cut_inside_the_channels_give_the_one_pass_bytes(native, heads, ctx_spread):
    """3 channels x 10 windows at 7 windows per pass: five passes whose cuts fall inside channels 0, 1 and 2 (and a pass that holds
    the end of one channel and the start of the next); the float64 sums carried through memory give the one-pass bytes."""
    sr, ch, fmt = 16000, 3, "pcm16"
    rec = _rec(sr, ch, fmt)
    nw = native.separation_plan(sr, rec[1].frames, T.B1_REGIONS)["windows_run"]
    assert nw > 7 and nw % 7 != 0
    small = T._head_ctx(native, heads["spread"], chunk=7, profile=True)
    try:
        small.reset_stats()
        a = small.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS)
        st = {k["name"]: k["launches"] for k in small.kernel_stats()}
        assert st.get("sep_accumulate_kernel") == -(-ch * nw // 7), st
        maps_small = [small.separation_maps(c, 300, 200) for c in range(ch)]
    finally:
        small.close()
    b = ctx_spread.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS)
    assert a.tobytes() == b.tobytes()
    for c in range(ch):
        assert np.array_equal(maps_small[c], ctx_spread.separation_maps(c, 300, 200))


def test_kernel_statistics_one_pass_one_accumulate_and_the_each_form_only(native, ctx_spread):
    sr, ch, fmt = K.MAIN_CASE
    rec = _rec(sr, ch, fmt)
    nw = native.separation_plan(sr, rec[1].frames, T.B1_REGIONS)["windows_run"]
    assert 2 * nw <= 1024                                                      # both channels' windows fit one pass of the default chunk
    ctx_spread.reset_stats()
    ctx_spread.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS)
    st = {k["name"]: k["launches"] for k in ctx_spread.kernel_stats()}
    assert st.get("sep_accumulate_kernel") == 1 and st.get("sep_finalize_kernel") == 1, st
    assert st.get("sep_stft_each_kernel<1024>", 0) >= 1 and st.get("sep_blend_kernel", 0) >= 1, st
    assert not [k for k in st if k.startswith("sep_stft_kernel")], st
    ctx_spread.reset_stats()
    ctx_spread.separate_pcm(*_args(rec, sr), T.B1_REGIONS)
    st = {k["name"]: k["launches"] for k in ctx_spread.kernel_stats()}
    assert st.get("sep_stft_kernel<1024>", 0) >= 1 and st.get("sep_accumulate_kernel") == 1, st
    assert not [k for k in st if k.startswith("sep_stft_each_kernel")], st


_CUT_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from softspoken_amd import synth, native
import separation_ref as R
import test_gpu_separation as T
import test_gpu_separation_channels as TC
ctx = T._head_ctx(native, R.spread_head(synth.make_state_dict(0)))
for sr, ch, fmt in ((48000, 2, "pcm16"), (16000, 3, "pcm16")):
    rec = TC._rec(sr, ch, fmt)
    ctx.debug_set_separation_budget(0)
    r = TC._bound_case(native, ctx, "cuts %d/%d default budget" % (sr, ch), rec, sr, T.B1_REGIONS)
    hop = r["plan"]["hop"]
    for budget in (16, 17, 23):
        ctx.debug_set_separation_budget(budget)
        got = ctx.separate_pcm_channels(*TC._args(rec, sr), T.B1_REGIONS)
        bad = np.flatnonzero((got != r["got"]).any(axis=1))
        assert bad.size == 0, (sr, ch, budget, bad[:8])
        assert (1.6 - 0.9) * sr > 2 * (budget - 8) * hop                # the merged interval takes more than two pieces
print("CUTS_OK")
"""


def test_every_cut_alignment_gives_the_same_bytes(build_all):
    """ss_debug_set_separation_budget (development build) at 16, 17 and 23 frames -- pieces of 8, 9 and 15 hops, several chunks per
    call -- gives the default budget's bytes, which pass the bound."""
    import subprocess, sys
    from softspoken_amd import build as hip_build
    tests = os.path.dirname(os.path.abspath(__file__))
    e = dict(os.environ); e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
    r = subprocess.run([sys.executable, "-c", _CUT_SCRIPT.format(root=os.path.dirname(tests), tests=tests)], env=e, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "CUTS_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


# ---- behaviour -----------------------------------------------------------------------------------------------------------------
def test_two_calls_identical_one_reset_each_files_are_the_channels(native, ctx_spread):
    sr, ch, fmt = 16000, 3, "pcm16"
    rec = _rec(sr, ch, fmt)
    plan, first, by_win = _channel_maps(native, ctx_spread, rec, sr, T.B1_REGIONS)
    g0 = ctx_spread.reset_generation()
    a = ctx_spread.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS, fade_s=0.02, min_gain=0.1)
    assert ctx_spread.reset_generation() == g0 + 1
    b = ctx_spread.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS, fade_s=0.02, min_gain=0.1)
    assert ctx_spread.reset_generation() == g0 + 2 and a.tobytes() == b.tobytes()
    # files 0 .. C - 1 are the channels: their signals, and their maps equal the average of the device's own spec outputs bit for bit
    ctx_spread.reset()
    f2 = ctx_spread.add_pcm_channels(*_args(rec, sr))
    sigs = [ctx_spread.read_signal(f2 + c) for c in range(ch)]
    ctx_spread.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS)
    rg = plan["ranges"][1]
    bins = range(rg["bin_first"], rg["bin_last"] + 1)
    for c in range(ch):
        assert np.array_equal(ctx_spread.read_signal(c), sigs[c])
        got = ctx_spread.separation_maps(c, bins[0], len(bins))
        assert got.dtype == np.float32 and np.array_equal(got, R.average_maps(by_win[c], bins)) and got.any()
    with pytest.raises((native.NativeError, ValueError)):
        ctx_spread.read_signal(ch)                                            # and no further file


def test_refusals(native, ctx_spread):
    sr, ch, fmt = K.MAIN_CASE
    rec = _rec(sr, ch, fmt)
    audio = native.Context(None, 0)
    try:
        with pytest.raises(native.NativeError) as e:
            audio.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS)
        assert e.value.code == 4                                              # SS_ERR_STATE: audio-only
    finally:
        audio.close()
    with pytest.raises(native.NativeError) as e:
        ctx_spread.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS, min_gain=2.0)
    assert e.value.code == 1
    with pytest.raises(native.NativeError) as e:
        ctx_spread.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS, speech_channel=2)
    assert e.value.code == 1


def test_a_stream_opened_before_the_call_is_untouched(native, ctx_spread):
    import test_gpu_stream as S
    from softspoken_amd import synth
    sr, ch, fmt = K.MAIN_CASE
    rec = _rec(sr, ch, fmt)
    clip = synth.to_pcm16(synth.synth_audio(31, 12.0, 16000, 1))
    pieces = [16000] * 12
    want = S.streamed(ctx_spread, clip, native.PCM_S16, 16000, 1, pieces)
    steps = []

    def on_step(sid, r, a, i):
        steps.append(len(steps))
        if len(steps) in (3, 8):
            ctx_spread.separate_pcm_channels(*_args(rec, sr), T.B1_REGIONS)
    got = S.streamed(ctx_spread, clip, native.PCM_S16, 16000, 1, pieces, on_step=on_step)
    assert len(steps) >= 9
    S.assert_same(got, want)


# ---- SilenceJob ----------------------------------------------------------------------------------------------------------------
def test_silence_job_each_mode(tmp_path, native, heads, ctx_spread, ctx_f16):
    import torch
    from root.code.backend.pytorch_neural_nets import SpecUNet_2D
    from softspoken_amd import silence, synth
    sr, ch, fmt = K.MAIN_CASE
    src = tmp_path / "in"
    src.mkdir()
    a_data, a_info, _, a_wav = _rec(sr, ch, fmt)
    (src / "a.wav").write_bytes(a_wav)
    x = (0.5 * np.ascontiguousarray(synth.synth_audio(61, 4.0, 16000, 2, with_silence=False).T.reshape(-1, 2))).astype(np.float32)
    x[16000 * 2, 1] = np.float32("nan")                                      # one channel, inside the interval: f16x2 refuses the file
    nan_wav = synth.wav_bytes(x, 16000, "f32")
    (src / "nan.wav").write_bytes(nan_wav)
    df = pd.DataFrame({"ID": [1, 2, 3], "file_path": [str(src)] * 3, "file_name": ["a.wav", "a.wav", "nan.wav"],
                       "start_time": [0.9, 1.35, 1.5], "end_time": [1.4, 1.6, 2.5], "erase": [1, 1, 1]})
    m = SpecUNet_2D(precision="f16x2")
    with torch.no_grad():
        m.load_state_dict(synth.to_torch_state_dict(heads["spread"]))
    m.eval()
    kw = dict(min_gain=0.05)
    regions_a = [(0.9, 1.4), (1.35, 1.6)]
    each_a = ctx_f16.separate_pcm_channels(a_data, a_info.format, sr, ch, a_info.frames, regions_a, **kw)
    mix_a = ctx_f16.separate_pcm(a_data, a_info.format, sr, ch, a_info.frames, regions_a, **kw)
    assert not np.array_equal(each_a, mix_a)
    n_info = native.wav_parse(nan_wav)
    n_data = np.frombuffer(nan_wav, dtype=np.uint8, count=n_info.data_bytes, offset=n_info.data_offset)
    with pytest.raises(native.NativeError) as e:
        ctx_f16.separate_pcm_channels(n_data, n_info.format, 16000, 2, n_info.frames, [(1.5, 2.5)], **kw)
    assert e.value.code == native.SS_ERR_RANGE
    each_n = ctx_spread.separate_pcm_channels(n_data, n_info.format, 16000, 2, n_info.frames, [(1.5, 2.5)], **kw)

    out = tmp_path / "each"
    out.mkdir()
    job = silence.SilenceJob(df, str(out), method="separate", model=m, channel_mode="each", **kw)
    paths = job.run()
    assert sorted(os.listdir(out)) == ["a_silenced.wav", "nan_silenced.wav"] and not job.errors and len(paths) == 2
    assert (out / "a_silenced.wav").read_bytes() == native.wav_header_pcm16(sr, ch, a_info.frames) + each_a.tobytes()
    assert (out / "nan_silenced.wav").read_bytes() == native.wav_header_pcm16(16000, 2, n_info.frames) + each_n.tobytes()
    assert m.effective_precision() == "f16x2"                                  # one refused input: run on the fp32 side context

    # no mode given: the detector's setting, whose shipped default is the mix -- the bytes this job wrote before
    from root.code.backend import voice_activity
    want = mix_a if voice_activity.channel_mode() == "mix" else each_a
    out2 = tmp_path / "default"
    out2.mkdir()
    job = silence.SilenceJob(df[df["file_name"] == "a.wav"], str(out2), method="separate", model=m, **kw)
    job.run()
    assert not job.errors
    assert (out2 / "a_silenced.wav").read_bytes() == native.wav_header_pcm16(sr, ch, a_info.frames) + want.tobytes()
