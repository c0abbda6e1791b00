"""Per-channel separation (ss_separate_pcm_channels) without a GPU: the conditions on the inputs of test_gpu_separation_channels.py's
cases, met with the fp32 CPU oracle in the device's place (as test_separation_host.py does for the mix), the export, and SilenceJob's
routing by channel mode with a fake model and context."""
import os

import numpy as np
import pandas as pd
import pytest

import separation_channels_cases as K
import separation_ref as R


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


@pytest.fixture(scope="module")
def oracle_channels(native, sd_np):
    """get(head, sr, ch, fmt) -> (x, plan, maps): the case's recording, its plan and the oracle's per-window spec maps of the plan's
    windows, maps[c] for channel c run alone (ss_add_pcm_channels' signal: the channel's samples resampled, no mixdown) and maps["mix"]
    for the mixdown (ss_add_pcm's)."""
    import test_gpu_separation as T
    from oracle import oracle_np as O
    heads = dict(spread=R.spread_head(sd_np), mixed=R.mixed_head(sd_np))
    cache = {}

    def get(head, sr, ch, fmt, mix=False):
        key = (head, sr, ch, fmt)
        if key not in cache:
            _, info, x, _ = T._make(fmt, sr, ch, T.B1_SECONDS, T.B1_SEED, scale=0.5)
            plan = native.separation_plan(sr, info.frames, T.B1_REGIONS)
            cache[key] = (x, plan, {})
        x, plan, maps = cache[key]
        wins = K.plan_windows(plan)
        for c in list(range(ch)) + (["mix"] if mix else []):
            if c not in maps:
                sig = O.resample(O.to_mono(x) if c == "mix" else x[:, c], sr)
                spec = R._oracle_spec(heads[head], O.pad_3s(sig), wins)
                maps[c] = {w: spec[t] for t, w in enumerate(wins)}
        return x, plan, maps
    return get


def _check_head(head, sr, ch, fmt, get, **params):
    x, plan, maps = get(head, sr, ch, fmt)
    assert plan["n_fft"] == K.N_FFT[sr] and len(plan["ranges"]) == 4
    Gs = [K.interval_gains(plan, maps[c], params.get("speech_channel", 1), params.get("min_gain", 0.0)) for c in range(ch)]
    for c in range(ch):                                                       # every channel on its own is a good parity case
        st = R.gain_stats(Gs[c])
        print(head, sr, ch, fmt, "channel", c, st)
        (R.assert_spread if head == "spread" else R.assert_mixed)(st)
    for a in range(ch):                                                       # and no two channels share their gains
        for b in range(a + 1, ch):
            d = K.pair_distance(Gs[a], Gs[b])
            print(head, sr, ch, fmt, "pair", a, b, f"mean |Ga - Gb| = {d:.3f}")
            assert d >= K.PAIR_DISTANCE, (sr, ch, a, b, d)


@pytest.mark.parametrize("sr,ch,fmt", K.BOUND_CASES + [K.MONO_CASE])
def test_bound_cases_have_distinct_spread_gains_per_channel(oracle_channels, sr, ch, fmt):
    _check_head("spread", sr, ch, fmt, oracle_channels)


@pytest.mark.parametrize("sr,ch,fmt", K.MIXED_CASES)
def test_mixed_cases_have_distinct_mixed_gains_per_channel(oracle_channels, sr, ch, fmt):
    _check_head("mixed", sr, ch, fmt, oracle_channels)


def test_main_case_meets_the_conditions_under_the_parameter_set(oracle_channels):
    """MAIN_CASE with the spread head: the f16x2 context's case, the cuts', the behaviour's, the equal-channels file's (its two
    channels are this recording's channel 0: the pair distance does not apply to it) -- and under PARAMS (the other orientation of
    the head, a floor of 0.1)."""
    _check_head("spread", *K.MAIN_CASE, oracle_channels)
    _check_head("spread", *K.MAIN_CASE, oracle_channels, **K.PARAMS)


@pytest.mark.parametrize("sr,ch,fmt", K.SWAP_CASES)
def test_the_gain_a_channel_gets_matters(oracle_channels, sr, ch, fmt):
    """A channel separated with another channel's maps, or with the mix's (what ss_separate_pcm gives it), lies far from the channel
    separated with its own: more than 2 LSB on at least half the interval samples -- 4 times the whole bound of the GPU cases."""
    import test_gpu_separation as T
    x, plan, maps = oracle_channels("spread", sr, ch, fmt, mix=True)
    m = T._mask(len(x), sr, T.B1_REGIONS)
    assert m.sum() > 0.4 * len(x)
    for c in range(ch):
        xc = x[:, c:c + 1]
        own = R.separate(xc, sr, T.B1_REGIONS, maps[c], unrounded=True)[1]
        for other in [d for d in range(ch) if d != c] + ["mix"]:
            y = R.separate(xc, sr, T.B1_REGIONS, maps[other], unrounded=True)[1]
            share = K.moved_share(own, y, m)
            d = np.abs(own - y)[m]
            print(f"{sr}/{ch} channel {c} with the maps of {other}: > {K.SWAP_LSB} LSB on {100 * share:.1f} %, median {np.median(d):.1f} LSB")
            assert share >= K.SWAP_SHARE, (sr, c, other, share)


def test_the_export_is_declared_and_bound(native):
    hdr = open(os.path.join(os.path.dirname(native.__file__), "..", "include", "softspoken.h")).read()
    name = "ss_separate_pcm_channels"
    assert name in native.EXPORTS and name + "(" in hdr and getattr(native.lib(), name) is not None
    assert native.lib().ss_abi_version() == 3 == native.ABI_VERSION
    assert callable(native.Context.separate_pcm_channels)
    import inspect
    a, b = inspect.signature(native.Context.separate_pcm_channels), inspect.signature(native.Context.separate_pcm)
    assert list(a.parameters.items()) == list(b.parameters.items())


# ---- SilenceJob's routing ------------------------------------------------------------------------------------------------------
class _Ctx:
    def __init__(self, log):
        self.log = log

    def _out(self, name, channels, frames, kw):
        self.log.append((name, channels, kw))
        return np.full((frames, channels), len(self.log), dtype=np.int16)

    def separate_pcm(self, pcm, fmt, sr, channels, frames, regions, **kw):
        return self._out("mix", channels, frames, kw)

    def separate_pcm_channels(self, pcm, fmt, sr, channels, frames, regions, **kw):
        return self._out("each", channels, frames, kw)

    def silence_pcm(self, pcm, fmt, sr, channels, frames, regions):
        return self._out("zero", channels, frames, {})


class _Model:
    def __init__(self):
        self.log, self.keys = [], []

    def with_range_fallback(self, fn, key=None):
        self.keys.append(key)
        return fn(_Ctx(self.log))


@pytest.fixture()
def review(tmp_path, native):
    from softspoken_amd import synth
    src = tmp_path / "in"
    src.mkdir()
    (tmp_path / "out").mkdir()
    rng = np.random.default_rng(5)
    for name, ch in (("stereo.wav", 2), ("mono.wav", 1)):
        pcm = rng.integers(-3000, 3000, size=(4000, ch)).astype(np.int16)
        (src / name).write_bytes(synth.wav_bytes(pcm[:, 0] if ch == 1 else pcm, 8000))
    df = pd.DataFrame({"ID": [1, 2], "file_path": [str(src)] * 2, "file_name": ["stereo.wav", "mono.wav"], "start_time": [0.1, 0.2],
                       "end_time": [0.3, 0.4], "erase": [1, 1]})
    return df, str(tmp_path / "out")


def _routes(review, monkeypatch, setting=None, **kw):
    """{file name: entry point} of one job."""
    from root.code.backend import settings
    from softspoken_amd import silence
    df, out = review
    if setting is not None:
        monkeypatch.setattr(settings, "hip_channel_mode", setting, raising=False)
    m = _Model()
    ctx = _Ctx(m.log)
    job = silence.SilenceJob(df, out, ctx=ctx, model=m, **kw)
    paths = job.run()
    assert not job.errors and len(paths) == 2 == len(m.log)
    by_ch = {2: "stereo.wav", 1: "mono.wav"}
    if kw.get("method") == "separate":
        assert all(k[0] == "separate" for k in m.keys) and all(e[2] == job.sep_params for e in m.log)
    return {by_ch[e[1]]: e[0] for e in m.log}


def test_silence_job_routes_by_channel_mode(review, monkeypatch):
    assert _routes(review, monkeypatch, method="separate", channel_mode="each") == {"stereo.wav": "each", "mono.wav": "mix"}
    assert _routes(review, monkeypatch, method="separate", channel_mode="mix") == {"stereo.wav": "mix", "mono.wav": "mix"}
    # None: the detector's setting, whose shipped default is mix
    assert _routes(review, monkeypatch, setting="mix", method="separate") == {"stereo.wav": "mix", "mono.wav": "mix"}
    assert _routes(review, monkeypatch, setting="each", method="separate") == {"stereo.wav": "each", "mono.wav": "mix"}
    assert _routes(review, monkeypatch, setting="each", method="separate", channel_mode="mix") == {"stereo.wav": "mix", "mono.wav": "mix"}
    for mode in (None, "mix", "each"):                                           # the zeroing silencer has no use for the mode
        assert _routes(review, monkeypatch, setting="each", method="zero", channel_mode=mode) == {"stereo.wav": "zero", "mono.wav": "zero"}


def test_silence_job_refuses_an_unknown_channel_mode(review):
    from softspoken_amd import silence
    df, out = review
    for method in ("zero", "separate"):
        for bad in ("both", "", "EACH", 1):
            with pytest.raises(ValueError):
                silence.SilenceJob(df, out, method=method, model=_Model(), channel_mode=bad)
    with pytest.raises(ValueError):
        silence.silence_files(df, out, method="separate", model=_Model(), channel_mode="all")


def test_the_shipped_default_mode_is_mix():
    from root.code.backend import voice_activity
    if "SOFTSPOKEN_CHANNELS" not in os.environ:
        assert voice_activity.channel_mode() == "mix"
