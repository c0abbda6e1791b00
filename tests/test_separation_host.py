"""The separation silencer's host side (ss_separation_plan, no GPU) against a brute-force reading of its definition
(include/softspoken.h "separation silencer"), and the float64 reference of tests/separation_ref.py: its STFT -> ISTFT round trip."""
from fractions import Fraction

import numpy as np
import pytest

import separation_ref as R


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


@pytest.mark.parametrize("sr,n_fft", [(8000, 256), (16000, 512), (22050, 512), (44100, 1024), (48000, 1024), (96000, 2048),
                                      (192000, 4096), (768000, 8192)])
def test_plan_fft_size(native, sr, n_fft):
    p = native.separation_plan(sr, sr * 2, [(0.5, 1.0)])
    assert (p["n_fft"], p["hop"]) == (n_fft, n_fft // 4)
    assert R.fft_size(sr) == n_fft


def _brute_plan(sr, frames, regions):
    """Every quantity straight from the definition: sample sets, frame supports, exact bin times, every window."""
    N = R.fft_size(sr)
    hop = N // 4
    W, n_bins = R.file_geometry(sr, frames)
    covered = np.zeros(n_bins + 300, dtype=bool)
    for i in range(W):
        covered[R.win_start(i):R.win_start(i) + 256] = True
    assert covered[:n_bins].all() and not covered[n_bins:].any()
    mask = np.zeros(frames, dtype=bool)
    for s, e in regions:
        a, b = s * sr, e * sr
        if a != a or b != b:
            continue
        mask[max(0, min(round(a), frames)):max(0, min(round(b), frames))] = True
    edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
    out = []
    for a, b in zip(edges[0::2], edges[1::2]):
        a, b = int(a), int(b)
        ks = [k for k in range((a - N) // hop - 2, (b + N) // hop + 3) if k * hop - N // 2 < b and k * hop + N // 2 > a]
        bins = set()
        for k in ks:
            u = (Fraction(k * hop, sr) + 3) * Fraction(256, 3) - Fraction(1, 2)       # position among the bin centres
            j0 = u.numerator // u.denominator                                           # floor
            if j0 < 0:
                bins.add(0)
            elif j0 >= n_bins - 1:
                bins.add(n_bins - 1)
            else:
                bins.update((j0, j0 + 1))
        wins = [i for i in range(W) if any(0 <= j - R.win_start(i) < 256 for j in bins)]
        out.append(dict(frame_begin=a, frame_end=b, stft_first=min(ks), stft_last=max(ks), bin_first=min(bins), bin_last=max(bins),
                        win_first=min(wins), win_last=max(wins)))
        assert wins == list(range(min(wins), max(wins) + 1)) and sorted(bins) == list(range(min(bins), max(bins) + 1))
    run = set()
    for r in out:
        run.update(range(r["win_first"], r["win_last"] + 1))
    return dict(n_fft=N, hop=hop, n_windows=W, n_bins=n_bins, windows_run=len(run), ranges=out)


@pytest.mark.parametrize("sr,seconds,regions", [
    (48000, 20.0, [(12.0, 13.5), (1.0, 2.0), (1.5, 3.25), (-5.0, 0.3), (19.2, 40.0), (7.0, 7.0), (8.0, 7.5), (5.0, 5.00001)]),
    (16000, 7.3, [(0.0, 7.3), (3.0, 4.0)]),
    (8000, 3.0, [(0.001, 0.002), (2.99, 3.0)]),
    (44100, 61.7, [(t, t + 0.37) for t in np.arange(0.0, 62.0, 2.9)]),
    (96000, 4.0, [(0.2, 0.21), (0.215, 0.3), (3.9, 9.0)]),
    (22050, 12.0, [(6.0, 6.5), (6.6, 7.0), (float("nan"), 1.0)]),
    (768000, 0.4, [(0.1, 0.2)]),
    (11025, 0.0, [(0.0, 1.0)]),
])
def test_plan_matches_brute_force(native, sr, seconds, regions):
    frames = int(round(seconds * sr))
    got = native.separation_plan(sr, frames, regions)
    assert got == _brute_plan(sr, frames, regions)


def test_plan_errors(native):
    for kw in (dict(speech_channel=2), dict(speech_channel=-1), dict(fade_s=-0.001), dict(fade_s=float("nan")), dict(min_gain=-0.1),
               dict(min_gain=1.5), dict(min_gain=float("nan")), dict(above_fmax=2), dict(above_fmax=-1)):
        with pytest.raises(native.NativeError) as e:
            native.separation_plan(48000, 48000, [(0.1, 0.2)], **kw)
        assert e.value.code == 1, kw                                          # SS_ERR_ARG
    for kw in (dict(), dict(speech_channel=0, fade_s=0.0, min_gain=1.0, above_fmax="keep"), dict(min_gain=0.0, above_fmax=0)):
        native.separation_plan(48000, 48000, [(0.1, 0.2)], **kw)
    with pytest.raises(native.NativeError) as e:
        native.separation_plan(0, 48000, [])
    assert e.value.code == 1


def test_reference_stft_roundtrip():
    """All gains 1: the float64 STFT -> ISTFT of the reference gives back the signal (Hann^2 at hop N/4 sums to 1.5 everywhere)."""
    rng = np.random.default_rng(3)
    for sr, ch in ((48000, 2), (8000, 1), (96000, 3), (22050, 1)):
        frames = int(0.8 * sr)
        x = rng.uniform(-1, 1, size=(frames, ch)).astype(np.float32)
        N = R.fft_size(sr)
        for a, b in ((0, frames), (0, 17), (frames // 3, frames // 2), (frames - 5, frames)):
            p = R.resynth(x, sr, a, b, lambda k: np.ones(N // 2 + 1))
            assert p.shape == (b - a, ch)
            assert np.abs(p - x[a:b].astype(np.float64)).max() <= 1e-12


def test_reference_gains():
    y = np.array([0.0, 1e-30, 0.3, 2.0, 30.0, 3e19], dtype=np.float32)
    maps = np.stack([np.repeat(y[:, None], 128, 1)[None, :, :][0], np.zeros((6, 128), np.float32)])    # env = y, speech = 0
    g = R.band_gains(maps, speech_channel=1)
    assert np.array_equal(g, np.ones_like(g))
    g = R.band_gains(maps[::-1].copy(), speech_channel=1)                                              # speech = y, env = 0
    assert g[0, 0] == 1.0 and (g[1:] == 0.0).all()
    m = np.stack([np.full((1, 128), 3e19, np.float32), np.full((1, 128), 3e19, np.float32)])
    assert np.allclose(R.band_gains(m), 0.5) and np.isfinite(R.band_gains(m)).all()
    m = np.stack([np.full((1, 128), 0.5, np.float32), np.full((1, 128), 0.5, np.float32)])
    assert np.allclose(R.band_gains(m, min_gain=0.7), 0.7)
    w = R.freq_weights(1024, 48000)
    assert np.allclose(w.sum(axis=1)[: int(8000 * 1024 / 48000) + 1], 1.0) and not w[int(np.ceil(8000 * 1024 / 48000)):].any()


# ---- the unrounded output, the float32 restatement and the crafted heads (CPU oracle only) -------------------------------------
def _random_case(sr, ch, seconds, seed):
    """A recording, regions and per-window maps from a seeded generator (no network): enough for the reference's own arithmetic."""
    rng = np.random.default_rng(seed)
    frames = int(seconds * sr)
    x = rng.uniform(-0.5, 0.5, size=(frames, ch)).astype(np.float32)
    W, _ = R.file_geometry(sr, frames)
    base = rng.uniform(0.0, 1.2, size=(2, 128, 256 + 52 * W))
    by_win = {i: np.maximum(base[:, :, R.win_start(i):R.win_start(i) + 256] - 0.2, 0.0).astype(np.float32) for i in range(W)}
    return x, [(-1.0, 0.11), (0.3, 0.3 + 1.0 / sr), (0.5, 0.74), (0.7, 0.8), (seconds - 0.1, 99.0)], by_win


# sha256 of separate()'s int16 bytes as it stood before it learnt to return the unrounded output, on _random_case's inputs
_BEFORE = {(48000, 2): "29054345f876556921bae8c80e6c3f0f29600770ca45bff307d9c291f227b12a", (8000, 1): "1634bd9aa4ee26e649adb6af93049fd7c92fa76083469f180d4be370efe2390b", (96000, 3): "7dcc6903948e708dc8ec074cf0c3f0ad1ea9264fa94c693f93e9973e37762fbc"}


@pytest.mark.parametrize("sr,ch", list(_BEFORE))
def test_unrounded_output_rounds_to_the_int16_output(sr, ch):
    import hashlib
    x, regions, by_win = _random_case(sr, ch, 1.0, 7)
    kw = dict(fade_s=0.02, min_gain=0.05, above_fmax="keep")
    out = R.separate(x, sr, regions, by_win, **kw)
    out2, y64 = R.separate(x, sr, regions, by_win, unrounded=True, **kw)
    assert out.dtype == np.int16 and np.array_equal(out, out2)
    assert hashlib.sha256(out.tobytes()).hexdigest() == _BEFORE[(sr, ch)]
    assert y64.dtype == np.float64 and np.array_equal(np.rint(y64).astype(np.int64).astype(np.int16), out)
    m = np.zeros(len(x), dtype=bool)
    for a, b in R.merged_intervals(regions, sr, len(x)):
        m[a:b] = True
    assert np.array_equal(y64[~m], (x[~m] * np.float32(32767.0)).astype(np.float64))        # outside: the float32 transcode's value
    y32 = R.separate_f32(x, sr, regions, by_win, **kw)
    assert y32.dtype == np.float32 and np.array_equal(y32[~m].astype(np.float64), y64[~m])
    assert 0.0 < np.abs(y32.astype(np.float64) - y64).max() <= 0.05


@pytest.fixture(scope="module")
def oracle_cases(sd_np):
    """The GPU tests' FFT-size cases (test_gpu_separation.B1_CASES) with the fp32 CPU oracle in the device's place: per case and head,
    the recording and the spec maps of the plan's windows."""
    import test_gpu_separation as T
    from softspoken_amd import native
    from oracle import oracle_np as O
    heads = dict(spread=R.spread_head(sd_np), mixed=R.mixed_head(sd_np))
    cache = {}

    def get(head, sr, ch, fmt):
        key = (head, sr, ch, fmt)
        if key not in cache:
            data, info, x, wav = T._make(fmt, sr, ch, T.B1_SECONDS, T.B1_SEED, scale=0.5)
            plan = native.separation_plan(sr, info.frames, T.B1_REGIONS)
            wins = sorted({i for r in plan["ranges"] for i in range(r["win_first"], r["win_last"] + 1)})
            sig, _, _ = O.load_audio_from_bytes(wav)
            spec = R._oracle_spec(heads[head], O.pad_3s(sig), wins)
            cache[key] = (x, {w: spec[t] for t, w in enumerate(wins)}, plan)
        return cache[key]
    return get


def test_crafted_heads_meet_their_conditions(oracle_cases):
    """Conditions on the inputs of the GPU parity cases, met by the oracle alone: the spread head's gains move with band and with time
    around 0.5; the mixed head has cells of gain exactly 0, exactly 1 and in between."""
    import test_gpu_separation as T
    for sr, ch, fmt in [c[0:1] + c[2:] for c in T.B1_CASES] + [(48000, 2, "pcm16")]:
        x, by_win, plan = oracle_cases("spread", sr, ch, fmt)
        st = R.gain_stats([R.band_gains(R.average_maps(by_win, range(r["bin_first"], r["bin_last"] + 1))) for r in plan["ranges"]])
        print("spread", sr, ch, st)
        R.assert_spread(st)
        assert st["zero"] == 0.0 and st["one"] == 0.0
    for sr, ch, fmt in ((48000, 2, "pcm16"), (8000, 1, "pcm16")):
        x, by_win, plan = oracle_cases("mixed", sr, ch, fmt)
        st = R.gain_stats([R.band_gains(R.average_maps(by_win, range(r["bin_first"], r["bin_last"] + 1))) for r in plan["ranges"]])
        print("mixed", sr, ch, st)
        R.assert_mixed(st)


def test_float32_restatement_stays_near_the_reference(oracle_cases):
    """separate_f32 (complex64 FFTs, float32 overlap-add and blend) against the unrounded float64 output on the GPU tests' cases: a
    sanity cap of 0.05 LSB (measured: 0.0008 - 0.0012), so that tau = 4 e32 of the device's bound stays far below the rounding's 0.5."""
    import test_gpu_separation as T
    for sr, n_fft, ch, fmt in T.B1_CASES:
        x, by_win, plan = oracle_cases("spread", sr, ch, fmt)
        ivs = []
        out, y64 = R.separate(x, sr, T.B1_REGIONS, by_win, unrounded=True, info=ivs)
        y32 = R.separate_f32(x, sr, T.B1_REGIONS, by_win)
        e32 = float(np.abs(y32.astype(np.float64) - y64).max())
        print(f"N={n_fft} sr={sr} ch={ch} {fmt}: e32 = {e32:.5f} LSB")
        assert plan["n_fft"] == n_fft and len(ivs) == 4 and 0.0 < e32 <= 0.05
        assert np.array_equal(np.rint(y64).astype(np.int64).astype(np.int16), out)
