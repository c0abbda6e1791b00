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
