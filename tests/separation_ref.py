"""float64 numpy statement of the separation silencer (include/softspoken.h "separation silencer"), steps 1-4,
for the tests: test_separation_host.py checks its STFT round trip on the CPU, test_gpu_separation.py holds the device to it.

Not imported by the library.  Every function takes plain numpy arrays; the per-window spec-head outputs come from the caller (the
device's ss_infer_windows in the GPU tests)."""
from __future__ import annotations

import math

import numpy as np

WIN_STEP = 13230
WIN_LEN = 66150


def fft_size(sr: int) -> int:
    e = round(math.log2(sr * 512 / 22050))
    return 1 << min(13, max(8, e))


def merged_intervals(regions, sr: int, frames: int):
    """silence_ranges (host.hip): Python round of start / end times sr, clamped to the file, sorted, overlaps merged."""
    r = []
    for s, e in regions:
        a, b = float(s) * sr, float(e) * sr
        if a != a or b != b:
            continue
        lo, hi = min(max(round(a), 0), frames), min(max(round(b), 0), frames)
        if hi > lo:
            r.append((lo, hi))
    out = []
    for lo, hi in sorted(r):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [tuple(x) for x in out]


def win_start(i: int) -> int:
    return (512 * i + 5) // 10


def file_geometry(sr: int, frames: int):
    """(W, n_bins): windows of ss_run's plan and the bins 0 .. n_bins - 1 that have a window."""
    n22 = -(-frames * 22050 // sr)
    n_padded = n22 + 2 * WIN_LEN
    L = round(frames / sr * 22050.0) + 6.0 * 22050.0
    W = max(0, math.ceil((L - 66150.0) / 13230.0))
    while W > 0 and (W - 1) * WIN_STEP + WIN_LEN > n_padded:
        W -= 1
    nb = round(n_padded / 22050.0 * 256.0 / 3.0)
    return W, min(nb, win_start(W - 1) + 256)


def frame_bins(k: int, hop: int, sr: int, n_bins: int):
    """Bins j0, j1 around frame k's time and the weight of j1 (exact: u = (512 (k hop + 3 sr) - 3 sr) / (6 sr)), clamped."""
    num, den = 512 * (k * hop + 3 * sr) - 3 * sr, 6 * sr
    j0 = num // den
    alpha = (num - j0 * den) / den
    if j0 < 0:
        return 0, 0, 0.0
    if j0 >= n_bins - 1:
        return n_bins - 1, n_bins - 1, 0.0
    return j0, j0 + 1, alpha


def frame_range(a: int, b: int, N: int):
    hop = N // 4
    return (a - N // 2) // hop + 1, -((-(b + N // 2)) // hop) - 1


def average_maps(spec_by_window: dict, bins) -> np.ndarray:
    """Step 1: [2][len(bins)][128] float32 averages of spec_by_window[i] ([2][128][256]) over the windows covering each bin, a float64
    sum in ascending window order divided by the count."""
    out = np.zeros((2, len(bins), 128), dtype=np.float32)
    for t, j in enumerate(bins):
        s = np.zeros((2, 128), dtype=np.float64)
        n = 0
        for i in sorted(spec_by_window):
            d = j - win_start(i)
            if 0 <= d < 256:
                s = s + spec_by_window[i][:, :, d].astype(np.float64)
                n += 1
        assert n > 0, j
        out[:, t, :] = (s / n).astype(np.float32)
    return out


def log_power(y) -> np.ndarray:
    a = np.asarray(y, dtype=np.float64) ** 2 * math.log(10.0)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        lp = np.where(a > 30.0, a + np.log1p(-np.exp(-np.minimum(a, 745.0))), np.log(np.expm1(np.minimum(a, 30.0))))
    return np.where(a == 0.0, -np.inf, lp)


def band_gains(maps: np.ndarray, speech_channel: int = 1, min_gain: float = 0.0) -> np.ndarray:
    """Step 2: [n_bins][128] G' = max(P_env / (P_env + P_speech), min_gain) from float32 maps [2][n_bins][128]."""
    le, ls = log_power(maps[1 - speech_channel]), log_power(maps[speech_channel])
    with np.errstate(over="ignore", invalid="ignore"):
        g = 1.0 / (1.0 + np.exp(ls - le))
    g = np.where((le == -np.inf) & (ls == -np.inf), 1.0, g)
    return np.fmax(g, min_gain)


def mel_points() -> np.ndarray:
    """The front-end's HTK mel points (torchaudio's recipe in float32, weights.hip build_tables) as float64."""
    mmax = np.float32(2595.0 * math.log10(1.0 + 8000.0 / 700.0))
    step = np.float32(mmax / np.float32(129.0))
    f = np.zeros(130)
    for i in range(130):
        mp = np.float32(step * np.float32(i)) if i < 65 else np.float32(mmax - np.float32(step * np.float32(129 - i)))
        f[i] = float(np.float32(np.float32(700.0) * (np.float32(np.power(np.float32(10.0), np.float32(mp / np.float32(2595.0)))) - np.float32(1.0))))
    return f


def freq_weights(N: int, sr: int) -> np.ndarray:
    """[N/2 + 1][128] weights T_m(f) / sum_m T_m(f) of STFT bin f = q sr / N (row 0: band 0; rows at >= 8 kHz: all zero)."""
    fp = mel_points()
    wts = np.zeros((N // 2 + 1, 128))
    for q in range(N // 2 + 1):
        f = q * sr / N
        if f >= 8000.0:
            continue
        if q == 0:
            wts[q, 0] = 1.0
            continue
        T = np.maximum(0.0, np.minimum((f - fp[:128]) / (fp[1:129] - fp[:128]), (fp[2:130] - f) / (fp[2:130] - fp[1:129])))
        if T.sum() == 0.0:
            wts[q, 127 if f >= fp[128] else 0] = 1.0
        else:
            wts[q] = T / T.sum()
    return wts


def resynth(x: np.ndarray, sr: int, a: int, b: int, gain_of_frame) -> np.ndarray:
    """Step 3 for one interval: p[b - a][ch] (float64), gain_of_frame(k) -> [N/2 + 1] real gains."""
    frames, ch = x.shape
    N = fft_size(sr)
    hop = N // 4
    n = np.arange(N)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N)
    k0, k1 = frame_range(a, b, N)
    lo = k0 * hop - N // 2
    acc = np.zeros(((k1 - k0) * hop + N, ch))
    for k in range(k0, k1 + 1):
        idx = k * hop - N // 2 + n
        ok = (idx >= 0) & (idx < frames)
        seg = np.zeros((N, ch))
        seg[ok] = x[idx[ok]].astype(np.float64)
        X = np.fft.rfft(seg * w[:, None], axis=0)
        y = np.fft.irfft(X * gain_of_frame(k)[:, None], n=N, axis=0)
        acc[idx[0] - lo: idx[0] - lo + N] += y * w[:, None] / 1.5
    return acc[a - lo: b - lo]


def fade_weights(a: int, b: int, F: int) -> np.ndarray:
    n = np.arange(a, b)
    d = np.minimum(n - a, b - 1 - n).astype(np.float64)
    if F <= 0:
        return np.ones(b - a)
    return np.where(d < F, 0.5 - 0.5 * np.cos(np.pi * (d + 0.5) / F), 1.0)


def separate(x: np.ndarray, sr: int, regions, spec_by_window: dict, fade_s: float = 0.01, min_gain: float = 0.0,
             above_fmax: str = "mute", speech_channel: int = 1) -> np.ndarray:
    """Steps 1-4: x float32 (frames, ch) as decode_pcm gives it, spec_by_window {window i: [2][128][256]} for (at least) every window
    that covers a needed bin -> int16 (frames, ch)."""
    frames, ch = x.shape
    N = fft_size(sr)
    hop = N // 4
    W, n_bins = file_geometry(sr, frames)
    fw = freq_weights(N, sr)
    hi = fw.sum(axis=1) == 0.0
    gain_hi = 1.0 if above_fmax == "keep" else min_gain
    y = (x.astype(np.float32) * np.float32(32767.0)).astype(np.float32)
    out = np.rint(y).astype(np.int64).astype(np.int16)
    F = round(fade_s * sr)
    for a, b in merged_intervals(regions, sr, frames):
        k0, k1 = frame_range(a, b, N)
        j_lo, j_hi = frame_bins(k0, hop, sr, n_bins)[0], frame_bins(k1, hop, sr, n_bins)[1]
        bins = list(range(j_lo, j_hi + 1))
        G = band_gains(average_maps(spec_by_window, bins), speech_channel, min_gain)

        def gain_of_frame(k):
            j0, j1, al = frame_bins(k, hop, sr, n_bins)
            gt = (1.0 - al) * G[j0 - j_lo] + al * G[j1 - j_lo]
            g = fw @ gt
            g[hi] = gain_hi
            return g

        p = resynth(x, sr, a, b, gain_of_frame)
        xs = x[a:b].astype(np.float64)
        wv = fade_weights(a, b, F)[:, None]
        ys = xs + wv * (p - xs)
        out[a:b] = np.rint(ys * 32767.0).astype(np.int64).astype(np.int16)
    return out
