"""float64 numpy statement of the separation silencer (include/softspoken.h "separation silencer"), steps 1-4,
for the tests: test_separation_host.py checks its STFT round trip on the CPU, test_gpu_separation.py holds the device to it.

Not imported by the library.  Every function takes plain numpy arrays; the per-window spec-head outputs come from the caller (the
device's ss_infer_windows in the GPU tests).  separate() also gives its output before the rounding, separate_f32 restates steps 3 and 4
in float32 (the yardstick of the device's bound), and spread_head / mixed_head craft the checkpoints whose gains the parity cases need."""
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


def _interval_gains(sr, frames, regions, spec_by_window, min_gain, above_fmax, speech_channel):
    """Steps 1-2 and the gain of every STFT frame, per merged interval: dicts with a, b, k0, k1, G ([bins][128] band gains G'), g
    ([k1 - k0 + 1][N/2 + 1] float64 gains of the STFT bins) and clamp_lo / clamp_hi (a frame's time lay before the first / from the
    last bin that has a window on)."""
    N = fft_size(sr)
    hop = N // 4
    W, n_bins = file_geometry(sr, frames)
    fw = freq_weights(N, sr)
    hi = fw.sum(axis=1) == 0.0
    gain_hi = 1.0 if above_fmax == "keep" else min_gain
    out = []
    for a, b in merged_intervals(regions, sr, frames):
        k0, k1 = frame_range(a, b, N)
        j_lo, j_hi = frame_bins(k0, hop, sr, n_bins)[0], frame_bins(k1, hop, sr, n_bins)[1]
        bins = list(range(j_lo, j_hi + 1))
        G = band_gains(average_maps(spec_by_window, bins), speech_channel, min_gain)
        g = np.empty((k1 - k0 + 1, N // 2 + 1))
        lo = hi_c = False
        for k in range(k0, k1 + 1):
            j0, j1, al = frame_bins(k, hop, sr, n_bins)
            num = 512 * (k * hop + 3 * sr) - 3 * sr
            lo, hi_c = lo or num < 0, hi_c or num // (6 * sr) >= n_bins - 1
            gt = (1.0 - al) * G[j0 - j_lo] + al * G[j1 - j_lo]
            g[k - k0] = fw @ gt
            g[k - k0, hi] = gain_hi
        out.append(dict(a=a, b=b, k0=k0, k1=k1, G=G, g=g, clamp_lo=lo, clamp_hi=hi_c))
    return out


def separate(x: np.ndarray, sr: int, regions, spec_by_window: dict, fade_s: float = 0.01, min_gain: float = 0.0,
             above_fmax: str = "mute", speech_channel: int = 1, unrounded: bool = False, info: list | None = None):
    """Steps 1-4: x float32 (frames, ch) as decode_pcm gives it, spec_by_window {window i: [2][128][256]} for (at least) every window
    that covers a needed bin -> int16 (frames, ch).  unrounded: -> (int16, float64 (frames, ch)), the second being the output before
    its rounding, in LSB: 32767 ys inside the intervals, the float32 transcode x * 32767 outside.  info (a list) receives
    _interval_gains' dicts: the gains this call used."""
    frames, ch = x.shape
    y = (x.astype(np.float32) * np.float32(32767.0)).astype(np.float32)
    out = np.rint(y).astype(np.int64).astype(np.int16)
    y64 = y.astype(np.float64)
    F = round(fade_s * sr)
    for iv in _interval_gains(sr, frames, regions, spec_by_window, min_gain, above_fmax, speech_channel):
        a, b, k0, g = iv["a"], iv["b"], iv["k0"], iv["g"]
        if info is not None:
            info.append(iv)
        p = resynth(x, sr, a, b, lambda k: g[k - k0])
        xs = x[a:b].astype(np.float64)
        wv = fade_weights(a, b, F)[:, None]
        ys = xs + wv * (p - xs)
        y64[a:b] = ys * 32767.0
        out[a:b] = np.rint(ys * 32767.0).astype(np.int64).astype(np.int16)
    return (out, y64) if unrounded else out


def resynth_f32(x: np.ndarray, sr: int, a: int, b: int, k0: int, g: np.ndarray) -> np.ndarray:
    """resynth in float32: float32 window and gains, complex64 FFTs (torch.fft; numpy's computes in double), the overlap-add a float32
    sum in ascending frame order.  g [frames][N/2 + 1] as _interval_gains gives it."""
    import torch
    frames, ch = x.shape
    N = fft_size(sr)
    hop = N // 4
    n = np.arange(N)
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * n / N)).astype(np.float32)
    k1 = k0 + len(g) - 1
    assert (k0, k1) == frame_range(a, b, N)
    lo = k0 * hop - N // 2
    xp = np.zeros(((k1 - k0) * hop + N, ch), dtype=np.float32)
    s0, s1 = max(lo, 0), min(lo + len(xp), frames)
    xp[s0 - lo: s1 - lo] = x[s0:s1]
    acc = np.zeros_like(xp)
    g32 = torch.from_numpy(g.astype(np.float32))
    wt = torch.from_numpy(w)
    step = max(1, (1 << 24) // (N * ch))                                     # frames per FFT call
    for f0 in range(0, len(g), step):
        f1 = min(len(g), f0 + step)
        seg = torch.from_numpy(np.stack([xp[f * hop: f * hop + N] for f in range(f0, f1)]))          # [f][N][ch]
        X = torch.fft.rfft(seg * wt[None, :, None], dim=1)
        assert X.dtype == torch.complex64
        yy = torch.fft.irfft(X * g32[f0:f1, :, None], n=N, dim=1)
        yy = (yy * wt[None, :, None] / np.float32(1.5)).numpy()
        assert yy.dtype == np.float32
        for f in range(f0, f1):
            acc[f * hop: f * hop + N] += yy[f - f0]
    return acc[a - lo: b - lo]


def separate_f32(x: np.ndarray, sr: int, regions, spec_by_window: dict, fade_s: float = 0.01, min_gain: float = 0.0,
                 above_fmax: str = "mute", speech_channel: int = 1) -> np.ndarray:
    """Steps 3 and 4 of separate() restated in float32, on the same frames and the same gains (cast to float32): the unrounded output
    in LSB as float32 (frames, ch).  It says how far plain float32 arithmetic of this definition lies from the float64 reference --
    the yardstick of the device's bound --; it is compared with the reference, never with the device."""
    frames, ch = x.shape
    y = (x.astype(np.float32) * np.float32(32767.0)).astype(np.float32)
    F = round(fade_s * sr)
    for iv in _interval_gains(sr, frames, regions, spec_by_window, min_gain, above_fmax, speech_channel):
        a, b = iv["a"], iv["b"]
        p = resynth_f32(x, sr, a, b, iv["k0"], iv["g"])
        xs = x[a:b].astype(np.float32)
        wv = fade_weights(a, b, F).astype(np.float32)[:, None]
        ys = xs + wv * (p - xs)
        y[a:b] = ys * np.float32(32767.0)
    return y


# ---- crafted spec heads: checkpoints whose gains move with band and time ------------------------------------------------------
# The session checkpoint's speech map is 0 on more than 99 % of (band, bin) cells, so its gain is exactly 1 almost everywhere and a test
# on it checks the transcode.  These two heads replace spec_output_conv.1 (Conv2d(32, 2, 1) + ReLU) of a checkpoint; the body stays.
HEAD_SEED = 12
HEAD_MEDIAN = 1.0                 # 0.6 and 0.8 left the 5th percentile of G at 0.385 - 0.405 on some of the tests' recordings, 0.9 the
                                  # mean |dG| between bins of the 15 s interval at 0.0201: no margin
MIXED_BIAS = (-1.05 * HEAD_MEDIAN, -0.95 * HEAD_MEDIAN)
_CAL_WINDOWS = (3, 20, 41, 60)    # of the C1 signal (60 s, 16 kHz mono, seed 1001)


def _oracle_spec(sd_np, padded, wins):
    """fp32 CPU oracle: spec head [len(wins)][2][128][256] on windows `wins` (indices at the default step) of a padded 22.05 kHz signal."""
    import torch
    from softspoken_amd import synth
    from oracle import oracle_np as O
    sig = torch.from_numpy(np.ascontiguousarray(padded, dtype=np.float32))
    with torch.no_grad():
        sl = torch.stack([sig[i * WIN_STEP: i * WIN_STEP + WIN_LEN] for i in wins])
        spec, _ = O.model_forward(synth.to_torch_state_dict(sd_np), sl, want_spec=True)
    return spec.numpy()


def spread_head(sd_np, seed: int = HEAD_SEED, median: float = HEAD_MEDIAN) -> dict:
    """`spread`: 16 of the 32 input channels (a seeded permutation) feed the env row and the other 16 the speech row, weights from
    U(0.05, 0.4), bias 0 -- the rows see different features, both maps are positive everywhere.  Each row is then scaled so that its
    map's median over four windows of the C1 signal is `median` (the oracle measures it: P = 10^(y^2) - 1 makes the scale matter
    exponentially; a factor 5 on one row drives every gain to 1)."""
    from softspoken_amd import synth
    from oracle import oracle_np as O
    rng = np.random.default_rng(seed)
    w = np.zeros_like(sd_np["spec_output_conv.1.weight"])
    perm = rng.permutation(32)
    w[0, perm[:16], 0, 0] = rng.uniform(0.05, 0.4, 16)
    w[1, perm[16:], 0, 0] = rng.uniform(0.05, 0.4, 16)
    sd = dict(sd_np)
    sd["spec_output_conv.1.weight"] = w.astype(np.float32)
    sd["spec_output_conv.1.bias"] = np.zeros(2, dtype=np.float32)
    sig, _, _ = O.load_audio_from_bytes(synth.wav_bytes(synth.to_pcm16(synth.synth_audio(1001, 60.0, 16000, 1)), 16000))
    m = _oracle_spec(sd, O.pad_3s(sig), _CAL_WINDOWS)                         # weights > 0 on ReLU'd features: linear in the scale
    scale = np.array([median / np.median(m[:, 0]), median / np.median(m[:, 1])], dtype=np.float64)
    sd["spec_output_conv.1.weight"] = (w * scale[:, None, None, None]).astype(np.float32)
    return sd


def mixed_head(sd_np, seed: int = HEAD_SEED, median: float = HEAD_MEDIAN) -> dict:
    """`mixed`: the spread head with both biases near minus the median, so that either map is 0 on a good share of cells: G is exactly
    0 (env 0, speech > 0), exactly 1 (speech 0) or an ordinary value, side by side."""
    sd = spread_head(sd_np, seed, median)
    sd["spec_output_conv.1.bias"] = np.array(MIXED_BIAS, dtype=np.float32)
    return sd


def gain_stats(Gs) -> dict:
    """The conditions on a head, from the band gains G [bins][128] of a case's intervals (a list: neighbours are taken inside one)."""
    G = np.concatenate([g.ravel() for g in Gs])
    return dict(p5=float(np.percentile(G, 5)), p95=float(np.percentile(G, 95)),
                d_band=float(np.concatenate([np.abs(np.diff(g, axis=1)).ravel() for g in Gs]).mean()),
                d_bin=float(np.concatenate([np.abs(np.diff(g, axis=0)).ravel() for g in Gs if len(g) > 1]).mean()),
                zero=float((G == 0.0).mean()), one=float((G == 1.0).mean()), inside=float(((G > 0.1) & (G < 0.9)).mean()))


def assert_spread(st: dict):
    assert st["p5"] <= 0.4 and st["p95"] >= 0.6 and st["d_band"] >= 0.02 and st["d_bin"] >= 0.02, st


def assert_mixed(st: dict):
    assert st["zero"] >= 0.02 and st["one"] >= 0.02 and st["inside"] >= 0.30, st
