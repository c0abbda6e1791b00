"""float64 numpy statement of the band silencer (include/softspoken.h "band silencer") for the tests:
test_box_host.py checks it on the CPU (and ss_box_plan against it), test_gpu_box_silence.py holds the device to it.

Not imported by the library.  A box is a tuple (start_s, end_s, low_hz, high_hz, channel): NaN or None edges mean "no estimate" (low 0,
high +infinity), channel -1 or None every channel.  The STFT, the overlap-add, the fade and the float32 restatement are
separation_ref's (steps 3 and 4 of the separation silencer are the band silencer's steps 2 and 4); this file adds where the gains come
from.  box_silence() also gives its output before the rounding; box_silence_f32 restates the resynthesis and the blend in float32 on the
same gains (cast to float32): the yardstick of the device's bound, compared with the reference, never with the device."""
from __future__ import annotations

import math

import numpy as np

import separation_ref as R


def _norm(box):
    s, e, lo, hi = box[:4]
    ch = box[4] if len(box) > 4 else None
    lo = 0.0 if lo is None or lo != lo else float(lo)
    hi = math.inf if hi is None or hi != hi else float(hi)
    return float(s), float(e), lo, hi, -1 if ch is None else int(ch)


def box_range(box, sr: int, frames: int):
    """[a, b) of one box, ss_silence_pcm's rounding and clamp; None when empty."""
    s, e = _norm(box)[:2]
    iv = R.merged_intervals([(s, e)], sr, frames)
    return iv[0] if iv else None


def merged_intervals(boxes, sr: int, frames: int):
    return R.merged_intervals([(b[0], b[1]) for b in boxes], sr, frames)


def plan(sr: int, frames: int, boxes) -> dict:
    """What ss_box_plan reports."""
    N = R.fft_size(sr)
    ranges, seen = [], set()
    for a, b in merged_intervals(boxes, sr, frames):
        k0, k1 = R.frame_range(a, b, N)
        ranges.append(dict(frame_begin=a, frame_end=b, stft_first=k0, stft_last=k1))
        seen.update(range(k0, k1 + 1))
    return dict(n_fft=N, hop=N // 4, n_frames=len(seen), ranges=ranges)


def chunk_count(sr: int, frames: int, boxes, budget: int) -> int:
    """Chunks of a frame budget: an interval is cut into pieces of (budget - 8) hops, a piece opens a new chunk when its frames would pass
    the budget -- one STFT launch and one blend launch each."""
    N = R.fft_size(sr)
    piece, n, held = (budget - 8) * (N // 4), 0, None
    for a, b in merged_intervals(boxes, sr, frames):
        for s0 in range(a, b, piece):
            k0, k1 = R.frame_range(s0, min(b, s0 + piece), N)
            if held is None or held + (k1 - k0 + 1) > budget:
                n, held = n + 1, 0
            held += k1 - k0 + 1
    return n


def bin_range(N: int, sr: int, low_hz: float, high_hz: float):
    """(q_lo, q_hi, lo_b, hi_b) of the definition; q_lo > q_hi: no bin inside."""
    lo_b, hi_b = low_hz * N / sr, high_hz * N / sr
    q_lo = math.ceil(lo_b) if lo_b <= N // 2 else N // 2 + 1
    q_hi = N // 2 if hi_b >= N // 2 else math.floor(hi_b)
    return q_lo, q_hi, lo_b, hi_b


def profile(N: int, sr: int, low_hz: float, high_hz: float, edge_hz: float) -> np.ndarray:
    """v(q) for q = 0 .. N/2."""
    q_lo, q_hi, lo_b, hi_b = bin_range(N, sr, low_hz, high_hz)
    e_b = edge_hz * N / sr
    v = np.zeros(N // 2 + 1)
    for q in range(N // 2 + 1):
        if q_lo <= q <= q_hi:
            v[q] = 1.0
            continue
        d = lo_b - q if q < q_lo else q - hi_b
        if e_b > 0.0 and d < e_b:
            v[q] = (1.0 + math.cos(math.pi * d / e_b)) / 2.0
    return v


def frame_gains(sr: int, frames: int, channels: int, boxes, min_gain: float, edge_hz: float):
    """(N, {k: G [channels][N/2 + 1]}) for every frame k that is active for a box: the minimum over the boxes active at k that act on the
    channel, 1 where there is none."""
    N = R.fft_size(sr)
    G = {}
    for box in boxes:
        s, e, lo, hi, ch = _norm(box)
        r = box_range(box, sr, frames)
        if r is None:
            continue
        g = 1.0 - (1.0 - min_gain) * profile(N, sr, lo, hi, edge_hz)
        k0, k1 = R.frame_range(r[0], r[1], N)             # the frames whose support meets [a, b)
        for k in range(k0, k1 + 1):
            Gk = G.setdefault(k, np.ones((channels, N // 2 + 1)))
            for c in (range(channels) if ch < 0 else (ch,)):
                Gk[c] = np.minimum(Gk[c], g)
    return N, G


def _run(x, sr, boxes, fade_s, min_gain, edge_hz, f32):
    frames, ch = x.shape
    N, G = frame_gains(sr, frames, ch, boxes, min_gain, edge_hz)
    F = round(fade_s * sr)
    ones = np.ones(N // 2 + 1)
    out = []
    for a, b in merged_intervals(boxes, sr, frames):
        k0, k1 = R.frame_range(a, b, N)
        p = np.empty((b - a, ch), dtype=np.float32 if f32 else np.float64)
        for c in range(ch):
            g = np.stack([G[k][c] if k in G else ones for k in range(k0, k1 + 1)])
            xc = np.ascontiguousarray(x[:, c:c + 1])
            p[:, c] = (R.resynth_f32(xc, sr, a, b, k0, g) if f32 else R.resynth(xc, sr, a, b, lambda k: g[k - k0]))[:, 0]
        out.append((a, b, p, R.fade_weights(a, b, F)))
    return out


def box_silence(x: np.ndarray, sr: int, boxes, fade_s: float = 0.01, min_gain: float = 0.0, edge_hz: float = 100.0, unrounded: bool = False):
    """x float32 (frames, ch) as the decode gives it -> int16 (frames, ch).  unrounded: -> (int16, float64 (frames, ch)): the output before
    its rounding in LSB, 32767 y inside the merged intervals, the float32 transcode x * 32767 outside."""
    y = (x.astype(np.float32) * np.float32(32767.0)).astype(np.float32)
    out = np.rint(y).astype(np.int64).astype(np.int16)
    y64 = y.astype(np.float64)
    for a, b, p, w in _run(x, sr, boxes, fade_s, min_gain, edge_hz, False):
        xs = x[a:b].astype(np.float64)
        ys = xs + w[:, None] * (p - xs)
        y64[a:b] = ys * 32767.0
        out[a:b] = np.rint(ys * 32767.0).astype(np.int64).astype(np.int16)
    return (out, y64) if unrounded else out


def box_silence_f32(x: np.ndarray, sr: int, boxes, fade_s: float = 0.01, min_gain: float = 0.0, edge_hz: float = 100.0) -> np.ndarray:
    """box_silence's resynthesis and blend in float32 on the same gains: the unrounded output in LSB as float32 (frames, ch)."""
    y = (x.astype(np.float32) * np.float32(32767.0)).astype(np.float32)
    for a, b, p, w in _run(x, sr, boxes, fade_s, min_gain, edge_hz, True):
        xs = x[a:b].astype(np.float32)
        ys = xs + w.astype(np.float32)[:, None] * (p - xs)
        y[a:b] = ys * np.float32(32767.0)
    return y
