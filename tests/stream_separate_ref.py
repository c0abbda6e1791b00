"""Plain-Python statement of the separation streams' host rule (include/softspoken.h "separation streams"), for
the tests: the limit frame, D_sep, and what a returned frame's output depends on -- its merged interval, its capped distance to the
interval's ends, the bins and weights of its four STFT frames.

Not imported by the library."""
from __future__ import annotations

import math

import numpy as np

import separation_ref as S
import stream_output_ref as R


def separate_limit(sr: int, frames_decoded: int, bins_final: int, pending, pad_s: float, min_len_s: float, fade_s: float,
                   without_fade: bool = False) -> int:
    """The smallest of the three conditions' limits, before the clamp to [frames_out, frames decoded].  without_fade: condition 1
    stated wrongly as n < Lz (what the tests show to be caught)."""
    N = S.fft_size(sr)
    hop = N // 4
    F = 0 if without_fade else round(fade_s * sr)
    lz = min(max(R.output_limit(sr, bins_final, pending, pad_s, min_len_s), 0), frames_decoded)
    c1 = lz - F
    c2 = frames_decoded - N
    c3 = 0
    if bins_final >= 1:
        # the largest frame k whose unclamped bins are j0, j0 + 1 <= bins_final - 1; frame n needs frame n // hop + 2
        k = (sr * (6 * bins_final - 1539) - 1) // 512 // hop
        c3 = (k - 1) * hop
    return min(c1, c2, c3)


def d_sep(sr: int, break_s: float, pad_s: float, min_len_s: float, fade_s: float) -> float:
    half = 0 if sr == 22050 else math.ceil(32 / min(1.0, 22050 / sr))
    B = 3.0 + 2.0 * (3.0 / 256.0) + half / sr
    return B + break_s + pad_s + min_len_s + fade_s + (S.fft_size(sr) + 1) / sr


def bound_b(sr: int) -> float:
    half = 0 if sr == 22050 else math.ceil(32 / min(1.0, 22050 / sr))
    return 3.0 + 2.0 * (3.0 / 256.0) + half / sr


def blend_state(intervals, lo: int, hi: int, F: int):
    """For the frames [lo, hi): (interval start or -1, min(d_start, d_end) capped at F or -1) under the merged intervals given."""
    a_of = np.full(hi - lo, -1, dtype=np.int64)
    d_of = np.full(hi - lo, -1, dtype=np.int64)
    n = np.arange(lo, hi, dtype=np.int64)
    for a, e in intervals:
        m = (n >= a) & (n < e)
        if m.any():
            a_of[m] = a
            d_of[m] = np.minimum(np.minimum(n[m] - a, e - 1 - n[m]), F)
    return a_of, d_of


def frame_gain_rows(lo: int, hi: int, sr: int, n_bins: int):
    """[(k, j0, j1, alpha)] of the STFT frames over the output frames [lo, hi): frames lo // hop - 1 .. (hi - 1) // hop + 2."""
    hop = S.fft_size(sr) // 4
    return [(k,) + tuple(S.frame_bins(k, hop, sr, n_bins)) for k in range(lo // hop - 1, (hi - 1) // hop + 3)]
