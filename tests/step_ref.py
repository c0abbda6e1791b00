"""The reference's window plan, overlap averaging and region finding with the window step as an argument, restated in plain Python and
numpy for the tests of settings.step_size (test_step_host.py on the CPU, test_gpu_step.py on the device).

Restated from the reference's root/code/frontend/NNDetector.py:55-82 (plan_detection_job), :153-190 (average_overlapping_detections) and
:103-143 (find_speech_regions), with root/code/backend/worker.py:100's shift by the 3 s of padding; Python's own round, math.floor and
np.ceil, in the reference's operation order.  Not imported by the library and not derived from it.

Two places where the reference has no answer and the project's rule is stated instead:
  * clamp_plan: a window that does not fit the padded signal is dropped (the reference's torch.stack fails on the short slice) -- the plan
    comes from the header duration, the samples from the resampler;
  * average: a window whose 256 bins run past the last bin adds the bins that exist (numpy raises on the short slice in the reference).
"""
from __future__ import annotations

import math

import numpy as np

SR = 22050                          # settings.vad_resample
WINDOW = 3 * SR                     # NNDetector.py:74
TIME_RESOLUTION = 3 / 256           # NNDetector.py:172
STEP_MIN, STEP_MAX = 0.1, 3.0       # the range include/softspoken.h accepts


def per_step(step: float) -> int:
    return math.floor(SR * step)                                         # NNDetector.py:75


def plan(duration_s: float, step: float) -> np.ndarray:
    """NNDetector.py:66-80 -> int64 start indexes into the 3 s-padded signal."""
    audio_data_length = round(duration_s * SR) + (3 * 2 * SR)            # :72
    num_windows = int(np.ceil((audio_data_length - WINDOW) / per_step(step)))   # :77
    return np.arange(max(num_windows, 0), dtype=np.int64) * per_step(step)       # :78


def clamp_plan(starts: np.ndarray, n_padded: int) -> np.ndarray:
    """Drop the windows that do not fit n_padded samples."""
    return starts[starts + WINDOW <= n_padded]


def start_bin(i: int, step: float) -> int:
    return int(round(i * step / TIME_RESOLUTION))                        # NNDetector.py:175


def n_bins(n_padded: int) -> int:
    return int(round((n_padded / SR) * 256 / 3))                         # NNDetector.py:168 (worker.py:89 hands it len(padded) / rate)


def average(window_logits: np.ndarray, n_padded: int, step: float):
    """NNDetector.py:168-188 -> (avg float64[kept], bin numbers int64[kept]): float64 sums in window order, bins with a count >= 1."""
    n = n_bins(n_padded)
    s = np.zeros(n)
    c = np.zeros(n)
    for i, w in enumerate(np.asarray(window_logits)):
        at = start_bin(i, step)
        seg = s[at:at + 256]
        seg += w.reshape(-1)[:len(seg)]
        c[at:at + 256] += 1
    keep = np.nonzero(c >= 1)[0]
    return s[keep] / c[keep], keep.astype(np.int64)


def time_str(idx: int) -> str:
    return f"{idx / (256 / 3):.4f}"                                       # NNDetector.py:185


def find_regions(avg, idx, threshold: float, break_duration: float = 0.5):
    """NNDetector.py:109-141 on (value, time string) pairs, then worker.py:100 -> [(start_s, end_s)] as floats minus 3."""
    regions, start, end = [], None, None
    for v, i in zip(avg, idx):
        t = time_str(int(i))
        if v > threshold:
            if start is None:
                start = t
            end = t
        elif start is not None:
            regions.append((start, end))
            start = None
    if start is not None:
        regions.append((start, end))
    merged = []
    if regions:
        cur = regions[0]
        for nxt in regions[1:]:
            if float(nxt[0]) - float(cur[1]) <= break_duration:
                cur = (cur[0], nxt[1])
            else:
                merged.append(cur)
                cur = nxt
        merged.append(cur)
    return [(float(a) - 3, float(b) - 3) for a, b in merged]


def covering_windows(j: int, n_windows: int, step: float):
    """Brute force: every window i < n_windows whose bins [start, start + 256) hold bin j."""
    return [i for i in range(n_windows) if 0 <= j - start_bin(i, step) < 256]
