"""The cases of per-channel separation (ss_separate_pcm_channels), shared by test_separation_channels_host.py
(the fp32 CPU oracle in the device's place: the conditions on the inputs) and test_gpu_separation_channels.py (the device).

Every recording is test_gpu_separation._make(fmt, sr, ch, 2.5, 51, scale=0.5) with B1_REGIONS.  Not imported by the library."""
from __future__ import annotations

import numpy as np

import separation_ref as R

# (sample rate, channels, format): every FFT size 256 .. 8192, odd channel counts (a last channel without a partner), every format
BOUND_CASES = [(8000, 2, "u8"), (16000, 3, "pcm16"), (22050, 2, "f32"), (44100, 2, "pcm24"), (96000, 5, "pcm32"), (192000, 2, "pcm16"),
               (384000, 3, "pcm24")]
N_FFT = {8000: 256, 16000: 512, 22050: 512, 44100: 1024, 48000: 1024, 96000: 2048, 192000: 4096, 384000: 8192}
MIXED_CASES = [(48000, 2, "pcm16"), (8000, 2, "pcm16")]
MAIN_CASE = (48000, 2, "pcm16")                     # the f16x2 context, the parameter set, the cuts, the behaviour, SilenceJob
MONO_CASE = (44100, 1, "pcm24")                     # channels == 1
# test_gpu_separation.PARAM_CASES[3] (speech_channel 0, keep) with min_gain 0.1
PARAMS = dict(fade_s=0.02, min_gain=0.1, above_fmax="keep", speech_channel=0)
# cases whose channels are also run with a partner's and with the mix's maps: the gain a channel gets must matter
SWAP_CASES = [(48000, 2, "pcm16"), (16000, 3, "pcm16"), (8000, 2, "u8")]
PAIR_DISTANCE = 0.05                                # mean |Ga - Gb| over the band gains of a case's intervals, at least
SWAP_LSB, SWAP_SHARE = 2.0, 0.5                     # ... moves the float64 output by more than 2 LSB on at least half the interval samples


def plan_windows(plan) -> list:
    return sorted({i for r in plan["ranges"] for i in range(r["win_first"], r["win_last"] + 1)})


def interval_gains(plan, by_win, speech_channel: int = 1, min_gain: float = 0.0) -> list:
    """Band gains G' [bins][128] of each merged interval of the plan, from one signal's per-window maps."""
    return [R.band_gains(R.average_maps(by_win, range(r["bin_first"], r["bin_last"] + 1)), speech_channel, min_gain) for r in plan["ranges"]]


def pair_distance(Ga: list, Gb: list) -> float:
    return float(np.concatenate([np.abs(a - b).ravel() for a, b in zip(Ga, Gb)]).mean())


def moved_share(y_a: np.ndarray, y_b: np.ndarray, mask: np.ndarray, lsb: float = SWAP_LSB) -> float:
    """Share of the interval samples on which two unrounded outputs (in LSB) lie more than `lsb` apart."""
    d = np.abs(y_a - y_b)[mask]
    return float((d > lsb).mean())
