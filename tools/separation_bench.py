"""Separation silencer timing (ss_separate_pcm), one JSON line.  Not the flagship benchmark (bench.py).

    python tools/separation_bench.py [--precision f16x2] [--reps 5]

A 10-minute 48 kHz stereo 16-bit recording with 20 erased intervals of 3 s (60 s in all).  Reports the wall time of ss_separate_pcm
(median of `reps` calls, no profiling) beside ss_silence_pcm's on the same file, and, from one more call with SS_FLAG_PROFILE, the
device time split into the model passes (front-end + U-Net + spec head), the separation kernels (sep_*: accumulate, finalize, STFT,
blend) and upload / decode (resampling for the arena, the transcode); the rest of the wall time is host work and copies.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from softspoken_amd import checkpoint, native, synth  # noqa: E402

SR, CH, SECONDS = 48000, 2, 600
REGIONS = [(5.0 + 30.0 * i, 8.0 + 30.0 * i) for i in range(20)]


def recording():
    rng = np.random.default_rng(9)
    t = np.arange(SR * SECONDS) / SR
    x = 0.05 * rng.standard_normal((SR * SECONDS, CH)) + 0.2 * np.sin(2 * np.pi * 440 * t)[:, None] * (1 + 0.5 * np.sin(2 * np.pi * 0.3 * t))[:, None]
    return np.clip(np.rint(x * 32767), -32768, 32767).astype(np.int16)


def classify(name):
    if name.startswith("sep_transcode") or name.startswith(("decode_mono", "resample")):
        return "upload_decode"
    if name.startswith("sep_"):
        return "separation_kernels"
    return "model_passes"


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x2", choices=native.PRECISIONS)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pcm = recording()
    frames = pcm.shape[0]
    blob = checkpoint.pack_state_dict(synth.make_state_dict(0))
    plan = native.separation_plan(SR, frames, REGIONS)
    ctx = native.Context(blob, 0, precision=a.precision)
    ctx.separate_pcm(pcm, native.PCM_S16, SR, CH, frames, REGIONS)          # warm-up: workspace, tables, code objects
    ctx.silence_pcm(pcm, native.PCM_S16, SR, CH, frames, REGIONS)
    sep_ms = timed(lambda: ctx.separate_pcm(pcm, native.PCM_S16, SR, CH, frames, REGIONS), a.reps)
    zero_ms = timed(lambda: ctx.silence_pcm(pcm, native.PCM_S16, SR, CH, frames, REGIONS), a.reps)
    ctx.close()
    prof = native.Context(blob, 0, precision=a.precision, profile=True)
    prof.separate_pcm(pcm, native.PCM_S16, SR, CH, frames, REGIONS)
    prof.reset_stats()
    t0 = time.perf_counter()
    prof.separate_pcm(pcm, native.PCM_S16, SR, CH, frames, REGIONS)
    prof_wall = 1e3 * (time.perf_counter() - t0)
    split = {"model_passes": 0.0, "separation_kernels": 0.0, "upload_decode": 0.0}
    kernels = {}
    for s in prof.kernel_stats():
        name, ms = s["name"], s["total_ms"]
        split[classify(name)] += ms
        if name.startswith("sep_"):
            kernels[name] = round(ms, 4)
    prof.close()
    print(json.dumps(dict(
        workload=f"{SECONDS // 60} min {SR // 1000} kHz {CH} ch PCM16, {len(REGIONS)} intervals / {sum(b - a for a, b in REGIONS):.0f} s",
        precision=a.precision, n_fft=plan["n_fft"], windows_run=plan["windows_run"], windows_file=plan["n_windows"],
        separate_ms=round(sep_ms, 3), silence_zero_ms=round(zero_ms, 3),
        profiled_wall_ms=round(prof_wall, 3), device_ms={k: round(v, 3) for k, v in split.items()},
        host_and_copies_ms=round(prof_wall - sum(split.values()), 3), sep_launches_ms=kernels)))


if __name__ == "__main__":
    main()
