"""Band silencer timing (ss_box_silence_pcm), one JSON line.  Not the flagship benchmark (bench.py).

    python tools/box_silence_bench.py [--precision f16x2] [--reps 5]

tools/separation_bench.py's recording and intervals: 10 minutes of 48 kHz stereo 16-bit, 20 erased intervals of 3 s (60 s in all), every
interval a box 300 .. 3400 Hz on both channels.  Reports the wall time of ss_box_silence_pcm (median of `reps` calls, no profiling)
beside ss_silence_pcm's and ss_separate_pcm's on the same file, intervals and build, and, from one more call with SS_FLAG_PROFILE, the
device time of the call's launches; the rest of the wall time is host work and the copies to and from the device.  --precision is the
separation silencer's (the band silencer runs no model pass and has none).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from softspoken_amd import checkpoint, native, synth  # noqa: E402
from separation_bench import CH, REGIONS, SECONDS, SR, recording, timed  # noqa: E402

BAND = (300.0, 3400.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x2", choices=native.PRECISIONS)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pcm = recording()
    frames = pcm.shape[0]
    boxes = native.boxes_array([(s, e, BAND[0], BAND[1]) for s, e in REGIONS])
    plan = native.box_plan(SR, frames, boxes)
    ctx = native.Context(checkpoint.pack_state_dict(synth.make_state_dict(0)), 0, precision=a.precision)
    calls = {"box_silence_ms": lambda: ctx.box_silence_pcm(pcm, native.PCM_S16, SR, CH, boxes),
             "silence_zero_ms": lambda: ctx.silence_pcm(pcm, native.PCM_S16, SR, CH, frames, REGIONS),
             "separate_ms": lambda: ctx.separate_pcm(pcm, native.PCM_S16, SR, CH, frames, REGIONS)}
    for fn in calls.values():                                         # warm-up: workspace, tables, code objects
        fn()
    ms = {k: round(timed(fn, a.reps), 3) for k, fn in calls.items()}
    ctx.close()
    prof = native.Context(None, 0, profile=True)
    prof.box_silence_pcm(pcm, native.PCM_S16, SR, CH, boxes)
    prof.reset_stats()
    t0 = time.perf_counter()
    prof.box_silence_pcm(pcm, native.PCM_S16, SR, CH, boxes)
    prof_wall = 1e3 * (time.perf_counter() - t0)
    kernels = {s["name"]: round(s["total_ms"], 4) for s in prof.kernel_stats()}
    prof.close()
    print(json.dumps(dict(
        tool="box_silence_bench",
        workload=f"{SECONDS // 60} min {SR // 1000} kHz {CH} ch PCM16, {len(REGIONS)} boxes / {sum(b - a for a, b in REGIONS):.0f} s, {BAND[0]:.0f}-{BAND[1]:.0f} Hz",
        precision=a.precision, n_fft=plan["n_fft"], stft_frames=plan["n_frames"], **ms,
        profiled_wall_ms=round(prof_wall, 3), launches_ms=kernels, host_and_copies_ms=round(prof_wall - sum(kernels.values()), 3))))


if __name__ == "__main__":
    main()
