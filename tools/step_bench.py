"""Detection throughput against the window step (settings.step_size, ss_set_window_step), one JSON line.  Not the flagship benchmark
(bench.py, which stays on the default step).

    python tools/step_bench.py [--files 10] [--minutes 10] [--steps 0.3,0.6,1.5,3.0] [--runs 3] [--precision f16x2] [--chunk 0]

`files` recordings of `minutes` minutes (16 kHz, 16-bit mono), resident in HBM.  Per step: one warm-up job, then `runs` timed jobs --
ss_reset + decode / resample of the batch + ss_run, host clock around work that ends with the run's results on the host -- and per step
the windows of the job, the median audio-s/s with the range of the runs, the ratio to the default step's figure and, beside it, the
ratio the window count alone would give (windows at 0.6 s / windows at this step): what is left between the two is the part of a job
that does not scale with the windows -- decode, resample, the plan and the host side.

Nothing here says anything about detection QUALITY against the step: that needs the real checkpoint and labelled recordings.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=10)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--steps", default="0.3,0.6,1.5,3.0")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--precision", default="f16x2", choices=list(native.PRECISIONS))
    ap.add_argument("--chunk", type=int, default=0, help="windows per pass (0: the library's default)")
    a = ap.parse_args()
    steps = [native.check_step(s) for s in a.steps.split(",")]
    sr, seconds = 16000, 60.0 * a.minutes
    pcm = np.concatenate([synth.to_pcm16(synth.synth_audio(3000 + k, seconds, sr, 1)) for k in range(a.files)])
    frames = np.full(a.files, len(pcm) // a.files, dtype=np.int64)
    ctx = native.Context(checkpoint.pack_state_dict(synth.make_state_dict(0)), 0, precision=a.precision, chunk=a.chunk or None)
    dev = ctx.device_alloc(pcm.nbytes + 64)
    ctx.device_upload(dev, pcm)

    def job():
        ctx.reset()
        first = ctx.add_pcm_batch_device(dev, native.PCM_S16, sr, 1, frames)
        ctx.run(0.1, 0.5)
        return first

    rows = {}
    for step in steps:
        ctx.set_window_step(step)
        first = job()                                      # warm-up: workspace of this step's passes, tap tables, kernels
        windows = sum(ctx.num_windows(first + k) for k in range(a.files))
        regions = sum(len(ctx.regions(first + k)) for k in range(a.files))
        t = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            job()
            t.append(time.perf_counter() - t0)
        rate = [a.files * seconds / x for x in t]
        rows[step] = dict(step_s=step, windows=int(windows), regions=int(regions), job_ms=round(1e3 * float(np.median(t)), 2),
                          audio_s_per_s=round(float(np.median(rate)), 1), audio_s_per_s_min=round(min(rate), 1),
                          audio_s_per_s_max=round(max(rate), 1), device_ms=round(ctx.last_run_device_ms(), 2))
    ctx.device_free(dev)
    ctx.close()
    base = rows.get(native.DEFAULT_STEP)
    if base:
        for r in rows.values():
            r["ratio_to_default"] = round(r["audio_s_per_s"] / base["audio_s_per_s"], 3)
            r["ratio_of_windows"] = round(base["windows"] / r["windows"], 3)
    print(json.dumps(dict(tool="step_bench", files=a.files, minutes=a.minutes, precision=a.precision, runs=a.runs, steps=list(rows.values()))))


if __name__ == "__main__":
    main()
