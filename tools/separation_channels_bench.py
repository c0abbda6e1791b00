"""Per-channel separation timing (ss_separate_pcm_channels), one JSON line.  Not the flagship benchmark (bench.py).

    python tools/separation_channels_bench.py [--precision f16x2] [--reps 7]

The file of tools/separation_bench.py (10 min, 48 kHz stereo 16-bit, 20 erased intervals of 3 s).  After a warm-up of every call, `reps`
calls each, reported as median [min, max] of the wall time in ms:
  each         ss_separate_pcm_channels
  mix          ss_separate_pcm on the same file (run tools/separation_bench.py at the parent commit for the parent's own number)
  mono_calls   one ss_separate_pcm call per de-interleaved mono file, added up: what a user could do before
and, from `reps` more calls of each and mix on a context with SS_FLAG_PROFILE, the device time per call of sep_stft_each_kernel<1024>
against sep_stft_kernel<1024> (all launches of a call added up), of the other sep_* kernels and of the model passes.
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
from separation_bench import CH, REGIONS, SECONDS, SR, classify, recording  # noqa: E402


def spread(ts):
    ts = [float(t) for t in ts]
    return dict(median=round(float(np.median(ts)), 3), min=round(min(ts), 3), max=round(max(ts), 3), n=len(ts))


def walls(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return spread(out)


def profiled(ctx, fn, reps):
    """Per call: device ms of every sep_* launch name, of the model passes and of upload / decode."""
    rows = []
    for _ in range(reps):
        ctx.reset_stats()
        fn()
        row = {"model_passes": 0.0, "upload_decode": 0.0}
        for s in ctx.kernel_stats():
            kind = classify(s["name"])
            if kind == "separation_kernels":
                row[s["name"]] = row.get(s["name"], 0.0) + s["total_ms"]
                row[s["name"] + " launches"] = s["launches"]
            else:
                row[kind] += s["total_ms"]
        rows.append(row)
    keys = sorted({k for r in rows for k in r})
    return {k: (rows[0][k] if k.endswith(" launches") else spread([r.get(k, 0.0) for r in rows])) for k in keys}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x2", choices=native.PRECISIONS)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    pcm = recording()
    frames = pcm.shape[0]
    monos = [np.ascontiguousarray(pcm[:, c]) for c in range(CH)]
    blob = checkpoint.pack_state_dict(synth.make_state_dict(0))
    plan = native.separation_plan(SR, frames, REGIONS)
    ctx = native.Context(blob, 0, precision=a.precision)

    def each():
        return ctx.separate_pcm_channels(pcm, native.PCM_S16, SR, CH, frames, REGIONS)

    def mix():
        return ctx.separate_pcm(pcm, native.PCM_S16, SR, CH, frames, REGIONS)

    def mono_calls():
        return [ctx.separate_pcm(m, native.PCM_S16, SR, 1, frames, REGIONS) for m in monos]
    for fn in (each, mix, mono_calls, each, mix, mono_calls):              # warm-up: workspace, tables, code objects, clocks
        fn()
    res = dict(each=walls(each, a.reps), mix=walls(mix, a.reps), mono_calls=walls(mono_calls, a.reps))
    ctx.close()
    prof = native.Context(blob, 0, precision=a.precision, profile=True)
    p_each = lambda: prof.separate_pcm_channels(pcm, native.PCM_S16, SR, CH, frames, REGIONS)      # noqa: E731
    p_mix = lambda: prof.separate_pcm(pcm, native.PCM_S16, SR, CH, frames, REGIONS)                # noqa: E731
    for fn in (p_each, p_mix, p_each, p_mix):
        fn()
    dev = dict(each=profiled(prof, p_each, a.reps), mix=profiled(prof, p_mix, a.reps))
    prof.close()
    print(json.dumps(dict(
        workload=f"{SECONDS // 60} min {SR // 1000} kHz {CH} ch PCM16, {len(REGIONS)} intervals / {sum(b - a for a, b in REGIONS):.0f} s",
        precision=a.precision, n_fft=plan["n_fft"], windows_run_per_channel=plan["windows_run"], reps=a.reps,
        wall_ms=res, each_over_mix=round(res["each"]["median"] / res["mix"]["median"], 3),
        each_over_mono_calls=round(res["each"]["median"] / res["mono_calls"]["median"], 3), device_ms_per_call=dev)))


if __name__ == "__main__":
    main()
