"""Per-channel detection (ss_add_pcm_channels*, settings.hip_channel_mode = 'each'), one JSON line.  Not the flagship benchmark (bench.py).

    python tools/channels_bench.py [--minutes 10] [--rate 48000] [--channels 2] [--runs 5] [--reps 20] [--no-detect]

ingest:  a recording already in HBM through ss_add_pcm_channels_device, against what could be done before: the de-interleaved channels
         (also in HBM) through ss_add_pcm_device, one call per channel.  The two are timed alternately: `runs` runs of `reps` ingests each,
         host clock around work that ends in a device synchronise; median and range of the runs' per-ingest times, and whether the
         stored signals are bit-identical.
detect:  the whole file, ss_reset + ingest + ss_run, per channel against the mixdown (the network runs C times the windows), per
         precision.
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


def _stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(np.min(ms)), 4), max_ms=round(float(np.max(ms)), 4))


def ingest(ctx, pcm, sr, runs, reps):
    frames, ch = pcm.shape
    planes = np.ascontiguousarray(pcm.T)                   # [ch, frames]: the de-interleaved channels, back to back
    dev = ctx.device_alloc(pcm.nbytes + 64)
    dev_planes = ctx.device_alloc(planes.nbytes + 64)
    ctx.device_upload(dev, pcm)
    ctx.device_upload(dev_planes, planes)

    def each():
        ctx.reset()
        return ctx.add_pcm_channels_device(dev, native.PCM_S16, sr, ch, frames)

    def alone():
        ctx.reset()
        return [ctx.add_pcm_device(dev_planes + c * frames * 2, native.PCM_S16, sr, 1, frames) for c in range(ch)][0]

    first = each()
    got = [ctx.read_signal(first + c, padded=True) for c in range(ch)]
    first = alone()
    same = all(np.array_equal(got[c].view(np.uint32), ctx.read_signal(first + c, padded=True).view(np.uint32)) for c in range(ch))
    times = {"channels_call": [], "one_call_per_channel": []}
    for _ in range(runs):                                  # alternating, so that both see the same neighbours on the card
        for name, fn in (("channels_call", each), ("one_call_per_channel", alone)):
            fn(); ctx.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            ctx.sync()
            times[name].append(1e3 * (time.perf_counter() - t0) / reps)
    ctx.device_free(dev)
    ctx.device_free(dev_planes)
    out = {k: _stats(v) for k, v in times.items()}
    out["kernel_ms_per_ingest"] = kernel_times(pcm, planes, sr, reps)
    out.update(bit_identical=bool(same), ratio_of_medians=round(out["channels_call"]["median_ms"] / out["one_call_per_channel"]["median_ms"], 4),
               pcm_mb=round(pcm.nbytes / 1e6, 1), runs=runs, reps=reps)
    return out


def kernel_times(pcm, planes, sr, reps):
    """The launches alone (the library's event timing, ss_get_kernel_stats, on a profiling context): device ms per ingest by kernel name."""
    frames, ch = pcm.shape
    ctx = native.Context(None, 0, profile=True)
    dev = ctx.device_alloc(pcm.nbytes + 64)
    dev_planes = ctx.device_alloc(planes.nbytes + 64)
    ctx.device_upload(dev, pcm)
    ctx.device_upload(dev_planes, planes)
    out = {}
    for name in ("channels_call", "one_call_per_channel"):
        for timed in (False, True):                        # a warm-up round first
            ctx.reset_stats()
            for _ in range(reps):
                ctx.reset()
                if name == "channels_call":
                    ctx.add_pcm_channels_device(dev, native.PCM_S16, sr, ch, frames)
                else:
                    for c in range(ch):
                        ctx.add_pcm_device(dev_planes + c * frames * 2, native.PCM_S16, sr, 1, frames)
            if timed:
                out[name] = {k["name"]: round(k["total_ms"] / reps, 4) for k in ctx.kernel_stats()}
    ctx.close()
    return out


def detect(precision, blob, pcm, sr, runs):
    frames, ch = pcm.shape
    ctx = native.Context(blob, 0, precision=precision)
    flat = pcm.reshape(-1)

    def job(each):
        ctx.reset()
        (ctx.add_pcm_channels if each else ctx.add_pcm)(flat, native.PCM_S16, sr, ch, frames)
        ctx.run(0.1, 0.5)
        return ctx.regions_union(0, ch) if each else ctx.regions(0)

    times = {"each": [], "mix": []}
    tables = {}
    for each in (True, False):
        tables[each] = job(each)                            # warm-up: workspace, tap tables, kernels
    for _ in range(runs):
        for each in (True, False):
            t0 = time.perf_counter()
            job(each)
            times["each" if each else "mix"].append(1e3 * (time.perf_counter() - t0))
    ctx.close()
    out = {k: _stats(v) for k, v in times.items()}
    out.update(ratio_of_medians=round(out["each"]["median_ms"] / out["mix"]["median_ms"], 3), regions_each=len(tables[True]),
               regions_mix=len(tables[False]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--precisions", default="f16x2,fp32")
    ap.add_argument("--no-detect", action="store_true")
    a = ap.parse_args()
    pcm = np.ascontiguousarray(synth.to_pcm16(synth.synth_audio(3004, 60.0 * a.minutes, a.rate, a.channels)))     # [frames, channels]
    audio = native.Context(None, 0)
    out = dict(tool="channels_bench", minutes=a.minutes, rate=a.rate, channels=a.channels, ingest=ingest(audio, pcm, a.rate, a.runs, a.reps))
    audio.close()
    if not a.no_detect:
        blob = checkpoint.pack_state_dict(synth.make_state_dict(0))
        out["detect"] = {p: detect(p, blob, pcm, a.rate, a.runs) for p in a.precisions.split(",")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
