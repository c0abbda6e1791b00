"""Stream bands (ss_stream_open_bands) against the same streams with bands off and against the route a user had before, one JSON line.
Not the flagship benchmark (bench.py).

    python tools/stream_bands_bench.py [--precision f16x2] [--feeds 512] [--rounds 30] [--warmup 10] [--runs 3] [--limit-s 240]

The case is tools/stream_channels_bench.py's: N live feeds of 48 kHz 16-bit stereo, each pushed 0.6 s per round with one step per
round, timed after `warmup` rounds.  Four forms, run alternately `runs` times, a run's figure the median step over its rounds, reported
as median [min, max] over the runs:
  mix_off / mix_on:    N mix streams, bands off / on            each_off / each_on:  N each-channel streams (two lanes each)
kernels: one profiled pass of mix_on and each_on -- the two launches bands add and the spec head's share, per step, from
ss_get_kernel_stats (a profiling context times every launch with events, so only its device times are used).
old_route: what a user did before -- hold the recording, and at close ss_add_pcm + ss_run + ss_region_bands on a second context -- for one
recording of --old-seconds: its time, the bytes it holds per stream, and its latency to the first band.
Every phase has a time limit of its own (--limit-s); the tool exits with status 2 at the first phase that passes it, and any failed
call ends it with the library's error."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from softspoken_amd import checkpoint, native, synth  # noqa: E402

SR, PIECE = 48000, 28800                                  # 0.6 s
THR, BRK = 0.1, 0.5


class Limit:
    def __init__(self, seconds, what):
        self.end, self.what = time.monotonic() + seconds, what

    def check(self):
        if time.monotonic() > self.end:
            print(json.dumps(dict(tool="stream_bands_bench", error=f"time limit passed in {self.what}")), flush=True)
            sys.exit(2)


def _open(ctx, form, n):
    each, on = form.startswith("each"), form.endswith("_on")
    if on:
        return [ctx.stream_open_bands(native.PCM_S16, SR, 2, THR, BRK, None, False, each) for _ in range(n)]
    if each:
        return [ctx.stream_open_channels(native.PCM_S16, SR, 2, THR, BRK) for _ in range(n)]
    return [ctx.stream_open(native.PCM_S16, SR, 2, THR, BRK) for _ in range(n)]


def live(ctx, form, n, rounds, warmup, src, limit, stats_at=None):
    sids = _open(ctx, form, n)
    step, regions = [], 0
    for r in range(warmup + rounds):
        limit.check()
        if stats_at is not None and r == warmup:
            ctx.reset_stats()
        for k in range(n):
            at = ((r + 7 * k) * PIECE) % (len(src) - PIECE)
            ctx.stream_push(sids[k], src[at:at + PIECE], frames=PIECE)
        t1 = time.perf_counter()
        ctx.stream_step()
        t2 = time.perf_counter()
        if r >= warmup:
            step.append(t2 - t1)
            regions += len(ctx.stream_regions(sids[0]))
    state = ctx.stream_info(sids[0])["state_bytes"]
    for sid in sids:
        ctx.stream_free(sid)
    return dict(step_ms=1e3 * float(np.median(step)), state_bytes=state, regions_of_feed_0=regions)


def kernels(blob, precision, form, n, rounds, warmup, src, limit):
    ctx = native.Context(blob, 0, precision=precision, profile=True)
    live(ctx, form, n, rounds, warmup, src, limit, stats_at=warmup)
    st = ctx.kernel_stats()
    ctx.close()
    total = sum(s["total_ms"] for s in st)
    out = dict(all_launches_ms_per_step=round(total / rounds, 3))
    for s in st:
        if s["name"] in ("stream_map_kernel", "stream_band_kernel", "stream_average") or "spec" in s["name"]:
            out[s["name"]] = dict(ms_per_step=round(s["total_ms"] / rounds, 4), launches_per_step=round(s["launches"] / rounds, 2))
    return out


def old_route(ctx, seconds, src, limit):
    """Hold the recording; at close: add + run + region_bands on the regions the run found."""
    limit.check()
    pcm = np.ascontiguousarray(np.tile(src, (int(np.ceil(seconds * SR / len(src))), 1))[:int(seconds * SR)])
    raw = np.frombuffer(pcm.tobytes(), dtype=np.uint8)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.reset()
        fid = ctx.add_pcm(raw, native.PCM_S16, SR, 2, len(pcm))
        ctx.run(THR, BRK)
        regs = ctx.regions(fid)
        if regs:
            ctx.region_bands(fid, regs)
        times.append(time.perf_counter() - t0)
        limit.check()
    return dict(seconds=seconds, regions=len(regs), at_close_ms=round(1e3 * float(np.median(times)), 2), bytes_held_per_stream=int(raw.size),
                latency_to_first_band_s=seconds)


def summary(vals):
    return dict(median=round(float(np.median(vals)), 3), min=round(float(np.min(vals)), 3), max=round(float(np.max(vals)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x2")
    ap.add_argument("--feeds", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit-s", type=float, default=240.0)
    ap.add_argument("--old-seconds", type=float, default=600.0)
    ap.add_argument("--forms", default="mix_off,mix_on,each_off,each_on")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-old-route", action="store_true")
    a = ap.parse_args()
    blob = checkpoint.pack_state_dict(synth.make_state_dict(0))
    ctx = native.Context(blob, 0, precision=a.precision)
    src = np.ascontiguousarray(synth.to_pcm16(synth.synth_audio(3004, 120.0, SR, 2)))      # [frames, 2]
    forms = a.forms.split(",")
    live(ctx, forms[-1], 2, 4, 8, src, Limit(a.limit_s, "warm-up"))      # warm-up: workspace, tap tables, kernels
    runs = {f: [] for f in forms}
    state = {}
    for _ in range(a.runs):                                   # alternating
        for f in forms:
            res = live(ctx, f, a.feeds, a.rounds, a.warmup, src, Limit(a.limit_s, f))
            runs[f].append(res["step_ms"]); state[f] = res["state_bytes"]
    out = dict(tool="stream_bands_bench", precision=a.precision, feeds=a.feeds, rate=SR, channels=2, piece_s=0.6, rounds=a.rounds, runs=a.runs,
               step_ms={f: summary(v) for f, v in runs.items()}, state_bytes_per_stream=state)
    if not a.no_kernels:
        out["kernels"] = {f: kernels(blob, a.precision, f, a.feeds, min(a.rounds, 10), a.warmup, src, Limit(a.limit_s, "kernels " + f))
                          for f in forms if f.endswith("_on")}
    if not a.no_old_route:
        out["old_route"] = old_route(ctx, a.old_seconds, src, Limit(a.limit_s, "old route"))
        out["old_route"]["stream_latency_bound_s"] = "break_s + B (include/softspoken.h, streaming detection)"
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
