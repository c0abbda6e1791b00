"""Streaming detection throughput (ss_stream_*), one JSON line.  Not the flagship benchmark (bench.py).

    python tools/stream_bench.py [--precision f16x2] [--feeds 1,64,1024] [--rounds 40] [--warmup 10]

live feeds: N streams of 16 kHz 16-bit audio, each pushed 0.6 s per round with one step per round (after `warmup` rounds, when
            every stream runs one window per round): audio-s/s and step time p50 / p99
long:       one 10-minute recording pushed in 10 s pieces, a step after each, against ss_run on the same recording in the same process
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


def live(ctx, n_feeds, rounds, warmup, src):
    sids = [ctx.stream_open(native.PCM_S16, 16000, 1, 0.1, 0.5) for _ in range(n_feeds)]
    piece = 9600                                           # 0.6 s at 16 kHz
    times = []
    for r in range(warmup + rounds):
        for k, sid in enumerate(sids):
            at = ((r + 7 * k) * piece) % (len(src) - piece)
            ctx.stream_push(sid, src[at:at + piece])
        t0 = time.perf_counter()
        ctx.stream_step()
        if r >= warmup:
            times.append(time.perf_counter() - t0)
    for sid in sids:
        ctx.stream_free(sid)
    t = np.array(times)
    return dict(feeds=n_feeds, audio_s_per_s=round(n_feeds * 0.6 * len(t) / t.sum(), 1), step_ms_p50=round(1e3 * float(np.percentile(t, 50)), 3),
                step_ms_p99=round(1e3 * float(np.percentile(t, 99)), 3))


def long_recording(ctx, x, reps):
    best_s, best_r = 1e9, 1e9
    for _ in range(reps):
        sid = ctx.stream_open(native.PCM_S16, 16000, 1, 0.1, 0.5)
        t0 = time.perf_counter()
        for k in range(0, len(x), 160000):
            ctx.stream_push(sid, x[k:k + 160000])
            ctx.stream_step()
        ctx.stream_close(sid)
        ctx.stream_step()
        best_s = min(best_s, time.perf_counter() - t0)
        ctx.stream_free(sid)
        t0 = time.perf_counter()
        ctx.reset()
        ctx.add_pcm(x, native.PCM_S16, 16000, 1, len(x))
        ctx.run(0.1, 0.5)
        best_r = min(best_r, time.perf_counter() - t0)
    secs = len(x) / 16000.0
    return dict(seconds=secs, stream_audio_s_per_s=round(secs / best_s, 1), ss_run_audio_s_per_s=round(secs / best_r, 1),
                ratio=round(best_r / best_s, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x2")
    ap.add_argument("--feeds", default="1,64,1024")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    blob = checkpoint.pack_state_dict(synth.make_state_dict(0))
    ctx = native.Context(blob, 0, precision=a.precision)
    x = synth.to_pcm16(synth.synth_audio(3000, 600.0, 16000, 1))
    long_recording(ctx, x[: 16000 * 60], 1)                # warm-up: workspace, tap tables, kernels
    out = dict(tool="stream_bench", precision=a.precision, live=[live(ctx, int(n), a.rounds, a.warmup, x) for n in a.feeds.split(",")],
               long=long_recording(ctx, x, a.reps))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
