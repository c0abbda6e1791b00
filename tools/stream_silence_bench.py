"""Streaming silencer step time (ss_stream_open_output / ss_stream_output), one JSON line.  Not the flagship benchmark (bench.py).

    python tools/stream_silence_bench.py [--precision f16x2] [--feeds 1,64,1024] [--rounds 40] [--warmup 10] [--source]

N live feeds of 48 kHz stereo 16-bit audio, each pushed 0.6 s per round with one step per round (after `warmup` rounds, when every
stream runs one window per round and returns 0.6 s of output): step time p50 / p99 with output (the step, and the step plus reading
every stream's frames) and without (ss_stream_open on the same feeds), and from one more run on a profiling context the output
kernel's and the raw-PCM carry's device time and bytes per step (ss_get_kernel_stats).  --source adds the same rounds with every
stream's output in its own encoding (ss_stream_open_source / ss_stream_output_bytes) under "live_source".
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

SR, CH = 48000, 2
PIECE = 28800                                              # 0.6 s
ERASE = dict(pad_s=0.05, min_len_s=0.3)


def live(ctx, n_feeds, rounds, warmup, src, thr, with_output, read=True, source=False):
    if source:
        sids = [ctx.stream_open_source(native.PCM_S16, SR, CH, thr, 0.5, ERASE) for _ in range(n_feeds)]
    elif with_output:
        sids = [ctx.stream_open_output(native.PCM_S16, SR, CH, thr, 0.5, ERASE) for _ in range(n_feeds)]
    else:
        sids = [ctx.stream_open(native.PCM_S16, SR, CH, thr, 0.5) for _ in range(n_feeds)]
    step, total, frames, erased = [], [], 0, 0
    for r in range(warmup + rounds):
        for k, sid in enumerate(sids):
            at = ((r + 7 * k) * PIECE) % (len(src) - PIECE)
            ctx.stream_push(sid, src[at:at + PIECE])
        t0 = time.perf_counter()
        ctx.stream_step()
        t1 = time.perf_counter()
        if with_output and read:
            for sid in sids:
                frames += len(ctx.stream_output_bytes(sid, 2 * CH)[1] if source else ctx.stream_output(sid, CH)[1])
        t2 = time.perf_counter()
        if r >= warmup:
            step.append(t1 - t0); total.append(t2 - t0)
    if with_output:
        erased = sum(ctx.stream_output_info(sid)["frames_erased"] for sid in sids)
    state = ctx.stream_info(sids[0])["state_bytes"]
    for sid in sids:
        ctx.stream_free(sid)
    t, tt = np.array(step), np.array(total)
    out = dict(feeds=n_feeds, output=with_output, step_ms_p50=round(1e3 * float(np.percentile(t, 50)), 3),
               step_ms_p99=round(1e3 * float(np.percentile(t, 99)), 3), state_bytes_per_stream=int(state))
    if with_output:
        out.update(step_and_read_ms_p50=round(1e3 * float(np.percentile(tt, 50)), 3), step_and_read_ms_p99=round(1e3 * float(np.percentile(tt, 99)), 3),
                   erased_share=round(erased / max(frames, 1), 3))
    return out


def kernel_share(blob, precision, n_feeds, rounds, warmup, src, thr, source=False):
    ctx = native.Context(blob, 0, precision=precision, profile=True)
    live(ctx, n_feeds, 1, warmup, src, thr, True, read=False, source=source)
    ctx.reset_stats()
    live(ctx, n_feeds, rounds, 0, src, thr, True, read=False, source=source)
    steps = rounds
    out = dict(feeds=n_feeds)
    for st in ctx.kernel_stats():
        if st["name"] in ("stream_silence_kernel", "stream_silence_source_kernel", "stream_copy_bytes") and st["launches"]:
            out[st["name"]] = dict(ms_per_step=round(st["total_ms"] / steps, 4), bytes_per_step=int(st["bytes"] / steps))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x2")
    ap.add_argument("--feeds", default="1,64,1024")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--source", action="store_true")
    a = ap.parse_args()
    blob = checkpoint.pack_state_dict(synth.make_state_dict(0))
    ctx = native.Context(blob, 0, precision=a.precision)
    x = np.ascontiguousarray(synth.synth_audio(3000, 120.0, SR, CH).T)
    src = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    # a threshold inside the recording's own scores, so that the kernel has frames to erase and frames to keep
    ctx.reset()
    fid = ctx.add_pcm(src, native.PCM_S16, SR, CH, len(src))
    ctx.run(0.1, 0.5)
    thr = float(np.nanquantile(ctx.avg(fid)[0], 0.5))
    live(ctx, 4, 2, 8, src, thr, True)                     # warm-up: workspace, tap tables, kernels
    feeds = [int(n) for n in a.feeds.split(",")]
    out = dict(tool="stream_silence_bench", precision=a.precision, format="48 kHz stereo S16, 0.6 s per round", erase=ERASE,
               live=[live(ctx, n, a.rounds, a.warmup, src, thr, w) for n in feeds for w in (False, True)])
    if a.source:
        out["live_source"] = [live(ctx, n, a.rounds, a.warmup, src, thr, True, source=True) for n in feeds]
    ctx.close()
    out["kernels"] = [kernel_share(blob, a.precision, n, a.rounds, a.warmup, src, thr) for n in feeds]
    if a.source:
        out["kernels_source"] = [kernel_share(blob, a.precision, n, a.rounds, a.warmup, src, thr, source=True) for n in feeds]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
