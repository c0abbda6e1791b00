"""Each-channel streams (ss_stream_open_channels) against what could be done before, one JSON line.  Not the flagship benchmark
(bench.py).

    python tools/stream_channels_bench.py [--precision f16x2] [--feeds 1,64,512] [--rounds 40] [--warmup 10]

N live feeds of 48 kHz 16-bit stereo, each pushed 0.6 s per round with one step per round (timed after `warmup` rounds, when every
lane runs one window per round), in three forms:
  each:   N each-channel streams (two lanes each: 2 N windows per step, one merged table per feed)
  mono2:  the host de-interleaves every piece and pushes it to two mono streams per feed (2 N streams, 2 N windows, no merged table)
  mix:    N mix streams (N windows per step): what a stream did before
step p50 / p99: host clock around the pushes' step (ss_stream_step ends in a device synchronise); the de-interleave and the pushes are
timed apart (feed_ms_p50).  kernels: a second, profiled pass of the each form -- the two launches it adds, per step, from
ss_get_kernel_stats.
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

SR, PIECE = 48000, 28800                                  # 0.6 s


def _open(ctx, form, n):
    if form == "each":
        return [ctx.stream_open_channels(native.PCM_S16, SR, 2, 0.1, 0.5) for _ in range(n)]
    if form == "mix":
        return [ctx.stream_open(native.PCM_S16, SR, 2, 0.1, 0.5) for _ in range(n)]
    return [ctx.stream_open(native.PCM_S16, SR, 1, 0.1, 0.5) for _ in range(2 * n)]


def live(ctx, form, n, rounds, warmup, src):
    sids = _open(ctx, form, n)
    step, feed = [], []
    for r in range(warmup + rounds):
        t0 = time.perf_counter()
        for k in range(n):
            at = ((r + 7 * k) * PIECE) % (len(src) - PIECE)
            piece = src[at:at + PIECE]
            if form == "mono2":
                planes = np.ascontiguousarray(piece.T)     # the host de-interleave
                ctx.stream_push(sids[2 * k], planes[0], frames=PIECE)
                ctx.stream_push(sids[2 * k + 1], planes[1], frames=PIECE)
            else:
                ctx.stream_push(sids[k], piece, frames=PIECE)
        t1 = time.perf_counter()
        ctx.stream_step()
        t2 = time.perf_counter()
        if r >= warmup:
            feed.append(t1 - t0); step.append(t2 - t1)
    for sid in sids:
        ctx.stream_free(sid)
    t = np.array(step)
    return dict(step_ms_p50=round(1e3 * float(np.percentile(t, 50)), 3), step_ms_p99=round(1e3 * float(np.percentile(t, 99)), 3),
                feed_ms_p50=round(1e3 * float(np.percentile(feed, 50)), 3), audio_s_per_s=round(n * 0.6 * len(t) / (t.sum() + np.sum(feed)), 1))


def new_launches(blob, precision, n, rounds, warmup, src):
    ctx = native.Context(blob, 0, precision=precision, profile=True)
    sids = _open(ctx, "each", n)
    for r in range(warmup + rounds):
        if r == warmup:
            ctx.reset_stats()
        for k in range(n):
            at = ((r + 7 * k) * PIECE) % (len(src) - PIECE)
            ctx.stream_push(sids[k], src[at:at + PIECE], frames=PIECE)
        ctx.stream_step()
    st = {s["name"]: s for s in ctx.kernel_stats()}
    ctx.close()
    out = {}
    for name in ("stream_decode_channels", "stream_union", "stream_decode", "stream_average"):
        if name in st and st[name]["launches"]:
            out[name] = dict(us_per_step=round(1e3 * st[name]["total_ms"] / st[name]["launches"], 2), launches=st[name]["launches"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x2")
    ap.add_argument("--feeds", default="1,64,512")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    blob = checkpoint.pack_state_dict(synth.make_state_dict(0))
    ctx = native.Context(blob, 0, precision=a.precision)
    src = np.ascontiguousarray(synth.to_pcm16(synth.synth_audio(3004, 120.0, SR, 2)))      # [frames, 2]
    live(ctx, "each", 2, 4, 8, src)                        # warm-up: workspace, tap tables, kernels
    rows = []
    for n in (int(v) for v in a.feeds.split(",")):
        row = dict(feeds=n)
        for form in ("each", "mono2", "mix", "each", "mono2", "mix"):        # alternating: two runs of each, the better p50 kept
            res = live(ctx, form, n, a.rounds, a.warmup, src)
            if form not in row or res["step_ms_p50"] < row[form]["step_ms_p50"]:
                row[form] = res
        if not a.no_kernels:
            row["kernels"] = new_launches(blob, a.precision, n, min(a.rounds, 20), a.warmup, src)
        rows.append(row)
    ctx.close()
    print(json.dumps(dict(tool="stream_channels_bench", precision=a.precision, rate=SR, channels=2, piece_s=0.6, live=rows)))


if __name__ == "__main__":
    main()
