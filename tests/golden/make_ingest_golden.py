"""Records tests/golden/ingest_launch_plan.json: for each case of CASES, the ingest calls of one job on a profiling fp32 audio-only
context of the development build -- the table [kernel, launches, flops, bytes] of those calls (ss_get_kernel_stats), the file ids they
returned and the SHA-256 over every new signal's length and padded samples (ss_read_signal).  tests/test_gpu_ingest_plan.py repeats the
calls (run_cases) and asserts the same tables, ids and hashes.  Needs the GPU.

The file pins ingest's launches and stored samples to the commit it was recorded on: run this on a checkout of the commit whose
behaviour is to be kept (the parent of a refactor), never on the code under test.

    python tests/golden/make_ingest_golden.py [--out FILE]

The cases are the smallest that take every branch of the ingest plan: the three routes (straight decode, fused resampler, decode +
resample_batch pair) in the mono and the per-channel call, the fused kernels' fast and general fetch, both unfused resampler kernels, an
empty file, files one frame below and above a fused item's input span (24 rows x 320 = 7680 frames at 48 kHz), five channels (three
passes of two), and three calls whose slots lie behind one another in one job.  Every resampling case makes at least L outputs per
signal (441 at 16 kHz, 147 at 48 and 96 kHz), the files of 0 and 1 frames aside, so every row of the tap table is read."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "ingest_launch_plan.json")

FMT = {"u8": 1, "pcm16": 2, "pcm24": 3, "f32": 5}
BPS = {"u8": 1, "pcm16": 2, "pcm24": 3, "f32": 4}
SPAN48 = 7680                                             # input frames of one fused item at 48 kHz

# (name, environment of the development build, [(call, format, rate, channels, frames per file), ...]); call: add_pcm / channels (host
# pointer, one file), batch / channels_batch (device pointer), f32 (ss_add_f32_22k of `frames` samples)
CASES = [
    ("1 22k u8 mono", {}, [("add_pcm", "u8", 22050, 1, [1501])]),
    ("2 48k pcm16 stereo batch", {}, [("batch", "pcm16", 48000, 2, [0, 1, SPAN48 - 1, SPAN48 + 1, 9000])]),
    ("3 48k pcm24 3ch", {}, [("add_pcm", "pcm24", 48000, 3, [2003])]),
    ("4 16k pcm16 mono", {}, [("add_pcm", "pcm16", 16000, 1, [1999])]),
    ("5 44k f32 stereo batch", {}, [("batch", "f32", 44100, 2, [3001, 1234])]),
    ("6 96k pcm16 mono", {}, [("add_pcm", "pcm16", 96000, 1, [2501])]),
    ("7 22k pcm24 3ch channels", {}, [("channels", "pcm24", 22050, 3, [1203])]),
    ("8 48k pcm16 stereo channels batch", {}, [("channels_batch", "pcm16", 48000, 2, [SPAN48 - 1, SPAN48 + 1, 1])]),
    ("9 48k f32 5ch channels", {}, [("channels", "f32", 48000, 5, [1777])]),
    ("10 44k pcm16 stereo channels", {}, [("channels", "pcm16", 44100, 2, [2222])]),
    ("11 16k pcm16 1ch channels", {}, [("channels", "pcm16", 16000, 1, [1999])]),              # forwards to mono: case 4's table and samples
    ("12 48k pcm16 stereo batch unfused", {"SOFTSPOKEN_RES3": "0"}, [("batch", "pcm16", 48000, 2, [0, 1, SPAN48 - 1, SPAN48 + 1, 9000])]),
    ("13 three calls one job", {}, [("add_pcm", "pcm16", 48000, 2, [1001]), ("channels", "pcm24", 44100, 3, [1502]), ("f32", "f32", 22050, 1, [777]),
                                    ("channels_batch", "u8", 22050, 2, [5, 0, 9])]),
]
SEED_OF = {"4 16k pcm16 mono": 1004, "11 16k pcm16 1ch channels": 1004, "2 48k pcm16 stereo batch": 1002, "12 48k pcm16 stereo batch unfused": 1002}


NOTES = ("failed batch, on the recorded commit: both batch calls test every file's limits before they reserve anything, so a batch whose second "
         "file is above the frame limit returned SS_ERR_ARG and left the job as it was, as recorded here.  Behind the reservations -- an "
         "allocation or a launch failing -- that commit's per-channel call rolled its files back and its mixdown call did not: it left "
         "files and arena_used advanced, naming signals never written.  No test can provoke that failure; the guarantee for it is "
         "ingest_run's order (files, arena_used and logits_valid change behind the last launch).")


def pcm_bytes(rng, fmt, samples):
    """`samples` seeded samples of the format, as bytes"""
    if fmt == "f32":
        return rng.uniform(-1.0, 1.0, samples).astype(np.float32).view(np.uint8)
    return rng.integers(0, 256, samples * BPS[fmt], dtype=np.uint8)


def one_call(ctx, rng, call, fmt, sr, ch, frames):
    """-> (first file id, number of new signals)"""
    if call == "f32":
        return ctx.add_f32_22k(rng.uniform(-1.0, 1.0, frames[0]).astype(np.float32)), 1
    data = np.ascontiguousarray(pcm_bytes(rng, fmt, int(sum(frames)) * ch))
    each = call.startswith("channels")
    if call in ("add_pcm", "channels"):
        fid = (ctx.add_pcm_channels if each else ctx.add_pcm)(data, FMT[fmt], sr, ch, frames[0])
    else:
        dev = ctx.device_alloc(data.nbytes + 16)
        try:
            if data.nbytes:
                ctx.device_upload(dev, data)
            fid = (ctx.add_pcm_channels_batch_device if each else ctx.add_pcm_batch_device)(dev, FMT[fmt], sr, ch, frames, host_copy=data)
            ctx.sync()
        finally:
            ctx.device_free(dev)
    return fid, len(frames) * (ch if each else 1)


def failed_batch(ctx, native):
    """The transactional guarantee: a batch whose second file is above the frame limit returns its error, the next id names no signal
    afterwards, and a following good call gets the id the failed one would have returned."""
    ctx.reset()
    rng = np.random.default_rng(77)
    first, _ = one_call(ctx, rng, "add_pcm", "pcm16", 48000, 1, [600])
    out = {}
    for call in ("batch", "channels_batch"):
        dev = ctx.device_alloc(4096)
        try:
            fn = ctx.add_pcm_channels_batch_device if call == "channels_batch" else ctx.add_pcm_batch_device
            try:
                fn(dev, FMT["pcm16"], 48000, 2, [100, (1 << 36) + 1])
                err = None
            except native.NativeError as e:
                err = int(e.code)
        finally:
            ctx.device_free(dev)
        nxt = first + 1 + (0 if call == "batch" else 1)
        out[call] = {"error": err, "signal_length_next": int(ctx.signal_length(nxt)), "num_windows_next": int(ctx.num_windows(nxt))}
        good, _ = one_call(ctx, rng, "add_pcm", "pcm16", 48000, 1, [600])
        out[call]["good_id"] = int(good)
    return out


def run_cases():
    """-> {case name: {"stats": [[kernel, launches, flops, bytes], ...], "ids": [...], "sha256": hex}, "failed batch": {...}, "notes": text}; the
    process must have loaded the development build (SOFTSPOKEN_LIB)."""
    sys.path.insert(0, ROOT)
    from softspoken_amd import native
    ctx = native.Context(None, 0, profile=True)
    out = {}
    try:
        for i, (name, env, calls) in enumerate(CASES):
            rng = np.random.default_rng(SEED_OF.get(name, 2000 + i))
            for k, v in env.items():
                os.environ[k] = v
            try:
                ctx.reset()
                ctx.reset_stats()
                ids, h = [], hashlib.sha256()
                for call, fmt, sr, ch, frames in calls:
                    fid, n = one_call(ctx, rng, call, fmt, sr, ch, frames)
                    ids.append(int(fid))
                    for f in range(fid, fid + n):
                        x = ctx.read_signal(f, padded=True)
                        h.update(np.array([ctx.signal_length(f), x.size], dtype=np.int64).tobytes())
                        h.update(x.tobytes())
                stats = [[k["name"], int(k["launches"]), float(k["flops"]), float(k["bytes"])] for k in ctx.kernel_stats()]
                out[name] = {"stats": stats, "ids": ids, "sha256": h.hexdigest()}
            finally:
                for k in env:
                    del os.environ[k]
        out["failed batch"] = failed_batch(ctx, native)
        out["notes"] = NOTES
    finally:
        ctx.close()
    return out


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    with open(path, "w") as f:
        json.dump(run_cases(), f, indent=1)
        f.write("\n")
    print("wrote", path)
