"""Source-output silencing against the 16-bit path, one JSON line.  Not the flagship benchmark (bench.py).

    python tools/source_output_bench.py [--baseline-lib PATH] [--minutes 10] [--runs 5] [--skip-separation]

A recording of `minutes` of 48 kHz stereo with 60 s erased (six 10 s regions).  Every figure is the wall time of one call from host
memory to host memory (upload, kernel, download) into an output array allocated and touched beforehand (a fresh array's page faults
would be timed with the copy), one warm-up call and then `runs` timed ones, reported as median [min, max] in ms:

  zeroing     ss_silence_pcm (S16) of --baseline-lib (default: this tree's library; give the parent commit's build to compare the two
              trees) and ss_silence_pcm_source (S16) of this tree, alternating call by call in one process; then ss_silence_pcm_source
              for S24 and F32 (more output bytes; no bar)
  kernels     silence_source_kernel's and sep_blend_source_kernel's device time and bytes from a profiling context
  separation  ss_separate_pcm and ss_separate_pcm_source on the S24 recording, alternating (the session checkpoint, fp32)

The baseline library is driven through ctypes alone: it need not export what this tree added.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from softspoken_amd import checkpoint, native, synth  # noqa: E402

SR, CH = 48000, 2


def recording(minutes, fmt):
    """minutes of 48 kHz stereo: 20 s of synthetic audio tiled (the silencer's time does not depend on the samples)."""
    x = synth.synth_audio(5, 20.0, SR, CH, with_silence=False).T.reshape(-1, CH).astype(np.float32) * np.float32(0.5)
    x = np.tile(x, (int(np.ceil(minutes * 60 / 20.0)), 1))[: int(minutes * 60 * SR)]
    if fmt == native.PCM_S16:
        return np.rint(x * 32768).clip(-32768, 32767).astype("<i2").view(np.uint8).reshape(-1)
    if fmt == native.PCM_S24:
        v = np.rint(x.astype(np.float64) * 8388608).clip(-8388608, 8388607).astype("<i4").reshape(-1)
        return np.ascontiguousarray(v.view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)
    return x.astype("<f4").view(np.uint8).reshape(-1)


def regions(minutes):
    span = minutes * 60.0
    return [(span * (k + 0.5) / 6.0 - 5.0, span * (k + 0.5) / 6.0 + 5.0) for k in range(6)]


def stats(ms):
    a = np.array(ms)
    return dict(median_ms=round(float(np.median(a)), 3), min_ms=round(float(a.min()), 3), max_ms=round(float(a.max()), 3),
                spread_ms=round(float(a.max() - a.min()), 3))


class Baseline:
    """ss_silence_pcm of any build of the library, through ctypes."""
    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.ss_create.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_void_p)]
        self.L.ss_silence_pcm.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        self.L.ss_destroy.argtypes = [C.c_void_p]
        self.h = C.c_void_p()
        assert self.L.ss_create(0, None, 0, 0, C.byref(self.h)) == 0

    def silence_pcm(self, pcm, fmt, frames, regs, out):
        arr = native._regions(regs)
        rc = self.L.ss_silence_pcm(self.h, pcm.ctypes.data_as(C.c_void_p), fmt, SR, CH, frames, arr, len(regs), out.ctypes.data_as(C.c_void_p))
        assert rc == 0, rc

    def close(self):
        self.L.ss_destroy(self.h)


def source_call(ctx, name, data, fmt, frames, regs, out, params=None):
    """One *_source entry point of this tree into the caller's array."""
    arr = native._regions(regs)
    args = (ctx._h, native._ptr(data), fmt, SR, CH, frames, arr, len(regs)) + ((C.byref(params),) if params is not None else ())
    rc = getattr(native.lib(), name)(*args, native._ptr(out), out.nbytes)
    assert rc == 0, (name, rc)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def alternate(a, b, runs):
    a(); b()                                               # one warm-up each: the device buffers grow here
    ta, tb = [], []
    for _ in range(runs):
        ta.append(timed(a)); tb.append(timed(b))
    return stats(ta), stats(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=native.LIB_PATH)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-separation", action="store_true")
    args = ap.parse_args()
    regs = regions(args.minutes)
    out = dict(minutes=args.minutes, runs=args.runs, sample_rate=SR, channels=CH, erased_s=60.0, baseline_lib=os.path.relpath(args.baseline_lib, ROOT))

    s16 = recording(args.minutes, native.PCM_S16)
    frames = s16.size // (2 * CH)
    base = Baseline(args.baseline_lib)
    ctx = native.Context(None, 0)
    o16 = np.zeros((frames, CH), dtype=np.int16)
    ob = np.zeros(frames * CH * 4, dtype=np.uint8)          # room for every encoding measured here
    z_base, z_src = alternate(lambda: base.silence_pcm(s16, native.PCM_S16, frames, regs, o16),
                              lambda: source_call(ctx, "ss_silence_pcm_source", s16, native.PCM_S16, frames, regs, ob[:s16.size]), args.runs)
    out["zeroing_s16"] = dict(baseline_silence_pcm=z_base, silence_pcm_source=z_src,
                              within_baseline_spread=bool(z_src["median_ms"] <= z_base["median_ms"] + z_base["spread_ms"]))
    base.close()
    recs = {"s24": (native.PCM_S24, recording(args.minutes, native.PCM_S24)), "f32": (native.PCM_F32, recording(args.minutes, native.PCM_F32))}
    for name, (fmt, data) in recs.items():
        fn = lambda: source_call(ctx, "ss_silence_pcm_source", data, fmt, frames, regs, ob[:data.size])          # noqa: E731
        fn()
        out[f"zeroing_{name}"] = stats([timed(fn) for _ in range(args.runs)])
    ctx.close()

    prof = native.Context(None, 0, profile=True)
    kern = {}
    for name, (fmt, data) in dict(s16=(native.PCM_S16, s16), **recs).items():
        prof.silence_pcm_source(data, fmt, SR, CH, frames, regs)
        prof.reset_stats()
        for _ in range(args.runs):
            prof.silence_pcm_source(data, fmt, SR, CH, frames, regs)
        for st in prof.kernel_stats():
            if st["name"] == "silence_source_kernel":
                ms = st["total_ms"] / st["launches"]
                kern[f"silence_source_kernel_{name}"] = dict(ms=round(ms, 4), bytes=int(st["bytes"] / st["launches"]),
                                                            tb_per_s=round(st["bytes"] / st["launches"] / ms / 1e9, 3))
    prof.close()
    out["kernels"] = kern

    if not args.skip_separation:
        blob = checkpoint.pack_state_dict(synth.make_state_dict(0))
        sep = native.Context(blob, 0, precision="fp32", profile=True)
        fmt, data = recs["s24"]
        prm = native.separation_params(0.01, 0.0, "mute", 1)

        def sep16():
            rc = native.lib().ss_separate_pcm(sep._h, native._ptr(data), fmt, SR, CH, frames, native._regions(regs), len(regs), C.byref(prm),
                                              native._ptr(o16))
            assert rc == 0, rc
        a, b = alternate(sep16, lambda: source_call(sep, "ss_separate_pcm_source", data, fmt, frames, regs, ob[:data.size], prm), args.runs)
        out["separation_s24"] = dict(separate_pcm=a, separate_pcm_source=b)
        per = {}
        for st in sep.kernel_stats():
            if st["name"] in ("sep_blend_kernel", "sep_blend_source_kernel", "sep_transcode/silence_encode_kernel"):
                per[st["name"]] = dict(launches=int(st["launches"]), ms_per_launch=round(st["total_ms"] / max(st["launches"], 1), 4),
                                       bytes_per_launch=int(st["bytes"] / max(st["launches"], 1)))
        out["separation_kernels"] = per
        sep.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
