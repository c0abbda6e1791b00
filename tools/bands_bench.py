"""Region bands (ss_region_bands, settings.hip_region_bands = '1'), one JSON line.  Not the flagship benchmark (bench.py).

    python tools/bands_bench.py [--minutes 10] [--rate 48000] [--speech 60] [--runs 5] [--precisions f16x2,fp32]

A stereo recording with `speech` seconds of regions (2 s each, spread evenly over the file), per precision, mix and each:
  bands_call   ss_region_bands over all regions, host clock around the call (it ends in a device synchronise)
  maps_numpy   what could be done before: ss_separation_maps over each region's bins (one device -> host copy of 2 x n_bins x 128
               floats per region and channel) and the numpy reduction of tests/bands_ref.py on the host (its long-double profile
               and bounds)
  maps_only    the ss_separation_maps calls of that route alone: the route's floor whatever reduction the user writes
  kernel_ms    the library's event timing of one ss_region_bands call (a profiling context): the two band kernels against the
               call's other launches
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from softspoken_amd import checkpoint, native, synth  # noqa: E402
import bands_ref as B  # noqa: E402
import separation_ref as R  # noqa: E402


def _stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3), max_ms=round(float(np.max(ms)), 3))


def case(precision, blob, pcm, sr, regions, each, runs):
    frames, ch = pcm.shape
    flat = pcm.reshape(-1)
    nsig = ch if each else 1
    out = {}
    for profile in (False, True):
        ctx = native.Context(blob, 0, precision=precision, profile=profile)
        ctx.reset()
        fid = (ctx.add_pcm_channels if each else ctx.add_pcm)(flat, native.PCM_S16, sr, ch, frames)
        _, n_bins = R.file_geometry(sr, frames)

        def bands():
            return ctx.region_bands(fid, regions, nsig)

        def maps_only():
            got = []
            for s, e in regions:
                b0, cnt = native.region_bins(s, e, n_bins)
                got.append((b0, [ctx.separation_maps(fid + c, b0, cnt) for c in range(nsig)]) if cnt else (b0, None))
            return got

        def maps_numpy():
            rows = []
            for (s, e), (b0, maps) in zip(regions, maps_only()):
                rows.append([B.reference(m, b0, [(s, e)])[0] for m in maps] if maps else None)
            return rows

        if profile:
            bands()
            ctx.reset_stats()
            bands()
            st = {k["name"]: k["total_ms"] for k in ctx.kernel_stats()}
            band = sum(v for k, v in st.items() if k.startswith("band_"))
            out["kernel_ms"] = dict(band_profile_kernel=round(st.get("band_profile_kernel", 0.0), 4),
                                    band_bounds_kernel=round(st.get("band_bounds_kernel", 0.0), 4),
                                    all_launches=round(sum(st.values()), 3), band_share=round(band / max(sum(st.values()), 1e-12), 6))
        else:
            got = bands()
            ref = maps_numpy()
            same = all(r is None or all(int(g["band_low"]) == x["band_low"] and int(g["band_high"]) == x["band_high"] and
                                        int(g["band_peak"]) == x["band_peak"] for g, x in zip(np.atleast_1d(gr), r))
                       for gr, r in zip(got, ref))
            times = {"bands_call": [], "maps_numpy": [], "maps_only": []}
            for _ in range(runs):                                  # alternating, so that all see the same neighbours on the card
                for name, fn in (("bands_call", bands), ("maps_numpy", maps_numpy), ("maps_only", maps_only)):
                    t0 = time.perf_counter()
                    fn()
                    times[name].append(1e3 * (time.perf_counter() - t0))
            out.update({k: _stats(v) for k, v in times.items()})
            out.update(same_bands=bool(same), regions=len(regions), estimates=int((np.asarray(got)["band_low"] >= 0).sum()),
                       speedup_vs_maps_numpy=round(out["maps_numpy"]["median_ms"] / out["bands_call"]["median_ms"], 2),
                       speedup_vs_maps_only=round(out["maps_only"]["median_ms"] / out["bands_call"]["median_ms"], 2))
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--speech", type=float, default=60.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--precisions", default="f16x2,fp32")
    a = ap.parse_args()
    pcm = np.ascontiguousarray(synth.to_pcm16(synth.synth_audio(3004, 60.0 * a.minutes, a.rate, 2)))     # [frames, 2]
    n = max(1, int(round(a.speech / 2.0)))
    gap = 60.0 * a.minutes / n
    regions = [(k * gap + 0.5, k * gap + 2.5) for k in range(n)]
    blob = checkpoint.pack_state_dict(R.spread_head(synth.make_state_dict(0)))
    out = dict(tool="bands_bench", minutes=a.minutes, rate=a.rate, speech_s=a.speech, runs=a.runs)
    for p in a.precisions.split(","):
        out[p] = {mode: case(p, blob, pcm, a.rate, regions, mode == "each", a.runs) for mode in ("mix", "each")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
