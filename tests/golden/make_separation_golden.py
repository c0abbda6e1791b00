"""Records tests/golden/separation_launch_plan.json: for each case of CASES, one call on a profiling fp32 context of the development
build -- the table [kernel, launches, flops, bytes] of that call (ss_get_kernel_stats) and the SHA-256 of the bytes it returned (region
bands: the ss_region_band records, then the profiles).  tests/test_gpu_separation_plan.py repeats the calls (run_cases) and asserts the
same tables and hashes.  Needs the GPU.

The file pins the separation's launches and output bytes to the commit it was recorded on: run this on a checkout of the commit whose
behaviour is to be kept (the parent of a refactor), never on the code under test.

    python tests/golden/make_separation_golden.py [--out FILE]

The cases are the smallest that take every branch of the plan: every call form, pieces and chunks moved through short recordings by the
development build's budgets, intervals whose bins touch, an interval clamped at either end, no interval at all, and region bands cut
into pieces of one tile."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "separation_launch_plan.json")

# (name, call, fmt, sample rate, channels, seconds, seed, regions, budget: frames per chunk / bins per piece, 0: the product's)
CASES = [
    ("mix 8k mono u8", "separate_pcm", "u8", 8000, 1, 3.0, 81, [(0.5, 2.5)], 16),
    ("mix 48k stereo pcm16", "separate_pcm", "pcm16", 48000, 2, 4.0, 82, [(0.5, 1.5), (1.52, 9.0)], 17),
    ("each 22k 3ch pcm24", "separate_pcm_channels", "pcm24", 22050, 3, 3.0, 83, [(0.4, 2.2)], 0),
    ("each source 44k stereo f32", "separate_pcm_channels_source", "f32", 44100, 2, 3.0, 84, [(-0.5, 1.3)], 24),
    ("mix 192k mono pcm16 no region", "separate_pcm", "pcm16", 192000, 1, 1.0, 85, [], 0),
    ("bands 16k 2 files", "region_bands", "pcm16", 16000, 2, 6.0, 86, [(1.0, 2.5), (2.0, 3.5), (4.0, 4.0)], 64),
]


def run_cases():
    """-> {case name: {"stats": [[kernel, launches, flops, bytes], ...], "sha256": hex}}; the process must have loaded the development
    build (SOFTSPOKEN_LIB)."""
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from softspoken_amd import synth, native
    import separation_ref as R
    import test_gpu_separation as T
    ctx = T._head_ctx(native, R.spread_head(synth.make_state_dict(0)), profile=True)
    ctx.set_chunk(7)                                     # the sums of every case cross passes
    out = {}
    try:
        for name, call, fmt, sr, ch, seconds, seed, regions, budget in CASES:
            rec = T._make(fmt, sr, ch, seconds, seed, scale=0.5)
            data, info, _, _ = rec
            if call == "region_bands":
                ctx.reset()
                fid = ctx.add_pcm_channels(data, info.format, sr, ch, info.frames)
                ctx.debug_set_bands_budget(budget)
                ctx.reset_stats()
                bands, prof = ctx.region_bands(fid, regions, n_channels=ch, profile=True)
                blob = bands.tobytes() + prof.tobytes()
            else:
                if len(regions) == 2:                    # the two intervals stay two, and their bin ranges touch or overlap
                    rg = native.separation_plan(sr, info.frames, regions)["ranges"]
                    assert len(rg) == 2 and rg[1]["bin_first"] <= rg[0]["bin_last"] + 1, rg
                ctx.debug_set_separation_budget(budget)
                ctx.reset_stats()
                blob = getattr(ctx, call)(*T._sil_args(rec, sr), regions).tobytes()
            stats = [[k["name"], int(k["launches"]), float(k["flops"]), float(k["bytes"])] for k in ctx.kernel_stats()]
            out[name] = {"stats": stats, "sha256": hashlib.sha256(blob).hexdigest()}
    finally:
        ctx.close()
    return out


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    with open(path, "w") as f:
        json.dump(run_cases(), f, indent=1)
        f.write("\n")
    print("wrote", path)
