"""The host plan of PCM ingest, on the CPU: tests/ingest_plan_check.cpp puts seeded batches -- every format, rate, channel count, both
calls, files of 0 and 1 frames and around a fused item's input span, a used arena -- through softspoken_amd/csrc/ingest_plan.h and holds
every range the kernels would address through the plan (slots, PCM ranges, mono planes, descriptor regions, resampler inputs, LDS tiles)
to a restatement.  It is a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer (nothing is loaded into Python
under a sanitizer); it links the built library for ss_resampled_length.

The tap table: design_taps is bit for bit the table of the loop it was moved from, for every rate of the list -- the SHA-256 of each is
in tests/golden/resample_taps.json, recorded from that loop compiled verbatim on the commit before the move.  Against
oracle_np.resample_plan that loop's table is bit-identical at every rate of the list as well, and so must this one be."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 192000, 768000, 48001)
PROPERTIES = ("plan: rate rule and signal count", "route: the three conditions",
              "slots: aligned, ascending, disjoint, inside the extent, slack behind", "slots: the fill covers exactly the new extent",
              "slots: n_padded, out_off and duration by the parent's formulas", "channels: slots exactly out_stride apart",
              "channels: the pair route's BatchFiles address the ChanFile's planes", "pcm: ranges back to back inside sum(frames) ch bps",
              "mono: planes 16-byte aligned, disjoint, inside the mono size", "decode: 22 050 Hz files go straight into their slots",
              "descriptors: regions disjoint, sized, aligned", "resampler: input reads inside the file or on a zeroed side",
              "fused geometry: LDS, span, tile places, 16-byte reads, lanes", "unfused geometry: the plain kernel",
              "unfused geometry: LDS kernel, staged span", "items: items_per_file n_files < 2^30, or refused",
              "costs: the three (flops, bytes) pairs", "limits: check_pcm_args' bounds and the signal count", "taps: [L][2 half] floats")
# route and unfused kernel per rate, as the program prints them.  32 kHz (L 441, M 640, half 47) does not take the fused route: its tile
# and 441 tap rows of 95 floats come to 206 KB of LDS, and the 167 KB table alone is past the LDS resampler's 150 KB, so it runs the plain
# kernel -- as on the commit the geometry was moved from
ROUTES = {8000: ("fused", "LDS kernel, staged span"), 16000: ("fused", "LDS kernel, staged span"), 32000: ("pair", "plain kernel"),
          48000: ("fused", "LDS kernel, staged span"), 11025: ("pair", "LDS kernel, staged span"), 44100: ("pair", "LDS kernel, staged span"),
          88200: ("pair", "LDS kernel, staged span"), 96000: ("pair", "plain kernel"), 192000: ("pair", "plain kernel"),
          768000: ("pair", "plain kernel"), 48001: ("pair", "plain kernel"), 22050: ("straight decode", "-")}


def test_plan_header_needs_no_hip_header(tmp_path):
    """ingest_plan.h and what it includes compile with a plain C++ compiler and never name a HIP header."""
    csrc = os.path.join(ROOT, "softspoken_amd", "csrc")
    for h in ("ingest_plan.h", "hostdefs.h", "stream_desc.h"):
        with open(os.path.join(csrc, h)) as f:
            includes = [line for line in f if line.lstrip().startswith("#include")]
        assert includes and not any("hip" in line or "kernels.h" in line or "engine.h" in line for line in includes), (h, includes)
    src = tmp_path / "only_header.cpp"
    src.write_text('#include "%s"\nint main() { return 0; }\n' % os.path.join(csrc, "ingest_plan.h"))
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


@pytest.fixture(scope="module")
def check_run(build_all, tmp_path_factory):
    """(the program's output, the directory of the tables it wrote)"""
    from softspoken_amd import build as hip_build
    lib_dir = os.path.dirname(hip_build.LIB)
    tmp = tmp_path_factory.mktemp("ingest_plan")
    exe = str(tmp / "ingest_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
           os.path.join(HERE, "ingest_plan_check.cpp"), "-o", exe, "-L" + lib_dir, "-lsoftspoken_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "warning" not in r.stdout, r.stdout
    r = subprocess.run([exe, str(tmp)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ingest_plan_check: ok"), r.stdout
    assert "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout
    return r.stdout, str(tmp)


def test_every_plan_matches_its_restatement(check_run):
    out, _ = check_run
    m = re.search(r"^(\d+) seeded cases", out, re.M)
    assert m and int(m.group(1)) >= 512
    counts = {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"^  (\S.*?)\s+(\d+)$", out, re.M)}
    assert counts and all(v > 0 for v in counts.values()), counts        # every count the program prints
    for prop in PROPERTIES:                                              # and every property was checked
        assert counts.get(prop, 0) > 0, prop


def test_routes_per_rate(check_run):
    out, _ = check_run
    got = {int(m.group(1)): (m.group(2).strip(), m.group(3).strip())
           for m in re.finditer(r"^ +(\d+) Hz  L .*? half +\d+  (.{15}) unfused: (.*)$", out, re.M)}
    assert set(got) == set(RATES)
    for sr, want in ROUTES.items():
        assert got[sr] == want, (sr, got[sr])


def test_tap_table_is_the_recorded_one_and_the_oracle_s(check_run):
    from oracle import oracle_np as O
    _, tmp = check_run
    with open(os.path.join(HERE, "golden", "resample_taps.json")) as f:
        want = json.load(f)
    assert sorted(int(k) for k in want) == sorted(RATES)
    for sr in RATES:
        t = np.fromfile(os.path.join(tmp, "taps_%d.f32" % sr), dtype=np.float32)
        assert hashlib.sha256(t.tobytes()).hexdigest() == want[str(sr)]["sha256"], sr
        assert t.size == want[str(sr)]["floats"], sr
        L, M, half, taps = O.resample_plan(sr)[:4]
        o = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        assert (o.size == t.size and np.array_equal(o.view(np.uint32), t.view(np.uint32))) == want[str(sr)]["equals_oracle"], sr
