"""The host plan of the separation silencer and the region bands, on the CPU: tests/sep_plan_check.cpp puts seeded recordings, region
tables and budgets through softspoken_amd/csrc/sep_plan.h (plan_maps, plan_synthesis, plan_bands) and holds every index a kernel
would read -- gain rows, records, window slots, compact bins -- to a brute-force restatement.  It is a stand-alone program built with
AddressSanitizer and UndefinedBehaviorSanitizer (nothing is loaded into Python under a sanitizer); it links the built library for the
host rules the plans call (ss_plan_windows, ss_resampled_length, silence_ranges, rule 1 of the bands).

The blend's reads are checked at every sample of every segment in the cases that erase at most 400 000 samples.  In the longer cases
the program checks the first and the last sample of every hop block of a segment: inside a block kb = n / hop is fixed, so the four
records do not change and the position n - k hop + N / 2 rises with n, and the two ends bound every sample between them."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PROPERTIES = ("plan: FFT size and geometry", "synthesis: nothing without an interval", "bands: region ranges and union",
              "bands: pieces hold the union once", "maps: cbin ascending union", "maps: covering window has a slot", "maps: slots ascending", "maps: window offsets",
              "synthesis: segments partition the interval", "synthesis: segment length", "synthesis: chunk within budget",
              "synthesis: out0 ascends, lengths add up", "blend: reads inside the chunk's records", "synthesis: gain rows inside the table",
              "synthesis: frame bins and weight", "bands: tiles ascending and aligned", "bands: segment inside its piece",
              "bands: piece within budget", "bands: out indices each once", "bands: seg0 / nseg of the regions",
              "bands: seg0 / nseg of the pieces", "bands: caller's maps are one piece", "bands: caller's maps compact bin")


def test_plan_header_needs_no_hip_header(tmp_path):
    """sep_plan.h and what it includes compile with a plain C++ compiler and never name a HIP header."""
    csrc = os.path.join(ROOT, "softspoken_amd", "csrc")
    for h in ("sep_plan.h", "hostdefs.h"):
        with open(os.path.join(csrc, h)) as f:
            includes = [line for line in f if line.lstrip().startswith("#include")]
        assert includes and not any("hip" in line or "kernels.h" in line or "engine.h" in line for line in includes), (h, includes)
    src = tmp_path / "only_header.cpp"
    src.write_text('#include "%s"\nint main() { return 0; }\n' % os.path.join(csrc, "sep_plan.h"))
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_every_plan_matches_its_restatement(build_all, tmp_path):
    from softspoken_amd import build as hip_build
    lib_dir = os.path.dirname(hip_build.LIB)
    exe = str(tmp_path / "sep_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
           os.path.join(HERE, "sep_plan_check.cpp"), "-o", exe, "-L" + lib_dir, "-lsoftspoken_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "warning" not in r.stdout, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("sep_plan_check: ok"), r.stdout
    assert "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout
    counts = {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"^  (\S.*?)\s+(\d+)$", r.stdout, re.M)}
    assert counts and all(v > 0 for v in counts.values()), counts        # every count the program prints
    for prop in PROPERTIES:                                              # and every property was checked
        assert counts.get(prop, 0) > 0, prop
