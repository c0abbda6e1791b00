"""The host plan of the band silencer on the CPU: tests/box_plan_check.cpp puts seeded box tables, recordings and the frame budgets 16,
17, 23 and 64 through plan_boxes (softspoken_amd/csrc/sep_plan.h) and holds the merged intervals, every frame's active boxes (the support
rule walked sample by sample), every row's bins, and every segment, chunk and record index to a brute-force restatement; it also holds
plan_synthesis, which shares the cuts, to the loop it had before on the same inputs.  A stand-alone program built with AddressSanitizer
and UndefinedBehaviorSanitizer (nothing is loaded into Python under a sanitizer); it links the built library for the host rules the
plans call (silence_ranges, ss_plan_windows, ss_resampled_length)."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PROPERTIES = ("boxes: merged intervals and their frames", "boxes: rows", "boxes: nothing without an interval", "boxes: chunk within budget",
              "blend: reads inside the chunk's records", "boxes: segments of a chunk", "boxes: segments partition the interval",
              "boxes: active boxes of a frame", "synthesis: old vectors")


def test_box_plan_matches_its_restatement(build_all, tmp_path):
    from softspoken_amd import build as hip_build
    lib_dir = os.path.dirname(hip_build.LIB)
    exe = str(tmp_path / "box_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
           os.path.join(HERE, "box_plan_check.cpp"), "-o", exe, "-L" + lib_dir, "-lsoftspoken_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "warning" not in r.stdout, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("box_plan_check: ok"), r.stdout
    assert "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout
    counts = {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"^  (\S.*?)\s+(\d+)$", r.stdout, re.M)}
    assert counts.get("cases", 1) and all(v > 0 for v in counts.values()), counts
    for prop in PROPERTIES:
        assert counts.get(prop, 0) > 0, prop
