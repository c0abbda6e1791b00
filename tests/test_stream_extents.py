"""The extents of every stream step, on the CPU: tests/stream_extents.cpp drives the host-only stages of a step
(softspoken_amd/csrc/stream_plan.h: layout, upload packer, commit) over seeded populations of every stream kind with fake buffer
addresses and checks every range every descriptor reads or writes.  It is a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer (nothing is loaded into Python under a sanitizer); it links the built library for the host rules the
stages call (ss_resampled_length, ss_plan_windows_step, ss_window_start_bin, ss_stream_output_limit, the run merger, bin times)."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS = ("StreamCopy pre", "StreamCopy post", "StreamDecode", "StreamDecodeChannels", "StreamResample", "StreamAvg", "StreamUnion", "StreamMap",
         "window offset", "StreamSilence", "StreamSilenceSource", "StreamCopyBytes", "StreamBand", "StreamBandEv")


def test_plan_header_needs_no_hip_header(tmp_path):
    """stream_plan.h and what it includes compile with a plain C++ compiler and never name a HIP header."""
    csrc = os.path.join(ROOT, "softspoken_amd", "csrc")
    for h in ("stream_plan.h", "stream_desc.h", "hostdefs.h"):
        with open(os.path.join(csrc, h)) as f:
            includes = [line for line in f if line.lstrip().startswith("#include")]
        assert includes and not any("hip" in line or "kernels.h" in line or "engine.h" in line for line in includes), (h, includes)
    src = tmp_path / "only_header.cpp"
    src.write_text('#include "%s"\nint main() { return 0; }\n' % os.path.join(csrc, "stream_plan.h"))
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_every_step_stays_inside_its_buffers(build_all, tmp_path):
    from softspoken_amd import build as hip_build
    lib_dir = os.path.dirname(hip_build.LIB)
    exe = str(tmp_path / "stream_extents")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
           os.path.join(HERE, "stream_extents.cpp"), "-o", exe, "-L" + lib_dir, "-lsoftspoken_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "warning" not in r.stdout, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("stream_extents: ok"), r.stdout
    assert "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout
    for kind in KINDS:                                                  # every kind of descriptor was checked
        m = re.search(r"^\s+%s\s+(\d+)$" % re.escape(kind), r.stdout, re.M)
        assert m and int(m.group(1)) > 0, kind
    m = re.search(r"band lanes split over passes (\d+), passes shared by lanes (\d+), stream-steps before a first push (\d+), stream-steps from an image (\d+)", r.stdout)
    assert m and all(int(g) > 0 for g in m.groups()), r.stdout
