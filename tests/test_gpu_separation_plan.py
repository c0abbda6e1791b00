"""The separation silencer's and the region bands' launches and output bytes, pinned to tests/golden/separation_launch_plan.json: for
each case of tests/golden/make_separation_golden.py (every call form, the development build's budgets moving the cuts through short
recordings) the table [kernel, launches, flops, bytes] of the call and the SHA-256 of the bytes it returned are those recorded on the
commit before the host plan moved into sep_plan.h.  A difference is a finding about the code, never a reason to record the file anew."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_launch_tables_and_bytes_are_the_recorded_ones(build_all, tmp_path):
    from softspoken_amd import build as hip_build
    with open(os.path.join(GOLDEN, "separation_launch_plan.json")) as f:
        want = json.load(f)
    out = str(tmp_path / "plan.json")
    e = dict(os.environ); e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_separation_golden.py"), "--out", out], env=e, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    with open(out) as f:
        got = json.load(f)
    assert list(got) == list(want) and len(want) == 6
    for name in want:
        for g, w in zip(got[name]["stats"], want[name]["stats"]):
            assert g == w, (name, g, w)
        assert len(got[name]["stats"]) == len(want[name]["stats"]), name
        assert got[name]["sha256"] == want[name]["sha256"], name
