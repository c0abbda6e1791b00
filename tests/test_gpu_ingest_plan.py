"""Ingest's launches and stored samples, pinned to tests/golden/ingest_launch_plan.json: for each case of
tests/golden/make_ingest_golden.py (the three routes in the mixdown and the per-channel call, both fetch forms of the fused kernels, both
unfused resampler kernels, an empty file, an item boundary, three calls in one job) the table [kernel, launches, flops, bytes], the file
ids and the SHA-256 over every new signal's length and padded samples are those recorded on the commit before the host plan moved into
ingest_plan.h.  A difference is a finding about the code, never a reason to record the file anew.

The failed batch: a batch call whose second file is above the frame limit returns SS_ERR_ARG, leaves the next file id naming no signal,
and the good call behind it gets that id -- for the mixdown and the per-channel call alike.  (On the recorded commit this case behaved the
same: the limits are tested before anything is reserved.  What that commit did not guarantee, a mixdown batch failing behind its
reservations -- an allocation or a launch --, cannot be provoked from a test: the development build's allocation hook reaches the
workspaces only.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def plans(build_all, tmp_path_factory):
    from softspoken_amd import build as hip_build
    with open(os.path.join(GOLDEN, "ingest_launch_plan.json")) as f:
        want = json.load(f)
    out = str(tmp_path_factory.mktemp("ingest") / "plan.json")
    e = dict(os.environ); e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
    e.pop("SOFTSPOKEN_RES3", None)
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_ingest_golden.py"), "--out", out], env=e, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    with open(out) as f:
        return json.load(f), want


def test_launch_tables_ids_and_samples_are_the_recorded_ones(plans):
    got, want = plans
    assert list(got) == list(want) and len(want) == 15 and got["notes"] == want["notes"]
    for name in want:
        if name in ("failed batch", "notes"):
            continue
        assert got[name]["stats"] == want[name]["stats"], name
        assert got[name]["ids"] == want[name]["ids"], name
        assert got[name]["sha256"] == want[name]["sha256"], name


def test_one_channel_per_channel_call_is_the_mixdown_call(plans):
    got, _ = plans
    assert got["11 16k pcm16 1ch channels"] == got["4 16k pcm16 mono"]


def test_unfused_pair_stores_the_fused_route_s_samples(plans):
    got, _ = plans
    a, b = got["2 48k pcm16 stereo batch"], got["12 48k pcm16 stereo batch unfused"]
    assert a["sha256"] == b["sha256"] and [s[0] for s in a["stats"]] == ["resample_fused"]
    assert [s[0] for s in b["stats"]] == ["decode_mono_batch", "resample_batch"]


def test_failed_batch_leaves_the_job_as_it_was(plans):
    got, _ = plans
    for call, first_free in (("batch", 1), ("channels_batch", 2)):
        r = got["failed batch"][call]
        assert r["error"] == 1, (call, r)                                   # SS_ERR_ARG
        assert r["signal_length_next"] == -1 and r["num_windows_next"] == -1, (call, r)
        assert r["good_id"] == first_free, (call, r)
