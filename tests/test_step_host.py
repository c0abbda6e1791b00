"""settings.step_size on the host side (no GPU): ss_plan_windows_step and ss_window_start_bin against the reference restated in
tests/step_ref.py, the rounding of ties, the default step against the fixed-step entry points, the refusals, the claims
include/softspoken.h makes about the accepted range, and the drop-in handing the setting to every context it uses."""
import math
import os

import numpy as np
import pytest

import step_ref as R
from softspoken_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (0.1, 99 / 512, 0.3, 0.45, 0.6, 0.75, 1.0, 1.5, 2.999, 3.0)
DURATIONS = (0, 0.01, 2.9, 3.0, 59.99, 600, 86400)
BAD_STEPS = (0, -1, 0.0999, 3.0001, float("nan"), float("inf"))
N_WINDOWS = 4000


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


@pytest.mark.parametrize("step", STEPS)
def test_plan_and_start_bins_equal_the_reference(native, step):
    for d in DURATIONS:
        want = R.plan(d, step)
        got = native.plan_windows(d, step)
        assert got.dtype == np.int64 and np.array_equal(got, want), (step, d, len(got), len(want))
        assert native.lib().ss_plan_windows_step(float(d), step, None, 0) == len(want)          # the count alone
        if len(want) > 3:                                                                       # a short buffer: cap entries written
            buf = np.full(5, -7, dtype=np.int64)
            assert native.lib().ss_plan_windows_step(float(d), step, native._ptr(buf), 3) == len(want)
            assert buf.tolist() == want[:3].tolist() + [-7, -7]
    L = native.lib()
    got = [L.ss_window_start_bin(i, step) for i in range(N_WINDOWS + 1)]
    assert got == [R.start_bin(i, step) for i in range(N_WINDOWS + 1)]
    assert native.window_start_bin(N_WINDOWS, step) == got[-1]


def test_ties_round_to_even(native):
    """99 / 512 s is exact in binary and gives i x 16.5 bins: a tie at every odd i (round-half-up gives 17, 33, 50, 66, 83)."""
    step = 99 / 512
    assert [i * step / R.TIME_RESOLUTION for i in range(1, 6)] == [16.5, 33.0, 49.5, 66.0, 82.5]
    assert [native.window_start_bin(i, step) for i in range(1, 6)] == [16, 33, 50, 66, 82]
    assert [R.start_bin(i, step) for i in range(1, 6)] == [16, 33, 50, 66, 82]


def test_default_step_is_the_fixed_step_entry_point(native):
    L = native.lib()
    assert math.floor(22050 * 0.6) == 13230 == native.STEP_SAMPLES and native.DEFAULT_STEP == 0.6
    for d in DURATIONS + (1.234, 7199.99):
        n = L.ss_plan_windows(float(d), None, 0)
        a, b = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        assert L.ss_plan_windows_step(float(d), 0.6, native._ptr(b), n) == n
        L.ss_plan_windows(float(d), native._ptr(a), n)
        assert np.array_equal(a, b) and np.array_equal(native.plan_windows(d), a)
        assert np.array_equal(a, np.arange(n, dtype=np.int64) * 13230)
    # round(51.2 i) in integers (256 i / 5 is never a tie): the start table every earlier release used
    assert [L.ss_window_start_bin(i, 0.6) for i in range(N_WINDOWS + 1)] == [(512 * i + 5) // 10 for i in range(N_WINDOWS + 1)]


@pytest.mark.parametrize("bad", BAD_STEPS)
def test_steps_outside_the_range_are_refused(native, bad):
    L = native.lib()
    buf = np.full(4, -7, dtype=np.int64)
    assert L.ss_plan_windows_step(60.0, float(bad), native._ptr(buf), 4) == -1 and buf.tolist() == [-7] * 4
    assert L.ss_window_start_bin(3, float(bad)) == -1
    for call in (lambda: native.plan_windows(60.0, bad), lambda: native.window_start_bin(3, bad), lambda: native.check_step(bad)):
        with pytest.raises(ValueError) as e:
            call()
        assert "0.1" in str(e.value) and "3.0" in str(e.value)
    assert L.ss_set_window_step(None, float(bad)) == native.SS_ERR_ARG                          # (no context: refused as well)


def test_limits_themselves_are_accepted(native):
    for ok in (0.1, 3.0):
        assert native.lib().ss_plan_windows_step(60.0, ok, None, 0) == len(R.plan(60.0, ok)) > 0
        assert native.check_step(ok) == ok
    assert native.lib().ss_window_start_bin(-1, 0.6) == -1
    assert native.lib().ss_get_window_step(None) == -1.0


def test_new_exports_are_declared_and_bound(native):
    hdr = open(os.path.join(ROOT, "include", "softspoken.h")).read()
    for name in ("ss_plan_windows_step", "ss_window_start_bin", "ss_set_window_step", "ss_get_window_step"):
        assert name in native.EXPORTS and name + "(" in hdr and getattr(native.lib(), name) is not None
    assert native.lib().ss_abi_version() == 3 == native.ABI_VERSION
    for sym in ("#define SS_STEP_DEFAULT 0.6", "#define SS_STEP_MIN 0.1", "#define SS_STEP_MAX 3.0", "#define SS_STEP_SAMPLES 13230"):
        assert sym in hdr
    assert (native.STEP_MIN, native.STEP_MAX) == (R.STEP_MIN, R.STEP_MAX) == (0.1, 3.0)
    assert callable(native.Context.set_window_step) and isinstance(native.Context.window_step, property)


@pytest.mark.parametrize("step", STEPS)
def test_the_header_claims_about_the_accepted_range(step):
    """Over 4000 windows: every bin up to the last window's end has a window, at most 31 windows cover a bin, and the averaging kernels'
    candidate range lo = trunc((j - 255) / s_b) - 1 .. hi = trunc(j / s_b) + 1 (s_b = step x 256 / 3) holds every covering window."""
    starts = np.array([R.start_bin(i, step) for i in range(N_WINDOWS)], dtype=np.int64)
    assert np.all(np.diff(starts) >= 1) and np.all(np.diff(starts) <= 256)
    j = np.arange(starts[-1] + 256, dtype=np.int64)
    first = np.searchsorted(starts, j - 255, "left")                    # first window with start >= j - 255
    last = np.searchsorted(starts, j, "right") - 1                      # last window with start <= j
    n = last - first + 1
    assert n.min() >= 1 and n.max() <= 31
    assert n.max() <= math.ceil(256 / (step * 256 / 3)) + 1
    s_b = step * 256 / 3
    lo = np.maximum(np.trunc((j - 255) / s_b).astype(np.int64) - 1, 0)
    hi = np.minimum(np.trunc(j / s_b).astype(np.int64) + 1, N_WINDOWS - 1)
    assert np.all(lo <= first) and np.all(last <= hi)
    k = (0, 1, 255, 256, 257, len(j) // 2, len(j) - 1)                  # ... and the searchsorted reading against brute force
    for jj in k:
        assert R.covering_windows(int(jj), N_WINDOWS, step) == list(range(first[jj], last[jj] + 1))


def test_sample_step_and_bin_step_drift_as_in_the_reference():
    """floor(22050 step) samples against step x 256 / 3 bins: 99 / 512 s loses 0.48 s per hour, the reference's own arithmetic."""
    step = 99 / 512
    w = round(3600 / step)
    assert abs((w * step - w * R.per_step(step) / R.SR) - 0.48) < 0.005
    assert R.per_step(0.6) * 5 == R.WINDOW and R.per_step(3.0) == R.WINDOW           # no drift where 22050 step is an integer


# ---- the drop-in: settings.step_size reaches every context it makes or reuses ---------------------------------------------------
class _Ctx:
    def __init__(self, precision):
        self.precision, self.alive, self.window_step, self.sets = precision, True, 0.6, []

    def set_window_step(self, step):
        self.sets.append(step)
        self.window_step = step


def _model_with_fake_contexts(monkeypatch, step):
    from root.code.backend import settings
    from root.code.backend.pytorch_neural_nets import SpecUNet_2D
    monkeypatch.setattr(settings, "step_size", step)
    m = SpecUNet_2D(precision="f16x2")
    m._ctx, m._ctx2, m._fp32_tmp = _Ctx("f16x2"), _Ctx("f16x2"), _Ctx("fp32")
    m._ctx_version = m._weights_version()
    return m, settings


def test_dropin_hands_the_setting_to_every_context(native, monkeypatch):
    m, settings = _model_with_fake_contexts(monkeypatch, 1.5)
    ctxs = (m._ctx, m._ctx2, m._fp32_tmp)
    assert (m.hip_context(), m.hip_context(1), m.fp32_context()) == ctxs                    # reused, not rebuilt
    assert [c.sets for c in ctxs] == [[1.5]] * 3
    seen = []
    m.with_range_fallback(lambda c: seen.append(c.window_step))
    assert seen == [1.5] and [c.sets for c in ctxs] == [[1.5]] * 3                          # unchanged value: not set again
    monkeypatch.setattr(settings, "step_size", 0.3)                                         # edited between two jobs
    m.hip_context(1), m.fp32_context(), m.hip_context()
    assert [c.sets for c in ctxs] == [[1.5, 0.3]] * 3
    monkeypatch.setattr(settings, "step_size", 0.6)
    assert m.hip_context().window_step == 0.6


@pytest.mark.parametrize("bad", BAD_STEPS + ("fast", None))
def test_dropin_refuses_a_bad_setting_by_name_of_the_limits(native, monkeypatch, tmp_path, bad):
    from root.code.frontend.NNDetector import NNDetector
    m, settings = _model_with_fake_contexts(monkeypatch, bad)
    for call in (m.hip_context, lambda: m.hip_context(1), m.fp32_context):
        with pytest.raises(ValueError) as e:
            call()
        assert "0.1" in str(e.value) and "3.0" in str(e.value)
    assert not (m._ctx.sets or m._ctx2.sets or m._fp32_tmp.sets)
    det = NNDetector.__new__(NNDetector)
    det.detections_project = {}
    with pytest.raises(ValueError) as e:
        det.plan_detection_job()
    assert "0.1" in str(e.value) and "3.0" in str(e.value)


def test_dropin_plan_follows_the_setting(native, monkeypatch, tmp_path):
    from root.code.backend import settings
    from root.code.frontend.NNDetector import NNDetector
    path = str(tmp_path / "a.wav")
    with open(path, "wb") as fh:
        fh.write(synth.wav_bytes(np.zeros(16000 * 7 + 123, dtype=np.int16), 16000))
    for step in (0.6, 1.5, 99 / 512):
        monkeypatch.setattr(settings, "step_size", step)
        det = NNDetector.__new__(NNDetector)
        det.detections_project = {path: []}
        plan = det.plan_detection_job()[path]
        want = R.plan((16000 * 7 + 123) / 16000, step)
        assert np.array_equal(plan, want) and np.array_equal(native.plan_windows((16000 * 7 + 123) / 16000, step), want)
