"""The band silencer without a GPU (include/softspoken.h "band silencer"): the exported surface, ss_box_plan against tests/box_ref.py,
every refusal, the NaN rules, the float64 reference against its float32 restatement, and the conditions on the reference alone that keep
the GPU cases of test_gpu_box_silence.py from being vacuous (a box removes its own band and nothing else, on its own channel alone)."""
import math
import os

import numpy as np
import pytest

import box_ref as B
import separation_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


def test_surface(native):
    hdr = open(os.path.join(ROOT, "include", "softspoken.h")).read()
    for name in ("ss_box_plan", "ss_box_silence_pcm", "ss_box_silence_pcm_source"):
        assert name in native.EXPORTS and name + "(" in hdr and getattr(native.lib(), name) is not None
    assert native.BOX_DTYPE.itemsize == 40 and "} ss_box;" in hdr
    import ctypes as C
    assert C.sizeof(native.BoxParams) == 24 and C.sizeof(native.BoxRange) == 32
    assert native.lib().ss_abi_version() == 3                     # new symbols only


def _draw(rng, dur, n):
    boxes = []
    for _ in range(n):
        a = rng.uniform(-0.3, dur + 0.2)
        ln = rng.choice([0.0, rng.uniform(0, 0.003), rng.uniform(0, 0.4 * dur + 0.1), dur + 1.0])
        if boxes and rng.random() < 0.3:
            a = boxes[-1][1]                                      # touches the one before
        lo = rng.choice([NAN, 0.0, rng.uniform(0, 4000)])
        hi = rng.choice([NAN, 1e9]) if rng.random() < 0.3 else (0.0 if lo != lo else lo) + rng.uniform(0, 5000)
        boxes.append((a, a + ln, lo, hi, int(rng.integers(-1, 4))))
    return boxes


@pytest.mark.parametrize("sr", [8000, 16000, 22050, 44100, 48000, 96000, 192000, 384000])
def test_plan_matches_reference(native, sr):
    rng = np.random.default_rng(sr)
    for case in range(12):
        dur = [0.0, 0.004, 0.7, 2.5][case % 4]
        frames = int(dur * sr)
        boxes = _draw(rng, dur, int(rng.integers(0, 7)))
        got = native.box_plan(sr, frames, boxes)
        assert got == B.plan(sr, frames, boxes), (sr, frames, boxes)
        assert got["n_fft"] == R.fft_size(sr) and got["hop"] * 4 == got["n_fft"]


def test_plan_capacity(native):
    import ctypes as C
    arr = native.boxes_array([(0.1, 0.2, 0, 100), (0.5, 0.6, 0, 100)])
    info = native.BoxPlanInfo()
    rc = native.lib().ss_box_plan(8000, 8000, arr.ctypes.data_as(C.c_void_p), 2, None, C.byref(info))
    assert rc == native.SS_ERR_CAPACITY and info.n_ranges == 2


BAD_BOXES = {
    "start not finite": (NAN, 1.0, 0.0, 100.0, -1, 0),
    "end not finite": (0.0, math.inf, 0.0, 100.0, -1, 0),
    "end before start": (1.0, 0.5, 0.0, 100.0, -1, 0),
    "low above high": (0.0, 1.0, 300.0, 200.0, -1, 0),
    "low above high, NaN low is 0": (0.0, 1.0, NAN, -5.0, -1, 0),
    "negative high": (0.0, 1.0, -20.0, -10.0, -1, 0),
    "channel below -1": (0.0, 1.0, 0.0, 100.0, -2, 0),
    "channel past the limit": (0.0, 1.0, 0.0, 100.0, 256, 0),
    "reserved": (0.0, 1.0, 0.0, 100.0, -1, 7),
}


@pytest.mark.parametrize("why", sorted(BAD_BOXES))
def test_bad_box_is_refused(native, why):
    arr = np.array([(0.2, 0.4, 100.0, 900.0, 0, 0), BAD_BOXES[why]], dtype=native.BOX_DTYPE)
    with pytest.raises(native.NativeError) as e:
        native.box_plan(48000, 48000, arr)
    assert e.value.code == native.SS_ERR_ARG, why
    native.box_plan(48000, 48000, arr[:1])


@pytest.mark.parametrize("params", [dict(fade_s=-0.1), dict(fade_s=NAN), dict(fade_s=math.inf), dict(min_gain=-0.01), dict(min_gain=1.01),
                                    dict(min_gain=NAN), dict(edge_hz=-1.0), dict(edge_hz=NAN), dict(edge_hz=math.inf)])
def test_bad_params_are_refused(native, params):
    with pytest.raises(native.NativeError) as e:
        native.box_plan(48000, 48000, [(0.1, 0.2, 0.0, 100.0)], **params)
    assert e.value.code == native.SS_ERR_ARG
    native.box_plan(48000, 48000, [(0.1, 0.2, 0.0, 100.0)], fade_s=0.0, min_gain=1.0, edge_hz=0.0)


def test_nan_rules(native):
    sr, N = 48000, 1024
    for lo, hi in ((NAN, NAN), (NAN, 700.0), (500.0, NAN), (None, None)):
        assert native.box_plan(sr, sr, [(0.1, 0.2, lo, hi)])["ranges"] == B.plan(sr, sr, [(0.1, 0.2, lo, hi)])["ranges"]
    s, e, lo, hi, ch = B._norm((0.0, 1.0, NAN, NAN))
    assert (lo, hi, ch) == (0.0, math.inf, -1)
    assert np.array_equal(B.profile(N, sr, lo, hi, 100.0), np.ones(N // 2 + 1))          # no estimate: the whole band goes
    v = B.profile(N, sr, 0.0, 700.0, 0.0)                                               # NaN low = 0; the hard edge
    assert v[: 14 + 1].all() and not v[15:].any() and 14 == math.floor(700.0 * N / sr)
    arr = native.boxes_array([(0.0, 1.0, None, 700.0), (0.0, 1.0, 5.0, None, 1)])
    assert math.isnan(arr[0]["low_hz"]) and math.isnan(arr[1]["high_hz"]) and list(arr["channel"]) == [-1, 1]


def test_profile_follows_the_definition():
    sr, N = 48000, 1024
    q_lo, q_hi, lo_b, hi_b = B.bin_range(N, sr, 500.0, 2000.0)
    assert (q_lo, q_hi) == (11, 42) and abs(lo_b - 10.6667) < 1e-3 and abs(hi_b - 42.6667) < 1e-3
    v = B.profile(N, sr, 500.0, 2000.0, 100.0)                                          # e_b = 2.133 bins
    assert np.all(v[11:43] == 1.0) and v[8] == 0.0 and v[45] == 0.0
    assert abs(v[10] - (1 + math.cos(math.pi * (lo_b - 10) / (100.0 * N / sr))) / 2) < 1e-15 and 0 < v[9] < v[10] < 1
    assert abs(v[43] - (1 + math.cos(math.pi * (43 - hi_b) / (100.0 * N / sr))) / 2) < 1e-15 and 0 < v[44] < v[43] < 1
    # a box narrower than a bin that contains none: no gain below 1 with the hard edge
    q_lo, q_hi, _, _ = B.bin_range(N, sr, 480.0, 500.0)
    assert q_lo == q_hi + 1 and not B.profile(N, sr, 480.0, 500.0, 0.0).any()


def _tones(sr, secs, ch):
    t = np.arange(int(sr * secs)) / sr
    x = 0.3 * np.sin(2 * np.pi * 1000 * t) + 0.3 * np.sin(2 * np.pi * 12000 * t)
    return np.repeat(x[:, None], ch, axis=1).astype(np.float32)


def _tone_amplitude(y, sr, f):
    t = np.arange(len(y)) / sr
    A = np.stack([np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)], 1)
    c, *_ = np.linalg.lstsq(A, y, rcond=None)
    return float(np.hypot(*c))


def test_reference_removes_the_band_and_keeps_the_rest():
    sr = 48000
    x = _tones(sr, 2.0, 1)
    _, y64 = B.box_silence(x, sr, [(0.5, 1.5, 500.0, 2000.0)], min_gain=0.0, unrounded=True)
    inner = slice(int(0.6 * sr), int(1.4 * sr))
    got, ref = y64[inner, 0] / 32767.0, x[inner, 0].astype(np.float64)
    assert abs(_tone_amplitude(got, sr, 12000) / _tone_amplitude(ref, sr, 12000) - 1.0) <= 0.01
    assert _tone_amplitude(got, sr, 1000) <= 0.01 * _tone_amplitude(ref, sr, 1000)


def test_reference_acts_on_its_own_channel_alone():
    sr = 48000
    x = _tones(sr, 2.0, 2)
    _, y64 = B.box_silence(x, sr, [(0.5, 1.5, 500.0, 2000.0, 1)], min_gain=0.0, unrounded=True)
    inner = slice(int(0.6 * sr), int(1.4 * sr))
    plain = x.astype(np.float64) * 32767.0
    assert np.abs(y64[inner, 0] - plain[inner, 0]).max() <= 0.01                        # LSB
    assert _tone_amplitude(y64[inner, 1], sr, 1000) <= 0.01 * _tone_amplitude(plain[inner, 1], sr, 1000)


@pytest.mark.parametrize("sr,ch", [(8000, 1), (48000, 2), (96000, 3)])
def test_float32_restatement_stays_near_float64(sr, ch):
    """e32 is the yardstick of the device's bound 0.5 + 4 e32: it has to be small against the half LSB of the output rounding, or the bound
    would say nothing, and it cannot be zero (float32 arithmetic of 16-bit audio through two FFTs rounds)."""
    from softspoken_amd import synth
    x = (synth.synth_audio(5, 1.0, sr, ch, with_silence=False).T.reshape(-1, ch) * 0.5).astype(np.float32)
    boxes = [(0.2, 0.6, 300.0, 2500.0), (0.4, 0.8, 3000.0, NAN, ch - 1)]
    want, y64 = B.box_silence(x, sr, boxes, fade_s=0.02, min_gain=0.1, unrounded=True)
    y32 = B.box_silence_f32(x, sr, boxes, fade_s=0.02, min_gain=0.1)
    e32 = float(np.abs(y32.astype(np.float64) - y64).max())
    assert 0.0 < e32 < 0.125, e32
    assert np.array_equal(want, np.rint(y64).astype(np.int16))
    m = np.zeros(len(x), dtype=bool)
    for a, b in B.merged_intervals(boxes, sr, len(x)):
        m[a:b] = True
    plain = (x * np.float32(32767.0)).astype(np.float64)                                # the float32 transcode
    assert np.array_equal(y64[~m], plain[~m]) and np.abs(y64[m] - plain[m]).max() > 100.0
