"""The band silencer on a real MI355X (include/softspoken.h "band silencer"): the exact equalities with the zeroing silencer and the
transcode, parity with the float64 reference of tests/box_ref.py at every FFT size and gain source, the cuts of the frame budget, the
edges of a recording, and the launch structure.

The parity cases hold every output sample of the merged intervals to the reference's unrounded float64 output y64 (in LSB):
|got - y64| <= 0.5 + tau, 0.5 being the output rounding and tau = 4 e32, e32 the largest |box_silence_f32 - y64| of the same case, computed
on the CPU inside the test (the separation silencer's bound, DESIGN.md section 12, unchanged in form); the _source cases use
source_out_ref.separation_bound, the same bound in the units of the encoding.  The device's own error never sets tau.
test_box_host.py asserts on the reference alone that a box removes its band and nothing else, so the cases are not vacuous."""
import os

import numpy as np
import pytest

import box_ref as B
import source_out_ref as S

pytestmark = pytest.mark.gpu
NAN = float("nan")
FMT = {"u8": 1, "pcm16": 2, "pcm24": 3, "pcm32": 4, "f32": 5, "f64": 6, "s8": 7, "pcm16be": 8, "pcm24be": 9, "pcm32be": 10, "f32be": 11, "f64be": 12}


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(None, 0, profile=True)                     # audio-only: the band silencer needs no model
    yield c
    c.close()


def _rec(fmt, sr, ch, seconds, seed, frames=None):
    """(bytes uint8, decoded float32 (frames, ch)) of seeded noise plus tones, peak below 0.6 of full scale (the 16-bit path wraps)."""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * sr)) if frames is None else frames
    t = np.arange(n)[:, None] / sr
    f = np.array([220.0, 1000.0, 3100.0, 0.11 * sr, 0.31 * sr, 0.45 * sr])[None, :, None] * (1.0 + 0.07 * np.arange(ch))[None, None, :]
    x = 0.07 * np.sin(2 * np.pi * f * t[:, :, None] + rng.uniform(0, 6.28, (1, 6, ch))).sum(axis=1) + 0.04 * rng.standard_normal((n, ch))
    data = S.encode(x.astype(np.float32).reshape(-1), FMT[fmt])
    return data, S.decode(data, FMT[fmt]).reshape(n, ch)


def _mask(frames, sr, boxes):
    m = np.zeros(frames, dtype=bool)
    for a, b in B.merged_intervals(boxes, sr, frames):
        m[a:b] = True
    return m


def _bound_case(ctx, label, fmt, sr, ch, seconds, boxes, seed=61, frames=None, **params):
    """One 16-bit parity case: the bound inside the merged intervals, the transcode's bytes outside.  -> (got, rec, e32)."""
    data, x = _rec(fmt, sr, ch, seconds, seed, frames)
    n = len(x)
    _, y64 = B.box_silence(x, sr, boxes, unrounded=True, **params)
    e32 = float(np.abs(B.box_silence_f32(x, sr, boxes, **params).astype(np.float64) - y64).max())
    got = ctx.box_silence_pcm(data, FMT[fmt], sr, ch, boxes, **params)
    plain = ctx.silence_pcm(data, FMT[fmt], sr, ch, n, [])
    m = _mask(n, sr, boxes)
    assert got.shape == (n, ch) and got.dtype == np.int16
    assert np.array_equal(got[~m], plain[~m]), label
    excess = float(np.maximum(np.abs(got.astype(np.float64) - y64)[m] - 0.5, 0.0).max()) if m.any() else 0.0
    print(f"BOXBOUND {label}: sr={sr} N={B.R.fft_size(sr)} ch={ch} {fmt} e32={e32:.5f} tau={4 * e32:.5f} excess={excess:.5f} samples={int(m.sum()) * ch}")
    assert excess <= 4.0 * e32, (label, excess, 4.0 * e32)
    return got, (data, x), e32


# ---- 1. exact equalities -----------------------------------------------------------------------------------------------------
REGIONS = [(0.25, 0.5), (0.4, 0.75), (0.9, 99.0), (-2.0, 0.0105), (0.8, 0.8), (0.80005, 0.80015)]


@pytest.mark.parametrize("fmt,sr,ch,seconds", [("u8", 8000, 1, 1.0), ("pcm16", 48000, 2, 2.0), ("pcm24", 16000, 3, 1.0)])
@pytest.mark.parametrize("band", [(NAN, NAN), (0.0, 1e6)])
def test_full_band_box_is_the_zeroing_silencer(ctx, fmt, sr, ch, seconds, band):
    data, x = _rec(fmt, sr, ch, seconds, 62)
    boxes = [(s, e, band[0], band[1]) for s, e in REGIONS]
    got = ctx.box_silence_pcm(data, FMT[fmt], sr, ch, boxes, min_gain=0.0, fade_s=0.0)
    assert got.tobytes() == ctx.silence_pcm(data, FMT[fmt], sr, ch, len(x), REGIONS).tobytes()
    src = ctx.box_silence_pcm(data, FMT[fmt], sr, ch, boxes, min_gain=0.0, fade_s=0.0, encoding="source")
    assert src.tobytes() == ctx.silence_pcm_source(data, FMT[fmt], sr, ch, len(x), REGIONS).tobytes()


@pytest.mark.parametrize("fmt,sr,ch", [("pcm16", 48000, 2), ("f32", 22050, 3), ("pcm24be", 96000, 1)])
def test_no_boxes_is_the_transcode_and_two_calls_agree(ctx, fmt, sr, ch):
    data, x = _rec(fmt, sr, ch, 0.5, 63)
    plain = ctx.silence_pcm(data, FMT[fmt], sr, ch, len(x), [])
    for boxes in ([], [(0.2, 0.2, 100.0, 900.0), (0.7, 0.9, NAN, NAN), (-3.0, -1.0, 0.0, 50.0)]):        # none; all empty
        assert ctx.box_silence_pcm(data, FMT[fmt], sr, ch, boxes).tobytes() == plain.tobytes()
        assert ctx.box_silence_pcm(data, FMT[fmt], sr, ch, boxes, encoding="source").tobytes() == data.tobytes()
    boxes = [(0.1, 0.3, 400.0, 2500.0), (0.25, 0.4, 5000.0, NAN, ch - 1)]
    for enc in ("pcm16", "source"):
        a = ctx.box_silence_pcm(data, FMT[fmt], sr, ch, boxes, fade_s=0.02, min_gain=0.1, encoding=enc)
        b = ctx.box_silence_pcm(data, FMT[fmt], sr, ch, boxes, fade_s=0.02, min_gain=0.1, encoding=enc)
        assert a.tobytes() == b.tobytes()
        m = _mask(len(x), sr, boxes)
        want = plain if enc == "pcm16" else data.reshape(len(x), -1)
        assert np.array_equal(a[~m], want[~m]) and not np.array_equal(a[m], want[m])


def test_job_files_regions_and_an_open_stream_stay(native, blob):
    from softspoken_amd import synth
    c = native.Context(blob, 0)
    try:
        pcm = synth.to_pcm16(synth.synth_audio(7, 6.0, 16000, 1, with_silence=False))
        fid = c.add_pcm(pcm, 2, 16000, 1, len(pcm))
        assert c.run()
        regions, logits, gen = c.regions(fid), c.window_logits(fid).copy(), c.reset_generation()
        sid = c.stream_open(2, 16000, 1)
        c.stream_push(sid, pcm[:16000], 16000, 1)
        info = c.stream_info(sid)
        data, x = _rec("pcm16", 48000, 2, 0.5, 64)
        boxes = [(0.1, 0.3, 400.0, 2500.0)]
        got = c.box_silence_pcm(data, 2, 48000, 2, boxes)
        assert c.regions(fid) == regions and np.array_equal(c.window_logits(fid), logits) and c.reset_generation() == gen
        assert c.stream_info(sid) == info and c.num_windows(fid) == len(logits)
        c.stream_push(sid, pcm[16000:32000], 16000, 1)            # the stream goes on
        assert c.stream_info(sid)["frames_pushed"] == 32000
        c.stream_free(sid)
        with pytest.raises(native.NativeError) as e:                                     # a channel the file does not have
            c.box_silence_pcm(data, 2, 48000, 2, [(0.1, 0.3, 400.0, 2500.0, 2)])
        assert e.value.code == native.SS_ERR_ARG
        c.run_begin()
        with pytest.raises(native.NativeError) as e:                                     # a run in flight
            c.box_silence_pcm(data, 2, 48000, 2, boxes)
        assert e.value.code == native.SS_ERR_STATE
        c.run_end()
        assert c.box_silence_pcm(data, 2, 48000, 2, boxes).tobytes() == got.tobytes()
    finally:
        c.close()


# ---- 2. parity with float64 --------------------------------------------------------------------------------------------------
def _table(ch):
    return [(0.1, 0.4, 300.0, 3000.0), (0.3, 0.6, 5000.0, 9000.0, ch - 1), (0.7, 0.7004, 0.0, NAN), (0.85, 99.0, NAN, 1500.0)]


@pytest.mark.parametrize("sr,N,ch,fmt", [(8000, 256, 1, "u8"), (22050, 512, 2, "pcm16"), (48000, 1024, 2, "pcm24"), (96000, 2048, 5, "pcm16"),
                                         (192000, 4096, 2, "pcm32"), (384000, 8192, 3, "pcm16")])
def test_parity_at_every_fft_size(ctx, sr, N, ch, fmt):
    assert B.R.fft_size(sr) == N
    boxes = _table(ch) if sr > 8000 else [(0.1, 0.4, 300.0, 1200.0), (0.3, 0.6, 2000.0, 3000.0), (0.7, 0.7004, 0.0, NAN), (0.85, 99.0, NAN, 900.0)]
    _bound_case(ctx, f"fft {sr}/{ch}", fmt, sr, ch, 1.0, boxes)


GAIN_CASES = {
    "overlap, disjoint bands": (48000, 2, [(0.2, 0.6, 500.0, 2000.0), (0.4, 0.8, 6000.0, 9000.0)], {}),
    "overlap, nested bands": (48000, 2, [(0.2, 0.8, 300.0, 8000.0), (0.4, 0.6, 1000.0, 2000.0)], dict(min_gain=0.2)),
    "one channel of a pair": (48000, 2, [(0.2, 0.7, 500.0, 4000.0, 0)], {}),
    "the other channel of a pair": (16000, 3, [(0.2, 0.7, 500.0, 4000.0, 1)], {}),
    "the unpaired last channel": (16000, 3, [(0.2, 0.7, 500.0, 4000.0, 2)], {}),
    "different boxes on a pair": (48000, 2, [(0.2, 0.7, 500.0, 2000.0, 0), (0.3, 0.8, 3000.0, 7000.0, 1)], {}),
    "edge 0": (48000, 2, [(0.2, 0.7, 1000.0, 3000.0)], dict(edge_hz=0.0)),
    "edge 100": (48000, 2, [(0.2, 0.7, 1000.0, 3000.0)], dict(edge_hz=100.0)),
    "edge wider than the box": (48000, 2, [(0.2, 0.7, 1000.0, 1500.0)], dict(edge_hz=3000.0)),
    "low 0, high past Nyquist, NaN edges": (48000, 2, [(0.2, 0.5, 0.0, 1000.0), (0.55, 0.7, 8000.0, 30000.0), (0.75, 0.9, NAN, NAN, 1)], {}),
    "min_gain 0.45": (48000, 2, [(0.2, 0.7, 500.0, 4000.0)], dict(min_gain=0.45)),
    "min_gain 1": (48000, 2, [(0.2, 0.7, 500.0, 4000.0)], dict(min_gain=1.0)),
    "fade 0": (48000, 2, [(0.2, 0.7, 500.0, 4000.0)], dict(fade_s=0.0)),
    "fade 0.02": (16000, 3, [(0.2, 0.7, 500.0, 4000.0), (0.6, 0.9, 100.0, 300.0, 0)], dict(fade_s=0.02)),
    "fade 0.5": (48000, 2, [(0.2, 0.7, 500.0, 4000.0)], dict(fade_s=0.5)),
}


@pytest.mark.parametrize("label", sorted(GAIN_CASES))
def test_parity_over_the_gain_sources(ctx, label):
    sr, ch, boxes, params = GAIN_CASES[label]
    _bound_case(ctx, label, "pcm16", sr, ch, 1.0, boxes, **params)


def test_a_box_without_a_bin_changes_nothing(ctx):
    """480 .. 500 Hz at 48 kHz lies between bins 10 and 11 (46.875 Hz apart): with the hard edge the gain is 1 everywhere."""
    sr, boxes = 48000, [(0.2, 0.7, 480.0, 500.0)]
    got, (data, x), _ = _bound_case(ctx, "no bin inside", "pcm16", sr, 2, 1.0, boxes, edge_hz=0.0)
    plain = ctx.silence_pcm(data, 2, sr, 2, len(x), [])
    assert np.abs(got.astype(np.int32) - plain.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("fmt", ["pcm16be", "pcm24be", "f32", "f32be", "f64be", "u8"])
def test_parity_in_the_source_encoding(ctx, fmt):
    sr, ch = 48000, 3
    boxes = [(0.1, 0.4, 300.0, 3000.0), (0.3, 0.6, 5000.0, 9000.0, 2), (0.8, 99.0, NAN, 1500.0, 0)]
    params = dict(fade_s=0.02, min_gain=0.1)
    data, x = _rec(fmt, sr, ch, 1.0, 65)
    n, code = len(x), FMT[fmt]
    _, y64 = B.box_silence(x, sr, boxes, unrounded=True, **params)
    e32 = float(np.abs(B.box_silence_f32(x, sr, boxes, **params).astype(np.float64) - y64).max())
    out = ctx.box_silence_pcm(data, code, sr, ch, boxes, encoding="source", **params)
    m = _mask(n, sr, boxes)
    assert out.dtype == np.uint8 and out.shape == (n, ch * S.BPS[code])
    assert np.array_equal(out[~m], data.reshape(n, -1)[~m])                              # the input's bytes
    ref, tol = S.separation_bound(y64, e32, code)
    if code in S.BITS:
        val = S.codes(out.reshape(-1), code).reshape(n, ch).astype(np.float64)
    else:
        le = np.ascontiguousarray(S._samples_le(out.reshape(-1), code))
        val = le.view("<f4" if S.BPS[code] == 4 else "<f8").reshape(n, ch).astype(np.float64)
    excess = float((np.abs(val - ref) - tol)[m].max())
    print(f"BOXBOUND source {fmt}: e32={e32:.5f} worst |got - ref| - tol = {excess:.3e}")
    assert excess <= 0.0, (fmt, excess)


# ---- 3. cuts -----------------------------------------------------------------------------------------------------------------
_CUT_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from softspoken_amd import native
import box_ref as B
import test_gpu_box_silence as T
ctx = native.Context(None, 0, profile=True)
for sr, ch in ((48000, 2), (16000, 3)):
    boxes = [(0.013, 1.2, 300.0, 3000.0), (1.7, 2.95, 2000.0, float("nan"), ch - 1), (1.5, 1.5 + 1.0 / sr, 0.0, 900.0), (0.8, 1.4, 5000.0, 7000.0, 0)]
    assert [b - a for a, b in B.merged_intervals(boxes, sr, 3 * sr)][1] == 1
    ctx.debug_set_separation_budget(0)
    want, (data, x), _ = T._bound_case(ctx, "cuts %d/%d default budget" % (sr, ch), "pcm16", sr, ch, 3.0, boxes, seed=66)
    want_src = ctx.box_silence_pcm(data, 2, sr, ch, boxes, encoding="source")
    N = B.R.fft_size(sr)
    for budget in (16, 17, 23, 64):
        ctx.debug_set_separation_budget(budget)
        ctx.reset_stats()
        got = ctx.box_silence_pcm(data, 2, sr, ch, boxes)
        st = {{k["name"]: k["launches"] for k in ctx.kernel_stats()}}
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (sr, ch, budget, bad[:8])
        assert ctx.box_silence_pcm(data, 2, sr, ch, boxes, encoding="source").tobytes() == want_src.tobytes(), (sr, ch, budget)
        chunks = B.chunk_count(sr, len(x), boxes, budget)
        assert chunks > 2 and (1.4 - 0.013) * sr > 2 * (budget - 8) * (N // 4)
        assert st == {{"box_transcode/silence_encode_kernel": 1, "box_stft_kernel<%d>" % N: chunks, "sep_blend_kernel": chunks}}, (budget, chunks, st)
print("CUTS_OK")
"""


def test_every_cut_alignment_gives_the_same_bytes(build_all):
    """ss_debug_set_separation_budget (development build) moves the piece and chunk cuts through 3 s recordings with a one-sample box
    between two longer ones: every budget must give the default budget's bytes, which pass the bound, with one box_stft_kernel launch
    and one blend launch per chunk."""
    import subprocess, sys
    from softspoken_amd import build as hip_build
    tests = os.path.dirname(os.path.abspath(__file__))
    e = dict(os.environ); e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
    r = subprocess.run([sys.executable, "-c", _CUT_SCRIPT.format(root=os.path.dirname(tests), tests=tests)], env=e, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "CUTS_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,sr,ch,frames,boxes", [
    ("one frame", 48000, 2, 1, [(0.0, 1.0, 500.0, 4000.0)]),
    ("100 frames", 48000, 3, 100, [(0.0005, 0.0015, 2000.0, 9000.0, 2)]),
    ("0.05 s", 16000, 1, 800, [(0.01, 0.03, 300.0, 2000.0)]),
    ("a box of one sample", 48000, 2, 24000, [(0.25, 0.25 + 1.0 / 48000, 0.0, 6000.0)]),
    ("a box past both ends", 22050, 2, 11025, [(-5.0, 50.0, 1000.0, 5000.0)]),
])
def test_edges_of_a_recording(ctx, label, sr, ch, frames, boxes):
    before = _rec("pcm16", 44100, 2, 0.2, 67)
    regions = [(0.05, 0.1)]
    usual = ctx.silence_pcm(before[0], 2, 44100, 2, len(before[1]), regions)
    _bound_case(ctx, label, "pcm16", sr, ch, None, boxes, frames=frames, fade_s=0.0005)
    assert ctx.silence_pcm(before[0], 2, 44100, 2, len(before[1]), regions).tobytes() == usual.tobytes()      # the context works afterwards


# ---- 5. launch structure -----------------------------------------------------------------------------------------------------
def test_one_stft_launch_per_chunk_and_no_model_pass(ctx):
    sr, ch = 48000, 2
    data, x = _rec("pcm16", sr, ch, 1.0, 68)
    boxes = [(0.1, 0.4, 300.0, 3000.0), (0.6, 0.9, 5000.0, 9000.0, 1)]
    assert B.chunk_count(sr, len(x), boxes, (256 << 20) // (1024 * 8)) == 1
    ctx.reset_stats()
    ctx.box_silence_pcm(data, 2, sr, ch, boxes)
    st = {k["name"]: k["launches"] for k in ctx.kernel_stats()}
    assert st == {"box_transcode/silence_encode_kernel": 1, "box_stft_kernel<1024>": 1, "sep_blend_kernel": 1}, st
    ctx.reset_stats()
    ctx.box_silence_pcm(data, 2, sr, ch, boxes, encoding="source")
    st = {k["name"]: k["launches"] for k in ctx.kernel_stats()}
    assert st == {"box_stft_kernel<1024>": 1, "sep_blend_source_kernel": 1}, st
