"""The streaming silencer's host side, no GPU: ss_erase_table against a plain-Python restatement, the finality of every frame below
ss_stream_output_limit on random bin sequences (the frame's erased / kept state is the same whatever follows), the latency expression
of include/softspoken.h, and StreamDetector's fallback with output streams against a scripted context."""
import math
import os

import numpy as np
import pytest

import stream_output_ref as R
from softspoken_amd import native
from softspoken_amd.stream import StreamDetector, StreamWavWriter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADS = (0.0, 0.05, 0.7)
MIN_LENS = (0.0, 0.3, 2.0)


@pytest.fixture(scope="module")
def lib(build_all):
    return native.lib()


def _same_rows(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(np.array(g).view(np.int64), np.array(w, dtype=np.float64).view(np.int64)), (g, w)


@pytest.mark.parametrize("pad_s", PADS)
@pytest.mark.parametrize("min_len_s", MIN_LENS)
def test_erase_table_equals_the_restatement(lib, pad_s, min_len_s):
    rng = np.random.default_rng(int(pad_s * 100) * 7 + int(min_len_s * 10))
    for case in range(40):
        n = int(rng.integers(0, 30))
        start = rng.uniform(-4.0, 60.0, n)
        length = rng.choice([0.0, 0.0117, 0.3, 0.3000000001, 2.0, 5.0], n) * rng.choice([1.0, 1.0, rng.uniform(0, 1.5)], n)
        rows = [(float(s), float(s + d)) for s, d in zip(start, length)]        # unsorted, overlapping, zero-length
        if n and case % 3 == 0:
            rows[int(rng.integers(0, n))] = (float("nan"), 1.0)
            rows[int(rng.integers(0, n))] = (2.0, float("nan"))
        if n and case % 5 == 0:
            rows[int(rng.integers(0, n))] = (5.0, 4.0)                         # end before start
        got = native.erase_table(rows, pad_s, min_len_s)
        _same_rows(got, R.erase_table(rows, pad_s, min_len_s))
        for sr, frames in ((16000, 16000 * 50), (44100, 44100 * 70)):         # and through silence_ranges' rounding and merge
            assert R.silence_ranges(got, sr, frames) == R.silence_ranges(R.erase_table(rows, pad_s, min_len_s), sr, frames)


def test_erase_table_arguments(lib):
    assert native.erase_table([], 0.1, 0.1) == []
    for bad in ((-0.1, 0.0), (0.0, -1.0), (float("nan"), 0.0), (0.0, float("inf"))):
        with pytest.raises(native.NativeError) as e:
            native.erase_table([(0.0, 1.0)], *bad)
        assert e.value.code == native.SS_ERR_ARG
        with pytest.raises(ValueError):
            native.stream_output_limit(16000, 10, None, *bad)
    # the filter is the review screen's: a region exactly min_len_s long is dropped
    assert native.erase_table([(1.0, 1.5), (2.0, 2.5000001)], 0.0, 0.5) == [(2.0, 2.5000001)]


def _sequences():
    """>= 200 random (covered, above) sequences of <= 400 bins: densities from all-below to all-above, runs and gaps whose lengths
    straddle break_s (0 and 0.5 s: 0, 1, 42, 43 bins) and the filter lengths, bins no window covers in the middle and at the end."""
    rng = np.random.default_rng(20240607)
    out = []
    for k in range(220):
        n = int(rng.integers(1, 401)) if k % 4 else int(rng.integers(1, 40))
        kind = k % 5
        if kind == 0:                                        # independent bins of one density
            d = (0.0, 1.0, 0.02, 0.5, 0.98)[(k // 5) % 5]
            above = rng.random(n) < d
        else:                                                # alternating runs and gaps of chosen lengths
            above = np.zeros(n, dtype=bool)
            at, on = int(rng.integers(0, 10)), True
            while at < n:
                ln = int(rng.choice([1, 2, 3, 25, 26, 27, 60, 170, 171, 172]) if on else rng.choice([1, 2, 41, 42, 43, 44, 90]))
                if on:
                    above[at:at + ln] = True
                at, on = at + ln, not on
        covered = np.ones(n, dtype=bool)
        if kind == 2:                                        # uncovered bins in the middle (they neither open nor close a run)
            for _ in range(int(rng.integers(1, 4))):
                a = int(rng.integers(0, n)); covered[a:a + int(rng.integers(1, 50))] = False
        if kind == 3:                                        # ... and behind the last window, as a whole-file plan has them
            covered[n - int(rng.integers(1, 4)):] = False
        out.append((covered, above))
    return out


def _final_ranges(covered, above, brk, pad_s, min_len_s, sr, frames):
    idx = np.flatnonzero(covered).astype(np.int64)
    avg = above[idx].astype(np.float64)
    regions = native.find_regions(avg, idx, 0.5, brk)
    return R.silence_ranges(native.erase_table(regions, pad_s, min_len_s), sr, frames)


def _latency_terms():
    hdr = open(os.path.join(ROOT, "include", "softspoken.h")).read()
    assert "D = B + break_s + pad_s + min_len_s" in hdr
    return lambda brk, pad_s, min_len_s: brk + pad_s + min_len_s          # D - B


def test_frames_below_the_limit_are_final(lib):
    d_minus_b = _latency_terms()
    seqs = _sequences()
    assert len(seqs) >= 200
    tail = 400                                               # longer than break_s + min_len_s + pad_s in bins (2.7 s = 231 bins)
    checked = moved = 0
    for k, (covered, above) in enumerate(seqs):
        brk = (0.0, 0.5)[k % 2]
        pad_s, min_len_s = PADS[(k // 2) % 3], MIN_LENS[(k // 6) % 3]
        sr = (8000, 16000, 44100)[k % 3]
        n = len(covered)
        frames = 10 ** 9                                     # no clamp at the recording's end: the limit is clamped to decoded frames
        truth = _final_ranges(covered, above, brk, pad_s, min_len_s, sr, frames)
        ext_c = np.concatenate([covered, np.ones(tail, dtype=bool)])
        w = R.Walk(brk)
        all_covered = True
        for b in range(n + 1):                               # the state after b final bins
            P, _ = w.pending()
            lim = native.stream_output_limit(sr, b, P, pad_s, min_len_s)
            assert lim == R.output_limit(sr, b, P, pad_s, min_len_s)
            top = max(lim, 0)
            want = R.clip(truth, 0, top)
            # the step's own rule (returned regions, a final current region, P's certain part) gives these ranges ...
            assert R.decided_ranges(w, sr, pad_s, min_len_s, top) == want, (k, b)
            # ... and so does every continuation: all bins above, all bins below the threshold
            for fill in (True, False):
                ext_a = np.concatenate([above[:b], np.full(n - b + tail, fill)])
                assert R.clip(_final_ranges(ext_c, ext_a, brk, pad_s, min_len_s, sr, frames), 0, top) == want, (k, b, fill)
            # latency: the limit trails the last final bin by at most D - B (one frame for the rounding)
            if b >= 1 and all_covered:
                assert lim >= ((R.bin_time(b - 1) - 3.0) - d_minus_b(brk, pad_s, min_len_s)) * sr - 1.0, (k, b)
                checked += 1
            moved += top > 0
            if b < n:
                all_covered = all_covered and bool(covered[b])
                w.bin(bool(covered[b]), bool(above[b]))
        w.finish()
        idx = np.flatnonzero(covered).astype(np.int64)
        assert w.regions == native.find_regions(above[idx].astype(np.float64), idx, 0.5, brk)      # the walk is ss_find_regions'
    assert checked > 10000 and moved > 1000


def test_the_filter_reads_the_table_values(lib):
    """(end - 3) - (start - 3) and end - start can differ in the last bit: the limit follows the table's."""
    found = 0
    for first in range(0, 3000, 7):
        for ln in (25, 26, 170, 171):
            s, e = R.bin_time(first), R.bin_time(first + ln)
            for min_len_s in (0.3, 2.0, (e - 3.0) - (s - 3.0), e - s):
                lim = native.stream_output_limit(16000, first + ln + 1, (s, e), 0.05, min_len_s)
                keeps = bool(native.erase_table([(s - 3.0, e - 3.0)], 0.05, min_len_s))
                assert lim == round((((e - 3.0) + 0.05) if keeps else ((s - 3.0) - 0.05)) * 16000)
                found += ((e - 3.0) - (s - 3.0) <= min_len_s) != (e - s <= min_len_s)
    assert found > 0, "no pair of bin times at which the two differences disagree"


# ---- StreamDetector's fallback with output streams, against a scripted context (tests/test_stream_logic.py's style) ----
class _Ctx:
    """A step 'returns' every frame pushed so far, one int16 per frame; an f16x2 context refuses a step whose new frames hold a NaN
    and commits nothing of it, output included."""

    def __init__(self, precision):
        self.precision = precision
        self.s, self.next = {}, 0

    def _open(self, erase):
        sid = self.next
        self.next += 1
        self.s[sid] = dict(data=[], done=0, frames_out=0, last=(0, []), erase=erase, closed=False)
        return sid

    def stream_open(self, fmt, sr, ch, thr, brk):
        return self._open(None)

    def stream_open_output(self, fmt, sr, ch, thr, brk, erase=None):
        return self._open(dict(erase or dict(pad_s=0.0, min_len_s=0.0)))

    def stream_push(self, sid, a, frames=None):
        self.s[sid]["data"] += list(np.asarray(a, dtype=np.float64).reshape(-1))

    def stream_close(self, sid):
        self.s[sid]["closed"] = True

    def stream_info(self, sid):
        st = self.s[sid]
        return dict(windows_ready=len(st["data"]) - st["done"], closed=st["closed"])

    def stream_step(self):
        if self.precision == "f16x2" and any(np.isnan(st["data"][st["done"]:]).any() for st in self.s.values()):
            raise native.NativeError(native.SS_ERR_RANGE, "f16x2: not finite")
        for st in self.s.values():
            st["done"] = len(st["data"])
            if st["erase"] is not None:                     # output lags the input by one frame, so a move carries held frames
                upto = len(st["data"]) if st["closed"] else max(st["frames_out"], len(st["data"]) - 1)
                st["last"] = (st["frames_out"], [0 if v != v else int(v) for v in st["data"][st["frames_out"]:upto]])
                st["frames_out"] = upto

    def stream_avg(self, sid):
        return np.zeros(0), np.zeros(0, dtype=np.int64)

    def stream_regions(self, sid):
        return []

    def stream_output(self, sid, channels):
        st = self.s[sid]
        if st["erase"] is None:
            raise native.NativeError(native.SS_ERR_STATE, "opened without output")
        return st["last"][0], np.array(st["last"][1], dtype=np.int16).reshape(-1, channels)

    def stream_output_info(self, sid):
        st = self.s[sid]
        return dict(frames_out=st["frames_out"], frames_held=len(st["data"]) - st["frames_out"], frames_erased=0, **st["erase"])

    def stream_export(self, sid):
        st = self.s[sid]
        return dict(st, data=list(st["data"]), last=(st["frames_out"], []))

    def stream_import(self, image):
        sid = self.next
        self.next += 1
        self.s[sid] = dict(image, data=list(image["data"]))
        return sid

    def stream_free(self, sid):
        del self.s[sid]

    def close(self):
        pass


def test_a_moved_stream_keeps_its_erase_parameters_and_its_place():
    made = []

    def factory(p):
        made.append(_Ctx(p))
        return made[-1]
    det = StreamDetector(precision="f16x2", context_factory=factory)
    s = det.open(native.PCM_F32, 16000, 1, erase=dict(pad_s=0.05, min_len_s=0.3))
    plain = det.open(native.PCM_F32, 16000, 1)
    assert s.erase == dict(pad_s=0.05, min_len_s=0.3) and plain.erase is None
    got, at = [], 0

    def step():
        nonlocal at
        out = det.step()
        assert set(out) == {s, plain} and len(out[s]) == 3          # step()'s return value is what it was
        first, a = s.output()
        assert first == at and a.shape[1] == 1                      # contiguous across the move
        got.extend(a[:, 0].tolist())
        at += len(a)
    s.push(np.array([1.0, 2.0, 3.0])); plain.push(np.array([1.0]))
    step()
    assert s.precision == "f16x2" and s.output_info()["frames_held"] == 1
    s.push(np.array([4.0, np.nan, 6.0]))                                # refused on f16x2: nothing of the output advances there
    step()
    assert s.precision == "fp32" and plain.precision == "f16x2" and len(made) == 2
    assert s.output_info()["pad_s"] == 0.05 and s.output_info()["min_len_s"] == 0.3
    s.push(np.array([7.0])); s.close()
    step()
    assert got == [1, 2, 3, 4, 0, 6, 7]
    assert s.output_info()["frames_out"] == 7
    with pytest.raises(native.NativeError) as e:
        plain.output()
    assert e.value.code == native.SS_ERR_STATE


def test_stream_wav_writer(lib, tmp_path):
    path = tmp_path / "out.wav"
    a = np.arange(-6, 6, dtype=np.int16).reshape(-1, 2)
    with StreamWavWriter(path, 48000, 2) as w:
        w.write((0, a[:2]))
        w.write((2, a[2:2]))
        w.write((2, a[2:]))
        with pytest.raises(ValueError):
            w.write((5, a[:1]))                                     # not where the file ends
    assert path.read_bytes() == native.wav_header_pcm16(48000, 2, 6) + a.astype("<i2").tobytes()
