"""The separation streams' rule, no GPU: every frame below ss_stream_separate_limit has the same merged interval, the same capped
distance to the interval's ends and the same STFT gain rows under every continuation of the recording; the limit
with the fade term left out is caught; no returned frame lags the audio held by more than D_sep."""
import os

import numpy as np
import pytest

import separation_ref as S
import stream_output_ref as R
import stream_separate_ref as Q
from softspoken_amd import native
from test_stream_output_host import _sequences

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADS = (0.0, 0.05, 0.7)
MIN_LENS = (0.0, 0.3, 2.0)
FADES = (0.0, 0.01, 0.5)
RATES = (8000, 22050, 48000)
TAIL = 500                                                   # bins: longer than break_s + min_len_s + pad_s + fade_s (3.7 s = 316 bins)


@pytest.fixture(scope="module")
def lib(build_all):
    return native.lib()


def _held(b, sr):
    """The most audio a stream can hold with only b final bins (bound B of include/softspoken.h): frames."""
    return max(0, int((R.bin_time(b) - 3.0 + Q.bound_b(sr) - 3.0 / 256.0) * sr))


def _intervals(covered, above, brk, pad_s, min_len_s, sr, frames):
    idx = np.flatnonzero(covered).astype(np.int64)
    regions = native.find_regions(above[idx].astype(np.float64), idx, 0.5, brk)
    return R.silence_ranges(native.erase_table(regions, pad_s, min_len_s), sr, frames)


def _walk(covered, above, brk, pad_s, min_len_s, fade_s, sr, stats, without_fade=False):
    """One sequence bin by bin.  Returns the number of states at which a frame below the (possibly wrong) limit was NOT decided."""
    n = len(covered)
    F, N = round(fade_s * sr), S.fft_size(sr)
    ext_c = np.concatenate([covered, np.ones(TAIL, dtype=bool)])
    # the recordings the three continuations belong to: the true one ends where the sequence ends, the others TAIL bins later
    conts = [(covered, above, _held(n, sr), n)]
    w = R.Walk(brk)
    done = 0
    undecided = 0
    all_covered = True
    for b in range(n + 1):
        P, _ = w.pending()
        H = _held(b, sr)
        if without_fade:
            lim = Q.separate_limit(sr, H, b, P, pad_s, min_len_s, fade_s, without_fade=True)
        else:
            lim = native.stream_separate_limit(sr, H, b, P, pad_s, min_len_s, fade_s=fade_s)
            assert lim == Q.separate_limit(sr, H, b, P, pad_s, min_len_s, fade_s), (b, lim)
        top = min(max(lim, done), H)
        if top > done:
            states, rows = [], []
            for fill in (None, True, False):
                if fill is None:
                    c, a, frames, nb = conts[0]
                else:
                    c, a = ext_c, np.concatenate([above[:b], np.full(n - b + TAIL, fill)])
                    frames, nb = _held(n + TAIL, sr), n + TAIL
                if frames < top:                            # (the true recording may end below a later state's audio: not a continuation of it)
                    continue
                iv = _intervals(c, a, brk, pad_s, min_len_s, sr, frames)
                states.append(Q.blend_state(iv, done, top, F))
                rows.append(Q.frame_gain_rows(done, top, sr, nb))
            same = all(np.array_equal(s[0], states[0][0]) and np.array_equal(s[1], states[0][1]) for s in states[1:])
            if without_fade:
                undecided += not same
            else:
                assert same, ("interval or weight not decided", b, done, top)
                free = Q.frame_gain_rows(done, top, sr, 1 << 40)
                assert all(r == free for r in rows), ("gain rows not decided", b)
                assert all(j1 <= b - 1 for _, _, j1, _ in free) and top + N <= H
                stats["frames"] += top - done
                stats["inside"] += int((states[0][0] >= 0).sum())
                stats["fading"] += int(((states[0][1] >= 0) & (states[0][1] < F)).sum())
            done = top
        if not without_fade and b >= 1 and all_covered:
            slack = Q.d_sep(sr, brk, pad_s, min_len_s, fade_s) - (H - max(lim, 0)) / sr
            assert slack >= 0.0, (b, slack)
            stats["slack"] = min(stats["slack"], slack)
        if b < n:
            all_covered = all_covered and bool(covered[b])
            w.bin(bool(covered[b]), bool(above[b]))
    return undecided


def _params(k):
    return (0.0, 0.5)[k % 2], PADS[(k // 2) % 3], MIN_LENS[(k // 6) % 3], FADES[(k // 3) % 3], RATES[k % 3]


def test_frames_below_the_limit_are_final(lib):
    seqs = _sequences()
    assert len(seqs) >= 200
    stats = dict(frames=0, inside=0, fading=0, slack=1e9)
    for k, (covered, above) in enumerate(seqs):
        brk, pad_s, min_len_s, fade_s, sr = _params(k)
        _walk(covered, above, brk, pad_s, min_len_s, fade_s, sr, stats)
    print(f"STREAM_SEP host: frames={stats['frames']} inside={stats['inside']} fading={stats['fading']} smallest D_sep slack={stats['slack']:.4f} s")
    assert stats["frames"] > 5 * 10 ** 5 and stats["inside"] > 10 ** 5 and stats["fading"] > 10 ** 4
    assert stats["slack"] < 0.1                              # the bound is not idle: some walk comes within 0.1 s of it


def _bins(*runs):
    """above / covered from (gap, run) bin counts"""
    a = []
    for gap, run in runs:
        a += [False] * gap + [True] * run
    a = np.array(a + [False] * 60, dtype=bool)
    return np.ones(len(a), dtype=bool), a


def test_a_later_padded_region_joins_an_earlier_interval(lib):
    """break_s = 0, pad_s = 0.7: two regions 1.17 s apart are two rows of the table and one interval.  The earlier interval's
    fade-out is not final until the later region can no longer appear: 0.9 s behind the earlier region the zeroing limit enters the
    fade-out (F = 0.5 s), and the later region, which removes it, opens only then."""
    covered, above = _bins((300, 60), (100, 60))
    for sr in RATES:
        iv = _intervals(covered, above, 0.0, 0.7, 0.0, sr, 10 ** 9)
        assert len(iv) == 1
        stats = dict(frames=0, inside=0, fading=0, slack=1e9)
        _walk(covered, above, 0.0, 0.7, 0.0, 0.5, sr, stats)
        assert stats["fading"] > 0
        # with the fade term left out of condition 1 the walk returns frames of a fade-out that the join then removes
        assert _walk(covered, above, 0.0, 0.7, 0.0, 0.5, sr, stats, without_fade=True) > 0


def test_an_interval_shorter_than_two_fades(lib):
    covered, above = _bins((300, 25), (200, 26))
    for sr in RATES:
        F = round(0.5 * sr)
        iv = _intervals(covered, above, 0.0, 0.0, 0.0, sr, 10 ** 9)
        assert len(iv) == 2 and all(e - a < 2 * F for a, e in iv)
        stats = dict(frames=0, inside=0, fading=0, slack=1e9)
        _walk(covered, above, 0.0, 0.0, 0.0, 0.5, sr, stats)
        assert stats["inside"] == stats["fading"] > 0        # no sample of either interval reaches weight 1
        assert _walk(covered, above, 0.0, 0.0, 0.0, 0.5, sr, stats, without_fade=True) > 0


def test_the_limit_without_the_fade_term_is_caught(lib):
    caught = 0
    for k, (covered, above) in enumerate(_sequences()):
        brk, pad_s, min_len_s, fade_s, sr = _params(k)
        if fade_s > 0:
            caught += _walk(covered, above, brk, pad_s, min_len_s, fade_s, sr, {}, without_fade=True) > 0
    assert caught >= 5


def test_latency_expression_and_arguments(lib):
    hdr = open(os.path.join(ROOT, "include", "softspoken.h")).read()
    assert "D_sep = D + fade_s + (N + 1) / sample_rate" in hdr
    for sr in RATES + (16000, 384000):
        for brk, pad_s, min_len_s, fade_s in ((0.5, 0.05, 0.3, 0.01), (0.0, 0.7, 2.0, 0.5)):
            assert native.stream_separate_latency(sr, brk, pad_s, min_len_s, fade_s=fade_s) == pytest.approx(Q.d_sep(sr, brk, pad_s, min_len_s, fade_s), abs=1e-12)
    for bad in (dict(fade_s=-0.1), dict(min_gain=2.0), dict(speech_channel=3), dict(above_fmax=9)):
        with pytest.raises(ValueError):
            native.stream_separate_limit(16000, 1000, 10, None, 0.0, 0.0, **bad)
        with pytest.raises(ValueError):
            native.stream_separate_latency(16000, 0.5, 0.0, 0.0, **bad)
    with pytest.raises(ValueError):
        native.stream_separate_limit(16000, 1000, 10, None, -1.0, 0.0)
    # before any bin is final nothing is returned; the limit never passes the audio held less one FFT
    assert native.stream_separate_limit(16000, 16000, 0, None) <= 0
    assert native.stream_separate_limit(16000, 16000, 2000, None) == 16000 - 512
