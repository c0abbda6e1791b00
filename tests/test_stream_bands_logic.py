"""Stream bands, the event protocol, no GPU: the streamed accumulation of tests/stream_bands_ref.py -- running
tile sum, completed-tile sum, snapshot, parked profile, driven by the bin-by-bin region walk and cut into random steps -- against the
per-region definition as the two whole-file kernels evaluate it in float64, bit for bit, over several hundred seeded cases; and the
walk's table against the library's ss_find_regions."""
import numpy as np
import pytest

import stream_bands_ref as S
from bands_ref import region_bins


def _maps(rng, n_bins):
    """Random maps [2][n_bins][128] with the values the definition singles out: NaN, +-inf, 1e-20, values past the cap."""
    m = np.abs(rng.standard_normal((2, n_bins, 128))).astype(np.float32) * np.float32(rng.choice([0.3, 1.0, 3.0]))
    for v, p in ((np.nan, 0.01), (np.inf, 0.003), (-np.inf, 0.002), (1e-20, 0.02), (17.0, 0.01), (-2.5, 0.02), (0.0, 0.05)):
        m[rng.random(m.shape) < p] = np.float32(v)
    return m


def _flags(rng, n_bins, kind):
    """A flag series: runs and gaps of every length, single-bin runs, runs that start or end on a tile boundary."""
    f = np.ones(n_bins, dtype=np.uint8)                       # covered
    if kind == "all":
        f |= 2
    elif kind == "none":
        pass
    else:
        j = int(rng.integers(0, 40))
        while j < n_bins:
            run = int(rng.choice([1, 1, 2, 5, 20, 64, 100, 200]) if kind == "mixed" else rng.integers(1, 80))
            if rng.random() < 0.3:                               # start or end on a multiple of 64
                j = min(n_bins, (j + 63) // 64 * 64)
                if rng.random() < 0.5:
                    run = 64 * int(rng.integers(1, 3))
            f[j:j + run] |= 2
            j += run + int(rng.choice([1, 2, 3, 4, 5, 30, 50, 128, 300]))
    tail = int(rng.integers(0, 12))                              # bins no window covers, behind the last window only
    if tail:
        f[n_bins - tail:] = 0
    return f


def _cuts(rng, n_bins):
    kind = rng.integers(0, 4)
    if kind == 0:
        return [n_bins]
    if kind == 1:
        return list(range(1, n_bins + 1))                       # a step per bin
    if kind == 2:
        return sorted(set(rng.integers(1, n_bins, size=int(rng.integers(1, 30))).tolist()) | {n_bins})
    return sorted(set(range(51, n_bins, 51)) | {n_bins})        # the cadence of one window per step


def _run_stream(maps, flags, brk, cuts, snap_shift=0, empty_steps=None):
    st = S.StreamBands(brk, snap_shift)
    got = []
    for k, b1 in enumerate(cuts):
        if empty_steps is not None and k in empty_steps:
            got += st.step(maps, flags, st.bins_done, False)     # a step in which no bin became final
        got += st.step(maps, flags, b1, False)
    got += st.step(maps, flags, cuts[-1], True)                  # the close: no new bin, the last regions
    return got


def _check(maps, flags, brk, cuts, empty_steps=None):
    want_regions = S.whole_file_regions(flags, brk)
    got = _run_stream(maps, flags, brk, cuts, 0, empty_steps)
    assert [g[0] for g in got] == want_regions
    n_bins = len(flags)
    for (r, E, n) in got:
        b0, cnt = region_bins(r[0], r[1], 0, n_bins)
        assert n == cnt, (r, n, cnt)
        want = S.whole_file_profile(maps, b0, cnt)
        assert np.array_equal(S.bits(E), S.bits(want)), (r, b0, cnt)
    return got


@pytest.mark.parametrize("seed", range(40))
def test_streamed_accumulation_equals_the_definition_bit_for_bit(seed):
    rng = np.random.default_rng(9100 + seed)
    n_regions = 0
    for _ in range(8):                                           # 320 cases
        n_bins = int(rng.integers(70, 700))
        maps = _maps(rng, n_bins)
        flags = _flags(rng, n_bins, rng.choice(["runs", "mixed", "mixed", "all", "none"]))
        brk = float(rng.choice([0.0, 0.0118, 0.03, 0.05, 0.5, 5.0]))
        cuts = _cuts(rng, n_bins)
        empty = set(rng.integers(0, len(cuts), size=3).tolist()) if rng.random() < 0.5 else None
        n_regions += len(_check(maps, flags, brk, cuts, empty))
    assert n_regions > 0


def test_the_seams_by_hand():
    rng = np.random.default_rng(5)
    n_bins = 400
    maps = _maps(rng, n_bins)

    def flags_of(runs):
        f = np.ones(n_bins, dtype=np.uint8)
        for a, b in runs:
            f[a:b + 1] |= 2
        return f
    cases = [
        ([(64, 128)], 0.5),                      # starts on a tile boundary; its last bin (excluded by rule 1) is one too: ends on one
        ([(10, 63)], 0.5), ([(10, 64)], 0.5), ([(10, 65)], 0.5),
        ([(100, 100)], 0.5),                     # one bin: no bin at all under rule 1 -> "no estimate"
        ([(100, 101)], 0.5),                     # one bin used
        ([(20, 40), (45, 90)], 0.5),             # a gap that merges
        ([(20, 40), (45, 90)], 0.01),            # the same gap, not merged
        ([(20, 40), (42, 42), (130, 135), (137, 200)], 0.03),
        ([(0, 399)], 0.5),                       # open from the first bin to the last
        ([(0, 5), (390, 399)], 5.0),             # one region across everything
    ]
    for runs, brk in cases:
        flags = flags_of(runs)
        for cuts in ([n_bins], list(range(1, n_bins + 1)), [64, 128, 192, 400], [63, 65, 101, 102, 400], [41, 42, 43, 44, 45, 46, 400]):
            got = _check(maps, flags, brk, cuts)
            assert len(got) == len(S.whole_file_regions(flags, brk))
    one = _check(maps, flags_of([(100, 100)]), 0.5, [n_bins])
    assert one[0][2] == 0 and not one[0][1].any()
    # a region's profile crosses a tile boundary: more than one tile sum took part
    r = _check(maps, flags_of([(10, 200)]), 0.5, [50, 100, 400])[0]
    assert r[2] == 190


def test_a_snapshot_one_bin_off_is_noticed():
    rng = np.random.default_rng(77)
    n_bins = 300
    maps = _maps(rng, n_bins)
    flags = np.ones(n_bins, dtype=np.uint8)
    flags[30:120] |= 2
    flags[200:260] |= 2
    want = [S.whole_file_profile(maps, *region_bins(r[0], r[1], 0, n_bins)) for r in S.whole_file_regions(flags, 0.5)]
    for shift in (1, -1):
        got = _run_stream(maps, flags, 0.5, [100, 150, 300], snap_shift=shift)
        assert len(got) == len(want) == 2
        assert any(not np.array_equal(S.bits(g[1]), S.bits(w)) for g, w in zip(got, want))
    got = _run_stream(maps, flags, 0.5, [100, 150, 300])
    assert all(np.array_equal(S.bits(g[1]), S.bits(w)) for g, w in zip(got, want))


def test_state_does_not_depend_on_the_length():
    assert S.StreamBands(0.5).state_doubles() == 5 * 256


def test_the_walk_is_the_librarys(build_all):
    from softspoken_amd import native
    rng = np.random.default_rng(3)
    for _ in range(30):
        n_bins = int(rng.integers(50, 900))
        flags = _flags(rng, n_bins, "mixed")
        brk = float(rng.choice([0.0, 0.03, 0.05, 0.5, 5.0]))
        cov = np.nonzero(flags & 1)[0]
        avg = np.where(flags[cov] & 2, 1.0, 0.0)
        want = native.find_regions(avg, cov, 0.5, brk)
        assert S.whole_file_regions(flags, brk) == want
        # rule 1 keeps the walk's bins: a region runs from its first bin to just before the last bin of its last run
        for s, e in want:
            b0, cnt = native.region_bins(s, e, n_bins)
            assert (flags[b0] & 2) and (flags[b0 + cnt] & 2) and (cnt == 0 or b0 + cnt < n_bins)
