"""ss_find_regions_union (host only): the merged table of a recording whose channels were detected alone -- "speech on any channel".
By definition it is ss_find_regions on the element-wise, NaN-ignoring maximum of the channels' averaged scores, so the reference here
is the float64 oracle's find_regions on np.fmax over the channels."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle_np as O


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


def _want(avg, idx, threshold=0.1, break_s=0.5):
    return O.regions_minus_pad(O.find_regions(np.fmax.reduce(np.asarray(avg, dtype=np.float64), axis=0), idx, threshold, break_s))


def _series(rng, n_ch, n):
    """Random walks around the threshold (runs and short gaps both occur), a different one per channel."""
    return np.stack([np.cumsum(rng.standard_normal(n)) * 0.05 + 0.1 + rng.standard_normal(n) * 0.02 for _ in range(n_ch)]) if n \
        else np.zeros((n_ch, 0))


@pytest.mark.parametrize("n_ch", [1, 2, 5])
def test_union_matches_the_oracle_on_the_channel_maximum(native, n_ch):
    rng = np.random.default_rng(100 + n_ch)
    differs = 0
    for trial in range(40):
        n = int(rng.integers(0, 3000))
        avg = _series(rng, n_ch, n)
        if n:                                             # values exactly at the threshold (not above), on one channel and on all
            at = rng.integers(0, n, size=max(1, n // 20))
            avg[rng.integers(0, n_ch), at] = 0.1
            avg[:, at[: len(at) // 2]] = 0.1
            # a NaN in one channel where the others are above / are not above, and a bin that is NaN on every channel
            k = rng.integers(0, n, size=max(1, n // 25))
            avg[rng.integers(0, n_ch), k] = np.nan
            avg[:, k[: len(k) // 3]] = np.nan
        idx = np.sort(rng.choice(np.arange(n + 60), size=n, replace=False)).astype(np.int64) if n else np.zeros(0, np.int64)   # holes: uncovered bins
        got = native.find_regions_union(avg, idx)
        assert got == _want(avg, idx), (n_ch, trial)
        if n_ch == 1:
            assert got == native.find_regions(avg[0], idx)
        elif n:
            differs += any(got != native.find_regions(avg[c], idx) for c in range(n_ch))
    assert n_ch == 1 or differs > 20                      # (the merged table is not simply one channel's)


def test_nan_on_one_channel_does_not_hide_the_other(native):
    idx = np.arange(6, dtype=np.int64)
    nan = np.nan
    a = np.array([[nan, 0.5, nan, 0.0, nan, 0.5],
                  [0.5, nan, 0.0, nan, nan, 0.5]])
    # bins 0, 1 above (one channel each, the other NaN); 2, 3 not above (closes the run); 4 NaN on both: in the series, not above; 5 above
    assert native.find_regions_union(a, idx, break_s=0.0) == _want(a, idx, break_s=0.0)
    t = lambda i: float(O.time_str(i)) - 3
    assert native.find_regions_union(a, idx, break_s=0.0) == [(t(0), t(1)), (t(5), t(5))]
    assert native.find_regions_union(np.full((2, 4), nan), idx[:4]) == []
    # np.maximum would have lost bins 0 and 1
    assert O.find_regions(np.maximum(a[0], a[1]), idx, 0.1, 0.0) != O.find_regions(np.fmax(a[0], a[1]), idx, 0.1, 0.0)


def test_threshold_is_strict_and_a_gap_of_exactly_break_merges(native):
    idx = np.arange(400, dtype=np.int64)
    a = np.zeros((2, 400))
    a[0, 10:20] = 0.1                                     # exactly the threshold: no detection
    a[1, 1:5] = np.nextafter(0.1, 1.0)                    # the next double: a detection
    # runs on different channels whose distance in "%.4f" seconds is exactly / just over break_s: 0.75 s = 64 bins
    a[0, 100:109] = 1.0
    a[1, 108 + 64:190] = 1.0                              # first bin 172: 172 * 3 / 256 - 108 * 3 / 256 = 0.75
    a[0, 300:310] = 1.0
    a[1, 309 + 65:390] = 1.0                              # one bin more: not merged
    for brk in (0.75, 0.5):
        assert native.find_regions_union(a, idx, break_s=brk) == _want(a, idx, break_s=brk)
    got = native.find_regions_union(a, idx, break_s=0.75)
    t = lambda i: float(O.time_str(i)) - 3
    assert float(O.time_str(172)) - float(O.time_str(108)) == 0.75
    assert got == [(t(1), t(4)), (t(100), t(189)), (t(300), t(309)), (t(374), t(389))]


def test_capacity_and_argument_errors(native):
    L = native.lib()
    a = np.zeros((2, 8))
    a[0, 1] = a[1, 5] = 1.0
    idx = np.arange(8, dtype=np.int64)
    out = (native.Region * 4)()
    n = C.c_int64(-1)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert L.ss_find_regions_union(p(a), p(idx), 8, 2, 0.1, 0.0, out, 4, C.byref(n)) == native.SS_OK and n.value == 2
    n.value = -1
    assert L.ss_find_regions_union(p(a), p(idx), 8, 2, 0.1, 0.0, out, 1, C.byref(n)) == native.SS_ERR_CAPACITY and n.value == 2
    assert L.ss_find_regions_union(p(a), p(idx), 8, 0, 0.1, 0.0, out, 4, C.byref(n)) == native.SS_ERR_ARG
    assert L.ss_find_regions_union(p(a), p(idx), 8, -3, 0.1, 0.0, out, 4, C.byref(n)) == native.SS_ERR_ARG
    assert L.ss_find_regions_union(None, p(idx), 8, 2, 0.1, 0.0, out, 4, C.byref(n)) == native.SS_ERR_ARG
    assert L.ss_find_regions_union(p(a), None, 8, 2, 0.1, 0.0, out, 4, C.byref(n)) == native.SS_ERR_ARG
    assert L.ss_find_regions_union(p(a), p(idx), -1, 2, 0.1, 0.0, out, 4, C.byref(n)) == native.SS_ERR_ARG
    assert L.ss_find_regions_union(p(a), p(idx), 8, 2, 0.1, 0.0, out, 4, None) == native.SS_ERR_ARG
    assert L.ss_find_regions_union(None, None, 0, 3, 0.1, 0.0, out, 4, C.byref(n)) == native.SS_OK and n.value == 0
    with pytest.raises(ValueError):
        native.find_regions_union(np.zeros(8), idx)
    with pytest.raises(ValueError):
        native.find_regions_union(a, idx[:5])


def test_new_exports_are_declared_and_bound(native):
    hdr = open(os.path.join(os.path.dirname(native.__file__), "..", "include", "softspoken.h")).read()
    for name in ("ss_add_pcm_channels", "ss_add_pcm_channels_device", "ss_add_pcm_channels_batch_device", "ss_find_regions_union",
                 "ss_get_regions_union", "ss_get_region_peaks"):
        assert name in native.EXPORTS and name + "(" in hdr and getattr(native.lib(), name) is not None
    assert native.lib().ss_abi_version() == 3
    for meth in ("add_pcm_channels", "add_pcm_channels_device", "add_pcm_channels_batch_device", "regions_union", "region_peaks"):
        assert callable(getattr(native.Context, meth))
