"""Region bands, the host side (include/softspoken.h "region bands"), no GPU: ss_region_bins against the header's double expression
on every boundary it can trip over, ss_band_edges against the front-end's mel points, the refusals that need no device, and the
reference's own pieces (tests/bands_ref.py) against hand-made cases."""
import ctypes as C
import math

import numpy as np
import pytest

import bands_ref as B
import separation_ref as R


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


def _both(native, s, e, covered):
    got = native.region_bins(s, e, covered)
    want = B.region_bins(s, e, 0, covered)
    assert got == want, (s, e, covered, got, want)
    return got


def test_region_bins_equals_the_rule_on_every_boundary_and_centre(native):
    covered = 560                                                     # a file whose last covered bin lies inside the sweep
    xs = []
    for j in range(0, 601):
        for x in (j * 3 / 256 - 3, (j + 0.5) * 3 / 256 - 3):         # a bin's boundary, a bin's centre
            xs += [float(np.nextafter(x, -np.inf)), x, float(np.nextafter(x, np.inf))]
    xs = np.array(xs)
    for x in xs:
        first, cnt = _both(native, float(x), float(x) + 0.1, covered)
        _both(native, -4.0, float(x), covered)
        assert 0 <= first <= covered and 0 <= cnt <= covered - first
    # the centre rule itself, from the centres: bin j is inside exactly when start <= t_j < end
    t = (np.arange(covered) + 0.5) * 3 / 256 - 3
    for s, e in ((-3.0, -3.0 + 3 / 512), (-3.0, float(np.nextafter(-3.0 + 3 / 512, np.inf))), (1.0, 2.0), (0.123, 0.1235),
                 (float(t[100]), float(t[101])), (float(np.nextafter(t[100], np.inf)), float(t[101]))):
        first, cnt = _both(native, s, e, covered)
        inside = np.flatnonzero((t >= s) & (t < e))
        assert cnt == inside.size and (cnt == 0 or first == inside[0]), (s, e)


def test_region_bins_edges_of_the_file_and_empty_ranges(native):
    covered = 560
    assert _both(native, -3.0, 100.0, covered) == (0, covered)       # start = -3.0, end beyond the file
    assert _both(native, -50.0, -3.0, covered)[1] == 0               # wholly before
    assert _both(native, 50.0, 60.0, covered) == (covered, 0)        # wholly behind: no bin
    assert _both(native, 1.0, 1.0, covered)[1] == 0                  # empty
    assert _both(native, 1.0, 1.0 + 1e-9, covered)[1] == 0           # shorter than the distance to the next centre
    assert _both(native, 0.0, 1e300, covered)[1] == covered - 256
    assert _both(native, -1e300, 0.0, covered) == (0, 256)
    assert _both(native, 0.0, 1.0, 0) == (0, 0)                      # a file without a covered bin
    for bad in ((math.nan, 1.0), (0.0, math.inf), (-math.inf, 0.0), (1.0, 0.999)):
        with pytest.raises(native.NativeError) as e:
            native.region_bins(*bad, covered)
        assert e.value.code == native.SS_ERR_ARG
    with pytest.raises(native.NativeError):
        native.region_bins(0.0, 1.0, -1)


def test_the_detectors_four_decimals_never_move_a_bin(native):
    """A region of the detector's table runs from bin j's boundary to bin k's, both printed with "%.4f" (before the -3): the rounding
    moves a boundary by at most 0.05 ms, a centre is 5.9 ms away, so the region's bins are j .. k - 1 whatever the rounding did."""
    covered = 700
    for j in range(0, 601):
        s = float("%.4f" % (j * 3 / 256)) - 3.0
        e = float("%.4f" % ((j + 7) * 3 / 256)) - 3.0
        assert _both(native, s, e, covered) == (j, 7), j
        assert _both(native, float("%.4f" % (j * 3 / 256 - 3)), e, covered) == (j, 7), j


def test_band_edges_are_the_front_ends_mel_points(native):
    f = native.band_edges()
    want = R.mel_points()
    assert f.dtype == np.float64 and f.shape == (130,) and np.array_equal(f, want)
    assert f[0] == 0.0 and abs(f[129] - 8000.0) < 0.01 and (np.diff(f) > 0).all()


def _call(native, regions, n, q=(0.05, 0.95), sp=1, out=True, from_maps=False):
    L = native.lib()
    arr = native._regions(regions)
    p = native.BandParams(q[0], q[1], sp, 0)
    buf = (native.RegionBand * max(1, len(regions)))()
    o = buf if out else None
    if from_maps:
        m = np.zeros((1, 2, 4, 128), dtype=np.float32)
        rc = L.ss_region_bands_from_maps(None, native._ptr(m), 1, 0, 4, arr, n, C.byref(p), o, None)
    else:
        rc = L.ss_region_bands(None, 0, 1, arr, n, C.byref(p), o, None)
    msg = L.ss_last_error(None)
    return rc, (msg or b"").decode()


@pytest.mark.parametrize("from_maps", [False, True])
def test_refusals_that_need_no_device(native, from_maps):
    ok = [(0.0, 1.0)]
    for q in ((0.0, 0.95), (0.5, 0.5), (0.6, 0.4), (0.05, 1.0001), (-0.1, 0.9), (math.nan, 0.95), (0.05, math.nan)):
        rc, msg = _call(native, ok, 1, q=q, from_maps=from_maps)
        assert rc == native.SS_ERR_ARG and "q_low" in msg, (q, msg)
    rc, msg = _call(native, ok, 1, sp=2, from_maps=from_maps)
    assert rc == native.SS_ERR_ARG and "speech_channel" in msg
    for bad in ((math.nan, 1.0), (0.0, math.inf), (-math.inf, 1.0), (1.0, 0.5)):
        rc, msg = _call(native, [(0.0, 1.0), bad], 2, from_maps=from_maps)
        assert rc == native.SS_ERR_ARG and "region 1" in msg, (bad, msg)
    rc, msg = _call(native, ok, 1, out=False, from_maps=from_maps)
    assert rc == native.SS_ERR_ARG and "null output" in msg
    rc, msg = _call(native, ok, -1, from_maps=from_maps)
    assert rc == native.SS_ERR_ARG
    rc, msg = _call(native, ok, 1, from_maps=from_maps)                # nothing wrong but the missing context
    assert rc == native.SS_ERR_ARG and "null context" in msg
    assert C.sizeof(native.RegionBand) == 48 == native.REGION_BAND_DTYPE.itemsize and C.sizeof(native.BandParams) == 24


# ---- the reference's own pieces ------------------------------------------------------------------------------------------------
def test_reference_on_hand_made_maps():
    maps = np.zeros((2, 10, 128), dtype=np.float32)
    maps[1, :, 40] = 1.0                                              # P = 9 per bin
    maps[0, :, 3] = 1.0
    r = B.reference(maps, 100, [(B_t(100), B_t(110)), (B_t(103), B_t(105)), (50.0, 60.0)])
    assert [x["n_bins"] for x in r] == [10, 2, 0]
    assert (r[0]["band_low"], r[0]["band_high"], r[0]["band_peak"]) == (40, 40, 40)
    assert abs(float(r[0]["E"][1, 40]) - 90.0) < 1e-12 and abs(r[0]["speech_share"] - 0.5) < 1e-15
    f = R.mel_points()
    assert (r[0]["low_hz"], r[0]["high_hz"], r[0]["peak_hz"]) == (f[40], f[42], f[41])
    assert r[2]["band_low"] == -1 and math.isnan(r[2]["low_hz"]) and math.isnan(r[2]["speech_share"])
    assert float(B.power(np.float32("nan"))) == 0.0 and np.isfinite(float(B.power(np.float32("inf"))))
    assert float(B.power(np.float32(20.0))) == float(B.power(np.float32("inf")))           # both at the cap
    # quantiles: powers 1, 2, 3, 4 in bands 10 .. 13 -> C / T = .1, .3, .6, 1
    E = np.zeros((2, 128), dtype=np.longdouble)
    E[1, 10:14] = [1, 2, 3, 4]
    b = B.bounds(E, 0.05, 0.95)
    assert (b["band_low"], b["band_high"], b["band_peak"]) == (10, 13, 13)
    b = B.bounds(E, 0.3, 0.6)
    assert (b["band_low"], b["band_high"]) == (11, 12)                # C[m] >= q T with equality
    assert B.bounds(E, 0.05, 1.0)["band_high"] == 13                  # q_high = 1: the last band with power
    assert B.near_ties(E, B.bounds(E, 0.3, 0.6), 1e-15, 0.3, 0.6) == dict(low=True, high=True, peak=False)


def B_t(j):
    """bin j's boundary in seconds"""
    return j * 3 / 256 - 3


def test_map_error_margins_follow_the_derivative():
    """A band decision that a 1e-4 map error can flip is reported unsafe, one far from its quantile safe."""
    maps = np.zeros((2, 4, 128), dtype=np.float32)
    maps[1, :, 20] = 1.0
    maps[1, :, 60] = 1.0
    maps[1, :, 100] = 1.0                                             # C / T = 1/3, 2/3, 1
    reg = (B_t(0), B_t(4))
    assert B.map_error_margins(maps, 0, reg, q_low=0.05, q_high=0.95) == dict(low=True, high=True, peak=False)   # three equal peaks
    assert not B.map_error_margins(maps, 0, reg, q_low=1 / 3, q_high=0.95)["low"]
    maps[1, :, 60] = 1.2
    assert B.map_error_margins(maps, 0, reg)["peak"]
    # the size of the figure: dP = 2 y ln 10 (P + 1) dy
    y, dy = 1.0, 2.0 ** -13                                            # (both exact in float32)
    exact = float(B.power(np.float32(y + dy)) - B.power(np.float32(y)))
    assert exact <= 2 * (y + dy) * math.log(10) * (10 ** ((y + dy) ** 2)) * dy * (1 + 1e-6)
