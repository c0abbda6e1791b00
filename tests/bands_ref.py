"""numpy statement of the region bands (include/softspoken.h "region bands") for the tests: the bin rule as the
header's double expression, P and every sum in np.longdouble, the band decisions from those, and the two figures the tests hold the
device to -- the error bound on a profile value and what a map error can move C / T by.

Not imported by the library.  Maps are float32 [2][n_bins][128] for the bins first_bin .. (ss_separation_maps' layout)."""
from __future__ import annotations

import math

import numpy as np

from separation_ref import mel_points

LD = np.longdouble
LN10 = np.log(LD(10.0))
CAP = LD(600.0)
EPS = 2.0 ** -53
HEAD_ERROR = 1e-4                      # the project's bar on a head output against the CPU oracle


def edge_bin(x: float) -> int:
    """ceil((x + 3.0) * 256.0 / 3.0 - 0.5) in double, left to right: the first bin whose centre (j + 0.5) 3 / 256 - 3 is >= x."""
    return math.ceil((float(x) + 3.0) * 256.0 / 3.0 - 0.5)


def region_bins(start: float, end: float, lo: int, hi: int):
    """(first, count) of the bins of [start, end) among the bins [lo, hi)."""
    a = min(max(edge_bin(start), lo), hi)
    b = min(max(edge_bin(end), lo), hi)
    return a, max(0, b - a)


def power(y) -> np.ndarray:
    """P(y) = expm1(min(y^2 ln 10, 600)) in long double; NaN -> 0."""
    y = np.asarray(y, dtype=np.float32).astype(LD)
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.minimum(y * y * LN10, CAP)
    a = np.where(np.isnan(a), LD(0.0), a)
    return np.expm1(a)


def profile(maps: np.ndarray, first_bin: int, b0: int, cnt: int):
    """E [2][128] (long double) over the bins b0 .. b0 + cnt - 1, summed tile by tile (j >> 6) as the definition says; also the largest
    a = y^2 ln 10 (capped) of the sum and the number of tiles."""
    E = np.zeros((2, 128), dtype=LD)
    a_max, tiles = 0.0, 0
    b = b0
    while b < b0 + cnt:
        e = min(b0 + cnt, ((b >> 6) + 1) << 6)
        rows = maps[:, b - first_bin: e - first_bin, :]
        part = np.zeros((2, 128), dtype=LD)
        P = power(rows)
        for j in range(e - b):
            part = part + P[:, j, :]
        E = E + part
        with np.errstate(over="ignore", invalid="ignore"):
            a = np.minimum(rows.astype(np.float64) ** 2 * math.log(10.0), 600.0)
        if np.isfinite(a).any():
            a_max = max(a_max, float(np.nanmax(a)))
        tiles += 1
        b = e
    return E, a_max, tiles


def profile_bound(a_max: float, n_tiles: int) -> float:
    """Relative error bound of a device profile value, in units of 2^-53 (every term of the sum is >= 0, so the relative errors of the
    terms and of the two sequential sums add): 3 for expm1, 2 max(a, 1) for the two roundings of a (the double ln 10 and the product)
    carried through P's condition a / (1 - e^-a), 64 for the additions inside a tile, n_tiles for those across.  DESIGN.md section 18
    goes through the terms."""
    return (3 + 2 * max(a_max, 1.0) + 64 + n_tiles) * EPS


def bounds(E, q_low=0.05, q_high=0.95, speech_channel=1, n_bins=1, hz=None) -> dict:
    """Step 4 from a profile E [2][128]: band indices, frequencies, share; plus C and T (long double) for the margins."""
    hz = mel_points() if hz is None else hz
    Es = np.asarray(E[speech_channel], dtype=LD)
    C = np.cumsum(Es)
    T = C[127]
    Te = np.asarray(E[1 - speech_channel], dtype=LD).sum()
    if n_bins == 0 or not T > 0:
        return dict(band_low=-1, band_high=-1, band_peak=-1, low_hz=math.nan, high_hz=math.nan, peak_hz=math.nan,
                    speech_share=math.nan, n_bins=n_bins, C=C, T=T)
    lo = int(np.argmax(C >= LD(q_low) * T))
    hi = int(np.argmax(C >= LD(q_high) * T))
    pk = int(np.argmax(Es))
    return dict(band_low=lo, band_high=hi, band_peak=pk, low_hz=float(hz[lo]), high_hz=float(hz[hi + 2]), peak_hz=float(hz[pk + 1]),
                speech_share=float(T / (T + Te)), n_bins=n_bins, C=C, T=T)


def near_ties(E, b: dict, bound: float, q_low=0.05, q_high=0.95, speech_channel=1) -> dict:
    """Which of the three decisions lie near a tie: some |C[m] - q T| <= 2 bound T; the two largest E closer than 2 bound T."""
    if b["band_low"] < 0:
        return dict(low=False, high=False, peak=False)
    C, T = b["C"], b["T"]
    tol = LD(2.0 * bound) * T
    Es = np.sort(np.asarray(E[speech_channel], dtype=LD))
    return dict(low=bool((np.abs(C - LD(q_low) * T) <= tol).any()), high=bool((np.abs(C - LD(q_high) * T) <= tol).any()),
                peak=bool(Es[-1] - Es[-2] < tol))


def reference(maps, first_bin, regions, q_low=0.05, q_high=0.95, speech_channel=1):
    """Steps 1, 3, 4 for every region over maps [2][n_bins][128]: a list of dicts (bounds' keys, E, bound, ties)."""
    n_bins = maps.shape[1]
    hz = mel_points()
    out = []
    for s, e in regions:
        b0, cnt = region_bins(s, e, first_bin, first_bin + n_bins)
        E, a_max, tiles = profile(maps, first_bin, b0, cnt)
        r = bounds(E, q_low, q_high, speech_channel, cnt, hz)
        r["E"], r["first"] = E, b0
        r["bound"] = profile_bound(a_max, max(tiles, 1))
        r["ties"] = near_ties(E, r, r["bound"], q_low, q_high, speech_channel)
        out.append(r)
    return out


def profile_error_ratio(got, want, bound: float) -> float:
    """max over the cells of |got - want| / (bound * want) (0 where both are 0; inf where only the reference is 0)."""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(want > 0, err / (LD(bound) * want), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def map_error_margins(maps, first_bin, region, dy=HEAD_ERROR, q_low=0.05, q_high=0.95, speech_channel=1) -> dict:
    """Can a map error of |dy| per cell move a band decision of this region?  dP / dy = 2 y ln 10 (P + 1) grows with y, so by the mean
    value theorem |P(y + d) - P(y)| <= dE(y) := 2 (|y| + dy) ln 10 (P(|y| + dy) + 1) dy for |d| <= dy.  With D[m] the sum of dE over the
    region's bins in band m, Dc[m] = D[0] + .. + D[m], R = T - C[m] and Dr = D_total - Dc[m], the ratio C[m] / T stays inside
        [(C - Dc) / ((C - Dc) + (R + Dr)),  (C + Dc) / ((C + Dc) + (R - Dr))]      (numerators and R - Dr floored at 0)
    and a quantile decision is safe when q lies in none of the 128 intervals; the peak is safe when E[peak] - D[peak] exceeds every
    other E[m] + D[m].  -> dict(low=, high=, peak= booleans: safe), or all False for a region without an estimate."""
    n_bins = maps.shape[1]
    b0, cnt = region_bins(region[0], region[1], first_bin, first_bin + n_bins)
    E, _, _ = profile(maps, first_bin, b0, cnt)
    Es = E[speech_channel]
    T = Es.sum()
    if cnt == 0 or not T > 0:
        return dict(low=False, high=False, peak=False)
    y = np.abs(maps[speech_channel, b0 - first_bin: b0 - first_bin + cnt, :].astype(LD)) + LD(dy)
    D = (LD(2.0) * y * LN10 * (np.expm1(np.minimum(y * y * LN10, CAP)) + LD(1.0)) * LD(dy)).sum(axis=0)
    C, Dc = np.cumsum(Es), np.cumsum(D)
    Rr, Dr = T - C, Dc[127] - Dc
    zero = LD(0.0)
    c_lo, c_hi = np.maximum(C - Dc, zero), C + Dc
    r_lo_den, r_hi_den = c_lo + Rr + Dr, c_hi + np.maximum(Rr - Dr, zero)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.where(r_lo_den > 0, c_lo / r_lo_den, zero)
        hi = np.where(r_hi_den > 0, c_hi / r_hi_den, LD(1.0))
    safe = {}
    for name, q in (("low", q_low), ("high", q_high)):
        safe[name] = bool(((LD(q) < lo) | (LD(q) > hi)).all())
    pk = int(np.argmax(Es))
    others = np.delete(Es + D, pk)
    safe["peak"] = bool(Es[pk] - D[pk] > others.max())
    return safe
