"""numpy float64 statement of the stream bands' accumulation (include/softspoken.h "stream bands") for the
tests: the host's bin-by-bin region walk with the events it hands to the device, and the device's walk over the final bins -- one
running tile sum, one completed-tile sum, a snapshot of both, a parked profile -- cut into steps anywhere.  Beside it the per-region
definition as the two whole-file kernels evaluate it in float64 (tile sums from 0.0, added in ascending tile order from 0.0), which the
streamed form must reproduce bit for bit.

Not imported by the library.  Maps are float32 [2][n_bins][128] from bin 0; flags are the stream's two bits per bin (1: covered by a
window, 2: average above the threshold)."""
from __future__ import annotations

import math

import numpy as np

from bands_ref import region_bins

RESET, SNAP, PARK, EMIT_SNAP, EMIT_PARK = range(5)
NO_CLAMP = 1 << 40


def bin_time(j: int) -> float:
    """float(f"{idx / (256 / 3):.4f}"): the detector's time of a bin (before the -3 s)."""
    return float("%.4f" % (j / (256.0 / 3.0)))


def power64(y) -> np.ndarray:
    """P(y) = expm1(min(y^2 ln 10, 600)) in float64 as the device evaluates it; NaN -> 0."""
    y32 = np.asarray(y, dtype=np.float32)
    y = y32.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        a = y * y * 2.302585092994045684
        a = np.where(a < 600.0, a, 600.0)
        p = np.expm1(a)
    return np.where(np.isnan(y32), 0.0, p)


def whole_file_profile(maps: np.ndarray, b0: int, cnt: int) -> np.ndarray:
    """E [2][128] float64 of the bins b0 .. b0 + cnt - 1: band_profile_kernel's tile sums added as band_bounds_kernel adds them."""
    E = np.zeros((2, 128))
    b = b0
    while b < b0 + cnt:
        e = min(b0 + cnt, ((b >> 6) + 1) << 6)
        P = power64(maps[:, b:e, :])
        part = np.zeros((2, 128))
        for j in range(e - b):
            part = part + P[:, j, :]
        E = E + part
        b = e
    return E


def whole_file_regions(flags, brk: float):
    """The whole-file table of a flag series: runs of covered bins above the threshold, merged over gaps of at most brk (RunMerger)."""
    out, cur, first, last, is_open = [], None, 0, 0, False

    def add(a, b):
        nonlocal cur
        s0, e0 = bin_time(a), bin_time(b)
        if cur is not None and s0 - cur[1] <= brk:
            cur[1] = e0
            return
        if cur is not None:
            out.append((cur[0] - 3.0, cur[1] - 3.0))
        cur = [s0, e0]

    for j, f in enumerate(flags):
        if not f & 1:
            continue
        if f & 2:
            if not is_open:
                is_open, first = True, j
            last = j
        elif is_open:
            add(first, last)
            is_open = False
    if is_open:
        add(first, last)
    if cur is not None:
        out.append((cur[0] - 3.0, cur[1] - 3.0))
    return out


class StreamBands:
    """One lane of a band stream.  step(maps, flags, b1, closing) takes in the bins [bins_done, b1) and returns the regions that became
    final with their profiles and bin counts: [((start, end), E [2][128] float64, n_bins)].  snap_shift moves every snapshot by that many
    bins (0: the protocol; the tests use 1 to show that the comparison notices)."""

    def __init__(self, brk: float, snap_shift: int = 0):
        self.brk, self.snap_shift = float(brk), snap_shift
        self.bins_done = 0
        self.run_open, self.run_first, self.run_last = False, 0, 0
        self.have, self.cur = False, [0.0, 0.0]
        self.parked = False
        z = lambda: np.zeros((2, 128))
        self.done, self.tile, self.snap_done, self.snap_tile, self.park = z(), z(), z(), z(), z()

    # ---- the host's walk: regions and events ----
    @staticmethod
    def _pos(bin_t: float) -> int:
        return region_bins(bin_t - 3.0, bin_t - 3.0, 0, NO_CLAMP)[0]

    def _emit(self, out, ev):
        r = (self.cur[0] - 3.0, self.cur[1] - 3.0)
        ev.append((0, EMIT_PARK if self.parked else EMIT_SNAP, region_bins(r[0], r[1], 0, NO_CLAMP)[1], len(out)))
        out.append(r)
        self.parked = False
        self.have = False

    def _snap(self, ev, b0):
        pos = self._pos(bin_time(self.run_last)) + self.snap_shift
        if pos >= b0:
            ev.append((pos, SNAP, 0, 0))

    def _close_run(self, out, ev, b0):
        s0, e0 = bin_time(self.run_first), bin_time(self.run_last)
        if self.have and s0 - self.cur[1] <= self.brk:
            self.cur[1] = e0
        else:
            if self.have:
                self._emit(out, ev)
            self.cur, self.have = [s0, e0], True
        self.run_open = False
        self._snap(ev, b0)

    def _walk(self, flags, b0, b1, closing):
        out, ev = [], []
        for j in range(b0, b1):
            f = int(flags[j])
            if not f & 1:
                continue
            if f & 2:
                if not self.run_open:
                    self.run_open, self.run_first = True, j
                    if not (self.have and bin_time(j) - self.cur[1] <= self.brk):
                        if self.have:
                            ev.append((0, PARK, 0, 0))
                            self.parked = True
                        ev.append((self._pos(bin_time(j)), RESET, 0, 0))
                self.run_last = j
                continue
            if self.run_open:
                self._close_run(out, ev, b0)
            if self.have and bin_time(j) - self.cur[1] > self.brk:
                self._emit(out, ev)
        if closing:
            if self.run_open:
                self._close_run(out, ev, b0)
            if self.have:
                self._emit(out, ev)
        elif self.run_open:
            self._snap(ev, b0)
        return out, ev

    # ---- the device's walk over the step's final bins ----
    def _advance(self, P, j, to, b0):
        while j < to:
            self.tile = self.tile + P[:, j - b0, :]
            if (j & 63) == 63:
                self.done = self.done + self.tile
                self.tile = np.zeros((2, 128))
            j += 1
        return j

    def step(self, maps, flags, b1: int, closing: bool = False):
        b0 = self.bins_done
        regions, ev = self._walk(flags, b0, b1, closing)
        P = power64(maps[:, b0:b1, :])
        j, res = b0, [None] * len(regions)
        for pos, typ, n_bins, rec in ev:
            if typ in (RESET, SNAP):
                j = self._advance(P, j, min(max(pos, j), b1), b0)
                if typ == RESET:
                    self.done, self.tile = np.zeros((2, 128)), np.zeros((2, 128))
                else:
                    self.snap_done, self.snap_tile = self.done.copy(), self.tile.copy()
            elif typ == PARK:
                self.park = self.snap_done + self.snap_tile
            else:
                E = self.park.copy() if typ == EMIT_PARK else self.snap_done + self.snap_tile
                res[rec] = (regions[rec], E, n_bins)
        self._advance(P, j, b1, b0)
        self.bins_done = b1
        return res

    def state_doubles(self) -> int:
        return 5 * 256


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)
