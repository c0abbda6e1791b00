"""Plain-Python statement of the streaming silencer's host rules (include/softspoken.h "streaming silencer"), for
the tests: the erase table E(R), silence_ranges, the streaming region walk with its pending candidate P, and the limit time L.

Not imported by the library.  Every float operation is written in the order the header gives it, on Python floats (IEEE doubles)."""
from __future__ import annotations

import math


def bin_time(j: int) -> float:
    """NNDetector.py:185: the bin's time as the reference formats and re-reads it."""
    return float(f"{j / (256 / 3):.4f}")


def erase_table(regions, pad_s: float = 0.0, min_len_s: float = 0.0):
    """E(R) as regions: rows with end - start <= min_len_s dropped (a NaN row compares false and stays), the rest padded."""
    out = []
    for s, e in regions:
        if e - s <= min_len_s:
            continue
        out.append((s - pad_s, e + pad_s))
    return out


def silence_ranges(regions, sr: int, frames: int):
    """host.hip silence_ranges: Python round (half to even) of t * sr, clamped to [0, frames], sorted, overlapping or touching merged."""
    r = []
    for s, e in regions:
        a, b = float(s) * sr, float(e) * sr
        if a != a or b != b:
            continue
        a = -1e18 if a == -math.inf else 1e18 if a == math.inf else a
        b = -1e18 if b == -math.inf else 1e18 if b == math.inf else b
        lo, hi = min(max(round(a), 0), frames), min(max(round(b), 0), frames)
        if hi > lo:
            r.append((lo, hi))
    out = []
    for lo, hi in sorted(r):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [tuple(x) for x in out]


def clip(ranges, lo: int, hi: int):
    """The part of disjoint ascending ranges inside [lo, hi), touching pieces joined."""
    out = []
    for a, b in ranges:
        a, b = max(a, lo), min(b, hi)
        if b > a:
            if out and a <= out[-1][1]:
                out[-1][1] = max(out[-1][1], b)
            else:
                out.append([a, b])
    return [tuple(x) for x in out]


class Walk:
    """stream.hip walk_bin over (covered, above) bins in order, with RunMerger: `regions` are the returned (final) rows of the table."""

    def __init__(self, break_s: float):
        self.brk = break_s
        self.have, self.cur = False, [0.0, 0.0]               # RunMerger::cur: un-shifted bin times
        self.run_open, self.run_first, self.run_last = False, 0, 0
        self.regions = []
        self.bins = 0

    def _flush(self):
        if self.have:
            self.regions.append((self.cur[0] - 3.0, self.cur[1] - 3.0))
            self.have = False

    def _add(self, first, last):
        s0, e0 = bin_time(first), bin_time(last)
        if self.have and s0 - self.cur[1] <= self.brk:
            self.cur[1] = e0
            return
        self._flush()
        self.cur, self.have = [s0, e0], True

    def bin(self, covered: bool, above: bool):
        j = self.bins
        self.bins += 1
        if not covered:
            return
        if above:
            if not self.run_open:
                self.run_open, self.run_first = True, j
            self.run_last = j
            return
        if self.run_open:
            self._add(self.run_first, self.run_last)
            self.run_open = False
        if self.have and bin_time(j) - self.cur[1] > self.brk:
            self._flush()

    def finish(self):
        if self.run_open:
            self._add(self.run_first, self.run_last)
            self.run_open = False
        self._flush()

    def pending(self):
        """(P, D): P = (start, end) un-shifted bin times of the merged candidate that is not final yet, or None; D = the current
        region as a table row when the open run can no longer reach it (final though not returned), or None."""
        if self.run_open:
            rs, re = bin_time(self.run_first), bin_time(self.run_last)
            if self.have:
                if rs - self.cur[1] <= self.brk:
                    return (self.cur[0], re), None
                return (rs, re), (self.cur[0] - 3.0, self.cur[1] - 3.0)
            return (rs, re), None
        if self.have:
            return (self.cur[0], self.cur[1]), None
        return None, None


def output_limit(sr: int, bins_final: int, pending, pad_s: float, min_len_s: float) -> int:
    """nearbyint(L * sr) of the header's rule, before any clamp."""
    if pending is None:
        L = (bin_time(bins_final) - 3.0) - pad_s
    else:
        s, e = pending[0] - 3.0, pending[1] - 3.0
        L = (s - pad_s) if e - s <= min_len_s else (e + pad_s)
    return round(L * sr)


def decided_ranges(walk: Walk, sr: int, pad_s: float, min_len_s: float, limit: int):
    """What a step erases below `limit` (stream_plan.h plan_output): the returned regions, a final current region, P's certain part."""
    rows = list(walk.regions)
    P, D = walk.pending()
    if D is not None:
        rows.append(D)
    if P is not None:
        rows.append((P[0] - 3.0, P[1] - 3.0))
    return clip(silence_ranges(erase_table(rows, pad_s, min_len_s), sr, max(limit, 0)), 0, max(limit, 0))
