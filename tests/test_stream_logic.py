"""StreamDetector's range rule (softspoken_amd/stream.py) against a scripted context, no GPU: the first step the f16x2 mode refuses
moves exactly that step's streams to an fp32 context and repeats the step there; a second one moves everything, with one log line;
nothing is lost or duplicated across a move."""
import logging

import numpy as np
import pytest

from softspoken_amd import native
from softspoken_amd.stream import StreamDetector


class _Ctx:
    """Streams hold the frames pushed so far; a step 'finalises' every frame not yet returned as one bin per frame.  A step on an
    f16x2 context whose pending frames hold a NaN is refused (SS_ERR_RANGE) and commits nothing."""

    def __init__(self, precision, log):
        self.precision, self.log = precision, log
        self.s, self.next = {}, 0

    def stream_open(self, fmt, sr, ch, thr, brk):
        sid = self.next
        self.next += 1
        self.s[sid] = dict(fmt=fmt, data=[], done=0, out=[], closed=False)
        return sid

    def stream_push(self, sid, a, frames=None):
        self.s[sid]["data"] += list(np.asarray(a, dtype=np.float64).reshape(-1))

    def stream_close(self, sid):
        self.s[sid]["closed"] = True

    def stream_info(self, sid):
        st = self.s[sid]
        return dict(windows_ready=len(st["data"]) - st["done"], closed=st["closed"])

    def stream_step(self):
        self.log.append(("step", self.precision, sorted(self.s)))
        if self.precision == "f16x2" and any(np.isnan(st["data"][st["done"]:]).any() for st in self.s.values()):
            raise native.NativeError(native.SS_ERR_RANGE, "f16x2: not finite")
        for st in self.s.values():
            st["out"] = list(range(st["done"], len(st["data"])))
            st["done"] = len(st["data"])

    def stream_avg(self, sid):
        st = self.s[sid]
        return np.array([st["data"][j] for j in st["out"]], dtype=np.float64), np.array(st["out"], dtype=np.int64)

    def stream_regions(self, sid):
        return []

    def stream_export(self, sid):
        st = self.s[sid]
        return dict(st, data=list(st["data"]), out=[])

    def stream_import(self, image):
        sid = self.next
        self.next += 1
        self.s[sid] = dict(image, data=list(image["data"]), out=[])
        return sid

    def stream_free(self, sid):
        del self.s[sid]

    def close(self):
        pass


def _det():
    log, made = [], []

    def factory(p):
        made.append(_Ctx(p, log))
        return made[-1]
    return StreamDetector(precision="f16x2", context_factory=factory), made, log


def _collect(got, out):
    for s, (_, a, i) in out.items():
        got.setdefault(s, []).append((a, i))


def _joined(got, s):
    a = np.concatenate([x[0] for x in got[s]]); i = np.concatenate([x[1] for x in got[s]])
    return a, i


def test_first_refused_step_moves_exactly_its_streams(caplog):
    det, made, log = _det()
    a, b, c = (det.open(native.PCM_F32, 16000, 1) for _ in range(3))
    got = {}
    a.push(np.arange(3.0)); b.push(np.arange(3.0)); c.push(np.arange(3.0))
    _collect(got, det.step())
    a.push(np.array([5.0, np.nan, 7.0])); b.push(np.array([1.0]))            # c has nothing new: no windows in the refused step
    with caplog.at_level(logging.WARNING):
        _collect(got, det.step())
    assert [m.precision for m in made] == ["f16x2", "fp32"]
    assert a.precision == "fp32" and b.precision == "fp32" and c.precision == "f16x2"
    assert not [r for r in caplog.records if "every stream" in r.getMessage()]
    # the refused step on f16x2, then the same step again without the moved streams, then the step on fp32
    assert [e[1] for e in log] == ["f16x2", "f16x2", "f16x2", "fp32"]
    for s, want in ((a, [0, 1, 2, 5, np.nan, 7]), (b, [0, 1, 2, 1]), (c, [0, 1, 2])):
        v, i = _joined(got, s)
        assert np.array_equal(i, np.arange(len(want)))                       # nothing lost, nothing twice
        assert np.array_equal(v, np.array(want, dtype=np.float64), equal_nan=True)
    c.push(np.array([9.0]))
    _collect(got, det.step())
    assert np.array_equal(_joined(got, c)[1], np.arange(4))


def test_second_refused_step_switches_everything_once(caplog):
    det, made, log = _det()
    a, b = det.open(native.PCM_F32, 16000, 1), det.open(native.PCM_F32, 16000, 1)
    got = {}
    a.push(np.array([np.nan])); b.push(np.array([1.0]))
    _collect(got, det.step())                          # first: a and b move (both had windows)
    c = det.open(native.PCM_F32, 16000, 1)             # a new stream still opens on f16x2
    assert c.precision == "f16x2"
    d = det.open(native.PCM_F32, 16000, 1)
    c.push(np.array([np.nan, 2.0]))
    with caplog.at_level(logging.WARNING):
        _collect(got, det.step())                      # second: every stream, open or new, moves
        e = det.open(native.PCM_F32, 16000, 1)
        e.push(np.array([4.0])); d.push(np.array([3.0]))
        _collect(got, det.step())
    lines = [r for r in caplog.records if "every stream" in r.getMessage()]
    assert len(lines) == 1
    assert all(s.precision == "fp32" for s in (a, b, c, d, e))
    assert det.precision == "fp32"
    assert len(made) == 2                              # one fp32 context, shared
    assert np.array_equal(_joined(got, c)[1], [0, 1]) and np.isnan(_joined(got, c)[0][0])
    assert np.array_equal(_joined(got, d)[1], [0]) and np.array_equal(_joined(got, e)[1], [0])
    assert np.array_equal(_joined(got, b)[1], [0])


def test_other_errors_are_not_a_range_fallback():
    class _Bad(_Ctx):
        def stream_step(self):
            raise native.NativeError(2, "device lost")
    det = StreamDetector(precision="f16x2", context_factory=lambda p: _Bad(p, []))
    det.open(native.PCM_F32, 16000, 1)
    with pytest.raises(native.NativeError):
        det.step()
