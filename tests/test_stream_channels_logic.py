"""Each-channel streams without a GPU: the three functions are exported and bound, the ABI version stays, and StreamDetector routes
channel_mode through a scripted context -- "mix" by the unchanged stream_open / stream_open_output calls, "each" by
stream_open_channels, anything else refused before a context call -- and keeps the mode across the range rule's export / import."""
import ctypes

import numpy as np
import pytest

from softspoken_amd import native
from softspoken_amd.stream import Stream, StreamDetector

NEW = ("ss_stream_open_channels", "ss_stream_avg_channel", "ss_stream_region_peaks")


def test_the_library_exports_the_three_functions(build_all):
    L = native.lib()
    for name in NEW:
        assert name in native.EXPORTS
        assert isinstance(getattr(L, name), ctypes._CFuncPtr)
    assert L.ss_abi_version() == 3 == native.ABI_VERSION


def test_the_bindings_exist():
    for name in ("stream_open_channels", "stream_avg_channel", "stream_region_peaks"):
        assert callable(getattr(native.Context, name))
    for name in ("avg", "peaks"):
        assert callable(getattr(Stream, name))


class _Ctx:
    """Records every call.  A step 'finalises' one bin per pushed frame; an f16x2 step over a NaN is refused and commits nothing."""

    def __init__(self, precision, log):
        self.precision, self.log = precision, log
        self.s, self.next = {}, 0

    def _open(self, call, **kw):
        self.log.append((self.precision, call))
        sid = self.next
        self.next += 1
        self.s[sid] = dict(kw, data=[], done=0, out=[])
        return sid

    def stream_open(self, fmt, sr, ch, thr, brk):                        # the signatures StreamDetector has always called
        return self._open(("stream_open", fmt, sr, ch, thr, brk), each=False)

    def stream_open_output(self, fmt, sr, ch, thr, brk, erase):
        return self._open(("stream_open_output", fmt, sr, ch, thr, brk, erase), each=False)

    def stream_open_channels(self, fmt, sr, ch, thr, brk, erase=None, with_output=False):
        return self._open(("stream_open_channels", fmt, sr, ch, thr, brk, erase), each=True, ch=ch)

    def stream_push(self, sid, a, frames=None):
        self.s[sid]["data"] += list(np.asarray(a, dtype=np.float64).reshape(-1))

    def stream_info(self, sid):
        return dict(windows_ready=len(self.s[sid]["data"]) - self.s[sid]["done"])

    def stream_step(self):
        self.log.append((self.precision, ("step",)))
        if self.precision == "f16x2" and any(np.isnan(st["data"][st["done"]:]).any() for st in self.s.values()):
            raise native.NativeError(native.SS_ERR_RANGE, "f16x2: not finite")
        for st in self.s.values():
            st["out"] = list(range(st["done"], len(st["data"])))
            st["done"] = len(st["data"])

    def stream_avg(self, sid):
        st = self.s[sid]
        return np.array([st["data"][j] for j in st["out"]], dtype=np.float64), np.array(st["out"], dtype=np.int64)

    def stream_avg_channel(self, sid, channel):
        assert self.s[sid]["each"] and 0 <= channel < self.s[sid]["ch"]
        a, i = self.stream_avg(sid)
        return a + channel, i

    def stream_region_peaks(self, sid, channels):
        assert self.s[sid]["each"]
        return np.zeros((0, channels))

    def stream_regions(self, sid):
        return []

    def stream_export(self, sid):
        self.log.append((self.precision, ("export",)))
        return dict(self.s[sid], data=list(self.s[sid]["data"]), out=[])

    def stream_import(self, image):
        self.log.append((self.precision, ("import",)))
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


def test_an_unknown_channel_mode_is_refused_before_any_context_call():
    det, made, log = _det()
    for bad in ("left", "", None, "EACH"):
        with pytest.raises(ValueError):
            det.open(native.PCM_S16, 48000, 2, channel_mode=bad)
    assert log == [] and len(made) == 1 and made[0].s == {}


def test_mix_keeps_its_calls_and_each_goes_through_stream_open_channels():
    det, made, log = _det()
    a = det.open(native.PCM_S16, 48000, 2, 0.2, 0.4)
    b = det.open(native.PCM_S16, 48000, 2, 0.2, 0.4, erase=dict(pad_s=0.05), channel_mode="mix")
    c = det.open(native.PCM_S16, 48000, 2, 0.2, 0.4, channel_mode="each")
    d = det.open(native.PCM_S16, 48000, 2, 0.2, 0.4, erase={}, channel_mode="each")
    assert [e[1] for e in log] == [
        ("stream_open", native.PCM_S16, 48000, 2, 0.2, 0.4),
        ("stream_open_output", native.PCM_S16, 48000, 2, 0.2, 0.4, dict(pad_s=0.05, min_len_s=0.0)),
        ("stream_open_channels", native.PCM_S16, 48000, 2, 0.2, 0.4, None),
        ("stream_open_channels", native.PCM_S16, 48000, 2, 0.2, 0.4, dict(pad_s=0.0, min_len_s=0.0)),
    ]
    assert [s.channel_mode for s in (a, b, c, d)] == ["mix", "mix", "each", "each"]
    assert (c.erase, d.erase) == (None, dict(pad_s=0.0, min_len_s=0.0))


def test_a_refused_step_moves_an_each_channel_stream_and_it_stays_one():
    det, made, log = _det()
    s = det.open(native.PCM_F32, 48000, 2, channel_mode="each")
    m = det.open(native.PCM_F32, 48000, 2)
    s.push(np.array([1.0, 2.0])); m.push(np.array([4.0]))
    out = det.step()
    # step()'s value keeps its shape: {stream: (regions, avg, bin_idx)}
    assert set(out) == {s, m}
    for v in out.values():
        assert isinstance(v, tuple) and len(v) == 3 and v[0] == [] and v[1].dtype == np.float64 and v[2].dtype == np.int64
    assert np.array_equal(out[s][1], [1.0, 2.0]) and np.array_equal(s.avg(1)[0], [2.0, 3.0]) and s.peaks().shape == (0, 2)
    s.push(np.array([np.nan, 5.0]))
    out = det.step()
    assert [e[1][0] for e in log[-5:]] == ["step", "export", "import", "step", "step"]
    assert [e[0] for e in log[-5:]] == ["f16x2", "f16x2", "fp32", "f16x2", "fp32"]
    assert s.precision == "fp32" and m.precision == "f16x2"
    assert s.channel_mode == "each" and made[1].s[s._sid]["each"] and m.channel_mode == "mix"
    assert np.array_equal(out[s][2], [2, 3]) and np.array_equal(out[s][1], [np.nan, 5.0], equal_nan=True)
    assert np.array_equal(s.avg(1)[1], [2, 3])
