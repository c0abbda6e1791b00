"""SilenceJob(method="band") without a GPU, on a stub context: the (ID, file_name) lookup of a review row's band, per-channel rows,
the missing-row and NaN fallbacks (the whole band goes), the ValueErrors, and that the "zero" and "separate" paths still receive the
arguments they received before."""
import math
import os

import numpy as np
import pandas as pd
import pytest


@pytest.fixture(scope="module")
def silence(build_all):
    from softspoken_amd import silence
    return silence


class StubCtx:
    """Records every call; returns zeros of the shape the real call returns."""

    def __init__(self):
        self.calls = []

    def _out(self, fmt, channels, frames, source):
        from softspoken_amd import native
        return np.zeros((frames, channels * native._BPS[fmt]), dtype=np.uint8) if source else np.zeros((frames, channels), dtype=np.int16)

    def box_silence_pcm(self, pcm, fmt, sr, channels, boxes, **kw):
        self.calls.append(("box_silence_pcm", fmt, sr, channels, boxes, kw))
        return self._out(fmt, channels, kw["frames"], kw["encoding"] == "source")

    def silence_pcm(self, pcm, fmt, sr, channels, frames, regions):
        self.calls.append(("silence_pcm", fmt, sr, channels, frames, regions))
        return self._out(fmt, channels, frames, False)

    def silence_pcm_source(self, pcm, fmt, sr, channels, frames, regions):
        self.calls.append(("silence_pcm_source", fmt, sr, channels, frames, regions))
        return self._out(fmt, channels, frames, True)

    def separate_pcm(self, pcm, fmt, sr, channels, frames, regions, **kw):
        self.calls.append(("separate_pcm", fmt, sr, channels, frames, regions, kw))
        return self._out(fmt, channels, frames, False)

    def separate_pcm_channels(self, pcm, fmt, sr, channels, frames, regions, **kw):
        self.calls.append(("separate_pcm_channels", fmt, sr, channels, frames, regions, kw))
        return self._out(fmt, channels, frames, False)


class StubModel:
    def __init__(self, ctx):
        self.ctx, self.keys = ctx, []

    def with_range_fallback(self, fn, key=None):
        self.keys.append(key)
        return fn(self.ctx)


@pytest.fixture()
def files(tmp_path):
    from softspoken_amd import synth
    src = tmp_path / "in"
    src.mkdir()
    (tmp_path / "out").mkdir()
    for name, ch in (("a.wav", 2), ("b.wav", 1)):
        pcm = synth.to_pcm16(synth.synth_audio(3, 1.0, 16000, ch, with_silence=False))
        (src / name).write_bytes(synth.wav_bytes(pcm, 16000))
    df = pd.DataFrame({"ID": [1, 2, 3, 4, 5], "file_path": [str(src)] * 5, "file_name": ["a.wav", "a.wav", "b.wav", "a.wav", "b.wav"],
                       "start_time": [0.1, 0.4, 0.2, 0.7, 0.6], "end_time": [0.2, 0.5, 0.3, 0.8, 0.7], "erase": [1, 1, 1, 0, 1]})
    return df, str(tmp_path / "out"), str(src)


def _same(a, b):
    return len(a) == len(b) and all(x == y or (x != x and y != y) for p, q in zip(a, b) for x, y in zip(p, q))


def test_band_job_builds_the_boxes(silence, files, tmp_path):
    df, out, src = files
    nan = float("nan")
    bands = pd.DataFrame({"ID": [1, 1, 2, 2, 3, 5, 4],
                          "file_name": ["a.wav", "a.wav", "other.wav", None, "b.wav", "b.wav", "a.wav"],
                          "channel": [0, 1, nan, nan, nan, nan, nan],
                          "low_hz": [300.0, 400.0, 1.0, 250.0, nan, 100.0, 5.0],
                          "high_hz": [3000.0, 3500.0, 2.0, 2500.0, 4000.0, math.inf, 6.0]})
    ctx = StubCtx()
    job = silence.SilenceJob(df, out, ctx=ctx, method="band", bands=bands, fade_s=0.02, min_gain=0.1, edge_hz=50.0)
    paths = job.run()
    assert not job.errors and sorted(os.path.basename(p) for p in paths) == ["a_silenced.wav", "b_silenced.wav"]
    calls = {c[3]: c for c in ctx.calls}                               # by channel count: a.wav 2, b.wav 1
    assert len(ctx.calls) == 2 and all(c[0] == "box_silence_pcm" for c in ctx.calls)
    kw = dict(frames=16000, encoding="pcm16", fade_s=0.02, min_gain=0.1, edge_hz=50.0)
    assert calls[2][1:4] == (2, 16000, 2) and calls[2][5] == kw and calls[1][5] == kw
    # row 1: its two per-channel rows, each on its own channel; row 2: the entry without a file name (other.wav's is another recording's)
    assert _same(calls[2][4], [(0.1, 0.2, 300.0, 3000.0, 0), (0.1, 0.2, 400.0, 3500.0, 1), (0.4, 0.5, 250.0, 2500.0, None)])
    # row 3: a NaN edge, row 5: an infinite one -> the whole band; row 4 is not erased
    assert _same(calls[1][4], [(0.2, 0.3, nan, nan, None), (0.6, 0.7, nan, nan, None)])
    assert open(os.path.join(out, "a_silenced.wav"), "rb").read()[:4] == b"RIFF"


def test_band_job_reads_a_side_file_and_falls_back_without_a_row(silence, files, tmp_path):
    df, out, src = files
    side = tmp_path / "det_bands.csv"
    side.write_text("ID,file_name,channel,low_hz,high_hz,peak_hz,speech_share,n_bins\n"
                    "1,a.wav,,312.5,2890.25,800.0,0.9,40\n"
                    "3,b.wav,0,150.0,900.0,300.0,0.8,12\n")
    ctx = StubCtx()
    job = silence.SilenceJob(df, out, ctx=ctx, method="band", bands=str(side), encoding="source")
    job.run()
    assert not job.errors
    calls = {c[3]: c for c in ctx.calls}
    nan = float("nan")
    assert _same(calls[2][4], [(0.1, 0.2, 312.5, 2890.25, None), (0.4, 0.5, nan, nan, None)])           # row 2 has no band row
    assert _same(calls[1][4], [(0.2, 0.3, 150.0, 900.0, 0), (0.6, 0.7, nan, nan, None)])
    assert calls[2][5] == dict(frames=16000, encoding="source", fade_s=0.01, min_gain=0.0, edge_hz=100.0)
    want = open(os.path.join(src, "a.wav"), "rb").read()
    got = open(os.path.join(out, "a_silenced.wav"), "rb").read()
    assert len(got) == len(want) and got[:44] == want[:44]                # the source's own image around the new sample bytes
    assert silence.silence_files(df, out, ctx=StubCtx(), method="band", bands=str(side), edge_hz=10.0)


def test_value_errors(silence, files):
    df, out, _ = files
    with pytest.raises(ValueError):
        silence.SilenceJob(df, out, ctx=StubCtx(), method="band")
    with pytest.raises(ValueError):
        silence.SilenceJob(df, out, ctx=StubCtx(), method="band", bands=pd.DataFrame({"ID": [1], "low_hz": [1.0]}))
    with pytest.raises(ValueError):
        silence.SilenceJob(df, out, ctx=StubCtx(), method="bands", bands=pd.DataFrame())
    with pytest.raises(ValueError):
        silence.SilenceJob(df, out, method="separate")
    assert silence.SilenceJob.METHODS == ("zero", "separate", "band")
    import inspect
    assert inspect.signature(silence.SilenceJob.__init__).parameters["method"].default == "zero"
    assert inspect.signature(silence.silence_files).parameters["method"].default == "zero"


def test_zero_and_separate_receive_what_they_received(silence, files):
    df, out, src = files
    ctx = StubCtx()
    silence.SilenceJob(df, out, ctx=ctx).run()
    assert ctx.calls == [("silence_pcm", 2, 16000, 2, 16000, [(0.1, 0.2), (0.4, 0.5)]), ("silence_pcm", 2, 16000, 1, 16000, [(0.2, 0.3), (0.6, 0.7)])]
    ctx = StubCtx()
    silence.SilenceJob(df, out, ctx=ctx, encoding="source", bands="ignored-without-the-band-method.csv").run()
    assert [c[0] for c in ctx.calls] == ["silence_pcm_source"] * 2 and ctx.calls[0][1:] == (2, 16000, 2, 16000, [(0.1, 0.2), (0.4, 0.5)])
    ctx = StubCtx()
    model = StubModel(ctx)
    silence.SilenceJob(df, out, method="separate", model=model, min_gain=0.05, channel_mode="each").run()
    kw = dict(fade_s=0.01, min_gain=0.05, above_fmax="mute", speech_channel=1)
    assert ctx.calls == [("separate_pcm_channels", 2, 16000, 2, 16000, [(0.1, 0.2), (0.4, 0.5)], kw),
                         ("separate_pcm", 2, 16000, 1, 16000, [(0.2, 0.3), (0.6, 0.7)], kw)]
    assert model.keys == [("separate", os.path.join(src, "a.wav")), ("separate", os.path.join(src, "b.wav"))]
