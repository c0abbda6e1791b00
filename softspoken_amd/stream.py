"""Streaming detection on one device: many recordings whose PCM arrives in pieces, stepped together (ss_stream_* of
include/softspoken.h).  Every region and averaged bin a stream returns is final, and their concatenation equals what the whole-file
run gives for the same frames.

    det = StreamDetector(blob, precision="f16x2")
    s = det.open(PCM_S16, 16000, 1, threshold=0.1, break_s=0.5)
    s.push(samples)                    # any number of frames, as they arrive
    for stream, (regions, avg, bin_idx) in det.step().items(): ...
    s.close(); det.step()              # the last results

A stream opened with erase= also returns its frames as final 16-bit PCM with the detected speech zeroed (the streaming silencer):

    s = det.open(PCM_S16, 48000, 2, erase=dict(pad_s=0.05, min_len_s=0.3))
    with StreamWavWriter("feed.wav", 48000, 2) as w:
        ...; s.push(samples); det.step(); w.write(s.output())      # (first_frame, int16 [n, channels]): contiguous from step to step

encoding="source" keeps the stream's own sample encoding: output() returns the frames as bytes, the input's outside the erased intervals
(the concatenation equals native.Context.silence_pcm_source of the whole recording), and StreamWavWriter(..., fmt=) writes its header:

    s = det.open(PCM_S24, 48000, 2, erase=dict(pad_s=0.05), encoding="source")
    with StreamWavWriter("feed.wav", 48000, 2, fmt=PCM_S24) as w: ...; w.write(s.output())   # (first_frame, uint8 [n, 6])

A recording of several channels is detected on its channel mean by default; channel_mode="each" detects every channel alone (what
native.Context.add_pcm_channels is to add_pcm) and the stream's table is "speech on any channel":

    s = det.open(PCM_S16, 48000, 2, channel_mode="each")
    ...; regions, merged, bin_idx = det.step()[s]       # merged: per bin the highest of the channels' scores
    s.avg(1); s.peaks()                                 # channel 1's own series; [regions, channels] peaks of the step's regions

bands=True (or a dict of q_low, q_high, speech_channel, profile) gives every region its frequency extent, in the step that returns
the region and bytes equal to native.Context.region_bands on the whole recording (default window step only):

    s = det.open(PCM_S16, 16000, 1, bands=True)
    ...; regions, avg, bin_idx, bands = det.step()[s]   # bands: REGION_BAND_DTYPE records [regions, lanes]; also s.bands()

The f16x2 mode reports SS_ERR_RANGE for a step whose passes met a value without an f16 representation (a NaN or Inf sample of a
float stream), and commits nothing of it.  The rule of the drop-in (SpecUNet_2D.range_refused): the first such step says nothing about
the checkpoint -- the streams that had windows in it move to an fp32 context of the same weights (ss_stream_export / import) and
finish there, the others stay; a second one does, and every stream, open or new, moves to fp32 with one log line.
"""
from __future__ import annotations

import logging

import numpy as np

from . import native as _native


class Stream:
    """One recording of a StreamDetector.  Hashable: step() returns its results keyed by it."""

    def __init__(self, det: "StreamDetector", ctx, sid: int, fmt: int, sr: int, channels: int, erase=None, channel_mode: str = "mix",
                 band_params=None, encoding: str = "pcm16"):
        self.encoding = encoding                           # "pcm16": int16 output; "source": bytes in the stream's own encoding
        self.band_params = band_params                     # None: opened without bands; else dict(q_low, q_high, speech_channel, profile)
        self._det, self._ctx, self._sid = det, ctx, sid
        self.format, self.sample_rate, self.channels = fmt, sr, channels
        self.erase = erase                                 # None: opened without output
        self.channel_mode = channel_mode                   # "mix": the channel mean; "each": every channel alone, one merged table

    def push(self, pcm: np.ndarray):
        """Interleaved samples in the stream's encoding (int16 for PCM_S16, float32 for PCM_F32, raw bytes for 24-bit, ...)."""
        a = np.ascontiguousarray(pcm)
        frames = a.nbytes // (self.channels * _native._BPS[self.format])
        self._ctx.stream_push(self._sid, a, frames=frames)

    def close(self):
        self._ctx.stream_close(self._sid)

    def info(self) -> dict:
        return self._ctx.stream_info(self._sid)

    def avg(self, channel: int):
        """(avg float64[n], bin_idx int64[n]) of one channel of an each-channel stream: what the last step made final on it."""
        return self._ctx.stream_avg_channel(self._sid, channel)

    def peaks(self) -> np.ndarray:
        """float64 [regions the last step returned, channels]: each channel's highest score inside each region (each-channel streams of
        more than one channel)."""
        return self._ctx.stream_region_peaks(self._sid, self.channels)

    @property
    def lanes(self) -> int:
        return self.channels if self.channel_mode == "each" else 1

    def bands(self) -> np.ndarray:
        """REGION_BAND_DTYPE records [regions the last step returned, lanes] (lanes: 1, or the channels of an each-channel stream):
        each region's frequency extent.  Only on a stream opened with bands=."""
        return self._ctx.stream_bands(self._sid, self.lanes)[0]

    def band_profiles(self) -> np.ndarray:
        """float64 [regions the last step returned, lanes, 2, 128]: E of both spec channels (a stream opened with bands=dict(profile=True))."""
        return self._ctx.stream_bands(self._sid, self.lanes, profile=True)[1]

    def output(self):
        """The frames the last step returned: (first_frame, int16 array [n, channels]) -- final, contiguous from step to step, the
        detected speech zeroed.  Only on a stream opened with erase=.  A stream opened with encoding="source": (first_frame, uint8
        array [n, channels x bytes per sample]), the frames in the stream's own encoding."""
        if self.encoding == "source":
            return self._ctx.stream_output_bytes(self._sid, self.channels * _native._BPS[self.format])
        return self._ctx.stream_output(self._sid, self.channels)

    def output_info(self) -> dict:
        return self._ctx.stream_output_info(self._sid)

    @property
    def precision(self) -> str:
        return self._ctx.precision


class StreamDetector:
    def __init__(self, blob=None, device: int = 0, precision: str = "f16x2", chunk: int | None = None, context_factory=None,
                 step: float | None = None):
        """context_factory(precision) -> a native.Context (or a stand-in with its stream_* methods); default: one of `blob`'s weights
        on `device`.  step: seconds between window starts of the streams opened here (the reference's settings.step_size; None: the
        contexts' own, 0.6 s unless the factory set another) -- a stream keeps the step it was opened with, also across a move to fp32."""
        make = context_factory or (lambda p: _native.Context(blob, device, precision=p, chunk=chunk))
        self.window_step = None if step is None else _native.check_step(step)

        def factory(p):
            ctx = make(p)
            if self.window_step is not None:
                ctx.set_window_step(self.window_step)
            return ctx
        self._factory = factory
        self._main = self._factory(precision)
        self._fp32 = self._main if precision == "fp32" else None
        self._streams: list[Stream] = []
        self._refused_steps = 0
        self._switched = False

    @property
    def precision(self) -> str:
        return "fp32" if self._switched else self._main.precision

    def _fp32_ctx(self):
        if self._fp32 is None:
            self._fp32 = self._factory("fp32")
        return self._fp32

    def open(self, fmt: int, sr: int, channels: int = 1, threshold: float = 0.1, break_s: float = 0.5, erase=None,
             channel_mode: str = "mix", bands=False, encoding: str = "pcm16") -> Stream:
        """erase: None -- detection only; dict(pad_s=, min_len_s=) (either may be left out: 0) -- the stream also returns its frames
        as 16-bit PCM with the detected speech zeroed (Stream.output() after every step).
        channel_mode: "mix" -- detection on the channel mean; "each" -- on every channel alone: the regions and the series step()
        returns are the merged ones ("speech on any channel"), every channel is zeroed over them, Stream.avg(c) / Stream.peaks() give
        the channels' own.
        bands: False -- none; True or dict(q_low=.05, q_high=.95, speech_channel=1, profile=False) -- every region comes with its
        frequency extent (Stream.bands(), Stream.band_profiles(), the fourth entry of step()'s tuples).  Needs the 0.6 s window step.
        encoding: "pcm16" -- the output is 16-bit PCM; "source" -- it stays in the stream's own encoding (a stream with output, erase
        None meaning pad_s = min_len_s = 0; not together with bands)."""
        if encoding not in ("pcm16", "source"):
            raise ValueError(f"encoding must be 'pcm16' or 'source', not {encoding!r}")
        if encoding == "source" and bands:
            raise ValueError("band streams have no source-encoding output")
        if channel_mode not in ("mix", "each"):
            raise ValueError(f"channel_mode must be 'mix' or 'each', not {channel_mode!r}")
        bp = None
        if bands:
            bp = dict(q_low=.05, q_high=.95, speech_channel=1, profile=False)
            if bands is not True:
                unknown = set(bands) - set(bp)
                if unknown:
                    raise ValueError(f"bands: unknown keys {sorted(unknown)}")
                bp.update(bands)
            if self.window_step is not None and self.window_step != _native.check_step(0.6):
                raise ValueError(f"bands need the default 0.6 s window step, not {self.window_step}")
        ctx = self._fp32_ctx() if self._switched else self._main
        if erase is not None:
            erase = dict(pad_s=float(erase.get("pad_s", 0.0)), min_len_s=float(erase.get("min_len_s", 0.0)))
        if encoding == "source":
            erase = erase or dict(pad_s=0.0, min_len_s=0.0)
            sid = ctx.stream_open_source(fmt, sr, channels, threshold, break_s, erase, channel_mode == "each")
        elif bp is not None:
            sid = ctx.stream_open_bands(fmt, sr, channels, threshold, break_s, erase, False, channel_mode == "each", bp["q_low"], bp["q_high"],
                                        bp["speech_channel"], bp["profile"])
        elif channel_mode == "each":
            sid = ctx.stream_open_channels(fmt, sr, channels, threshold, break_s, erase)
        elif erase is None:
            sid = ctx.stream_open(fmt, sr, channels, threshold, break_s)
        else:
            sid = ctx.stream_open_output(fmt, sr, channels, threshold, break_s, erase)
        s = Stream(self, ctx, sid, fmt, sr, channels, erase, channel_mode, bp, encoding)
        self._streams.append(s)
        return s

    def free(self, s: Stream):
        s._ctx.stream_free(s._sid)
        self._streams.remove(s)

    def _move(self, s: Stream):
        image = s._ctx.stream_export(s._sid)
        ctx = self._fp32_ctx()
        sid = ctx.stream_import(image)
        s._ctx.stream_free(s._sid)
        s._ctx, s._sid = ctx, sid

    def _step_main(self):
        """Step the first context; on SS_ERR_RANGE apply the range rule and step it again without the streams that moved."""
        while True:
            try:
                self._main.stream_step()
                return
            except _native.NativeError as e:
                if e.code != _native.SS_ERR_RANGE or self._main is self._fp32 or self._switched:
                    raise
                self._refused_steps += 1
                on_main = [s for s in self._streams if s._ctx is self._main]
                if self._refused_steps >= 2:
                    logging.warning("f16x2 mode refused a second streaming step (%s): every stream moves to the fp32 mode", e)
                    self._switched = True
                    for s in on_main:
                        self._move(s)
                    return
                for s in on_main:
                    if s.info()["windows_ready"] > 0:
                        self._move(s)

    def step(self) -> dict:
        """One step over every stream -> {stream: (regions [(start, end)], avg float64[n], bin_idx int64[n])}: what became final (an
        each-channel stream: its merged regions and merged series).  A stream opened with bands= has a fourth entry: Stream.bands()."""
        if not self._switched:
            self._step_main()
        if self._fp32 is not None and self._fp32 is not self._main:
            self._fp32.stream_step()
        out = {}
        for s in self._streams:
            a, idx = s._ctx.stream_avg(s._sid)
            out[s] = (s._ctx.stream_regions(s._sid), a, idx) + ((s.bands(),) if s.band_params is not None else ())
        return out

    def close(self):
        for c in {id(c): c for c in (self._main, self._fp32) if c is not None}.values():
            if hasattr(c, "close"):
                c.close()


class StreamWavWriter:
    """A WAV file that grows with a stream's output: write() appends what a step returned, close() rewrites the 44-byte header with
    the final frame count.  fmt None: 16-bit PCM (ss_wav_header_pcm16); fmt one of the little-endian encodings 1-6: the output of a
    stream opened with encoding="source" (ss_wav_header; the AIFF encodings 7-12 have no WAV form and are refused).

        with StreamWavWriter(path, 16000, 1) as w:
            ...; det.step(); w.write(s.output())
    """

    def __init__(self, path, sr: int, channels: int, fmt: int | None = None):
        self.sample_rate, self.channels, self.frames = int(sr), int(channels), 0
        self.format = None if fmt is None else int(fmt)
        if self.format is not None and not (_native.PCM_U8 <= self.format <= _native.PCM_F64):
            raise ValueError(f"a WAV file holds the encodings 1-6, not {fmt!r}")
        self._f = open(path, "wb")
        self._f.write(self._header(0))

    def _header(self, frames: int) -> bytes:
        if self.format is None:
            return _native.wav_header_pcm16(self.sample_rate, self.channels, frames)
        return _native.wav_header(self.format, self.sample_rate, self.channels, frames)

    def write(self, output):
        """output: Stream.output()'s pair, or an int16 array [n, channels]; a pair must continue where the file ends."""
        if isinstance(output, tuple):
            first, a = output
            if first != self.frames:
                raise ValueError(f"output starts at frame {first}, the file holds {self.frames}")
        else:
            a = output
        if self.format is None:
            a = np.ascontiguousarray(a, dtype="<i2").reshape(-1, self.channels)
        else:
            a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, self.channels * _native._BPS[self.format])
        self._f.write(a.tobytes())
        self.frames += len(a)

    def close(self):
        if self._f is None:
            return
        self._f.seek(0)
        self._f.write(self._header(self.frames))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
