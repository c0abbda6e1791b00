"""Headless silencer: what the reference's SilenceWorker.run does
(root/code/frontend/silencer_ui.py:918-1015) without Qt -- every recording that has review rows with
erase == 1 is rewritten as `<name>_silenced.wav` with those intervals zeroed.

The samples go through `ss_silence_pcm` (decode, zero, 16-bit encode in one device pass); this module
only groups the rows, maps the file and writes header + samples.

method="separate" keeps the environmental sound of the erased intervals: `ss_separate_pcm` removes only the speech part of
their spectrum, with the gains of the model's spec head (SpecUNet_2D's spec_output_conv, "env / speech separation"; the
reference computes it and drops it).  Everything outside the intervals is what method="zero" writes.

channel_mode "each" (settings.hip_channel_mode / SOFTSPOKEN_CHANNELS when not given) makes method="separate" follow per-channel
detection: a recording of more than one channel goes through `ss_separate_pcm_channels`, every channel's gains from its own network
passes instead of the mono mix's.

encoding "source" (settings.hip_silence_encoding / SOFTSPOKEN_SILENCE_ENCODING when not given; default "pcm16", the reference's 16-bit
WAV) writes the source file's own image with only its sample bytes replaced by the `*_source` calls' output: outside the erased
intervals the copy equals the source byte for byte -- header, metadata chunks (bext, iXML, LIST, GUANO), pad bytes and container (WAV,
AIFF, AIFF-C) included --, inside them it holds the same audio in the same sample encoding.  It is written to
`<name>_silenced<the source's extension>`.
"""
from __future__ import annotations

import os

from root.code.backend import voice_activity
from . import native


class SilenceJob:
    """Signals of the reference's worker (silencer_ui.py:908-916) as plain callbacks; `stop()` as there."""

    METHODS = ("zero", "separate")
    CHANNEL_MODES = ("mix", "each")
    ENCODINGS = ("pcm16", "source")

    def __init__(self, review_df, output_dir, ctx=None, file_started=None, file_complete=None,
                 overall_progress=None, finished=None, method="zero", model=None, fade_s=0.01, min_gain=0.0,
                 above_fmax="mute", speech_channel=1, channel_mode=None, encoding=None):
        """method "zero": the reference's silencer (ctx: any context, default the shared audio context).  method "separate":
        ss_separate_pcm through `model` (a SpecUNet_2D, e.g. NNDetector(...).model) and its with_range_fallback, so that an input
        the f16x2 mode cannot represent runs in fp32; fade_s, min_gain, above_fmax ("mute" / "keep") and speech_channel are its
        parameters (include/softspoken.h).  The model's device context must not be in use by another thread meanwhile.
        channel_mode "mix" / "each" (None: voice_activity.channel_mode(), the detector's setting): with method "separate", "each"
        sends a file of more than one channel through ss_separate_pcm_channels; method "zero" has no use for it.
        encoding "pcm16" / "source" (None: voice_activity.silence_encoding(), read when the job runs): "source" keeps the file's own
        image and sample encoding (the *_source calls); "pcm16" writes what was always written."""
        if method not in self.METHODS:
            raise ValueError(f"method must be one of {self.METHODS}, not {method!r}")
        if channel_mode is not None and channel_mode not in self.CHANNEL_MODES:
            raise ValueError(f"channel_mode must be None or one of {self.CHANNEL_MODES}, not {channel_mode!r}")
        if encoding is not None and encoding not in self.ENCODINGS:
            raise ValueError(f"encoding must be None or one of {self.ENCODINGS}, not {encoding!r}")
        if method == "separate" and model is None:
            raise ValueError('method="separate" needs the model (a SpecUNet_2D) whose spec head gives the gains')
        self.review_df, self.output_dir = review_df, output_dir
        self.ctx = ctx
        self.method, self.model = method, model
        self.channel_mode = channel_mode
        self.encoding = encoding
        self.sep_params = dict(fade_s=fade_s, min_gain=min_gain, above_fmax=above_fmax, speech_channel=speech_channel)
        self.file_started, self.file_complete = file_started, file_complete
        self.overall_progress, self.finished = overall_progress, finished
        self.stop_requested = False
        self.errors: dict[str, str] = {}
        self.outputs: list[str] = []

    def stop(self):
        self.stop_requested = True

    def _emit(self, cb, *a):
        if cb is not None:
            cb(*a)

    def run(self):
        erase = self.review_df[self.review_df['erase'] == 1]
        if erase.empty:
            self._emit(self.finished)
            return self.outputs
        ctx = (self.ctx or voice_activity.audio_context()) if self.method == "zero" else None
        each = self.method == "separate" and (self.channel_mode or voice_activity.channel_mode()) == "each"
        source = (self.encoding or voice_activity.silence_encoding()) == "source"
        groups = erase.groupby(['file_path', 'file_name'])
        total, done = len(groups), 0
        for (fpath, fname), rows in groups:
            if self.stop_requested:
                break
            src = os.path.join(fpath, fname)
            self._emit(self.file_started, src)
            stem, ext = os.path.splitext(fname)
            out_path = os.path.join(self.output_dir, f"{stem}_silenced{ext if source else '.wav'}")
            try:
                buf = voice_activity._map_file(src)
                info = native.wav_parse(buf)
                pcm = buf[info.data_offset: info.data_offset + info.data_bytes]
                regions = [(float(s), float(e)) for s, e in zip(rows['start_time'], rows['end_time'])]
                sfx = "_source" if source else ""
                if self.method == "zero":
                    with voice_activity._audio_lock:
                        out = getattr(ctx, "silence_pcm" + sfx)(pcm, info.format, info.sample_rate, info.channels, info.frames, regions)
                elif each and info.channels > 1:
                    out = self.model.with_range_fallback(
                        lambda c: getattr(c, "separate_pcm_channels" + sfx)(pcm, info.format, info.sample_rate, info.channels, info.frames, regions,
                                                          **self.sep_params), key=("separate", src))
                else:
                    out = self.model.with_range_fallback(
                        lambda c: getattr(c, "separate_pcm" + sfx)(pcm, info.format, info.sample_rate, info.channels, info.frames, regions,
                                                                   **self.sep_params), key=("separate", src))
                with open(out_path, "wb") as fh:
                    if source:      # the file's own image, the sample bytes replaced: no header writer
                        fh.write(bytes(buf[:info.data_offset]))
                        fh.write(out.tobytes())
                        fh.write(bytes(buf[info.data_offset + out.nbytes:]))
                    else:
                        fh.write(native.wav_header_pcm16(info.sample_rate, info.channels, info.frames))
                        fh.write(out.tobytes())
                self.outputs.append(out_path)
                self._emit(self.file_complete, out_path)
            except Exception as exc:            # the reference logs and moves on to the next file (:963-969, :996-997)
                self.errors[src] = str(exc)
                print(f"Error silencing {src}: {exc}")
            done += 1
            self._emit(self.overall_progress, int(done / total * 100))
        self._emit(self.finished)
        return self.outputs


def silence_files(review_df, output_dir, ctx=None, method="zero", model=None, fade_s=0.01, min_gain=0.0, above_fmax="mute",
                  speech_channel=1, channel_mode=None, encoding=None):
    """-> list of written paths."""
    return SilenceJob(review_df, output_dir, ctx=ctx, method=method, model=model, fade_s=fade_s, min_gain=min_gain,
                      above_fmax=above_fmax, speech_channel=speech_channel, channel_mode=channel_mode, encoding=encoding).run()
