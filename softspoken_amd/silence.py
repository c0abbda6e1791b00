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

method="band" erases only each detection's own frequency band: `ss_box_silence_pcm` with one box per review row, its band looked up in
the region bands of the detection run (`bands=`: the `<detections stem>_bands.csv` side file or a DataFrame of its columns) by
(ID, file_name), as the Raven export looks its boxes up.  No model: the audio context does it.  A bands row with a channel number (the
per-channel side file) acts on that channel alone, one without on every channel; a review row without a bands row, or with an edge that
is not a finite number, loses its whole band (privacy first).

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


def _band_rows(bands) -> dict:
    """{(ID, file_name or None): [(channel or None, low_hz, high_hz), ...]} from the region bands of a detection run, keyed as the Raven
    export keys its boxes (review_exporter._band_boxes): an entry with a file name serves rows of that recording only, one without any
    row of its ID.  Every row stays its own entry -- the per-channel side file has one per channel."""
    import pandas as pd
    if not isinstance(bands, pd.DataFrame):
        bands = pd.read_csv(os.fspath(bands))
    missing = [c for c in ("ID", "low_hz", "high_hz") if c not in bands.columns]
    if missing:
        raise ValueError(f"SilenceJob(bands=): missing column(s): {missing}")
    names = bands["file_name"] if "file_name" in bands.columns else [None] * len(bands)
    chans = pd.to_numeric(bands["channel"], errors="coerce") if "channel" in bands.columns else [None] * len(bands)
    rows = {}
    for key, name, ch, lo, hi in zip(bands["ID"], names, chans, pd.to_numeric(bands["low_hz"], errors="coerce"),
                                     pd.to_numeric(bands["high_hz"], errors="coerce")):
        try:
            key = int(key)
        except (TypeError, ValueError):
            continue
        name = None if name is None or name != name else str(name)
        rows.setdefault((key, name), []).append((None if ch is None or ch != ch else int(ch), float(lo), float(hi)))
    return rows


def _boxes(band_rows: dict, rows, file_name) -> list:
    """One file's review rows -> (start, end, low_hz, high_hz, channel) boxes: a row's bands entries by (ID, file_name), then by ID
    alone; none, or an edge that is no finite number: the whole band (NaN edges), on the entry's channel."""
    import pandas as pd
    ids = pd.to_numeric(rows["ID"], errors="coerce") if "ID" in rows.columns else [float("nan")] * len(rows)
    nan, boxes = float("nan"), []
    for i, s, e in zip(ids, rows["start_time"], rows["end_time"]):
        entries = (band_rows.get((int(i), str(file_name))) or band_rows.get((int(i), None))) if i == i else None
        for ch, lo, hi in entries or [(None, nan, nan)]:
            if lo != lo or hi != hi or abs(lo) == float("inf") or abs(hi) == float("inf"):
                lo = hi = nan
            boxes.append((float(s), float(e), lo, hi, ch))
    return boxes


class SilenceJob:
    """Signals of the reference's worker (silencer_ui.py:908-916) as plain callbacks; `stop()` as there."""

    METHODS = ("zero", "separate", "band")
    CHANNEL_MODES = ("mix", "each")
    ENCODINGS = ("pcm16", "source")

    def __init__(self, review_df, output_dir, ctx=None, file_started=None, file_complete=None,
                 overall_progress=None, finished=None, method="zero", model=None, fade_s=0.01, min_gain=0.0,
                 above_fmax="mute", speech_channel=1, channel_mode=None, encoding=None, bands=None, edge_hz=100.0):
        """method "zero": the reference's silencer (ctx: any context, default the shared audio context).  method "separate":
        ss_separate_pcm through `model` (a SpecUNet_2D, e.g. NNDetector(...).model) and its with_range_fallback, so that an input
        the f16x2 mode cannot represent runs in fp32; fade_s, min_gain, above_fmax ("mute" / "keep") and speech_channel are its
        parameters (include/softspoken.h).  The model's device context must not be in use by another thread meanwhile.
        channel_mode "mix" / "each" (None: voice_activity.channel_mode(), the detector's setting): with method "separate", "each"
        sends a file of more than one channel through ss_separate_pcm_channels; method "zero" has no use for it.
        encoding "pcm16" / "source" (None: voice_activity.silence_encoding(), read when the job runs): "source" keeps the file's own
        image and sample encoding (the *_source calls); "pcm16" writes what was always written.
        method "band": ss_box_silence_pcm on ctx (any context, default the shared audio context); bands: the region bands of the
        detection run, a DataFrame (ID, low_hz, high_hz and, as a rule, file_name and channel) or the path of a _bands.csv; fade_s and
        min_gain as for "separate", edge_hz the roll-off outside a box's band (include/softspoken.h "band silencer")."""
        if method not in self.METHODS:
            raise ValueError(f"method must be one of {self.METHODS}, not {method!r}")
        if channel_mode is not None and channel_mode not in self.CHANNEL_MODES:
            raise ValueError(f"channel_mode must be None or one of {self.CHANNEL_MODES}, not {channel_mode!r}")
        if encoding is not None and encoding not in self.ENCODINGS:
            raise ValueError(f"encoding must be None or one of {self.ENCODINGS}, not {encoding!r}")
        if method == "separate" and model is None:
            raise ValueError('method="separate" needs the model (a SpecUNet_2D) whose spec head gives the gains')
        if method == "band" and bands is None:
            raise ValueError('method="band" needs bands= (the region bands of the detection run: a DataFrame or the path of a _bands.csv)')
        self.band_rows = _band_rows(bands) if method == "band" else None
        self.box_params = dict(fade_s=fade_s, min_gain=min_gain, edge_hz=edge_hz)
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
        ctx = (self.ctx or voice_activity.audio_context()) if self.method in ("zero", "band") else None
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
                elif self.method == "band":
                    boxes = _boxes(self.band_rows, rows, fname)
                    with voice_activity._audio_lock:
                        out = ctx.box_silence_pcm(pcm, info.format, info.sample_rate, info.channels, boxes, frames=info.frames,
                                                  encoding="source" if source else "pcm16", **self.box_params)
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
                  speech_channel=1, channel_mode=None, encoding=None, bands=None, edge_hz=100.0):
    """-> list of written paths."""
    return SilenceJob(review_df, output_dir, ctx=ctx, method=method, model=model, fade_s=fade_s, min_gain=min_gain,
                      above_fmax=above_fmax, speech_channel=speech_channel, channel_mode=channel_mode, encoding=encoding, bands=bands,
                      edge_hz=edge_hz).run()
