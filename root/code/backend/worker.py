"""Background job driver of the voice detector (reference root/code/backend/worker.py:4-139).

Same class names, constructor, `signals`, `stop()` and `run()` contract as the reference, so
silencer_ui.py:234-243 can hand it to a QThreadPool unchanged.  PySide6 is optional: with it the
worker is a QRunnable with real Qt signals; without it (headless jobs, tests, the bench) `signals`
are small objects with the same connect()/emit() surface and run() is called directly.

Per file the behaviour seen by the caller is the reference's: fileStarted -> fileProgressChanged
after every batch of windows -> rows appended to detection_project.df (ID continues from the
current maximum, erase 0, empty comment/datetime) -> save_detections() -> fileDone ->
overallProgressChanged; finished at the end; stop() is honoured between files and between
batches and a file interrupted half-way leaves no rows (worker.py:72,86-87).
Differences: the file is decoded, mixed down, resampled, padded and kept in HBM by the library
(one upload per file, not per batch), averaging runs on the GPU, and a file that cannot be decoded
is reported through signals.message and skipped (the reference crashes on len(None), worker.py:60).
settings.step_size is applied to whichever device context a file runs on (SpecUNet_2D.hip_context / fp32_context read it on every
use), so the windows run and the totals of fileProgressChanged are the device's plan at that step; a value the library does not take
(outside 0.1 .. 3.0 s) raises from plan_detection_job, and a job started without it reports the same ValueError per file.
"""
from __future__ import annotations

import csv
import ctypes
import logging
from os.path import basename, dirname, exists, splitext

import numpy as np
import pandas as pd

from root.code.backend import settings

_SS_ERR_NOMEM = 6                                # include/softspoken.h (softspoken_amd.native.SS_ERR_NOMEM)

# NOTE: PySide6 is not in this image (nor on the GPU box): the Qt branch below (QRunnable + Signal classes, reference
# worker.py:4-32) has never executed here; every test drives the headless classes, which have the same connect()/emit() surface.
try:                                            # GUI build
    from PySide6.QtCore import QObject, QRunnable, Signal
    _HAVE_QT = True
except Exception:                               # headless
    _HAVE_QT = False


if _HAVE_QT:
    class WorkerSignals(QObject):
        fileProgressChanged = Signal(float)
        overallProgressChanged = Signal(float)
        fileStarted = Signal(str)
        fileDone = Signal(str)
        finished = Signal()
        message = Signal(str)

    _Base = QRunnable
else:
    class _PlainSignal:
        def __init__(self):
            self._slots = []

        def connect(self, fn):
            self._slots.append(fn)

        def emit(self, *a):
            for fn in list(self._slots):
                fn(*a)

    class WorkerSignals:
        def __init__(self):
            for name in ("fileProgressChanged", "overallProgressChanged", "fileStarted", "fileDone", "finished", "message"):
                setattr(self, name, _PlainSignal())

    class _Base:
        def __init__(self):
            pass


class ProcessWorker(_Base):
    def __init__(self, detector, detection_project, planned_work, parent=None):
        super().__init__()
        self.signals = WorkerSignals()
        self.detector = detector
        self.detection_project = detection_project
        self.planned_work = planned_work
        self.stop_requested = False
        self._stop_word = ctypes.c_int(0)       # polled by the library between chunks
        self._side_files_checked = set()        # side files (_channels.csv, _bands.csv) already cleared of rows beyond the detections CSV

    def stop(self):
        self.stop_requested = True
        self._stop_word.value = 1

    def _next_id(self):
        df = self.detection_project.df
        if not df.empty and 'ID' in df.columns:
            top = pd.to_numeric(df['ID'], errors='coerce').max()
            if not np.isnan(top):
                return int(top) + 1
        return 1

    def _append_rows(self, file, regions):
        """worker.py:103-125: one row per region, IDs continuing from the current maximum.  The first row is appended with the
        reference's statement -- on an empty frame it decides what the columns' dtypes become --, the others as one block of those
        dtypes (the statement costs ~0.8 ms per row: 50 ms for a 10-minute recording's 64 rows, twice its time on the GPU)."""
        if not regions:
            return
        df = self.detection_project.df
        file_path, file_name = dirname(file), basename(file)
        next_id = self._next_id()
        s0, e0 = regions[0]
        df.loc[len(df)] = {'ID': next_id, 'file_path': file_path, 'file_name': file_name, 'start_time': s0, 'end_time': e0,
                           'erase': 0, 'user_comment': '', 'review_datetime': ''}
        if len(regions) > 1:
            n = len(regions) - 1
            block = pd.DataFrame({'ID': np.arange(next_id + 1, next_id + 1 + n, dtype=np.int64), 'file_path': file_path, 'file_name': file_name,
                                  'start_time': pd.Series([r[0] for r in regions[1:]], dtype=object),
                                  'end_time': pd.Series([r[1] for r in regions[1:]], dtype=object),
                                  'erase': 0, 'user_comment': '', 'review_datetime': ''}, columns=list(df.columns))
            block.index = range(len(df), len(df) + n)
            self.detection_project.df = pd.concat([df, block.astype(df.dtypes.to_dict())])

    def _side_file(self, csv_path, suffix, first_id):
        """The path of the side file <detections stem><suffix>.  The first time a job asks for it, rows left by a detections CSV that has
        since been deleted or recreated are dropped: their IDs (first_id and up) are about to be handed out again."""
        side = splitext(csv_path)[0] + suffix
        if suffix not in self._side_files_checked and exists(side):
            with open(side, newline="") as fh:
                rows = list(csv.reader(fh))
            kept = [r for r in rows[1:] if r and r[0].isdigit() and int(r[0]) < first_id]
            if len(kept) != len(rows) - 1:
                with open(side, "w", newline="") as fh:
                    csv.writer(fh, lineterminator="\n").writerows(rows[:1] + kept)
        self._side_files_checked.add(suffix)
        return side

    def _append_channel_rows(self, file, first_id, n_regions):
        """settings.hip_channel_mode == 'each': which channel heard each of the file's regions, appended to <detections stem>_channels.csv
        beside the detections CSV -- ID (the region's row in the detections CSV), file_name, n_channels, heard (the channels whose peak is
        above the threshold, like 0;1) and peaks (every channel's highest averaged score inside the region).  Nothing for a detector
        without channel_detail or a project without a detections file (and run() does not call it in 'mix' mode)."""
        detail = getattr(self.detector, "channel_detail", None)
        project = getattr(getattr(self.detection_project, "settings", None), "current_project", None)
        csv_path = project.get("detections_file") if isinstance(project, dict) else None
        if not detail or file not in detail or not csv_path:
            return
        n_ch, peaks = detail[file]
        if len(peaks) != n_regions:
            logging.warning("%s: %d regions but channel detail for %d -- no rows in the channels file", file, n_regions, len(peaks))
            return
        side = self._side_file(csv_path, "_channels.csv", first_id)
        new = not exists(side)
        with open(side, "a", newline="") as fh:
            out = csv.writer(fh, lineterminator="\n")
            if new:
                out.writerow(["ID", "file_name", "n_channels", "heard", "peaks"])
            for k, row in enumerate(peaks):
                heard = ";".join(str(c) for c, v in enumerate(row) if v > settings.threshold)
                out.writerow([first_id + k, basename(file), n_ch, heard, ";".join("%.6f" % v for v in row)])

    def _append_band_rows(self, file, first_id, n_regions):
        """settings.hip_region_bands == '1': the frequency extent of each of the file's regions, appended to <detections stem>_bands.csv
        beside the detections CSV -- ID (the region's row in the detections CSV), file_name, channel ('each' mode: one row per channel;
        'mix': one row, the field empty), low_hz / high_hz / peak_hz (%.1f), speech_share, n_bins (the averaged bins used).  A region
        without an estimate has the five fields before n_bins empty.  Nothing for a detector without band_detail, a file the bands
        were refused for, or a project without a detections file.  Stale rows: _side_file's rule, as the channels file."""
        detail = getattr(self.detector, "band_detail", None)
        project = getattr(getattr(self.detection_project, "settings", None), "current_project", None)
        csv_path = project.get("detections_file") if isinstance(project, dict) else None
        if not detail or file not in detail or not csv_path:
            return
        n_ch, bands = detail[file]
        if len(bands) != n_regions:
            logging.warning("%s: %d regions but bands for %d -- no rows in the bands file", file, n_regions, len(bands))
            return
        side = self._side_file(csv_path, "_bands.csv", first_id)
        new = not exists(side)
        with open(side, "a", newline="") as fh:
            out = csv.writer(fh, lineterminator="\n")
            if new:
                out.writerow(["ID", "file_name", "channel", "low_hz", "high_hz", "peak_hz", "speech_share", "n_bins"])
            for k, row in enumerate(bands):
                for c, b in enumerate(row):
                    if int(b["band_low"]) < 0:
                        est = ["", "", "", ""]
                    else:
                        est = ["%.1f" % b["low_hz"], "%.1f" % b["high_hz"], "%.1f" % b["peak_hz"], "%.6f" % b["speech_share"]]
                    out.writerow([first_id + k, basename(file), c if n_ch >= 1 else ""] + est + [int(b["n_bins"])])

    def run(self):
        """The reference's signal sequence per file (worker.py:49-139), with the device ahead of the host: files alternate between
        two device contexts (settings.hip_file_contexts), so while file k's results are read, its rows appended and the CSV written,
        file k + 1 is already running on the other context's stream -- queued before file k's last launch ended, so the device never
        waits for the host between files --, file k + 2 starts as soon as k's context is free, and the samples of the files behind
        them are crossing PCIe."""
        det = self.detector
        files = list(self.planned_work.keys())
        total_files = len(files)
        files_done = 0
        # (a second context costs its creation and a second workspace: not for a job of one or two files)
        n_ctx = 2 if int(getattr(settings, "hip_file_contexts", 2)) >= 2 and total_files >= 3 else 1
        tokens, handles = {}, {}
        LATER = object()                 # a file whose turn on the one remaining context has not come yet

        def begin(i):                    # -> token, or the exception that file raised (reported when its turn comes)
            nonlocal n_ctx
            which = i % n_ctx
            try:
                return det.file_begin(files[i], handles.pop(i, None), which=which)
            except Exception as e:
                if which == 1 and getattr(e, "code", None) == _SS_ERR_NOMEM:
                    # the second context's workspace does not fit (a shared card, a large SOFTSPOKEN_CHUNK): its memory goes back and
                    # this file and every later one run on context 0, one after the other, as in round 2 -- no file is lost
                    logging.warning("second file context: %s -- continuing with one context", e)
                    det.model.drop_second_context()
                    n_ctx = 1
                    handles.clear()
                    return LATER
                return e

        def prefetch(i):
            if i < total_files and n_ctx > 1:
                try:
                    handles[i] = det.file_prefetch(files[i], which=i % n_ctx)
                except Exception:
                    pass                 # (file_begin walks the header again and raises in turn)

        for i in range(min(n_ctx, total_files)):
            if not self.stop_requested:
                tokens[i] = begin(i)
        for i in range(n_ctx, 2 * n_ctx):
            if not self.stop_requested:
                prefetch(i)
        for i, file in enumerate(files):
            if self.stop_requested:
                break
            self.signals.fileStarted.emit(file)
            regions, err = None, None
            token = tokens.pop(i, None)
            if token is LATER:                                  # (context 0 is free now: the file before this one has ended)
                token = begin(i)
            if token is None:                                   # (stop was requested before this file could start)
                break
            if isinstance(token, Exception):
                err = token
            else:
                progress = lambda done, total: self.signals.fileProgressChanged.emit((done / max(total, 1)) * 100.0)
                try:
                    det.file_poll(token, progress)
                    regions = det.file_end(token, progress)
                except Exception as e:
                    err = e
                    det.file_abort(token)                       # the context must not stay "run in flight" for the next file
            if self.stop_requested and err is None:             # interrupted: discard the partial file (worker.py:86-87)
                break
            nxt = i + n_ctx                                     # this file's context takes its next file before the rows are filed
            if nxt < total_files and not self.stop_requested and (nxt not in tokens or tokens[nxt] is LATER):
                tokens[nxt] = begin(nxt)
                if tokens[nxt] is not LATER and not isinstance(tokens[nxt], Exception):
                    prefetch(i + 2 * n_ctx)
            if err is not None:                                  # undecodable / failed file: reported and skipped; it still counts towards
                self.signals.message.emit(f"{file}: {err}")      # the overall progress, which would otherwise never reach 100 %
                files_done += 1
                self.signals.overallProgressChanged.emit((files_done / total_files) * 100.0)
                continue
            each = getattr(settings, "hip_channel_mode", "mix") == "each"
            bands = getattr(settings, "hip_region_bands", "0") == "1"
            first_id = self._next_id() if regions and (each or bands) else None
            self._append_rows(file, regions)
            self.detection_project.save_detections()
            if first_id is not None and each:
                self._append_channel_rows(file, first_id, len(regions))
            if first_id is not None and bands:
                self._append_band_rows(file, first_id, len(regions))
            self.signals.fileDone.emit(file)
            files_done += 1
            self.signals.overallProgressChanged.emit((files_done / total_files) * 100.0)
        for token in tokens.values():                            # files still in flight when the loop was left
            if token is not None and token is not LATER and not isinstance(token, Exception):
                det.file_abort(token)
        self.signals.finished.emit()
