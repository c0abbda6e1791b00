"""The drop-in's region bands without a GPU: settings.hip_region_bands, ProcessWorker.run's side file (<detections stem>_bands.csv)
against a scripted detector in the manner of tests/test_channels_logic.py, NNDetector's call on a scripted context, and the Raven
exporter's per-row boxes."""
import importlib
import os

import numpy as np
import pandas as pd
import pytest

from root.code.backend import settings
from root.code.backend.worker import ProcessWorker
from root.code.frontend import review_exporter as rx
from softspoken_amd import native
from softspoken_amd.detections import DetectionProject, ProjectSettings

NAN = float("nan")


def _band(low, high, peak, share, n_bins, idx=(10, 90, 40)):
    """One ss_region_band record; low None: no estimate."""
    b = np.zeros((), dtype=native.REGION_BAND_DTYPE)
    if low is None:
        b["low_hz"] = b["high_hz"] = b["peak_hz"] = b["speech_share"] = NAN
        b["band_low"] = b["band_high"] = b["band_peak"] = -1
    else:
        b["low_hz"], b["high_hz"], b["peak_hz"], b["speech_share"] = low, high, peak, share
        b["band_low"], b["band_high"], b["band_peak"] = idx
    b["n_bins"] = n_bins
    return b


class _Model:
    def drop_second_context(self):
        pass


class _Det:
    """file "fK": K + 1 regions; f0 mono, the others stereo ('each') or mixed down ('mix'); band_detail filled at file_end, as
    NNDetector does.  Region r of file k: low 100 k + 10 r + 0.04, ...; the last region of f2 has no estimate ('each': on channel 1
    only, where region 0 has none either)."""

    def __init__(self, each=False, with_detail=True, refuse=()):
        self.model = _Model()
        self.each, self.refuse = each, refuse
        if with_detail:
            self.band_detail = {}
        if each:
            self.channel_detail = {}

    def file_prefetch(self, file, which=0):
        return ("handle", file, which)

    def file_begin(self, file, handle=None, break_duration=0.5, which=0):
        return {"file": file}

    def file_poll(self, token, progress=None, block=True):
        progress(70, 70)

    def file_end(self, token, progress=None):
        file = token["file"]
        k = int(os.path.basename(file)[1:].split(".")[0])
        regions = [(10.0 * k + r, 10.0 * k + r + 0.5) for r in range(k + 1)]
        n_ch = (1 if k == 0 else 2) if self.each else 0
        if self.each:
            self.channel_detail[file] = (n_ch, [[0.5] * n_ch for _ in regions])
        if hasattr(self, "band_detail") and k not in self.refuse:
            rows = np.zeros((len(regions), max(n_ch, 1)), dtype=native.REGION_BAND_DTYPE)
            for r in range(len(regions)):
                for c in range(max(n_ch, 1)):
                    none = (k == 2 and r == 2 and c == max(n_ch, 1) - 1) or (k == 2 and r == 0 and c == 1)
                    rows[r, c] = _band(None, 0, 0, 0, 0 if r == 2 else 43) if none else \
                        _band(100.0 * k + 10 * r + 0.04 + 1000 * c, 3000.0 + r + 0.06 - 500 * c, 800.0 + 0.25 * r, 0.75, 43 + r)
            self.band_detail[file] = (n_ch, rows)
        return regions

    def file_abort(self, token):
        pass


def _run(det, files, csv_path):
    proj = DetectionProject(ProjectSettings(csv_path))
    w = ProcessWorker(det, proj, {f: None for f in files})
    done = []
    w.signals.fileDone.connect(done.append)
    w.run()
    assert done == files
    return proj


def test_setting_reads_the_environment_and_defaults_to_off(monkeypatch):
    try:
        monkeypatch.delenv("SOFTSPOKEN_BANDS", raising=False)
        assert importlib.reload(settings).hip_region_bands == "0"
        monkeypatch.setenv("SOFTSPOKEN_BANDS", "1")
        assert importlib.reload(settings).hip_region_bands == "1"
    finally:
        monkeypatch.undo()
        importlib.reload(settings)


def test_unknown_value_is_refused_where_it_is_read(monkeypatch):
    from root.code.backend import voice_activity
    monkeypatch.setattr(settings, "hip_region_bands", "yes")
    with pytest.raises(ValueError, match="'0' or '1'"):
        voice_activity.region_bands_enabled()
    monkeypatch.setattr(settings, "hip_region_bands", "1")
    assert voice_activity.region_bands_enabled() is True
    monkeypatch.setattr(settings, "hip_region_bands", "0")
    assert voice_activity.region_bands_enabled() is False


def test_mix_mode_side_file_text_and_ids(monkeypatch, tmp_path):
    monkeypatch.setattr(settings, "hip_region_bands", "1")
    monkeypatch.setattr(settings, "hip_channel_mode", "mix")
    csv_path = str(tmp_path / "detections.csv")
    files = [str(tmp_path / f"f{k}.wav") for k in (0, 1, 2, 3)]
    proj = _run(_Det(), files[:3], csv_path)
    side = str(tmp_path / "detections_bands.csv")
    assert list(proj.df["ID"]) == [1, 2, 3, 4, 5, 6]
    want = ["ID,file_name,channel,low_hz,high_hz,peak_hz,speech_share,n_bins",
            "1,f0.wav,,0.0,3000.1,800.0,0.750000,43",
            "2,f1.wav,,100.0,3000.1,800.0,0.750000,43",
            "3,f1.wav,,110.0,3001.1,800.2,0.750000,44",
            "4,f2.wav,,200.0,3000.1,800.0,0.750000,43",
            "5,f2.wav,,210.0,3001.1,800.2,0.750000,44",
            "6,f2.wav,,,,,,0"]                                         # no estimate: empty fields, the bins used stay
    assert open(side).read().splitlines() == want
    assert not os.path.exists(tmp_path / "detections_channels.csv")
    # a second job on the project: IDs go on, the side file is appended to (one header)
    proj2 = _run(_Det(), files[3:], csv_path)
    assert list(proj2.df["ID"]) == list(range(1, 11))
    lines = open(side).read().splitlines()
    assert lines[:7] == want and [ln.split(",")[0] for ln in lines[7:]] == ["7", "8", "9", "10"]
    main = pd.read_csv(csv_path)
    for ln in lines[1:]:
        i, name = ln.split(",")[:2]
        assert main.loc[main["ID"] == int(i), "file_name"].item() == name
    # pandas reads the empty fields as NaN: what ReviewTable.save_review hands to the exporter
    b = pd.read_csv(side)
    assert np.isnan(b.loc[b["ID"] == 6, "low_hz"].item()) and b.loc[b["ID"] == 5, "high_hz"].item() == 3001.1


def test_each_mode_one_row_per_channel(monkeypatch, tmp_path):
    monkeypatch.setattr(settings, "hip_region_bands", "1")
    monkeypatch.setattr(settings, "hip_channel_mode", "each")
    files = [str(tmp_path / f"f{k}.wav") for k in (0, 2)]
    _run(_Det(each=True), files, str(tmp_path / "d.csv"))
    want = ["ID,file_name,channel,low_hz,high_hz,peak_hz,speech_share,n_bins",
            "1,f0.wav,0,0.0,3000.1,800.0,0.750000,43",
            "2,f2.wav,0,200.0,3000.1,800.0,0.750000,43",
            "2,f2.wav,1,,,,,43",
            "3,f2.wav,0,210.0,3001.1,800.2,0.750000,44",
            "3,f2.wav,1,1210.0,2501.1,800.2,0.750000,44",
            "4,f2.wav,0,220.0,3002.1,800.5,0.750000,45",
            "4,f2.wav,1,,,,,0"]
    assert open(tmp_path / "d_bands.csv").read().splitlines() == want
    assert os.path.exists(tmp_path / "d_channels.csv")                  # the channels file is written as before


def test_off_writes_no_side_file_and_the_same_csv(monkeypatch, tmp_path):
    files = [str(tmp_path / f"f{k}.wav") for k in (0, 1, 2)]
    monkeypatch.setattr(settings, "hip_region_bands", "1")
    _run(_Det(), files, str(tmp_path / "on.csv"))
    monkeypatch.setattr(settings, "hip_region_bands", "0")
    _run(_Det(), files, str(tmp_path / "off.csv"))
    assert not os.path.exists(tmp_path / "off_bands.csv") and os.path.exists(tmp_path / "on_bands.csv")
    assert open(tmp_path / "off.csv").read() == open(tmp_path / "on.csv").read()


def test_detector_without_band_detail_or_a_refused_file_still_runs(monkeypatch, tmp_path):
    monkeypatch.setattr(settings, "hip_region_bands", "1")
    files = [str(tmp_path / f"f{k}.wav") for k in (0, 1, 2)]
    proj = _run(_Det(with_detail=False), files[:2], str(tmp_path / "d.csv"))
    assert len(proj.df) == 3 and not os.path.exists(tmp_path / "d_bands.csv")
    proj = _run(_Det(refuse=(1,)), files, str(tmp_path / "e.csv"))     # f1's bands were refused: its regions stand, no band rows
    assert list(proj.df["ID"]) == [1, 2, 3, 4, 5, 6]
    assert [ln.split(",")[0] for ln in open(tmp_path / "e_bands.csv").read().splitlines()[1:]] == ["1", "4", "5", "6"]


def test_rows_of_a_recreated_detections_csv_do_not_stay_in_the_side_file(monkeypatch, tmp_path):
    monkeypatch.setattr(settings, "hip_region_bands", "1")
    csv_path = str(tmp_path / "detections.csv")
    side = str(tmp_path / "detections_bands.csv")
    files = [str(tmp_path / f"f{k}.wav") for k in (0, 1, 2)]
    _run(_Det(), files, csv_path)
    first = open(side).read()
    os.remove(csv_path)                                                # the project starts over: IDs begin at 1 again
    _run(_Det(), files[1:], csv_path)
    lines = open(side).read().splitlines()
    assert [ln.split(",")[:2] for ln in lines[1:]] == [["1", "f1.wav"], ["2", "f1.wav"], ["3", "f2.wav"], ["4", "f2.wav"], ["5", "f2.wav"]]
    assert lines[0] == first.splitlines()[0]


# ---- NNDetector._file_regions on a scripted context ----------------------------------------------------------------------------
class _Ctx:
    """The library's state rule included: region_bands hands the run's device buffers to its passes, after which the peaks (as the
    averages and window logits) answer SS_ERR_STATE until the next run; the region tables stay."""

    def __init__(self, refuse=False):
        self.calls, self.refuse, self.buffers = [], refuse, True

    def reset(self):
        pass

    def run(self, *a):
        self.buffers = True
        return True

    def regions(self, fid):
        return [(0.5 + fid, 1.25 + fid), (2.0 + fid, 2.5 + fid)]

    def regions_union(self, fid, n):
        return self.regions(fid) + [(3.0 + fid, 3.5 + fid)]

    def region_peaks(self, fid, n):
        if not self.buffers:
            raise native.NativeError(native.SS_ERR_STATE, "ss_get_region_peaks: no completed ss_run (or a newer job has taken its device buffers)")
        return np.full((3, n), 0.5)

    def region_bands(self, fid, regions, n_channels=1):
        self.calls.append((fid, list(regions), n_channels))
        self.buffers = False
        if self.refuse:
            raise native.NativeError(native.SS_ERR_RANGE, "f16x2: left the range")
        out = np.zeros((len(regions), n_channels), dtype=native.REGION_BAND_DTYPE)
        out["low_hz"] = 100.0
        return out[:, 0] if n_channels == 1 else out


def _detector():
    from root.code.frontend.NNDetector import NNDetector
    d = NNDetector.__new__(NNDetector)
    d.channel_detail, d.band_detail = {}, {}
    return d


def test_file_regions_calls_region_bands_only_when_on(monkeypatch, caplog):
    d, ctx = _detector(), _Ctx()
    monkeypatch.setattr(settings, "hip_region_bands", "0")
    want = [(4.5, 5.25), (6.0, 6.5)]
    assert d._file_regions(ctx, 4, 0, "a.wav") == want and not ctx.calls and not d.band_detail
    monkeypatch.setattr(settings, "hip_region_bands", "1")
    assert d._file_regions(ctx, 4, 0, "a.wav") == want
    assert ctx.calls == [(4, want, 1)]
    n_ch, bands = d.band_detail["a.wav"]
    assert n_ch == 0 and bands.shape == (2, 1) and bands.dtype == native.REGION_BAND_DTYPE
    ctx.run()                                                            # the next file's run on this context
    assert len(d._file_regions(ctx, 7, 2, "b.wav")) == 3 and ctx.calls[-1][0] == 7 and ctx.calls[-1][2] == 2
    assert d.band_detail["b.wav"][0] == 2 and d.band_detail["b.wav"][1].shape == (3, 2)
    # SS_ERR_RANGE: one warning, the regions stand, the file's earlier bands are gone
    bad = _Ctx(refuse=True)
    with caplog.at_level("WARNING"):
        assert d._file_regions(bad, 4, 0, "a.wav") == want
    assert "a.wav" not in d.band_detail and len([r for r in caplog.records if "no region bands" in r.getMessage()]) == 1
    monkeypatch.setattr(settings, "hip_region_bands", "on")
    with pytest.raises(ValueError, match="SOFTSPOKEN_BANDS"):
        d._file_regions(ctx, 4, 0, "a.wav")


class _JobModel:
    def __init__(self, ctx):
        self.ctx = ctx

    def with_range_fallback(self, run, key=None):
        return run(self.ctx)


class _Info:
    channels = 2


@pytest.mark.parametrize("mode", ["mix", "each"])
def test_detect_files_reads_every_files_results_before_the_first_bands_call(monkeypatch, mode):
    """One run, three stereo files on one context: the first region_bands call takes the run's device buffers, so the peaks of all
    files ('each' mode) must have been read by then."""
    from root.code.frontend import NNDetector as mod
    d, ctx = _detector(), _Ctx()
    d.model, d._resident = _JobModel(ctx), None
    files = ["a.wav", "b.wav", "c.wav"]
    fids = {f: 2 * k if mode == "each" else k for k, f in enumerate(files)}
    monkeypatch.setattr(mod, "add_file_to_context", lambda c, f: (fids[f], _Info()))
    monkeypatch.setattr(settings, "hip_channel_mode", mode)
    monkeypatch.setattr(settings, "hip_region_bands", "0")
    off = d.detect_files(files) if mode == "each" else {f: ctx.regions(fids[f]) for f in files}
    assert not ctx.calls and not d.band_detail
    monkeypatch.setattr(settings, "hip_region_bands", "1")
    got = d.detect_files(files)
    n_sig = 2 if mode == "each" else 1
    assert got == off and list(got) == files                              # the regions are those of a job with the setting off
    assert ctx.calls == [(fids[f], got[f], n_sig) for f in files]
    for f in files:
        assert d.band_detail[f][0] == (2 if mode == "each" else 0) and d.band_detail[f][1].shape == (len(got[f]), n_sig)
        if mode == "each":
            assert d.channel_detail[f] == (2, np.full((3, 2), 0.5).tolist())


# ---- the Raven exporter --------------------------------------------------------------------------------------------------------
def _table(tmp_path):
    return pd.DataFrame({"ID": [1, 2, 3, 4, 5], "file_path": [str(tmp_path)] * 5, "file_name": ["a.wav"] * 3 + ["b.wav"] * 2,
                         "start_time": [0.5, 2.0, 4.0, 1.0, 3.0], "end_time": [1.0, 2.5, 4.5, 1.5, 3.5], "erase": [0, 1, 0, 0, 0],
                         "user_comment": [""] * 5, "review_datetime": [""] * 5})


def _raven(tmp_path, name, df, **kw):
    rx.RavenTxtTransform()(df, base_dir=tmp_path, project_name=name, **kw)
    return (tmp_path / "Raven Outputs" / name / f"{name}.txt").read_bytes()


def test_raven_per_row_boxes_and_fallback_rows(tmp_path):
    df = _table(tmp_path)
    bands = pd.DataFrame({"ID": [1, 2, 2, 3, 5, 5], "file_name": ["a.wav"] * 4 + ["b.wav"] * 2, "channel": [NAN, 0, 1, NAN, 0, 1],
                          "low_hz": [120.4, 300.0, 250.5, NAN, NAN, 410.6], "high_hz": [3100.5, 2800.0, 2900.4, NAN, NAN, 5000.2]})
    text = _raven(tmp_path, "p", df, bands=bands).decode()
    rows = [ln.split("\t") for ln in text.splitlines()]
    lo, hi = rows[0].index("Low Freq (Hz)"), rows[0].index("High Freq (Hz)")
    got = [(r[lo], r[hi]) for r in rows[1:]]
    # ID 1: its own box; 2: lowest low and highest high over its channels; 3: no estimate; 4: no band row (a manual row); 5: one channel
    assert got == [("120", "3100"), ("250", "2900"), ("0", "8000"), ("0", "8000"), ("411", "5000")]
    # a mapping gives the same; other constants for the fallback rows
    mapping = {1: (120.4, 3100.5), 2: [(300.0, 2800.0), (250.5, 2900.4)], 3: (NAN, NAN), 5: [(NAN, NAN), (410.6, 5000.2)]}
    assert _raven(tmp_path, "q", df, bands=mapping).decode() == text
    text = _raven(tmp_path, "r", df, bands=mapping, low_freq=50, high_freq=11000).decode()
    assert [tuple(ln.split("\t")[lo:hi + 1]) for ln in text.splitlines()[1:]][2:4] == [("50", "11000")] * 2
    # a band row serves its own recording only: a manual row on b.wav that was given ID 6, which a later job handed to a detection on
    # c.wav, keeps the constants (a mapping keyed by (ID, file_name) does the same; one keyed by the ID alone serves any row of that ID)
    manual = pd.concat([df, pd.DataFrame({"ID": [6], "file_path": [str(tmp_path)], "file_name": ["b.wav"], "start_time": [5.0],
                                          "end_time": [5.5], "erase": [0], "user_comment": [""], "review_datetime": [""]})], ignore_index=True)
    later = pd.concat([bands, pd.DataFrame({"ID": [6], "file_name": ["c.wav"], "channel": [NAN], "low_hz": [700.0], "high_hz": [900.0]})])
    last = lambda t: tuple(t.decode().splitlines()[-1].split("\t")[lo:hi + 1])
    assert last(_raven(tmp_path, "m", manual, bands=later)) == ("0", "8000")
    assert last(_raven(tmp_path, "m", manual, bands={(6, "c.wav"): (700.0, 900.0)})) == ("0", "8000")
    assert last(_raven(tmp_path, "m", manual, bands={(6, "b.wav"): (700.0, 900.0)})) == ("700", "900")
    assert last(_raven(tmp_path, "m", manual, bands={6: (700.0, 900.0)})) == ("700", "900")
    # a table without an ID column: every row keeps the constants
    base = _raven(tmp_path, "s", df.drop(columns=["ID"]))
    assert _raven(tmp_path, "s", df.drop(columns=["ID"]), bands=bands) == base


def test_raven_without_bands_is_byte_for_byte_the_old_call(tmp_path):
    df = _table(tmp_path)
    old = _raven(tmp_path, "p", df)
    assert _raven(tmp_path, "p", df, bands=None) == old
    assert _raven(tmp_path, "p", df, bands={}) == old
    assert _raven(tmp_path, "p", df, bands=pd.DataFrame({"ID": [], "low_hz": [], "high_hz": []})) == old
    assert b"\t0\t8000\t" in old
    with pytest.raises(ValueError, match="missing column"):
        _raven(tmp_path, "p", df, bands=pd.DataFrame({"ID": [1], "low_hz": [1.0]}))


def test_save_review_passes_the_side_file_when_it_exists(tmp_path, monkeypatch):
    from softspoken_amd import review

    class _PM:
        pass
    pm = _PM()
    pm.projects_folder = str(tmp_path)
    det = tmp_path / "det.csv"
    _table(tmp_path).to_csv(det, index=False)
    pm.current_project = {"detections_file": str(det), "review_file": str(tmp_path / "rev.csv"), "name": "proj"}
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(settings, "minimum_detection_len", 0.1)
    review.ReviewTable(pm).save_review(persist=True)
    out = tmp_path / "Raven Outputs" / "proj" / "proj.txt"
    plain = out.read_bytes()
    assert plain.count(b"\t0\t8000\t") == 5
    (tmp_path / "det_bands.csv").write_text("ID,file_name,channel,low_hz,high_hz,peak_hz,speech_share,n_bins\n"
                                            "2,a.wav,,250.5,2900.4,800.0,0.750000,43\n4,b.wav,,,,,,0\n")
    review.ReviewTable(pm).save_review(persist=True)
    with_bands = out.read_bytes()
    assert with_bands.count(b"\t0\t8000\t") == 4 and b"\t250\t2900\t" in with_bands
    assert with_bands.replace(b"\t250\t2900\t", b"\t0\t8000\t") == plain
