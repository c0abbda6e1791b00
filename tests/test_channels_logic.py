"""The drop-in's channel mode without a GPU: settings.hip_channel_mode, and ProcessWorker.run's side file (<detections stem>_channels.csv)
against a scripted detector in the manner of tests/test_worker_logic.py."""
import importlib
import os

import pytest

from root.code.backend import settings
from root.code.backend.worker import ProcessWorker
from softspoken_amd.detections import DetectionProject, ProjectSettings


class _Model:
    def drop_second_context(self):
        pass


class _Det:
    """file "fK": K + 1 regions; channels: f0 mono, the others stereo; channel_detail filled at file_end, as NNDetector does."""

    def __init__(self, with_detail=True):
        self.model = _Model()
        if with_detail:
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
        if hasattr(self, "channel_detail"):
            n_ch = 1 if k == 0 else 2
            # region r of a stereo file: heard by channel r % 2 alone, by both when r == 2 (threshold 0.1: exactly 0.1 is not heard)
            self.channel_detail[file] = (n_ch, [[0.25 + r] if n_ch == 1 else
                                                [0.5 if (r % 2 == 0 or r == 2) else 0.1, 0.75 if (r % 2 == 1 or r == 2) else -1.5]
                                                for r in range(k + 1)])
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


def test_setting_reads_the_environment_and_defaults_to_mix(monkeypatch):
    try:
        monkeypatch.delenv("SOFTSPOKEN_CHANNELS", raising=False)
        assert importlib.reload(settings).hip_channel_mode == "mix"
        monkeypatch.setenv("SOFTSPOKEN_CHANNELS", "each")
        assert importlib.reload(settings).hip_channel_mode == "each"
    finally:
        monkeypatch.undo()
        importlib.reload(settings)


def test_unknown_mode_is_refused(monkeypatch, build_all):
    from root.code.backend import voice_activity
    monkeypatch.setattr(settings, "hip_channel_mode", "left")
    with pytest.raises(ValueError, match="'mix' or 'each'"):
        voice_activity.channel_mode()
    monkeypatch.setattr(settings, "hip_channel_mode", "each")
    assert voice_activity.channel_mode() == "each"


def test_each_mode_writes_the_side_file_with_the_rows_ids(monkeypatch, tmp_path):
    monkeypatch.setattr(settings, "hip_channel_mode", "each")
    monkeypatch.setattr(settings, "threshold", 0.1)
    csv_path = str(tmp_path / "detections.csv")
    files = [str(tmp_path / f"f{k}.wav") for k in (0, 1, 2, 3)]
    proj = _run(_Det(), files[:3], csv_path)
    side = str(tmp_path / "detections_channels.csv")
    assert list(proj.df["ID"]) == [1, 2, 3, 4, 5, 6]
    want = ["ID,file_name,n_channels,heard,peaks",
            "1,f0.wav,1,0,0.250000",
            "2,f1.wav,2,0,0.500000;-1.500000",
            "3,f1.wav,2,1,0.100000;0.750000",
            "4,f2.wav,2,0,0.500000;-1.500000",
            "5,f2.wav,2,1,0.100000;0.750000",
            "6,f2.wav,2,0;1,0.500000;0.750000"]
    assert open(side).read().splitlines() == want
    # a second job on the project: IDs go on from the CSV that is there, the side file is appended to (one header)
    proj2 = _run(_Det(), files[3:], csv_path)
    assert list(proj2.df["ID"]) == list(range(1, 11))
    lines = open(side).read().splitlines()
    assert lines[:7] == want and [ln.split(",")[0] for ln in lines[7:]] == ["7", "8", "9", "10"]
    assert all(ln.split(",")[1] == "f3.wav" for ln in lines[7:]) and lines[10] == "10,f3.wav,2,1,0.100000;0.750000"
    # the IDs of the side file are the IDs of the same regions' rows in the detections CSV
    import pandas as pd
    main = pd.read_csv(csv_path)
    for ln in lines[1:]:
        i, name = ln.split(",")[:2]
        assert main.loc[main["ID"] == int(i), "file_name"].item() == name


def test_mix_mode_writes_no_side_file_and_the_same_csv(monkeypatch, tmp_path):
    monkeypatch.setattr(settings, "hip_channel_mode", "each")
    files = [str(tmp_path / f"f{k}.wav") for k in (0, 1, 2)]
    _run(_Det(), files, str(tmp_path / "each.csv"))
    monkeypatch.setattr(settings, "hip_channel_mode", "mix")
    _run(_Det(), files, str(tmp_path / "mix.csv"))
    assert not os.path.exists(tmp_path / "mix_channels.csv") and os.path.exists(tmp_path / "each_channels.csv")
    assert open(tmp_path / "mix.csv").read() == open(tmp_path / "each.csv").read()


def test_detector_without_channel_detail_still_runs(monkeypatch, tmp_path):
    monkeypatch.setattr(settings, "hip_channel_mode", "each")
    files = [str(tmp_path / f"f{k}.wav") for k in (0, 1)]
    proj = _run(_Det(with_detail=False), files, str(tmp_path / "d.csv"))
    assert len(proj.df) == 3 and not os.path.exists(tmp_path / "d_channels.csv")


def test_rows_of_a_recreated_detections_csv_do_not_stay_in_the_side_file(monkeypatch, tmp_path):
    monkeypatch.setattr(settings, "hip_channel_mode", "each")
    csv_path = str(tmp_path / "detections.csv")
    side = str(tmp_path / "detections_channels.csv")
    files = [str(tmp_path / f"f{k}.wav") for k in (0, 1, 2)]
    _run(_Det(), files, csv_path)
    first = open(side).read()
    os.remove(csv_path)                                   # the project starts over: IDs begin at 1 again
    _run(_Det(), files[1:], csv_path)
    lines = open(side).read().splitlines()
    assert [ln.split(",")[:2] for ln in lines[1:]] == [["1", "f1.wav"], ["2", "f1.wav"], ["3", "f2.wav"], ["4", "f2.wav"], ["5", "f2.wav"]]
    assert lines[0] == first.splitlines()[0]
