"""Stream bands (ss_stream_open_bands / ss_stream_bands) on a real MI355X.  The yardstick is bytes: the records
and profiles a stream returned, concatenated, against ss_region_bands on the stream's own regions after ss_add_pcm(_channels) + ss_run
of the whole recording -- for any split into pieces, any cadence of steps, whatever shares the steps, and across export / import.
Everything else a band stream returns is compared with the same stream opened with bands off.

Recordings are 12 s (20 windows, about 1500 bins, 24 tiles); the heads are the crafted `spread` and `mixed` heads of
tests/separation_ref.py on the session checkpoint's body (the session head's speech map is 0 almost everywhere)."""
import json
import math
import os
import struct

import numpy as np
import pytest

import separation_ref as R
import test_gpu_separation as T
from softspoken_amd import synth

pytestmark = pytest.mark.gpu
SECONDS = 12.0
SEED = 4107                                    # chosen on the device's fp32 table (test_runs_and_gaps asserts the conditions)
LAYOUTS = {"mono16": (16000, 1, False), "mix48": (48000, 2, False), "each48": (48000, 2, True), "each22x3": (22050, 3, True)}
NEW_KERNELS = ("stream_map_kernel", "stream_band_kernel")
ERASE = dict(pad_s=0.05, min_len_s=0.1)


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native as N
    return N


@pytest.fixture(scope="module")
def heads(sd_np):
    spread = R.spread_head(sd_np)
    zero = dict(spread)                                              # the speech row all zero: no power, "no estimate" everywhere
    w = spread["spec_output_conv.1.weight"].copy()
    w[1] = 0.0
    zero["spec_output_conv.1.weight"] = w
    zero["spec_output_conv.1.bias"] = np.zeros(2, dtype=np.float32)
    return dict(spread=spread, mixed=R.mixed_head(sd_np), zero=zero)


@pytest.fixture(scope="module")
def ctxs(native, heads):
    made = {}

    def get(head, prec, key=0, **kw):
        if (head, prec, key) not in made:
            made[(head, prec, key)] = T._head_ctx(native, heads[head], prec, **kw)
        return made[(head, prec, key)]
    yield get
    for c in made.values():
        c.close()


_REC = {}


def rec(layout, seconds=SECONDS, seed=SEED):
    """int16 [frames, ch] of a layout's recording (seeded, made once)."""
    sr, ch, _ = LAYOUTS[layout]
    if (layout, seconds, seed) not in _REC:
        _REC[(layout, seconds, seed)] = np.ascontiguousarray(synth.to_pcm16(synth.synth_audio(seed, seconds, sr, ch)).reshape(-1, ch))
    return _REC[(layout, seconds, seed)]


def _bytes(pcm):
    return np.frombuffer(np.ascontiguousarray(pcm).tobytes(), dtype=np.uint8)


def add_whole(native, ctx, pcm, layout):
    sr, ch, each = LAYOUTS[layout]
    ctx.reset()
    if each:
        return ctx.add_pcm_channels(_bytes(pcm), native.PCM_S16, sr, ch, len(pcm)), ch
    return ctx.add_pcm(_bytes(pcm), native.PCM_S16, sr, ch, len(pcm)), 1


_MEDIAN = {}


def median_threshold(native, ctx, layout, key):
    """The median of the recording's own whole-file averages (the merged series of an each-channel layout)."""
    if key not in _MEDIAN:
        pcm = rec(layout)
        fid, n = add_whole(native, ctx, pcm, layout)
        ctx.run(0.1, 0.5)
        a = np.fmax.reduce(np.asarray([ctx.avg(fid + c)[0] for c in range(n)]), axis=0)
        _MEDIAN[key] = float(np.median(a))
    return _MEDIAN[key]


def whole_table(native, ctx, pcm, layout, thr, brk):
    fid, n = add_whole(native, ctx, pcm, layout)
    ctx.run(thr, brk)
    return ctx.regions_union(fid, n) if n > 1 else ctx.regions(fid)


def reference(native, ctx, pcm, layout, regions, **params):
    """ss_add_pcm(_channels) + ss_run + ss_region_bands on the given regions: (records [n, lanes], profiles [n, lanes, 2, 128])."""
    fid, n = add_whole(native, ctx, pcm, layout)
    ctx.run(0.1, 0.5)
    if not regions:
        return np.zeros((0, n), dtype=native.REGION_BAND_DTYPE), np.zeros((0, n, 2, 128))
    out, prof = ctx.region_bands(fid, regions, n, profile=True, **params)
    return out.reshape(len(regions), n), prof.reshape(len(regions), n, 2, 128)


class Got:
    """What a stream returned, step by step."""

    def __init__(self, lanes, ch, bands=True, profile=True, out_on=False):
        self.lanes, self.ch, self.on, self.profile, self.out_on = lanes, ch, bands, profile, out_on
        self.regs, self.avg, self.idx, self.bands, self.profs, self.peaks, self.out, self.when = [], [], [], [], [], [], [], []

    def take(self, ctx, sid, step_no=0):
        r = ctx.stream_regions(sid)
        a, i = ctx.stream_avg(sid)
        self.regs += r; self.avg.append(a); self.idx.append(i); self.when += [step_no] * len(r)
        if self.on:
            b, p = ctx.stream_bands(sid, self.lanes, profile=self.profile)
            assert b.shape == (len(r), self.lanes)                  # a region's bands arrive in the step that returns the region
            self.bands.append(b)
            if self.profile:
                self.profs.append(p)
        if self.lanes > 1:
            self.peaks.append(ctx.stream_region_peaks(sid, self.lanes))
        if self.out_on:
            self.out.append(ctx.stream_output(sid, self.ch)[1])

    def all_bands(self):
        return np.concatenate(self.bands)

    def all_profs(self):
        return np.concatenate(self.profs)

    def plain(self):
        """everything but the bands, as bytes"""
        return (list(self.regs), np.concatenate(self.avg).tobytes(), np.concatenate(self.idx).tobytes(),
                np.concatenate(self.peaks).tobytes() if self.peaks else b"", np.concatenate(self.out).tobytes() if self.out else b"")


def split_plan(kind, total, sr, seed=0):
    """(pieces, step_after): frame counts and whether a step follows each push."""
    if kind == "one":
        return [total], [True]
    if kind == "at_close":
        n = sr
        p = [n] * (total // n) + ([total % n] if total % n else [])
        return p, [False] * len(p)
    if kind == "tenth":
        n = sr // 10
        p = [n] * (total // n) + ([total % n] if total % n else [])
        return p, [True] * len(p)
    rng = np.random.default_rng(seed)
    p, left = [], total
    while left > 0:
        n = int(min(left, rng.integers(1, 2 * sr + 1) if rng.random() < 0.7 else rng.integers(1, 200)))
        p.append(n); left -= n
    return p, [bool(rng.random() < 0.4) for _ in p]


def open_stream(native, ctx, layout, thr, brk, bands=True, profile=True, erase=None, **params):
    sr, ch, each = LAYOUTS[layout]
    if bands:
        return ctx.stream_open_bands(native.PCM_S16, sr, ch, thr, brk, erase, False, each, profile=profile, **params)
    if each:
        return ctx.stream_open_channels(native.PCM_S16, sr, ch, thr, brk, erase)
    if erase is not None:
        return ctx.stream_open_output(native.PCM_S16, sr, ch, thr, brk, erase)
    return ctx.stream_open(native.PCM_S16, sr, ch, thr, brk)


def run_stream(native, ctx, layout, pcm, thr, brk, plan, bands=True, profile=True, erase=None, **params):
    sr, ch, each = LAYOUTS[layout]
    sid = open_stream(native, ctx, layout, thr, brk, bands, profile, erase, **params)
    g = Got(ch if each else 1, ch, bands, profile, erase is not None)
    at = 0
    for k, (n, st) in enumerate(zip(*plan)):
        ctx.stream_push(sid, pcm[at:at + n], frames=n)
        at += n
        if st:
            ctx.stream_step()
            g.take(ctx, sid, k)
    assert at == len(pcm)
    ctx.stream_close(sid)
    ctx.stream_step()
    g.take(ctx, sid, len(plan[0]))
    assert ctx.stream_info(sid)["finished"] == 1
    ctx.stream_free(sid)
    return g


def assert_bytes(g, want, label=""):
    wb, wp = want
    assert g.all_bands().shape == wb.shape, label
    assert g.all_bands().tobytes() == wb.tobytes(), (label, g.all_bands(), wb)
    if g.profile:
        assert g.all_profs().tobytes() == wp.tobytes(), label


# ---- 1. equality over splits ----------------------------------------------------------------------------------------------------
# every value of every axis at least once per split kind
MATRIX = [("fp32", "spread", "mono16"), ("f16x2", "mixed", "mix48"), ("fp32", "mixed", "each48"), ("f16x2", "spread", "each22x3")]


@pytest.mark.parametrize("split", ["one", "tenth", "random", "at_close"])
@pytest.mark.parametrize("prec,head,layout", MATRIX)
def test_equality_over_splits(native, ctxs, prec, head, layout, split):
    ctx = ctxs(head, prec)
    pcm = rec(layout)
    thr = median_threshold(native, ctx, layout, (head, prec, layout))
    g = run_stream(native, ctx, layout, pcm, thr, 0.05, split_plan(split, len(pcm), LAYOUTS[layout][0], seed=11))
    assert g.regs == whole_table(native, ctx, pcm, layout, thr, 0.05) and len(g.regs) >= 3
    want = reference(native, ctx, pcm, layout, g.regs)
    assert_bytes(g, want, (prec, head, layout, split))
    b = g.all_bands()
    assert (b["band_low"] >= 0).any() and (b["n_bins"] > 64).any()   # estimates, and regions that cross a tile boundary
    if split in ("tenth", "random"):
        assert len(set(g.when)) > 1                                   # regions came back in different steps, before the close


def test_other_parameters(native, ctxs):
    ctx = ctxs("spread", "fp32")
    pcm = rec("mix48")
    thr = median_threshold(native, ctx, "mix48", ("spread", "fp32", "mix48"))
    prm = dict(q_low=0.2, q_high=0.7, speech_channel=0)
    g = run_stream(native, ctx, "mix48", pcm, thr, 0.05, split_plan("tenth", len(pcm), 48000), **prm)
    assert_bytes(g, reference(native, ctx, pcm, "mix48", g.regs, **prm))
    dflt = reference(native, ctx, pcm, "mix48", g.regs)
    assert g.all_bands().tobytes() != dflt[0].tobytes()


# ---- 2. runs and gaps of every length -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,layout", [("fp32", "mono16"), ("f16x2", "each48")])
def test_runs_and_gaps(native, ctxs, prec, layout):
    ctx = ctxs("spread", prec)
    pcm = rec(layout)
    thr = median_threshold(native, ctx, layout, ("spread", prec, layout))
    tables = {brk: whole_table(native, ctx, pcm, layout, thr, brk) for brk in (0.0, 0.05, 0.5, 5.0)}
    print("STREAM_BANDS regions per break_s:", {k: len(v) for k, v in tables.items()})
    assert len(tables[0.05]) >= 6
    assert len(tables[0.5]) < len(tables[0.0]) and len(tables[0.5]) >= 1    # at least one region merged a gap at 0.5
    assert len(tables[5.0]) == 1
    for brk, table in tables.items():
        g = run_stream(native, ctx, layout, pcm, thr, brk, split_plan("random", len(pcm), LAYOUTS[layout][0], seed=int(brk * 100) + 3))
        assert g.regs == table
        assert_bytes(g, reference(native, ctx, pcm, layout, g.regs), (prec, layout, brk))


# ---- 3. extremes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,head,layout", [("fp32", "mixed", "mono16"), ("f16x2", "spread", "each48")])
def test_threshold_minus_infinity_is_one_region_returned_at_close(native, ctxs, prec, head, layout):
    ctx = ctxs(head, prec)
    pcm = rec(layout)
    plan = split_plan("tenth", len(pcm), LAYOUTS[layout][0])
    g = run_stream(native, ctx, layout, pcm, -math.inf, 0.5, plan, erase=dict(pad_s=0.0, min_len_s=0.0))
    assert len(g.regs) == 1 and g.when == [len(plan[0])]
    W, n_bins = R.file_geometry(LAYOUTS[layout][0], len(pcm))
    assert int(g.all_bands()[0, 0]["n_bins"]) == n_bins - 1          # every covered bin but the last (rule 1 on the last bin's time)
    assert_bytes(g, reference(native, ctx, pcm, layout, g.regs))


def test_threshold_plus_infinity_is_no_region(native, ctxs):
    ctx = ctxs("spread", "fp32")
    pcm = rec("mono16")
    g = run_stream(native, ctx, "mono16", pcm, math.inf, 0.5, split_plan("tenth", len(pcm), 16000), erase=dict(pad_s=0.0, min_len_s=0.0))
    assert g.regs == [] and g.all_bands().shape == (0, 1) and g.all_profs().shape == (0, 1, 2, 128)


def test_no_estimate(native, ctxs):
    """A head whose speech row is all zero: T == 0 in every region; and single-bin runs, which hold no bin under rule 1."""
    ctx = ctxs("zero", "fp32")
    pcm = rec("mono16")
    thr = median_threshold(native, ctx, "mono16", ("zero", "fp32", "mono16"))
    g = run_stream(native, ctx, "mono16", pcm, thr, 0.0, split_plan("tenth", len(pcm), 16000))
    want = reference(native, ctx, pcm, "mono16", g.regs)
    assert len(g.regs) >= 3 and (want[0]["band_low"] == -1).all() and np.isnan(want[0]["low_hz"]).all()
    assert_bytes(g, want)
    ctx2 = ctxs("spread", "fp32")
    thr2 = median_threshold(native, ctx2, "mono16", ("spread", "fp32", "mono16"))
    g2 = run_stream(native, ctx2, "mono16", pcm, thr2, 0.0, split_plan("random", len(pcm), 16000, seed=5))
    print("STREAM_BANDS regions without a bin at break_s 0:", int((g2.all_bands()["n_bins"] == 0).sum()), "of", len(g2.regs))
    assert_bytes(g2, reference(native, ctx2, pcm, "mono16", g2.regs))


# ---- 4. company -------------------------------------------------------------------------------------------------------------------
def _company(native, ctx, thr, which):
    """One step sequence over the streams named in `which`, every stream pushed at its own cadence; -> {name: Got}."""
    spec = {  # name: (layout, bands, erase, piece seconds, step every n-th round)
        "band_mix": ("mix48", True, None, 0.25), "band_each_out": ("each48", True, ERASE, 0.4), "plain": ("mono16", False, None, 0.7),
        "out": ("mix48", False, ERASE, 0.3), "each": ("each22x3", False, None, 0.55)}
    st = {}
    for name in which:
        layout, bands, erase, piece = spec[name]
        sr, ch, each = LAYOUTS[layout]
        st[name] = dict(layout=layout, sid=open_stream(native, ctx, layout, thr, 0.05, bands, True, erase), at=0, pcm=rec(layout),
                        n=int(piece * sr), got=Got(ch if each else 1, ch, bands, True, erase is not None), closed=False)
    rnd = 0
    while not all(s["closed"] for s in st.values()):
        for k, (name, s) in enumerate(st.items()):
            if s["closed"] or (rnd + k) % 3 == 2:                    # a round in three, a stream pushes nothing
                continue
            n = min(s["n"], len(s["pcm"]) - s["at"])
            ctx.stream_push(s["sid"], s["pcm"][s["at"]:s["at"] + n], frames=n)
            s["at"] += n
            if s["at"] == len(s["pcm"]):
                ctx.stream_close(s["sid"]); s["closed"] = True
        ctx.stream_step()
        for s in st.values():
            s["got"].take(ctx, s["sid"], rnd)
        rnd += 1
    for s in st.values():
        assert ctx.stream_info(s["sid"])["finished"] == 1
        ctx.stream_free(s["sid"])
    return {name: s["got"] for name, s in st.items()}


@pytest.mark.parametrize("prec", ["fp32", "f16x2"])
def test_company(native, ctxs, prec):
    ctx = ctxs("spread", prec)
    thr = median_threshold(native, ctx, "mix48", ("spread", prec, "mix48"))
    names = ["band_mix", "band_each_out", "plain", "out", "each"]
    together = _company(native, ctx, thr, names)
    for name in names:
        alone = _company(native, ctx, thr, [name])[name]
        assert together[name].plain() == alone.plain(), name
        if alone.on:
            assert together[name].all_bands().tobytes() == alone.all_bands().tobytes(), name
            assert together[name].all_profs().tobytes() == alone.all_profs().tobytes(), name
    no_bands = _company(native, ctx, thr, ["plain", "out", "each"])       # no band stream on the context in these steps
    for name in ("plain", "out", "each"):
        assert together[name].plain() == no_bands[name].plain(), name
    for name, layout in (("band_mix", "mix48"), ("band_each_out", "each48")):
        g = together[name]
        assert len(g.regs) >= 3
        assert_bytes(g, reference(native, ctx, rec(layout), layout, g.regs), name)


# ---- 5. bands off is today's path ---------------------------------------------------------------------------------------------
def _stats_script(native, ctx, thr, with_band_first):
    """The same steps over a plain, an output and an each-channel stream; optionally a band stream opened and freed before them."""
    if with_band_first:
        sid = open_stream(native, ctx, "mix48", thr, 0.05, True)
        ctx.stream_free(sid)
    ctx.reset_stats()
    _company(native, ctx, thr, ["plain", "out", "each"])
    return {s["name"]: s["launches"] for s in ctx.kernel_stats()}


def test_bands_off_is_the_old_path(native, ctxs):
    ctx = ctxs("spread", "fp32", "profile", profile=True)
    thr = median_threshold(native, ctx, "mix48", ("spread", "fp32", "mix48"))
    off = _stats_script(native, ctx, thr, False)
    after = _stats_script(native, ctx, thr, True)
    assert off == after and off["stream_average"] > 10
    assert not any(k in off for k in NEW_KERNELS)
    ctx.reset_stats()
    _company(native, ctx, thr, ["band_mix"])
    on = {s["name"]: s["launches"] for s in ctx.kernel_stats()}
    assert all(on.get(k, 0) > 0 for k in NEW_KERNELS)


@pytest.mark.parametrize("prec,layout,erase", [("fp32", "mono16", None), ("f16x2", "mix48", ERASE), ("f16x2", "each48", ERASE), ("fp32", "each22x3", None)])
def test_a_band_stream_returns_what_it_returns_with_bands_off(native, ctxs, prec, layout, erase):
    ctx = ctxs("mixed", prec)
    pcm = rec(layout)
    thr = median_threshold(native, ctx, layout, ("mixed", prec, layout))
    plan = split_plan("random", len(pcm), LAYOUTS[layout][0], seed=21)
    on = run_stream(native, ctx, layout, pcm, thr, 0.05, plan, True, True, erase)
    off = run_stream(native, ctx, layout, pcm, thr, 0.05, plan, False, False, erase)
    assert on.plain() == off.plain() and len(on.regs) >= 3


# ---- 6. images --------------------------------------------------------------------------------------------------------------------
def _moved(native, src, dst, layout, pcm, thr, brk, cut_frames, stage_frames, erase=None):
    """Push and step up to cut_frames, stage stage_frames more without a step, export, import into dst, finish there."""
    sr, ch, each = LAYOUTS[layout]
    sid = open_stream(native, src, layout, thr, brk, True, True, erase)
    g = Got(ch if each else 1, ch, True, True, erase is not None)
    at, n = 0, sr // 4
    while at < cut_frames:
        k = min(n, cut_frames - at)
        src.stream_push(sid, pcm[at:at + k], frames=k); at += k
        src.stream_step(); g.take(src, sid)
    if stage_frames:
        src.stream_push(sid, pcm[at:at + stage_frames], frames=stage_frames); at += stage_frames
    image = src.stream_export(sid)
    assert image[:8] == b"SSSTRM05"
    info = src.stream_info(sid)
    src.stream_free(sid)
    sid = dst.stream_import(image)
    assert dst.stream_info(sid)["state_bytes"] == info["state_bytes"]
    assert dst.stream_export(sid) == image                             # an image read and written again
    while at < len(pcm):
        k = min(n, len(pcm) - at)
        dst.stream_push(sid, pcm[at:at + k], frames=k); at += k
        dst.stream_step(); g.take(dst, sid)
    dst.stream_close(sid); dst.stream_step(); g.take(dst, sid)
    dst.stream_free(sid)
    return g, image


@pytest.mark.parametrize("prec,layout,erase", [("fp32", "mono16", None), ("f16x2", "each48", ERASE)])
def test_images(native, ctxs, prec, layout, erase):
    a, b = ctxs("spread", prec), ctxs("spread", prec, "second")
    sr = LAYOUTS[layout][0]
    pcm = rec(layout)
    thr = median_threshold(native, a, layout, ("spread", prec, layout))
    table = whole_table(native, a, pcm, layout, thr, 0.5)
    unmoved = run_stream(native, a, layout, pcm, thr, 0.5, split_plan("tenth", len(pcm), sr), True, True, erase)
    assert unmoved.regs == table and len(table) >= 2
    s0, e0 = table[0]
    gaps = [(table[i][1], table[i + 1][0]) for i in range(len(table) - 1)]
    mid_region = int(((s0 + e0) / 2 + 3.2) * sr)                        # the frames whose bins are final lie about 3 s back
    mid_gap = int(((gaps[0][0] + gaps[0][1]) / 2 + 3.2) * sr)
    for cut, stage in ((mid_region, 0), (mid_gap, 0), (mid_region, sr // 3), (sr // 10, 0)):
        cut = max(1, min(cut, len(pcm) - sr))
        g, image = _moved(native, a, b, layout, pcm, thr, 0.5, cut, stage, erase)
        assert g.plain() == unmoved.plain(), (cut, stage)
        assert g.all_bands().tobytes() == unmoved.all_bands().tobytes() and g.all_profs().tobytes() == unmoved.all_profs().tobytes(), (cut, stage)


HDR = 8 + 8 * 4 + 4 * 8 + 14 * 8                                   # ImageHdr: magic, 8 int32, 4 doubles, 14 int64


def _old_image_length(image, lanes):
    """The length of an "SSSTRM01" .. "04" image from its own header, by the layout those images have always had."""
    i64 = struct.unpack_from("<14q", image, 8 + 32 + 32)
    staged, mono_n, sig_n, lg_n = i64[2], i64[4], i64[6], i64[8]
    n = HDR + staged + 4 * lanes * (mono_n + sig_n + lg_n * 256)
    tag = image[:8]
    if tag == b"SSSTRM01":
        return n
    n += 8                                                            # the step
    at = HDR + 8
    if tag == b"SSSTRM04":
        il_lanes, with_out = struct.unpack_from("<2i", image, at)
        assert il_lanes == lanes
        n += 8 + 24 * lanes
        at += 8 + 24 * lanes
    else:
        with_out = tag == b"SSSTRM03"
    if with_out:
        raw_bytes, n_er = struct.unpack_from("<2q", image, at + 32)
        n += 48 + 8 * n_er + raw_bytes
    return n


def test_images_of_streams_without_bands_are_unchanged(native, ctxs):
    """A stream opened by the old calls writes the image it always wrote: tag and length by the old layout's arithmetic, and the same
    bytes whether or not a band stream shares its steps."""
    ctx = ctxs("spread", "fp32")
    for layout, erase, tag in (("mono16", None, b"SSSTRM01"), ("mix48", ERASE, b"SSSTRM03"), ("each48", None, b"SSSTRM04"),
                               ("each48", ERASE, b"SSSTRM04")):
        sr, ch, each = LAYOUTS[layout]
        lanes = ch if each else 1
        pcm = rec(layout)
        images = []
        for company in (False, True):
            sid = open_stream(native, ctx, layout, 0.1, 0.5, False, False, erase)
            bid = open_stream(native, ctx, layout, 0.1, 0.5, True, False, erase) if company else None
            for at in (0, sr * 2):
                ctx.stream_push(sid, pcm[at:at + sr * 2], frames=sr * 2)
                if company:
                    ctx.stream_push(bid, pcm[at:at + sr * 2], frames=sr * 2)
                ctx.stream_step()
            ctx.stream_push(sid, pcm[sr * 4:sr * 4 + 777], frames=777)              # staged
            images.append(ctx.stream_export(sid))
            ctx.stream_free(sid)
            if company:
                bimage, info = ctx.stream_export(bid), ctx.stream_info(bid)
                ctx.stream_free(bid)
                assert bimage[:8] == b"SSSTRM05" and len(bimage) > len(images[0]) + lanes * 5 * 256 * 8
                assert info["state_bytes"] >= lanes * 5 * 256 * 8
        assert images[0][:8] == tag and len(images[0]) == _old_image_length(images[0], lanes), (layout, len(images[0]))
        assert images[1] == images[0], layout


def test_a_finished_band_stream_exports_after_later_steps(native, ctxs):
    """A finished stream is planned no more, so it must keep nothing in the arena: its image after steps of other streams reads and
    writes again, and imports as a finished stream without regions."""
    ctx = ctxs("spread", "fp32", "finished")                           # a fresh context: one arena half exists when the stream finishes
    pcm = rec("each48")
    y = open_stream(native, ctx, "each48", 0.1, 0.5, True, True, None)
    ctx.stream_push(y, pcm, frames=len(pcm)); ctx.stream_close(y); ctx.stream_step()
    assert ctx.stream_info(y)["finished"] == 1
    first = ctx.stream_export(y)
    z = open_stream(native, ctx, "mono16", 0.1, 0.5, True, True, None)
    small = rec("mono16")
    for at in range(0, 16000 * 4, 8000):
        ctx.stream_push(z, small[at:at + 8000], frames=8000); ctx.stream_step()
        assert ctx.stream_regions(y) == [] and ctx.stream_bands(y, 2)[0].shape == (0, 2)
    image = ctx.stream_export(y)
    assert image == first and image[:8] == b"SSSTRM05"
    assert len(image) == HDR + 8 + 48 + 24 * 2 + 8 * 2 * 256 * 5 and not any(image[-8 * 2 * 256 * 5:])
    assert ctx.stream_info(y)["state_bytes"] < 4096
    back = ctx.stream_import(image)
    assert ctx.stream_info(back)["finished"] == 1 and ctx.stream_export(back) == image
    ctx.stream_step()
    assert ctx.stream_regions(back) == []
    for sid in (y, z, back):
        ctx.stream_free(sid)


def test_malformed_band_images(native, ctxs):
    ctx = ctxs("spread", "fp32")
    pcm = rec("each48")
    sid = open_stream(native, ctx, "each48", 0.1, 0.5, True, True, None)
    ctx.stream_push(sid, pcm[:48000 * 4], frames=48000 * 4); ctx.stream_step()
    image = ctx.stream_export(sid)
    ctx.stream_free(sid)
    hdr = HDR                                                          # ImageHdr; then the step (a double), then ImageBands (lanes first)
    assert struct.unpack_from("<d", image, hdr)[0] == 0.6 and struct.unpack_from("<i", image, hdr + 8)[0] == 2
    bad = {
        "truncated": image[:-8], "longer": image + b"\0" * 8, "cut in the band block": image[:hdr + 20],
        "lanes 3": image[:hdr + 8] + struct.pack("<i", 3) + image[hdr + 12:],
        "lanes 0": image[:hdr + 8] + struct.pack("<i", 0) + image[hdr + 12:],
        "step 0.3": image[:hdr] + struct.pack("<d", 0.3) + image[hdr + 8:],
        "q_low 0": image[:hdr + 8 + 24] + struct.pack("<d", 0.0) + image[hdr + 8 + 32:],
    }
    for name, img in bad.items():
        with pytest.raises(native.NativeError) as e:
            ctx.stream_import(img)
        assert e.value.code == native.SS_ERR_ARG, name
    sid = ctx.stream_import(image)                                     # the context works afterwards
    ctx.stream_push(sid, pcm[48000 * 4:], frames=len(pcm) - 48000 * 4)
    ctx.stream_close(sid); ctx.stream_step()
    assert ctx.stream_info(sid)["finished"] == 1
    ctx.stream_free(sid)


# ---- 7. state ---------------------------------------------------------------------------------------------------------------------
def _state_series(native, ctx, seconds, thr, brk, erase):
    """state_bytes behind every 10 s piece of a recording that repeats the 12 s one"""
    base = rec("mono16")
    reps = int(math.ceil(seconds * 16000 / len(base)))
    pcm = np.tile(base, (reps, 1))[:int(seconds * 16000)]
    sid = open_stream(native, ctx, "mono16", thr, brk, True, False, erase)
    out = []
    for at in range(0, len(pcm), 160000):
        ctx.stream_push(sid, pcm[at:at + 160000], frames=min(160000, len(pcm) - at))
        ctx.stream_step()
        out.append(ctx.stream_info(sid)["state_bytes"])
    ctx.stream_free(sid)
    return out


def test_state_is_bounded(native, ctxs):
    """As tests/test_gpu_stream.py compares a plain stream: at 60 s and at 600 s, both behind a 10 s piece (the same phase of the window
    grid: 10 s is 16.67 steps, 60 s and 600 s are whole numbers of them).  With the threshold -inf one region is open from the first bin
    to the close; that stream has output (an infinite threshold needs it), whose held PCM is bounded and at the same phase too."""
    ctx = ctxs("spread", "f16x2")
    med = median_threshold(native, ctx, "mono16", ("spread", "f16x2", "mono16"))
    for thr, erase in ((-math.inf, dict(pad_s=0.0, min_len_s=0.0)), (med, None)):
        long_ = _state_series(native, ctx, 600.0, thr, 0.5, erase)
        print("STREAM_BANDS state_bytes thr", thr, "at 60 s", long_[5], "at 600 s", long_[59])
        assert long_[59] == long_[5], (thr, long_[5], long_[59])
        assert long_[59] < 5 * 256 * 8 + 330 * 2048 + 400_000         # the header's figures: accumulators, about 0.6 MB of sums, a plain stream's state
    # break_s adds nothing to the band state (the header: "a gap is walked through, not held")
    a = _state_series(native, ctx, 30.0, med, 0.05, None)
    b = _state_series(native, ctx, 30.0, med, 5.0, None)
    assert a == b


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(native, ctxs, heads):
    ctx = ctxs("spread", "fp32")
    S16 = native.PCM_S16
    for kw in (dict(q_low=0.0), dict(q_low=0.6, q_high=0.5), dict(q_high=1.5), dict(speech_channel=2)):
        with pytest.raises(native.NativeError) as e:
            ctx.stream_open_bands(S16, 16000, 1, 0.1, 0.5, **kw)
        assert e.value.code == native.SS_ERR_ARG, kw
    ctx.set_window_step(0.3)
    try:
        with pytest.raises(native.NativeError) as e:
            ctx.stream_open_bands(S16, 16000, 1, 0.1, 0.5)
        assert e.value.code == native.SS_ERR_STATE
        plain = ctx.stream_open(S16, 16000, 1, 0.1, 0.5)               # a stream with another step: no band image can carry it
        assert ctx.stream_export(plain)[:8] == b"SSSTRM02"
        ctx.stream_free(plain)
    finally:
        ctx.set_window_step(0.6)
    audio = native.Context(None, 0)
    try:
        with pytest.raises(native.NativeError) as e:
            audio.stream_open_bands(S16, 16000, 1, 0.1, 0.5)
        assert e.value.code == native.SS_ERR_STATE
    finally:
        audio.close()
    plain = ctx.stream_open(S16, 16000, 1, 0.1, 0.5)
    with pytest.raises(native.NativeError) as e:
        ctx.stream_bands(plain)
    assert e.value.code == native.SS_ERR_STATE
    ctx.stream_free(plain)
    sid = ctx.stream_open_bands(S16, 16000, 1, 0.1, 0.5, profile=False)
    assert ctx.stream_bands(sid)[0].shape == (0, 1)
    with pytest.raises(native.NativeError) as e:
        ctx.stream_bands(sid, profile=True)
    assert e.value.code == native.SS_ERR_STATE
    ctx.stream_free(sid)


def _nan_case(sr=16000):
    """float32 mono with one NaN sample at 6 s: the recording the whole-file band test refuses under f16x2 (tests/test_gpu_bands.py)"""
    y = (0.5 * synth.synth_audio(61, 10.0, sr, 1, with_silence=False).T.reshape(-1, 1)).astype(np.float32)
    y[sr * 6, 0] = np.float32("nan")
    return y


def test_f16x2_refuses_the_step_and_commits_nothing(native, ctxs):
    c = ctxs("spread", "f16x2")
    x = _nan_case()
    sid = c.stream_open_bands(native.PCM_F32, 16000, 1, 0.1, 0.5, profile=True)
    c.stream_push(sid, x[:16000 * 5]); c.stream_step()
    info, image = c.stream_info(sid), c.stream_export(sid)
    assert info["windows_run"] > 0
    c.stream_push(sid, x[16000 * 5:16000 * 8])
    staged_image = c.stream_export(sid)
    with pytest.raises(native.NativeError) as e:
        c.stream_step()
    assert e.value.code == native.SS_ERR_RANGE
    assert c.stream_export(sid) == staged_image                       # nothing committed, band state included
    assert len(staged_image) == len(image) + 3 * 16000 * 4
    c.stream_free(sid)


def test_a_stream_moved_before_its_first_window_gives_the_fp32_bands(native, ctxs):
    f16, f32 = ctxs("spread", "f16x2"), ctxs("spread", "fp32")
    pcm = rec("mix48")
    thr = median_threshold(native, f32, "mix48", ("spread", "fp32", "mix48"))
    sid = open_stream(native, f16, "mix48", thr, 0.05, True, True)
    f16.stream_push(sid, pcm[:4800], frames=4800)                      # staged, no step yet
    image = f16.stream_export(sid)
    f16.stream_free(sid)
    sid = f32.stream_import(image)
    g = Got(1, 2, True, True)
    at = 4800
    while at < len(pcm):
        k = min(24000, len(pcm) - at)
        f32.stream_push(sid, pcm[at:at + k], frames=k); at += k
        f32.stream_step(); g.take(f32, sid)
    f32.stream_close(sid); f32.stream_step(); g.take(f32, sid)
    f32.stream_free(sid)
    assert g.regs == whole_table(native, f32, pcm, "mix48", thr, 0.05)
    assert_bytes(g, reference(native, f32, pcm, "mix48", g.regs))


# ---- 9. Python --------------------------------------------------------------------------------------------------------------------
def test_stream_detector_with_bands(native, ctxs, heads, caplog):
    from softspoken_amd.stream import StreamDetector
    made = []

    def factory(p):
        made.append(T._head_ctx(native, heads["spread"], p))
        return made[-1]
    det = StreamDetector(context_factory=factory, precision="f16x2")
    try:
        pcm = rec("each48")
        ref_ctx = ctxs("spread", "f16x2")
        thr = median_threshold(native, ref_ctx, "each48", ("spread", "f16x2", "each48"))
        s = det.open(native.PCM_S16, 48000, 2, threshold=thr, break_s=0.05, channel_mode="each", bands=dict(profile=True))
        plain = det.open(native.PCM_S16, 48000, 2, threshold=thr, break_s=0.05)
        regs, bands, profs = [], [], []
        for at in range(0, len(pcm), 24000):
            s.push(pcm[at:at + 24000]); plain.push(pcm[at:at + 24000])
            res = det.step()
            assert len(res[plain]) == 3 and len(res[s]) == 4
            assert res[s][3].tobytes() == s.bands().tobytes() and res[s][3].shape == (len(res[s][0]), 2)
            regs += res[s][0]; bands.append(res[s][3]); profs.append(s.band_profiles())
        s.close(); plain.close()
        res = det.step()
        regs += res[s][0]; bands.append(res[s][3]); profs.append(s.band_profiles())
        fid = ref_ctx.reset() or ref_ctx.add_pcm_channels(_bytes(pcm), native.PCM_S16, 48000, 2, len(pcm))
        ref_ctx.run(thr, 0.05)
        assert regs == ref_ctx.regions_union(fid, 2) and len(regs) >= 3
        want, wprof = ref_ctx.region_bands(fid, regs, 2, profile=True)
        assert np.concatenate(bands).tobytes() == want.tobytes() and np.concatenate(profs).tobytes() == wprof.tobytes()
        # _move keeps the mode: the image carries it
        s2 = det.open(native.PCM_S16, 16000, 1, threshold=thr, bands=True)
        s2.push(rec("mono16")[:8000])
        det._move(s2)
        assert s2.precision == "fp32" and s2.band_params is not None
        s2.push(rec("mono16")[8000:]); s2.close()
        res = det.step()
        assert len(res[s2]) == 4 and res[s2][3].shape == (len(res[s2][0]), 1) and len(res[s2][0]) >= 1
        # ... and on a finished band stream the user has not freed (what a second refused step does to every stream)
        assert s.info()["finished"] == 1
        det._move(s)
        res = det.step()
        assert s.precision == "fp32" and res[s][0] == [] and res[s][3].shape == (0, 2)
    finally:
        det.close()


def test_move_carries_the_band_state(native, ctxs, heads):
    """_move in the middle of a recording, with accumulators, snapshot and map sums alive.  On an fp32 detector the move is an export
    and import on one context, so everything after it must still be the fp32 whole-file bytes."""
    from softspoken_amd.stream import StreamDetector
    ctx = ctxs("spread", "fp32")
    det = StreamDetector(context_factory=lambda p: ctx, precision="fp32")
    pcm = rec("each48")
    thr = median_threshold(native, ctx, "each48", ("spread", "fp32", "each48"))
    s = det.open(native.PCM_S16, 48000, 2, threshold=thr, break_s=0.5, channel_mode="each", bands=dict(profile=True))
    regs, bands, profs = [], [], []
    pieces = list(range(0, len(pcm), 12000))
    moved_with_state = 0
    for k, at in enumerate(pieces):
        s.push(pcm[at:at + 12000])
        res = det.step()
        regs += res[s][0]; bands.append(res[s][3]); profs.append(s.band_profiles())
        if k % 5 == 4:                                                # mid-region, mid-gap, wherever the cadence falls
            before = s.info()["state_bytes"]
            moved_with_state += before > 2 * 5 * 256 * 8 + 100_000
            det._move(s)
            assert s.info()["state_bytes"] == before and s.band_params is not None
    s.close()
    res = det.step()
    regs += res[s][0]; bands.append(res[s][3]); profs.append(s.band_profiles())
    det.free(s)
    assert moved_with_state >= 3
    assert regs == whole_table(native, ctx, pcm, "each48", thr, 0.5) and len(regs) >= 2
    want, wprof = reference(native, ctx, pcm, "each48", regs)
    assert np.concatenate(bands).tobytes() == want.tobytes() and np.concatenate(profs).tobytes() == wprof.tobytes()


class _NoContext:
    def set_window_step(self, step):
        pass


def test_a_window_step_other_than_the_default_is_a_value_error_where_open_is_called(native):
    from softspoken_amd.stream import StreamDetector
    with pytest.raises(ValueError):
        StreamDetector(context_factory=lambda p: _NoContext(), precision="fp32", step=0.3).open(native.PCM_S16, 16000, 1, bands=True)
    with pytest.raises(ValueError):
        StreamDetector(context_factory=lambda p: _NoContext(), precision="fp32").open(native.PCM_S16, 16000, 1, bands=dict(q=1))


# ---- 10. the structure of a step ------------------------------------------------------------------------------------------------
# A context whose passes hold four windows: a band lane's windows of one step span several passes, passes are shared by lanes of
# different streams, and one band stream is stepped before its first push.  What the streams return is the whole-file bytes; what
# every step launches is held to the table recorded before the step was split into layout, run and commit
# (tests/golden/stream_step_plan.json, tests/golden/make_stream_step_plan.py).
STEP_PLAN_SECONDS = 8.0
STEP_PLAN_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_step_plan.json")
# name: (layout, bands, piece seconds, the round of its first push)
STEP_PLAN_STREAMS = {"band_each": ("each48", True, 0.5, 0), "plain": ("mono16", False, 1.3, 0), "band_late": ("mix48", True, 0.9, 3)}


def step_plan_threshold(native, ctx):
    fid, n = add_whole(native, ctx, rec("each48", STEP_PLAN_SECONDS), "each48")
    ctx.run(0.1, 0.5)
    return float(np.median(np.fmax.reduce(np.asarray([ctx.avg(fid + c)[0] for c in range(n)]), axis=0)))


def step_plan_run(native, ctx, thr):
    """The three streams, every one pushed a piece per round from its first round on, one step per round on a profiling context of
    chunk 4; -> ({name: (Got, every lane's averages step by step)}, [[[kernel, launches, bytes], ...] per step])."""
    st = {}
    for name, (layout, bands, piece, first) in STEP_PLAN_STREAMS.items():
        sr, ch, each = LAYOUTS[layout]
        st[name] = dict(sid=open_stream(native, ctx, layout, thr, 0.05, bands, True), at=0, pcm=rec(layout, STEP_PLAN_SECONDS), n=int(piece * sr),
                        first=first, got=Got(ch if each else 1, ch, bands, True), lane_avg=[[] for _ in range(ch if each else 1)], closed=False)
    table, rnd = [], 0
    while not all(s["closed"] for s in st.values()):
        for s in st.values():
            if s["closed"] or rnd < s["first"]:
                continue
            n = min(s["n"], len(s["pcm"]) - s["at"])
            ctx.stream_push(s["sid"], s["pcm"][s["at"]:s["at"] + n], frames=n)
            s["at"] += n
            if s["at"] == len(s["pcm"]):
                ctx.stream_close(s["sid"]); s["closed"] = True
        ctx.reset_stats()
        ctx.stream_step()
        table.append([[k["name"], int(k["launches"]), float(k["bytes"])] for k in ctx.kernel_stats()])
        for s in st.values():
            s["got"].take(ctx, s["sid"], rnd)
            for c, lane in enumerate(s["lane_avg"]):
                lane.append(ctx.stream_avg_channel(s["sid"], c)[0])
        rnd += 1
    for s in st.values():
        assert ctx.stream_info(s["sid"])["finished"] == 1
        ctx.stream_free(s["sid"])
    return {name: (s["got"], s["lane_avg"]) for name, s in st.items()}, table


def test_step_structure_chunk_4(native, ctxs):
    ctx = ctxs("spread", "fp32", "chunk4", chunk=4, profile=True)
    thr = step_plan_threshold(native, ctx)
    got, table = step_plan_run(native, ctx, thr)
    maps = [sum(n for name, n, _ in step if name == "stream_map_kernel") for step in table]
    print("STREAM_STEP_PLAN steps:", len(table), "stream_map_kernel launches per step:", maps)
    assert max(maps) >= 3                                              # band windows of one step over several passes
    for name, (layout, bands, _, _) in STEP_PLAN_STREAMS.items():
        (g, lane_avg), pcm = got[name], rec(layout, STEP_PLAN_SECONDS)
        fid, n = add_whole(native, ctx, pcm, layout)
        ctx.run(thr, 0.05)
        assert g.regs == (ctx.regions_union(fid, n) if n > 1 else ctx.regions(fid)) and len(g.regs) >= 1, name
        for c in range(n):                                            # the averages of every lane, bit for bit
            a, i = ctx.avg(fid + c)
            assert np.array_equal(np.concatenate(g.idx), i) and np.concatenate(lane_avg[c]).tobytes() == a.tobytes(), (name, c)
        if bands:
            assert_bytes(g, reference(native, ctx, pcm, layout, g.regs), name)
    with open(STEP_PLAN_GOLDEN) as f:
        want = json.load(f)["steps"]
    assert len(table) == len(want)
    for k, (a, b) in enumerate(zip(table, want)):
        assert a == b, (k, a, b)
