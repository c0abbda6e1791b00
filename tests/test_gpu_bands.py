"""Region bands on a real MI355X (include/softspoken.h "region bands"): ss_region_bands_from_maps on crafted
maps against the long-double reference of tests/bands_ref.py (profiles to its bound, band indices equal), the cuts into pieces, the
call through the network against the device's own maps and against the CPU oracle network's, the each-channel form, the state rules
and that nothing of it runs when it is off.

A test prints its worst ratio of profile error to bound as `BANDS ratio ...`; DESIGN.md section 18 records them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bands_ref as B
import separation_ref as R
import test_gpu_separation as T

pytestmark = pytest.mark.gpu

FIRST = 1000                                                      # crafted maps: bins 1000 .. 1199, tiles cut at 1024, 1088, 1152
NB = 200


def t_of(j):
    """bin j's boundary in seconds: between the centres of bins j - 1 and j"""
    return j * 3 / 256 - 3


def _bins(a, b):
    return (t_of(a), t_of(b))


CRAFTED_REGIONS = [
    _bins(1010, 1011),                                            # 1 bin
    _bins(1024, 1087), _bins(1025, 1088),                         # 63 bins ending before / on an absolute multiple of 64
    _bins(1024, 1088), _bins(1024, 1089),                         # 64 bins: one whole tile; 65: one bin past it
    _bins(1100, 1120),                                            # inside one tile, from its middle
    (-3.0, t_of(1005)),                                           # from the start of all bins: clamped to the first that exists
    (t_of(1199), 99.0),                                           # the last bin, end beyond it
    _bins(1030, 1100), _bins(1060, 1130),                         # two that overlap
    _bins(1020, 1160),                                            # four tiles
    _bins(1030, 1100),                                            # the first of the pair again: an identical row
    (1.0, 1.0),                                                   # empty
    (50.0, 60.0), (-3.0, -2.9),                                   # wholly outside
    (0.0, 200.0),                                                 # everything
]


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


@pytest.fixture(scope="module")
def audio_ctx(native):
    """ss_region_bands_from_maps needs a device, no weights"""
    c = native.Context(None, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def heads(sd_np):
    return dict(spread=R.spread_head(sd_np), mixed=R.mixed_head(sd_np))


_CTX = {}


@pytest.fixture(scope="module")
def head_ctx(native, heads):
    def get(head, prec):
        if (head, prec) not in _CTX:
            _CTX[(head, prec)] = T._head_ctx(native, heads[head], prec, profile=(head, prec) == ("spread", "fp32"))
        return _CTX[(head, prec)]
    yield get
    for c in _CTX.values():
        c.close()
    _CTX.clear()


# ---- crafted maps ---------------------------------------------------------------------------------------------------------------
def _smooth(seed, n_bins=NB, top=3.5):
    """[2][n_bins][128] in [0, top]: a few random sinusoids over bins and bands"""
    rng = np.random.default_rng(seed)
    j, m = np.arange(n_bins)[None, :, None], np.arange(128)[None, None, :]
    y = np.zeros((2, n_bins, 128))
    for _ in range(6):
        a, b, p, q = rng.uniform(0.01, 0.2), rng.uniform(0.02, 0.3), rng.uniform(0, 6.3, (2, 1, 1)), rng.uniform(0, 6.3, (2, 1, 1))
        y += rng.uniform(0.3, 1.0) * np.sin(a * j + p) * np.cos(b * m + q)
    y = (y - y.min()) / (y.max() - y.min()) * top
    return y.astype(np.float32)


def _contents():
    c = {}
    c["smooth"] = _smooth(1)
    c["zeros"] = np.zeros((2, NB, 128), dtype=np.float32)
    one = np.zeros((2, NB, 128), dtype=np.float32)
    one[1, :, 37] = _smooth(2)[1, :, 37] + 0.1
    one[0] = _smooth(2)[0]
    c["one_band"] = one
    c["tiny"] = np.full((2, NB, 128), 1e-20, dtype=np.float32)
    cap = _smooth(3, top=2.0)
    cap[1, 40:42, 20] = 20.0                                      # y^2 ln 10 = 921 > 600, in two bins no region boundary separates
    cap[1, 95, 90] = np.inf
    cap[0, 150, 5] = np.inf
    c["cap"] = cap
    nans = _smooth(4)
    rng = np.random.default_rng(5)
    nans[rng.random(nans.shape) < 0.05] = np.nan
    nans[1, 12, :] = np.nan                                       # a whole row of a one-bin region's neighbour
    c["nans"] = nans
    eq = _smooth(6, top=1.75)
    eq[1, :, 50] = 2.5 + 0.3 * _smooth(7)[1, :, 3] / 3.5
    eq[1, :, 70] = eq[1, :, 50]                                   # bit-equal columns, both above every other band
    c["equal_bands"] = eq
    cut = _smooth(8)
    cut[:, :, 100:] = 0.0                                         # no power from band 100 on
    c["cut"] = cut
    return c


CONTENTS = _contents()
# (the two signals of one call, designed exact ties per signal: decisions that must still be equal -- equal inputs give equal sums)
CRAFTED_CASES = [("smooth", "zeros", (), ()), ("one_band", "tiny", (), ("peak",)), ("cap", "nans", (), ()),
                 ("equal_bands", "cut", ("peak",), ())]
_RATIOS = []


def _check_signal(native, got, prof, maps, first, regions, label, designed=(), max_ties=0, **params):
    """One signal's rows against the reference: n_bins, profile to the bound, indices, the frequencies of the device's own indices,
    the share.  A decision near a tie may land on a neighbour, but at most one region of a whole test case may be near a tie that
    was not designed: the crafted maps are chosen so that the reference finds none (max_ties = 0 for every call on them); the network
    case calls this region by region with max_ties = 1 and counts over its regions itself."""
    ref = B.reference(maps, first, regions, **params)
    hz = native.band_edges()
    sp = params.get("speech_channel", 1)
    worst, ties = 0.0, 0
    for i, (g, r) in enumerate(zip(got, ref)):
        assert int(g["n_bins"]) == r["n_bins"], (label, i)
        ratio = B.profile_error_ratio(prof[i], r["E"], r["bound"])
        worst = max(worst, ratio)
        assert ratio <= 1.0, (label, i, ratio)
        assert np.isfinite(prof[i]).all() and (prof[i] >= 0).all(), (label, i)
        if r["band_low"] < 0:
            assert (int(g["band_low"]), int(g["band_high"]), int(g["band_peak"])) == (-1, -1, -1), (label, i)
            assert all(np.isnan(g[k]) for k in ("low_hz", "high_hz", "peak_hz", "speech_share")), (label, i)
            continue
        tie = {k: v and k not in designed for k, v in r["ties"].items()}
        ties += any(tie.values())
        top2 = set(np.argsort(np.asarray(r["E"][sp], dtype=np.float64), kind="stable")[-2:].tolist())
        for k in ("low", "high"):
            d = abs(int(g["band_" + k]) - r["band_" + k])
            assert d == 0 or (tie[k] and d == 1), (label, i, k, int(g["band_" + k]), r["band_" + k])
        assert int(g["band_peak"]) == r["band_peak"] or (tie["peak"] and int(g["band_peak"]) in top2), (label, i)
        assert g["low_hz"] == hz[g["band_low"]] and g["high_hz"] == hz[g["band_high"] + 2] and g["peak_hz"] == hz[g["band_peak"] + 1]
        tol = 2 * (r["bound"] + 128 * B.EPS) + 2 * B.EPS          # T and T_env: the profile's bound and a 128-term sequential sum each
        assert abs(g["speech_share"] - r["speech_share"]) <= tol * r["speech_share"] + 1e-300, (label, i)
    assert ties <= max_ties, (label, ties)
    _RATIOS.append((label, worst))
    print(f"BANDS ratio {label}: worst profile error / bound = {worst:.4f} over {len(regions)} regions")
    return ref


@pytest.mark.parametrize("a,b,des_a,des_b", CRAFTED_CASES)
def test_crafted_maps_against_the_reference(native, audio_ctx, a, b, des_a, des_b):
    maps = np.stack([CONTENTS[a], CONTENTS[b]])
    got, prof = audio_ctx.region_bands_from_maps(maps, FIRST, CRAFTED_REGIONS, profile=True)
    assert got.shape == (len(CRAFTED_REGIONS), 2) and prof.shape == (len(CRAFTED_REGIONS), 2, 2, 128)
    refs = [_check_signal(native, got[:, s], prof[:, s], maps[s], FIRST, CRAFTED_REGIONS, f"crafted {n}", designed=d)
            for s, (n, d) in enumerate(((a, des_a), (b, des_b)))]
    want_bins = [1, 63, 63, 64, 65, 20, 5, 1, 70, 70, 140, 70, 0, 0, 0, NB]
    assert [int(x) for x in got["n_bins"][:, 0]] == want_bins
    assert got[8].tobytes() == got[11].tobytes() and prof[8].tobytes() == prof[11].tobytes()       # the region listed twice
    got2, prof2 = audio_ctx.region_bands_from_maps(maps, FIRST, CRAFTED_REGIONS, profile=True)
    assert got.tobytes() == got2.tobytes() and prof.tobytes() == prof2.tobytes()                   # two calls, identical bytes
    assert audio_ctx.region_bands_from_maps(maps, FIRST, CRAFTED_REGIONS).tobytes() == got.tobytes()   # without the profile
    for s, name in enumerate((a, b)):
        est = np.array([r["band_low"] >= 0 for r in refs[s]])
        if name == "zeros":
            assert not est.any()                                  # all zero: no estimate anywhere
        else:
            assert est.tolist() == [n > 0 for n in want_bins], name
        if name == "one_band":
            for q in ((0.05, 0.95), (0.5, 1.0), (0.999, 1.0)):    # one band with power: low = high = peak = that band for any q
                g = audio_ctx.region_bands_from_maps(maps[s], FIRST, CRAFTED_REGIONS, q_low=q[0], q_high=q[1])
                assert all((int(x["band_low"]), int(x["band_high"]), int(x["band_peak"])) == (37, 37, 37) for x in g[est]), q
        if name == "tiny":
            assert all((int(x["band_low"]), int(x["band_high"]), int(x["band_peak"])) == (6, 121, 0) for x in got[est, s])
        if name == "equal_bands":
            assert all(int(x["band_peak"]) == 50 for x in got[est, s])                              # the lower of the two equal bands
        if name == "cap":
            capv = float(np.expm1(np.float64(600.0)))
            assert prof[15, s, 1, 20] >= 2 * capv * (1 - 1e-12) and prof[15, s, 1, 90] >= capv * (1 - 1e-12)
            assert prof[15, s, 0, 5] >= capv * (1 - 1e-12) and np.isfinite(prof[:, s]).all()
            assert (int(got[15, s]["band_low"]), int(got[15, s]["band_high"]), int(got[15, s]["band_peak"])) == (20, 90, 20)
        if name == "nans":
            assert prof[0, s].sum() > 0                           # the NaN cells add nothing, the others count


def test_crafted_maps_parameters(native, audio_ctx):
    maps = CONTENTS["cut"]
    # q_high = 1: the last band with power
    got, prof = audio_ctx.region_bands_from_maps(maps, FIRST, CRAFTED_REGIONS, q_high=1.0, profile=True)
    _check_signal(native, got, prof, maps, FIRST, CRAFTED_REGIONS, "crafted cut q_high=1", designed=("high",), q_high=1.0)
    est = got["band_low"] >= 0
    assert est.sum() == 13 and (got["band_high"][est] == 99).all()
    # other quantiles
    sm = CONTENTS["smooth"]
    got, prof = audio_ctx.region_bands_from_maps(sm, FIRST, CRAFTED_REGIONS, q_low=0.25, q_high=0.5, profile=True)
    _check_signal(native, got, prof, sm, FIRST, CRAFTED_REGIONS, "crafted smooth q=.25/.5", q_low=0.25, q_high=0.5)
    # speech_channel = 0 swaps the roles: the reference with channel 0, and the swapped maps with channel 1 give the same rows
    got0, prof0 = audio_ctx.region_bands_from_maps(sm, FIRST, CRAFTED_REGIONS, speech_channel=0, profile=True)
    _check_signal(native, got0, prof0, sm, FIRST, CRAFTED_REGIONS, "crafted smooth speech_channel=0", speech_channel=0)
    got1, prof1 = audio_ctx.region_bands_from_maps(np.ascontiguousarray(sm[::-1]), FIRST, CRAFTED_REGIONS, profile=True)
    assert got0.tobytes() == got1.tobytes() and np.array_equal(prof0, prof1[:, ::-1])
    base = audio_ctx.region_bands_from_maps(sm, FIRST, CRAFTED_REGIONS)
    assert got0.tobytes() != base.tobytes()
    # n = 0, and maps that begin at bin 0: start = -3 is bin 0 itself
    assert audio_ctx.region_bands_from_maps(sm, FIRST, []).shape == (0,)
    low = _smooth(9, n_bins=70)
    regs = [(-3.0, t_of(3)), (-5.0, t_of(1)), _bins(0, 64), _bins(0, 65), _bins(63, 70), (-3.0, -3.0)]
    got, prof = audio_ctx.region_bands_from_maps(low, 0, regs, profile=True)
    _check_signal(native, got, prof, low, 0, regs, "crafted bins from 0")
    assert [int(x) for x in got["n_bins"]] == [3, 1, 64, 65, 7, 0]
    for bad in (dict(q_low=0.0), dict(q_low=0.5, q_high=0.5), dict(q_high=1.5), dict(speech_channel=2)):
        with pytest.raises(native.NativeError) as e:
            audio_ctx.region_bands_from_maps(sm, FIRST, CRAFTED_REGIONS, **bad)
        assert e.value.code == native.SS_ERR_ARG
    with pytest.raises(native.NativeError) as e:
        audio_ctx.region_bands_from_maps(sm, FIRST, [(0.0, 1.0), (2.0, 1.5)])
    assert e.value.code == native.SS_ERR_ARG


# ---- pieces ---------------------------------------------------------------------------------------------------------------------
NET_SECONDS, NET_SEED, NET_SR = 12.0, 71, 48000
# (with the CPU oracle alone -- its own resampler's signal -- every one of these passes bands_ref.map_error_margins on both heads)
NET_REGIONS = [(-1.0, 0.4), (0.7, 0.73), (0.0, 2.0), (1.0, 3.5), (2.0, 2.7), (4.0, 9.5), (9.0, 14.0), (11.9, 12.5), (20.0, 21.0)]

_PIECES_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from softspoken_amd import synth, native
import separation_ref as R
import test_gpu_separation as T
import test_gpu_bands as TB
ctx = T._head_ctx(native, R.spread_head(synth.make_state_dict(0)), profile=True)
data, info, x, _ = T._make("pcm16", 16000, 1, TB.NET_SECONDS, TB.NET_SEED, scale=0.5)
fid = ctx.add_pcm(data, info.format, 16000, 1, info.frames)
b0, cnt = native.region_bins(0.0, 2.0, 10 ** 6)
assert (b0 + cnt - 1) // 64 - b0 // 64 == 2                          # the region (0, 2) s lies across three tiles
def run(budget):
    ctx.debug_set_bands_budget(budget)
    ctx.reset_stats()
    out, prof = ctx.region_bands(fid, TB.NET_REGIONS, profile=True)
    st = {{k["name"]: k["launches"] for k in ctx.kernel_stats()}}
    return out, prof, st.get("band_profile_kernel", 0), st.get("band_bounds_kernel", 0)
want, wprof, n_prof, n_bounds = run(0)
assert (n_prof, n_bounds) == (1, 1) and (want["band_low"] >= 0).sum() >= 7
for budget, least in ((64, 12), (128, 6), (1, 12)):
    got, gprof, n_prof, n_bounds = run(budget)
    assert n_prof >= least and n_bounds == 1, (budget, n_prof)
    assert got.tobytes() == want.tobytes() and gprof.tobytes() == wprof.tobytes(), budget
print("PIECES_OK")
"""


def test_pieces_cut_at_tile_boundaries_give_the_same_bytes(build_all):
    """ss_debug_set_bands_budget (development build) at 64 and 128 bins -- a dozen rounds of passes, a region's tile sums waiting on the
    device across them -- gives the default budget's out and profile, bit for bit."""
    from softspoken_amd import build as hip_build
    tests = os.path.dirname(os.path.abspath(__file__))
    e = dict(os.environ)
    e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
    r = subprocess.run([sys.executable, "-c", _PIECES_SCRIPT.format(root=os.path.dirname(tests), tests=tests)], env=e, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "PIECES_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


# ---- through the network --------------------------------------------------------------------------------------------------------
_NET = {}


def _net_rec():
    if "rec" not in _NET:
        _NET["rec"] = T._make("pcm16", NET_SR, 2, NET_SECONDS, NET_SEED, scale=0.5)
    return _NET["rec"]


def _oracle_maps(heads, head, padded, W):
    """The CPU oracle network's spec maps of every window of the recording (once per head)."""
    if ("oracle", head) not in _NET:
        spec = R._oracle_spec(heads[head], padded, list(range(W)))
        _NET[("oracle", head)] = {i: spec[i] for i in range(W)}
    return _NET[("oracle", head)]


@pytest.mark.parametrize("head", ["spread", "mixed"])
@pytest.mark.parametrize("prec", ["fp32", "f16x2"])
def test_through_the_network(native, heads, head_ctx, head, prec):
    ctx = head_ctx(head, prec)
    data, info, x, _ = _net_rec()
    ctx.set_chunk(16)
    try:
        ctx.reset()
        fid = ctx.add_pcm(data, info.format, NET_SR, 2, info.frames)
        W, n_bins = R.file_geometry(NET_SR, info.frames)
        assert W > 16                                             # more than one pass
        got, prof = ctx.region_bands(fid, NET_REGIONS, profile=True)
        assert got.shape == (len(NET_REGIONS),) and prof.shape == (len(NET_REGIONS), 2, 128)
        # (a) against the reference on the device's own maps of the same bins
        worst, ties = 0.0, 0
        for i, reg in enumerate(NET_REGIONS):
            b0, cnt = native.region_bins(reg[0], reg[1], n_bins)
            assert (b0, cnt) == B.region_bins(reg[0], reg[1], 0, n_bins) and int(got[i]["n_bins"]) == cnt
            if cnt == 0:
                assert int(got[i]["band_low"]) == -1 and not prof[i].any()
                continue
            maps = ctx.separation_maps(fid, b0, cnt)
            label = f"net {head}/{prec} region {i}"
            r = _check_signal(native, got[i:i + 1], prof[i:i + 1], maps, b0, [reg], label, max_ties=1)[0]
            ties += any(r["ties"].values())
        assert ties <= 1                                          # over the regions of the case
        assert (got["band_low"] >= 0).sum() >= 6 and int(got[-1]["n_bins"]) == 0
        # (b) end to end against the CPU oracle network: equal decisions wherever a head error of 1e-4 cannot move them
        padded = ctx.read_signal(fid, padded=True)
        by_win = _oracle_maps(heads, head, padded, W)
        left_out, compared = 0, 0
        for i, reg in enumerate(NET_REGIONS):
            b0, cnt = B.region_bins(reg[0], reg[1], 0, n_bins)
            if cnt == 0:
                continue
            om = R.average_maps(by_win, range(b0, b0 + cnt))
            r = B.reference(om, b0, [reg])[0]
            safe = B.map_error_margins(om, b0, reg)
            if r["band_low"] < 0:                                 # the oracle sees no speech power at all: so must the device
                assert int(got[i]["band_low"]) == -1, (head, prec, i)
                continue
            if not all(safe.values()):
                left_out += 1
                continue
            compared += 1
            assert (int(got[i]["band_low"]), int(got[i]["band_high"]), int(got[i]["band_peak"])) == \
                (r["band_low"], r["band_high"], r["band_peak"]), (head, prec, i)
        print(f"BANDS oracle {head}/{prec}: {compared} regions compared, {left_out} under the margin")
        assert left_out <= 2 and compared >= 4
    finally:
        ctx.set_chunk(1024)


# ---- each-channel form ----------------------------------------------------------------------------------------------------------
def test_each_channel_form_equals_the_channels_alone(native, head_ctx):
    ctx = head_ctx("spread", "fp32")
    sr = 16000
    rec = T._make("pcm16", sr, 2, 6.0, 72, scale=0.5)
    data, info, x, _ = rec
    regions = [(-1.0, 0.4), (0.0, 2.0), (1.5, 1.52), (3.0, 7.0), (9.0, 10.0)]
    ctx.reset()
    first = ctx.add_pcm_channels(data, info.format, sr, 2, info.frames)
    got, prof = ctx.region_bands(first, regions, 2, profile=True)
    assert got.shape == (len(regions), 2) and prof.shape == (len(regions), 2, 2, 128)
    assert got[:, 0].tobytes() != got[:, 1].tobytes() and (got["band_low"][:4] >= 0).all()
    for c in range(2):
        mono = T._pack(np.ascontiguousarray(x[:, c:c + 1]), "pcm16", sr)
        ctx.reset()
        fid = ctx.add_pcm(mono[0], mono[1].format, sr, 1, mono[1].frames)
        one, oprof = ctx.region_bands(fid, regions, 1, profile=True)
        assert one.tobytes() == np.ascontiguousarray(got[:, c]).tobytes(), c
        assert oprof.tobytes() == np.ascontiguousarray(prof[:, c]).tobytes(), c
    # two equal channels: two equal columns
    twin = T._pack(np.ascontiguousarray(np.repeat(x[:, 0:1], 2, axis=1)), "pcm16", sr)
    ctx.reset()
    first = ctx.add_pcm_channels(twin[0], twin[1].format, sr, 2, twin[1].frames)
    tw, tprof = ctx.region_bands(first, regions, 2, profile=True)
    assert np.ascontiguousarray(tw[:, 0]).tobytes() == np.ascontiguousarray(tw[:, 1]).tobytes()
    assert np.array_equal(tprof[:, 0], tprof[:, 1]) and np.ascontiguousarray(tw[:, 0]).tobytes() == np.ascontiguousarray(got[:, 0]).tobytes()
    # files that are not the channels of one recording
    ctx.add_pcm(data[: len(data) // 2], info.format, sr, 2, info.frames // 2)
    with pytest.raises(native.NativeError) as e:
        ctx.region_bands(first + 1, regions, 2)
    assert e.value.code == native.SS_ERR_ARG
    with pytest.raises(native.NativeError) as e:
        ctx.region_bands(first, regions, 4)
    assert e.value.code == native.SS_ERR_ARG


# ---- state and refusals ---------------------------------------------------------------------------------------------------------
def test_state_rules_and_refusals(native, audio_ctx, head_ctx):
    from softspoken_amd import synth
    sr = 16000
    data, info, x, _ = T._make("pcm16", sr, 1, 6.0, 73, scale=0.5)
    regions = [(0.0, 2.0), (3.0, 3.5)]
    fid = audio_ctx.add_pcm(data, info.format, sr, 1, info.frames)
    with pytest.raises(native.NativeError) as e:
        audio_ctx.region_bands(fid, regions)
    assert e.value.code == native.SS_ERR_STATE                    # audio-only
    audio_ctx.reset()
    ctx = head_ctx("spread", "fp32")
    ctx.reset()
    fid = ctx.add_pcm(data, info.format, sr, 1, info.frames)
    ctx.run_begin()
    try:
        with pytest.raises(native.NativeError) as e:
            ctx.region_bands(fid, regions)
        assert e.value.code == native.SS_ERR_STATE                # a run in flight
        with pytest.raises(native.NativeError) as e:
            ctx.region_bands_from_maps(CONTENTS["smooth"], FIRST, CRAFTED_REGIONS)
        assert e.value.code == native.SS_ERR_STATE
    finally:
        ctx.run_end()
    table = ctx.regions(fid)
    ctx.avg(fid)
    gen = ctx.reset_generation()
    want = ctx.region_bands(fid, regions)
    assert ctx.regions(fid) == table and ctx.reset_generation() == gen         # the run's table stays; nothing was reset
    for read in (ctx.avg, ctx.window_logits):                                  # the run's device buffers went to the passes
        with pytest.raises(native.NativeError) as e:
            read(fid)
        assert e.value.code == native.SS_ERR_STATE
    assert ctx.region_bands(fid, []).shape == (0,)
    with pytest.raises(native.NativeError) as e:
        ctx.region_bands(fid + 1, regions)
    assert e.value.code == native.SS_ERR_ARG
    # the window step of the context does not reach the bands
    ctx.set_window_step(0.3)
    try:
        ctx.reset()
        fid = ctx.add_pcm(data, info.format, sr, 1, info.frames)
        assert ctx.region_bands(fid, regions).tobytes() == want.tobytes()
    finally:
        ctx.set_window_step(0.6)
    # a NaN sample: f16x2 refuses, fp32 answers
    y = (0.5 * synth.synth_audio(61, 4.0, sr, 1, with_silence=False).T.reshape(-1, 1)).astype(np.float32)
    y[sr * 2, 0] = np.float32("nan")
    wav = synth.wav_bytes(y, sr, "f32")
    winfo = native.wav_parse(wav)
    raw = np.frombuffer(wav, dtype=np.uint8, count=winfo.data_bytes, offset=winfo.data_offset)
    f16 = head_ctx("spread", "f16x2")
    f16.reset()
    fid = f16.add_pcm(raw, winfo.format, sr, 1, winfo.frames)
    with pytest.raises(native.NativeError) as e:
        f16.region_bands(fid, [(1.5, 2.5)])
    assert e.value.code == native.SS_ERR_RANGE
    ctx.reset()
    fid = ctx.add_pcm(raw, winfo.format, sr, 1, winfo.frames)
    ok = ctx.region_bands(fid, [(1.5, 2.5), (3.9, 3.95)])
    assert ok.shape == (2,) and int(ok[0]["n_bins"]) == 85


# ---- nothing new when off -------------------------------------------------------------------------------------------------------
def test_no_band_kernel_in_a_detection_or_a_separation_run(native, head_ctx):
    ctx = head_ctx("spread", "fp32")                              # (created with SS_FLAG_PROFILE)
    data, info, x, _ = T._make("pcm16", 16000, 2, 6.0, 74, scale=0.5)
    ctx.reset()
    ctx.reset_stats()
    fid = ctx.add_pcm(data, info.format, 16000, 2, info.frames)
    assert ctx.run()
    ctx.separate_pcm(data, info.format, 16000, 2, info.frames, [(0.5, 1.5)])
    ctx.separate_pcm_channels(data, info.format, 16000, 2, info.frames, [(0.5, 1.5)])
    names = [k["name"] for k in ctx.kernel_stats()]
    assert names and not [n for n in names if n.startswith("band_")], names
    ctx.region_bands(0, [(0.5, 1.5)], 2)
    st = {k["name"]: k["launches"] for k in ctx.kernel_stats()}
    assert st.get("band_profile_kernel") == 1 and st.get("band_bounds_kernel") == 1, st


class _PM:
    def __init__(self, files, detections_file):
        self.files = files
        self.current_project = {'detections_file': detections_file}

    def get_unprocessed_list(self):
        return list(self.files)


def _run_worker(files, csv, ck):
    from root.code.frontend.NNDetector import NNDetector
    from root.code.backend.worker import ProcessWorker
    from softspoken_amd.detections import DetectionProject
    pm = _PM(files, csv)
    det = NNDetector(pm, checkpoint_path=ck)
    w = ProcessWorker(det, DetectionProject(pm), det.plan_detection_job())
    msgs = []
    w.signals.message.connect(msgs.append)
    w.run()
    assert not msgs, msgs
    side = os.path.splitext(csv)[0] + "_bands.csv"
    return open(csv).read(), (open(side).read() if os.path.exists(side) else None), det


def test_drop_in_writes_the_side_file_only_when_on(native, tmp_path, monkeypatch):
    from root.code.backend import settings
    from root.code.backend.voice_activity import add_file_to_context
    from softspoken_amd import synth
    d = tmp_path / "site"
    d.mkdir()
    files = []
    for name, seed, secs, sr, ch in (("mono.wav", 1001, 20.0, 16000, 1), ("st.wav", 3004, 20.0, 48000, 2)):
        xs = synth.synth_audio(seed, secs, sr, ch)
        (d / name).write_bytes(synth.wav_bytes(synth.to_pcm16(xs if ch > 1 else xs[0]), sr))
        files.append(str(d / name))
    ck = str(d / "model_checkpoint.pth")
    synth.save_checkpoint(ck, 0, epoch=0)
    monkeypatch.delenv("SOFTSPOKEN_BANDS", raising=False)
    monkeypatch.setattr(settings, "hip_region_bands", "0")
    off, off_side, det_off = _run_worker(files, str(tmp_path / "off.csv"), ck)
    assert off_side is None and det_off.band_detail == {}
    monkeypatch.setattr(settings, "hip_region_bands", "1")
    on, on_side, det = _run_worker(files, str(tmp_path / "on.csv"), ck)
    assert on == off and on_side is not None and len(on.splitlines()) > 1
    lines = on_side.splitlines()
    assert lines[0] == "ID,file_name,channel,low_hz,high_hz,peak_hz,speech_share,n_bins"
    assert [ln.split(",")[0] for ln in lines[1:]] == [ln.split(",")[0] for ln in on.splitlines()[1:]]
    # the rows are the library's for the same files on a context of the detector's precision
    ctx = det.model.hip_context()
    k = 1
    for f in files:
        ctx.reset()
        fid, info = add_file_to_context(ctx, f)
        assert ctx.run()
        reg = ctx.regions(fid)
        bands = ctx.region_bands(fid, reg)
        assert det.band_detail[f][0] == 0 and det.band_detail[f][1][:, 0].tobytes() == bands.tobytes()
        for b in bands:
            want = f"{k},{os.path.basename(f)},," + (",,,," if b["band_low"] < 0 else
                                                       "%.1f,%.1f,%.1f,%.6f," % (b["low_hz"], b["high_hz"], b["peak_hz"], b["speech_share"])) + str(int(b["n_bins"]))
            assert lines[k] == want
            k += 1
    assert k == len(lines)


@pytest.mark.parametrize("mode", ["mix", "each"])
def test_detect_files_over_several_files_with_bands_on(native, tmp_path, monkeypatch, mode):
    """The whole-job path: one run over three files on one context.  The first bands call takes the run's device buffers, so every
    file's regions and peaks are read before it; the regions are those of a job with the setting off, the bands the library's for
    each file run alone."""
    from root.code.backend import settings
    from root.code.backend.voice_activity import add_file_to_context
    from root.code.frontend.NNDetector import NNDetector
    from softspoken_amd import synth
    files = []
    for name, seed, secs, sr, ch in (("st_a.wav", 3004, 20.0, 48000, 2), ("mono.wav", 1001, 20.0, 16000, 1), ("st_b.wav", 3002, 20.0, 48000, 2)):
        xs = synth.synth_audio(seed, secs, sr, ch)
        (tmp_path / name).write_bytes(synth.wav_bytes(synth.to_pcm16(xs if ch > 1 else xs[0]), sr))
        files.append(str(tmp_path / name))
    ck = str(tmp_path / "model_checkpoint.pth")
    synth.save_checkpoint(ck, 0, epoch=0)
    monkeypatch.setattr(settings, "hip_channel_mode", mode)
    monkeypatch.setattr(settings, "hip_region_bands", "0")
    det = NNDetector(_PM(files, None), checkpoint_path=ck)
    off = det.detect_files(files)
    assert det.band_detail == {} and sum(len(r) for r in off.values()) >= 3
    monkeypatch.setattr(settings, "hip_region_bands", "1")
    on = det.detect_files(files)
    assert on == off and sorted(det.band_detail) == sorted(files)
    ctx = det.model.hip_context()
    for f in files:
        ctx.reset()
        fid, info = add_file_to_context(ctx, f)
        assert ctx.run()
        n_ch = info.channels if mode == "each" else 0
        reg = ctx.regions_union(fid, n_ch) if n_ch > 1 else ctx.regions(fid)
        assert [(float(s), float(e)) for s, e in reg] == on[f]
        if mode == "each":
            assert det.channel_detail[f] == (n_ch, ctx.region_peaks(fid, n_ch).tolist())
        bands = np.asarray(ctx.region_bands(fid, reg, max(n_ch, 1))).reshape(len(reg), max(n_ch, 1))
        got_ch, got = det.band_detail[f]
        assert got_ch == n_ch and got.shape == bands.shape and got.tobytes() == bands.tobytes(), f
