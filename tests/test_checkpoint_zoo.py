"""The checkpoint zoo (tests/checkpoint_zoo.py) on the CPU: every member is what it says it is, and is a checkpoint the GPU tests may
hold the device to the float64 oracle on.

Reference: oracle_np.unet_forward in float64 on the oracle's fp32 mel features of windows of the C1 recording.  Measured here (max over
the windows, logits / spec maps):

  member vs the seed-0 checkpoint, float64, windows 0, 20, 50 (only the fp32 rounding of the transformed weights is left):
      spread3   3.9e-7 / 1.2e-7        spread6   5.0e-7 / 1.5e-7        tinyvar   2.2e-7 / 1.1e-7
  asserted at 4 x these (SAME_BOUND); 1e-5 would already mean a wrong consumer column (one column of one conv off by a factor 10
  moves the logits by ~1e-2).

  fp32 oracle vs float64 oracle, the eight windows of the end-to-end GPU test, relative to max(1, max |ref|):
      seed7     2.2e-6 / 1.2e-6        spread3   2.5e-6 / 1.1e-6        spread6   2.6e-6 / 1.2e-6        signs    1.4e-6 / 1.1e-6
      dead      3.4e-6 / 7.4e-7        tinyvar   8.3e-6 / 2.8e-6        runaway   9.1e-6 / 1.0e-5
  asserted at 2.5e-5, a quarter of the project's 1e-4 bar: the device is held to 1e-4 of the float64 oracle, and that says something
  about the device only where the reference's own fp32 arithmetic is well inside it.  (max |ref| is 1.7 / 0.5 for the seed-0 function,
  3.1 / 1.2 for signs, 1.4e33 / 8e36 for runaway.)
"""
import numpy as np
import pytest
import torch

import checkpoint_zoo as Z
import layer_ref as R
from softspoken_amd import synth

SAME_BOUND = {"spread3": (4 * 3.9e-7, 4 * 1.2e-7), "spread6": (4 * 5.0e-7, 4 * 1.5e-7), "tinyvar": (4 * 2.2e-7, 4 * 1.1e-7)}
QUARTER_BAR = 2.5e-5
_WINDOWS = sorted(set(Z.E2E_WINDOWS) | set(Z.SAME_WINDOWS))


@pytest.fixture(scope="module")
def feats(c1):
    return Z.c1_features(c1, _WINDOWS)


@pytest.fixture(scope="module")
def ref64(feats):
    """name -> float64 oracle (logits, spec) on _WINDOWS, computed once per checkpoint."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Z.oracle(Z.build(name), feats)
        return cache[name]
    return get


def _at(a, windows):
    return a[[_WINDOWS.index(w) for w in windows]]


@pytest.mark.parametrize("name", list(SAME_BOUND))
def test_function_preserving_members_are_the_seed0_function(name, ref64):
    m0, s0 = ref64("seed0")
    m, s = ref64(name)
    dm = float(np.abs(_at(m, Z.SAME_WINDOWS) - _at(m0, Z.SAME_WINDOWS)).max())
    ds = float(np.abs(_at(s, Z.SAME_WINDOWS) - _at(s0, Z.SAME_WINDOWS)).max())
    print(f"{name} vs seed 0, float64: logits {dm:.3g}, spec {ds:.3g}")
    assert dm <= SAME_BOUND[name][0] and ds <= SAME_BOUND[name][1], (dm, ds)


@pytest.mark.parametrize("name", list(Z.members()))
def test_fp32_oracle_is_well_inside_the_bar(name, feats, ref64):
    """The condition the GPU tests rely on: the reference's own fp32 arithmetic is within a quarter of the 1e-4 bar of the float64 oracle
    (relative to max |ref| where that exceeds 1: signs, runaway)."""
    m, s = (_at(a, Z.E2E_WINDOWS) for a in ref64(name))
    m32, s32 = Z.oracle(Z.build(name), feats[[_WINDOWS.index(w) for w in Z.E2E_WINDOWS]], torch.float32)
    assert np.isfinite(m32).all() and np.isfinite(s32).all()
    dm = float(np.abs(m32 - m).max() / max(1.0, np.abs(m).max()))
    ds = float(np.abs(s32 - s).max() / max(1.0, np.abs(s).max()))
    print(f"{name} fp32 vs float64 oracle: logits {dm:.3g}, spec {ds:.3g} (max |ref| {np.abs(m).max():.3g}, {np.abs(s).max():.3g})")
    assert dm <= QUARTER_BAR and ds <= QUARTER_BAR, (dm, ds)


def test_consumer_table_agrees_with_the_hostile_checkpoint():
    """consumers() derives from GRAPH what synth._CONSUMERS states by hand for five blocks."""
    for block, cons in synth._CONSUMERS.items():
        want = sorted((f"{c}.{conv}.weight", lo) for c, lo, _ in cons for conv in ("conv1.0", "residual.0"))
        assert sorted(Z.consumers(block)) == want, block
    assert Z.consumers("conv9_1") == [("spec_output_conv.0.conv1.0.weight", 0), ("spec_output_conv.0.residual.0.weight", 0),
                                      ("conv_flatten.weight", 0)]
    assert Z.consumers("conv8") == [("conv9_1.conv1.0.weight", 32), ("conv9_1.residual.0.weight", 32)]


def test_members_are_deterministic_and_in_the_layout():
    lay = synth.state_dict_layout()
    for name in Z.members():
        a, b = Z.build(name), Z.build(name)
        assert list(a) == list(lay)
        for k, (shape, _) in lay.items():
            assert a[k].shape == tuple(shape) and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (name, k)
            assert np.isfinite(a[k]).all(), (name, k)


# ---- each property is really there after the fold ---------------------------------------------------------------------------------
def test_dead_has_zero_rows_with_and_without_bias():
    sd = Z.build("dead")
    for name, _, _ in Z.RESBLOCKS_2D:
        W, d = R.block_weights(sd, name), Z.dead_channels(name)
        assert not W["w1"][d["hidden_zero"]].any() and W["b1"][d["hidden_zero"]] == 0
        assert not W["w1"][d["hidden_const"]].any() and W["b1"][d["hidden_const"]] > 0
        for c, kind in ((d["out_clipped"], "clipped"), (d["out_zero"], "zero")):
            assert not W["w2"][c].any() and not W["wr"][c].any()
            assert (W["b2"][c] + W["br"][c] < 0) if kind == "clipped" else (W["b2"][c] == 0 and W["br"][c] == 0)
    ex = Z.exponent_chain(sd)
    for name, _, _, hn, yn in Z.GRAPH:                       # est == 0 -> exponent 0; a zero row with a bias has the bias's exponent
        d = Z.dead_channels(name)
        assert ex[hn][d["hidden_zero"]] == 0 and ex[yn][d["out_zero"]] == 0
        b = R.block_weights(sd, name)["b1"][d["hidden_const"]]
        assert ex[hn][d["hidden_const"]] == -int(torch.round(torch.log2(b)))


def test_signs_has_negative_folded_scales_in_every_batchnorm():
    sd, sd0 = Z.build("signs"), synth.make_state_dict(0)
    for bn in Z.BN_2D:
        conv = bn[:-1] + "0"
        flipped = np.sign(sd[bn + ".weight"]) != np.sign(sd0[bn + ".weight"])
        assert 0.15 < flipped.mean() < 0.55, (bn, flipped.mean())
        w, _ = R.fold(sd, conv, bn)
        w0, _ = R.fold(sd0, conv, bn)
        assert torch.equal(w[flipped], -w0[flipped]) and torch.equal(w[~flipped], w0[~flipped])
        assert (sd[bn + ".weight"] < 0).any()


def test_tinyvar_folds_to_the_seed0_weights():
    """eps dominates the variance and mean x scale (~30) cancels against beta, yet the fp32 fold is the seed-0 fold within rounding: the
    scale within two fp32 roundings, the bias within 2^-21 (rounding beta ~ 30 alone would cost up to 2^-20; the member picks its means so
    that it costs less)."""
    sd, sd0 = Z.build("tinyvar"), synth.make_state_dict(0)
    for bn in Z.BN_ALL:
        changed = sd[bn + ".running_var"] != sd0[bn + ".running_var"]
        assert changed.any() and (sd[bn + ".running_var"][changed] <= 1e-12).all()
        if len(changed) >= 8:
            assert (sd[bn + ".running_mean"] >= Z.TINYVAR_MEAN).any()
        w, b = R.fold(sd, bn[:-1] + "0", bn)
        w0, b0 = R.fold(sd0, bn[:-1] + "0", bn)
        assert float(((w - w0).abs() / w0.abs().clamp_min(1e-30)).max()) < 2.0 ** -22
        assert float((b - b0).abs().max()) < 2.0 ** -21


def test_exponent_ranges():
    def span(name):
        e = torch.cat(list(Z.exponent_chain(Z.build(name)).values()))
        return int(e.min()), int(e.max())
    lo, hi = span("seed0")
    assert (lo, hi) == (-2, 2)                               # what every test had before the zoo
    lo, hi = span("spread3")
    assert hi - lo >= 15
    lo, hi = span("spread6")
    assert hi - lo >= 30
    assert span("runaway")[0] == -60                         # the clamp
    e = Z.exponent_chain(Z.build("runaway"))
    assert (e["hb"] == -60).any() or (e["bott"] == -60).any() or (e["he"] == -60).any() or (e["enc"] == -60).any()


# ---- the host emulation of the exponent chain ---------------------------------------------------------------------------------------
def test_exponent_chain_is_the_one_block_emulation_of_test_layer_ref():
    """exponent_chain on a decoder block (a concat input) equals the construction tests/test_layer_ref.py uses for one block, given
    the same input exponents; and the mismatch report excuses a rounding tie and nothing else."""
    sd = Z.build("spread3")
    ex, logs = Z.exponent_chain(sd, with_log2=True)
    W = R.block_weights(sd, "conv8")
    s_in = torch.cat([ex["c2"], ex["c7"]])
    s_h = R.norm_exponents(W["w1"], W["b1"], s_in)
    w2r = torch.cat([R.scale_w(W["w2"], None, s_h).flatten(1), W["wr"].flatten(1) * torch.pow(2.0, -s_in.double())], dim=1)
    s_y = R.norm_exponents(w2r, W["b2"] + W["br"], torch.zeros(w2r.shape[1], dtype=torch.int64))
    assert torch.equal(ex["h8"], s_h) and torch.equal(ex["c8"], s_y)
    for t in ex:
        if t == "flat_part":                                 # (its own rule: test_flatten_exponent_follows_the_filter_not_the_median)
            continue
        fin = torch.isfinite(logs[t])
        assert torch.equal(ex[t][fin], (-torch.round(logs[t][fin])).clamp(-60, 60).to(torch.int64))
    dev = {t: e.numpy().copy() for t, e in ex.items()}
    assert Z.exponent_mismatches(dev, sd) == ([], 0)
    dev["c7"][5] += 1
    bad, ties = Z.exponent_mismatches(dev, sd)
    assert bad == [("c7", 5, int(ex["c7"][5]) + 1, int(ex["c7"][5]))] and ties == 0


def test_flatten_exponent_follows_the_filter_not_the_median():
    """The common exponent of conv_flatten's partial sums puts the filter's rms at 2^-4 (+- half an octave) whatever the channels' scales.
    Where conv9_1's exponents lie together that is the median of those exponents, the earlier rule; on spread6 the median is -6 and
    would leave the filter at rms 2^-9, every low half of its f16 pairs a subnormal (the defect the zoo found: f16x2 logits 2.3e-5 from
    the float64 oracle against 6.3e-6 on spread3, same function; with this rule 4.8e-6, tests/test_gpu_checkpoints.py)."""
    for name in ["seed0", "hostile"] + list(Z.members()):
        sd = Z.build(name)
        e = Z.exponent_chain(sd)["c9"]
        s = R.flatten_scale(sd, e, "f16x2")
        assert abs(R.flatten_log2_rms(sd, e) + s + 4) <= 0.5, name
        assert R.flatten_scale(sd, e, "fp32") == 0 and R.flatten_scale(sd, e, "bf16") == 0
        median = int(torch.sort(e).values[len(e) // 2])
        if name in ("seed0", "hostile", "seed7", "signs", "tinyvar"):
            assert int(e.max() - e.min()) <= 1 and s == median == -1, (name, s, median)
        if name == "spread6":
            assert median == -6 and s != median, (s, median)
