"""The per-launch comparator of tests/layer_ref.py on the CPU: emulations of each mode's arithmetic pass it, and seeded defects fail it by
at least 10x their bound (the sensitivity the GPU tests in test_gpu_layers.py rely on).  Reduced shapes (16 x 32 pixels, two windows),
real block weights: conv8 (a decoder block: 64 skip + 64 upsampled channels -> 32) and conv2_1 (an encoder block, 32 -> 64)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_ref as R

MODES = ("fp32", "f16x2", "bf16")


@pytest.fixture(scope="module")
def sd():
    from softspoken_amd import synth
    return synth.make_state_dict(0)


def _inputs(c0, c1, H=16, W=32, seed=0):
    """Post-ReLU block inputs: window 0 ordinary activations, window 1 at the 1e-3 burst's scale (f16 low halves subnormal)."""
    g = torch.Generator().manual_seed(seed)
    x0 = F.relu(torch.randn(2, c0, H, W, generator=g, dtype=torch.float64))
    x1 = F.relu(torch.randn(2, c1, H // 2, W // 2, generator=g, dtype=torch.float64)) if c1 else None
    x0[1] *= 1e-2
    if x1 is not None:
        x1[1] *= 1e-2
    return x0, x1


def _store(y, mode, e=None, defect=None):
    """The device's store of y (layer units) -> decoded normalised value."""
    e = torch.zeros(y.shape[1], dtype=torch.int64) if e is None else e
    yn = R.scale(y, e).to(torch.float32).to(torch.float64)
    yn = F.relu(yn)
    if mode == "fp32":
        return yn
    if mode == "bf16":
        return R.bf16_trunc(yn) if defect == "truncate" else R.bf16_rn(yn)
    hi, lo = R.split_f16(yn)
    return hi + lo


def _quantise_input(x, mode, e):
    """A stored input: layer units -> (stored normalised value, pair halves for f16x2)."""
    xn = R.scale(x, e).to(torch.float32).to(torch.float64)
    if mode == "bf16":
        xn = R.bf16_rn(xn)
    if mode == "f16x2":
        hi, lo = R.split_f16(xn)
        return hi + lo, (hi, lo)
    return xn, None


def _emulated_conv(xn, pair, w, mode, s_out, s_in, pad, defect=None):
    """The device's product of a stored input (normalised) with a conv's weights as packed (normalised: w 2^(s_out - s_in))."""
    wn = R.scale_w(w, s_out, s_in)
    if mode == "bf16":
        return F.conv2d(xn, R.bf16_rn(wn), padding=pad)
    if mode == "fp32":
        return F.conv2d(xn, wn.to(torch.float32).to(torch.float64), padding=pad)
    xh, xl = pair
    if defect == "flush_subnormal_lo":
        xl = torch.where(xl.abs() < 2.0 ** -14, torch.zeros_like(xl), xl)
    wh, wl = R.split_f16(wn)
    prod_lh = F.conv2d(xh, wl, padding=pad)
    if defect == "drop_wlo_xhi":
        prod_lh[:, :32] = 0
    return F.conv2d(xh, wh, padding=pad) + F.conv2d(xl, wh, padding=pad) + prod_lh


def _exps(mode, W, s_in):
    if mode != "f16x2":
        z = torch.zeros(W["w1"].shape[0], dtype=torch.int64)
        return z, z
    s_h = R.norm_exponents(W["w1"], W["b1"], s_in)
    w2r = torch.cat([R.scale_w(W["w2"], None, s_h).flatten(1), W["wr"].flatten(1) * torch.pow(2.0, -s_in.double())], dim=1)
    s_y = R.norm_exponents(w2r, W["b2"] + W["br"], torch.zeros(w2r.shape[1], dtype=torch.int64))
    return s_h, s_y


def _launch_A(sd, name, mode, defect=None):
    W = R.block_weights(sd, name)
    c0 = W["w1"].shape[1] if name != "conv8" else 64
    c1 = W["w1"].shape[1] - c0
    x0, x1 = _inputs(c0, c1)
    s_in = torch.tensor([(-1) ** i * (i % 3) for i in range(c0 + c1)], dtype=torch.int64) if mode == "f16x2" else torch.zeros(c0 + c1, dtype=torch.int64)
    s_h, _ = _exps(mode, W, s_in)
    x = R.block_input(x0, x1)
    xn, pair = _quantise_input(x, mode, s_in)
    x_dev = R.scale(xn, -s_in)                            # what the device's tensors decode to, layer units
    pad = 1
    if defect == "wrap_border":
        xp = F.pad(xn, (1, 1, 1, 1), mode="circular")
        pair = tuple(F.pad(p, (1, 1, 1, 1), mode="circular") for p in pair) if pair else None
        xn, pad = xp, 0
    w1 = W["w1"].clone()
    if defect == "missing_tap":
        w1[:, :32, 0, 2] = 0
    acc = _emulated_conv(xn, pair, w1, mode, s_h, s_in, pad, defect)
    if defect == "parity_swap" and c1:
        up_part = _emulated_conv(xn[:, c0:], tuple(p[:, c0:] for p in pair) if pair else None, w1[:, c0:], mode, s_h, s_in[c0:], pad)
        sw = up_part.clone()
        sw[:, :, 0::2], sw[:, :, 1::2] = up_part[:, :, 1::2], up_part[:, :, 0::2]
        acc = acc - up_part + sw
    b1 = R.scale(W["b1"].view(1, -1, 1, 1), s_h)
    if defect == "missing_bias":
        b1 = b1.clone()
        b1[0, 5] = 0
    y = R.scale(acc + b1, -s_h)                           # layer units (the store re-applies the exponents)
    if defect == "neighbour_window":
        y = y.clone()
        y[0, :, 3, 7] = y[1, :, 3, 7]
    if defect == "exponent":
        y = y.clone()
        y[:, 3] *= 2.0
    stored = _store(y, mode, s_h, defect)
    ref = R.ref_A(W, x_dev, mode, s_in)
    return R.compare(stored, ref, s_h, mode)


def _launch_B(sd, name, mode, defect=None):
    W = R.block_weights(sd, name)
    cin = W["wr"].shape[1]
    x0, _ = _inputs(cin, 0, seed=1)
    h, _ = _inputs(W["w2"].shape[1], 0, seed=2)
    s_in = torch.tensor([(i % 4) - 2 for i in range(cin)], dtype=torch.int64) if mode == "f16x2" else torch.zeros(cin, dtype=torch.int64)
    s_h, s_y = _exps(mode, W, s_in)
    xn, xpair = _quantise_input(x0, mode, s_in)
    hn, hpair = _quantise_input(h, mode, s_h)
    x_dev, h_dev = R.scale(xn, -s_in), R.scale(hn, -s_h)
    pad = 1
    if defect == "wrap_border":
        hn = F.pad(hn, (1, 1, 1, 1), mode="circular")
        hpair = tuple(F.pad(p, (1, 1, 1, 1), mode="circular") for p in hpair) if hpair else None
        pad = 0
    w2 = W["w2"].clone()
    if defect == "missing_tap":
        w2[:, :32, 2, 1] = 0
    acc = _emulated_conv(hn, hpair, w2, mode, s_y, s_h, pad, defect) + _emulated_conv(xn, xpair, W["wr"], mode, s_y, s_in, 0, defect)
    b = R.scale((W["b2"] + W["br"]).to(torch.float32).to(torch.float64).view(1, -1, 1, 1), s_y)
    if defect == "missing_bias":
        b = b.clone()
        b[0, 5] = 0
    y = R.scale(acc + b, -s_y)
    if defect == "neighbour_window":
        y = y.clone()
        y[0, :, 3, 7] = y[1, :, 3, 7]
    if defect == "exponent":
        y = y.clone()
        y[:, 3] *= 2.0
    stored = _store(y, mode, s_y, defect)
    ref = R.ref_B(W, h_dev, x_dev, mode, r_stored=False, s_h=s_h, s_x=s_in)
    return R.compare(stored, ref, s_y, mode)


LAUNCHES = [("A", "conv8"), ("A", "conv2_1"), ("B", "conv8"), ("B", "conv2_1")]


def _run(sd, kind, name, mode, defect=None):
    return (_launch_A if kind == "A" else _launch_B)(sd, name, mode, defect)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,name", LAUNCHES)
def test_mode_emulation_passes(sd, kind, name, mode):
    rep = _run(sd, kind, name, mode)
    assert rep["over"] == 0 and rep["ratio"] <= 1.0, rep


# defect -> the modes it exists in; parity classes exist only where the input has an upsampled half (conv8.A)
DEFECTS = {"missing_tap": MODES, "missing_bias": MODES, "wrap_border": MODES, "neighbour_window": MODES, "parity_swap": MODES,
           "drop_wlo_xhi": ("f16x2",), "flush_subnormal_lo": ("f16x2",), "exponent": ("f16x2",), "truncate": ("bf16",)}
CASES = [(k, n, m, d) for d, modes in DEFECTS.items() for m in modes for k, n in LAUNCHES
         if d != "parity_swap" or (k, n) == ("A", "conv8")]


@pytest.mark.parametrize("kind,name,mode,defect", CASES)
def test_defect_fails_by_10x(sd, kind, name, mode, defect):
    rep = _run(sd, kind, name, mode, defect)
    assert rep["ratio"] >= 10.0, rep


def test_exact_checks():
    x = torch.rand(2, 4, 8, 8, dtype=torch.float64)
    assert R.pool_mismatches(x, F.max_pool2d(x, 2, 2)) == 0
    bad = F.max_pool2d(x, 2, 2).clone()
    bad[0, 1, 2, 3] = -1.0
    assert R.pool_mismatches(x, bad) == 1
    v = torch.rand(1000, dtype=torch.float64) * 3
    hi, lo = R.split_f16(v)
    h16 = hi.to(torch.float16).numpy().view(np.uint16)
    l16 = lo.to(torch.float16).numpy().view(np.uint16)
    assert R.canonical_split_mismatches(h16, l16) == 0
    # a pair whose low half carries a whole unit of the high half's last place is not canonical; exactly half of it (a tie) is
    ulp = (hi.to(torch.float16).numpy().view(np.uint16) + 1).view(np.float16).astype(np.float64) - hi.numpy()
    assert R.canonical_split_mismatches(h16, torch.tensor(ulp).to(torch.float16).numpy().view(np.uint16)) > 900
    assert R.canonical_split_mismatches(h16, torch.tensor(ulp / 2).to(torch.float16).numpy().view(np.uint16)) == 0


# ---- the other references: conv1_1.B from the features, the bf16 B launch that reads a bf16 r, spec_tail, conv_flatten, the head ----
def _features(seed=3, H=128, W=32):
    """Features as the front-end makes them (>= 0, up to ~6), window 1 quiet (the 1e-3 burst's scale)."""
    g = torch.Generator().manual_seed(seed)
    f = torch.rand(2, 1, H, W, generator=g, dtype=torch.float64) * 3.0
    f[1] *= 1e-2
    return f.to(torch.float32).to(torch.float64)


def _conv1_1(sd, mode, form="conv4", defect=None):
    """conv1_1.B as each form computes it: fp32; f16x2 with the features, first weights and h1 as f16 pairs; bf16 conv4.hip (features,
    first weights and h1 rounded, the residual as hi/lo products) or conv2.hip (h1 rounded alone)."""
    W = R.block_weights(sd, "conv1_1")
    f = _features(W=32)
    s_h = R.norm_exponents(W["w1"], W["b1"], torch.zeros(1, dtype=torch.int64)) if mode == "f16x2" else torch.zeros(32, dtype=torch.int64)
    s_y = torch.zeros(32, dtype=torch.int64)
    w1, w2 = W["w1"].clone(), W["w2"].clone()
    b1 = W["b1"].clone()
    if defect == "missing_tap1":
        w1[:, :, 0, 1] = 0
    if defect == "missing_tap2":
        w2[:, :16, 2, 2] = 0
    if defect == "missing_bias":
        b1[7] = 0
    pad_mode = "circular" if defect == "wrap_border" else "constant"
    cv = lambda x, w: F.conv2d(F.pad(x, (1, 1, 1, 1), mode=pad_mode), w)
    if mode == "fp32":
        h = F.relu(cv(f, w1) + b1.view(1, -1, 1, 1)).to(torch.float32).to(torch.float64)
        acc = cv(h, w2)
    elif mode == "bf16":
        fin, w1p = (R.bf16_rn(f), R.bf16_rn(w1)) if form == "conv4" else (f, w1)
        h = R.bf16_rn(F.relu(cv(fin, w1p) + b1.view(1, -1, 1, 1)).to(torch.float32).to(torch.float64))
        acc = cv(h, R.bf16_rn(w2))
    else:
        fh, fl = R.split_f16(f)
        w1n = R.scale_w(w1, s_h, None)
        wh, wl = R.split_f16(w1n)
        hn = F.relu(cv(fh, wh) + cv(fl, wh) + cv(fh, wl) + R.scale(b1.view(1, -1, 1, 1), s_h)).to(torch.float32).to(torch.float64)
        hh, hl = R.split_f16(hn)
        w2n = R.scale_w(w2, s_y, s_h)
        vh, vl = R.split_f16(w2n)
        acc = cv(hh, vh) + cv(hl, vh) + cv(hh, vl)
    y = acc + F.conv2d(f, W["wr"]) + (W["b2"] + W["br"]).view(1, -1, 1, 1)
    stored = _store(y, mode, s_y, defect)
    return R.compare(stored, R.ref_conv1_1(W, f, mode, s_h, form), s_y, mode)


C11 = [("fp32", "conv4"), ("f16x2", "conv4"), ("bf16", "conv4"), ("bf16", "conv2")]


@pytest.mark.parametrize("mode,form", C11)
def test_conv1_1_emulation_passes(sd, mode, form):
    rep = _conv1_1(sd, mode, form)
    assert rep["over"] == 0 and rep["ratio"] <= 1.0, rep


@pytest.mark.parametrize("defect", ["missing_tap1", "missing_tap2", "missing_bias", "wrap_border"])
@pytest.mark.parametrize("mode,form", C11)
def test_conv1_1_defect_fails_by_10x(sd, mode, form, defect):
    assert _conv1_1(sd, mode, form, defect)["ratio"] >= 10.0


def _bf16_B_with_r(sd, defect=None):
    """A bf16 B launch of the A + r / B form: r = bf16_rn(conv1x1(x) + br) written by A, added by B."""
    W = R.block_weights(sd, "conv2_1")
    x, _ = _inputs(W["wr"].shape[1], 0, seed=4)
    h, _ = _inputs(W["w2"].shape[1], 0, seed=5)
    x, h = R.bf16_rn(x), R.bf16_rn(h)
    r = F.conv2d(x, R.bf16_rn(W["wr"])) + W["br"].view(1, -1, 1, 1)
    r = R.bf16_trunc(r) if defect == "truncate_r" else R.bf16_rn(r)
    w2 = R.bf16_rn(W["w2"]).clone()
    if defect == "missing_tap":
        w2[:, 32:, 1, 0] = 0
    y = F.conv2d(h, w2, padding=1) + W["b2"].view(1, -1, 1, 1) + r
    return R.compare(_store(y, "bf16"), R.ref_B(W, h, x, "bf16", r_stored=True), None, "bf16")


def test_bf16_B_reading_r_passes_and_catches_defects(sd):
    rep = _bf16_B_with_r(sd)
    assert rep["over"] == 0 and rep["ratio"] <= 1.0, rep
    for d in ("missing_tap", "truncate_r"):
        assert _bf16_B_with_r(sd, d)["ratio"] >= 10.0, d


def _spec_tail(sd, defect=None):
    g = torch.Generator().manual_seed(6)
    s9 = F.relu(torch.randn(2, 32, 16, 32, generator=g, dtype=torch.float64)).to(torch.float32).to(torch.float64)
    w = torch.as_tensor(np.asarray(sd["spec_output_conv.1.weight"]), dtype=torch.float64).clone()
    b = torch.as_tensor(np.asarray(sd["spec_output_conv.1.bias"]), dtype=torch.float64).clone()
    if defect == "missing_bias":
        b[1] = 0
    if defect == "missing_channel":
        w[:, 5] = 0
    got = F.relu(F.conv2d(s9.to(torch.float32), w.to(torch.float32), b.to(torch.float32))).to(torch.float64)
    return R.compare(got, R.ref_spec_tail(sd, s9), None, "fp32")


def test_spec_tail_passes_and_catches_defects(sd):
    rep = _spec_tail(sd)
    assert rep["over"] == 0 and rep["ratio"] <= 1.0, rep
    for d in ("missing_bias", "missing_channel"):
        assert _spec_tail(sd, d)["ratio"] >= 10.0, d


def _flatten_head(sd, mode, defect=None, groups=8):
    """conv9_1's output c9 (H = 128 mel rows, 32 time bins) through conv_flatten as the B launch's epilogue computes it (partial sums per
    group of 16 mel rows, in 2^s_common units), then the mask head in fp32 from those partial sums.  -> (flatten report, head report)."""
    g = torch.Generator().manual_seed(8)
    c9 = F.relu(torch.randn(2, 32, 128, 32, generator=g, dtype=torch.float64)) * 0.3
    c9[1] *= 1e-2
    e = torch.tensor([(i % 5) - 2 for i in range(32)], dtype=torch.int64) if mode == "f16x2" else torch.zeros(32, dtype=torch.int64)
    c9n = R.scale(c9, e).to(torch.float32).to(torch.float64)
    wf, bfl = R.flatten_weights(sd)
    wfs = R.scale_w(wf, torch.full((4,), R.flatten_scale(sd, e, mode)), e).to(torch.float32).to(torch.float64)
    if mode == "bf16":
        c9n, wfs = R.bf16_rn(c9n), R.bf16_rn(wfs)
    if mode == "f16x2":
        hi, lo = R.split_f16(c9n)
        c9n = hi + lo
    wdev = wfs.clone()
    if defect == "dropped_mel_row":
        wdev[:, :, 77, :] = 0
    x = c9n.clone()
    if defect == "border_row":
        x[:, :, 0] = x[:, :, 1]                           # mel row 0 read from row 1
    rows = 128 // groups
    if mode == "f16x2":
        xh, xl = R.split_f16(x)
        wh, wl = R.split_f16(wdev)
        parts = torch.stack([(F.conv2d(xh[:, :, k:k + rows], wh[:, :, k:k + rows]) + F.conv2d(xl[:, :, k:k + rows], wh[:, :, k:k + rows]) +
                              F.conv2d(xh[:, :, k:k + rows], wl[:, :, k:k + rows])).squeeze(2) for k in range(0, 128, rows)], 1)
    else:
        parts = torch.stack([F.conv2d(x[:, :, k:k + rows], wdev[:, :, k:k + rows]).squeeze(2) for k in range(0, 128, rows)], 1)
    parts = parts.to(torch.float32).to(torch.float64)
    if defect == "neighbour_window_bin":
        parts[0, :, :, 9] = parts[1, :, :, 9]
    ref, bound = R.ref_flatten(sd, c9n, e, mode)
    flat_rep = R.ratio_report(parts.sum(1), ref, bound)
    # the head kernel (fp32) from the partial sums
    fscale = 2.0 ** -R.flatten_scale(sd, e, mode)
    s = (parts.sum(1) * fscale).to(torch.float32).to(torch.float64)
    b = torch.zeros_like(bfl) if defect == "missing_flatten_bias" else bfl
    xin = F.relu(s + b.view(1, -1, 1))
    if defect == "head_border_column":
        xin = torch.cat([xin[:, :, -1:], xin, xin[:, :, :1]], 2)   # the 1-D convs read the far end instead of zero padding
        got = _head_padded(sd, xin)
    elif defect == "head_neighbour_bin":
        xin = xin.clone()
        xin[0, :, 9] = xin[1, :, 9]
        got = R.mask_head(sd, xin)
    else:
        got = R.mask_head(sd, xin)
    got = got.to(torch.float32).to(torch.float64)
    lg, hb = R.ref_head(sd, parts, e, mode)
    return flat_rep, R.ratio_report(got, lg, hb)


def _head_padded(sd, xp):
    """The head on an input that already carries its one-bin border (xp: N x 4 x (T + 2))."""
    pfx = "mask_output_conv.0"
    w1, b1 = R.fold(sd, pfx + ".conv1.0", pfx + ".conv1.1")
    w2, b2 = R.fold(sd, pfx + ".conv2.0", pfx + ".conv2.1")
    wr, br = R.fold(sd, pfx + ".residual.0", pfx + ".residual.1")
    x = xp[:, :, 1:-1]
    h = F.relu(F.conv1d(xp, w1, b1))
    h = torch.cat([h[:, :, -1:], h, h[:, :, :1]], 2)
    out = F.relu(F.conv1d(h, w2, b2) + F.conv1d(x, wr, br))
    wo = torch.as_tensor(np.asarray(sd["mask_output_conv.1.weight"]), dtype=torch.float64)
    bo = torch.as_tensor(np.asarray(sd["mask_output_conv.1.bias"]), dtype=torch.float64)
    return F.conv1d(out, wo, bo)


@pytest.mark.parametrize("mode", MODES)
def test_flatten_and_head_emulation_passes(sd, mode):
    flat, head = _flatten_head(sd, mode)
    assert flat["over"] == 0 and flat["ratio"] <= 1.0, flat
    assert head["over"] == 0 and head["ratio"] <= 1.0, head


# defect -> which of the two checks must catch it
FLAT_DEFECTS = {"dropped_mel_row": 0, "border_row": 0, "neighbour_window_bin": 0, "missing_flatten_bias": 1, "head_border_column": 1,
                "head_neighbour_bin": 1}


@pytest.mark.parametrize("defect", list(FLAT_DEFECTS))
@pytest.mark.parametrize("mode", MODES)
def test_flatten_and_head_defect_fails_by_10x(sd, mode, defect):
    rep = _flatten_head(sd, mode, defect)[FLAT_DEFECTS[defect]]
    assert rep["ratio"] >= 10.0, rep
