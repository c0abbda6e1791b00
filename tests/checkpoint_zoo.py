"""A family of synthetic checkpoints for the conv stack, and the host emulation of the f16x2 channel exponents on a whole checkpoint.

Not imported by the library.  synth.make_state_dict(0) draws every BatchNorm gamma and running_var from U(0.5, 1.5): no negative
gamma, no dead channel, no variance near zero, and channel exponents that all lie in [-2, 2].  A trained checkpoint has all of these,
and the checkpoint decides most of what weights.hip does on the host (the fold, the power-of-two channel exponents with their zero-row
branch and clamp, the exponents of a concatenated input, the pre-summed taps of the sub-pixel packs, the flatten's common exponent, the
spec head's column scales).  members() -> {name: builder}; build(name) -> a state_dict of numpy arrays in synth.make_state_dict's layout.
Every member is seeded, and is a checkpoint the reference's fp32 classes evaluate without trouble (tests/test_checkpoint_zoo.py holds
each to that on the CPU).

  seed7             another draw.
  spread3, spread6  the seed-0 FUNCTION with per-channel gains 10^U(-k, k) on every hidden and every output channel of every ResBlock,
                    undone in the columns of whatever reads the channel (the generalisation of synth.HOSTILE_GAINS, whose gains are one
                    per tensor): channel exponents that differ by up to 2^40 inside one tensor, so that a wrong channel index in an
                    exponent table moves a value by orders of magnitude.
  signs             about a third of the gammas of every BatchNorm of the 2-D network negated.
  dead              in every block a hidden channel that is identically zero (zero row, zero bias: the est == 0 branch of
                    norm_exponent), one that is a constant (zero row, bias > 0), an output channel that is always clipped (zero rows,
                    bias < 0) and one that is identically zero (its consumers multiply an all-zero input).
  tinyvar           on one channel in eight of every BatchNorm running_var = 0 or 1e-12 (eps dominates 1 / sqrt(var + eps)), gamma
                    rescaled so that the folded scale stays; on half of them running_mean = 30 with beta compensated (mean x scale
                    cancels against beta in the fold).  The seed-0 function up to rounding.
  runaway           running_var = 0 on one channel in sixteen of every BatchNorm, NOT compensated: scale ~316 on those channels,
                    compounding through the blocks (float64 logits ~1e33; the channel exponents reach the -60 clamp).
"""
from __future__ import annotations

import numpy as np
import torch

import layer_ref as R
from softspoken_amd import synth
from softspoken_amd.layout import RESBLOCKS_2D

F32 = np.float32

# (block, first input tensor, second (upsampled) input tensor, hidden tensor, output tensor): the graph of pytorch_neural_nets.py:156-181
# with the names of the activation workspace (test_gpu_layers.py BLOCKS, weights.hip build_model)
GRAPH = [("conv1_1", None, None, "h1", "c1"), ("conv2_1", "c1", None, "h2", "c2"), ("conv3_1", "c2", None, "h3", "c3"),
         ("conv4_1", "c3", None, "h4", "c4"), ("conv_bottleneck", "c4", None, "hb", "bott"), ("encoder_out", "bott", None, "he", "enc"),
         ("conv6", "c4", "enc", "h6", "c6"), ("conv7", "c3", "c6", "h7", "c7"), ("conv8", "c2", "c7", "h8", "c8"),
         ("conv9_1", "c1", "c8", "h9", "c9"), ("spec_output_conv.0", "c9", None, "hs", "s9")]
COUT = {name: cout for name, _, cout in RESBLOCKS_2D}
BN_2D = [f"{name}.{bn}" for name, _, _ in RESBLOCKS_2D for bn in ("conv1.1", "conv2.1", "residual.1")]
BN_ALL = BN_2D + [f"mask_output_conv.0.{bn}" for bn in ("conv1.1", "conv2.1", "residual.1")]
EPS = 1e-5


def consumers(block: str):
    """[(weight key, first column)] of every conv that reads `block`'s output channels: conv1.0 and residual.0 of the blocks that take
    it as skip (offset 0) or as upsampled half (offset = the skip's channel count), conv_flatten and the spec head's 1x1."""
    out_of = {g[4]: g[0] for g in GRAPH}
    cons = []
    for name, x0, x1, _, _ in GRAPH:
        for tensor, off in ((x0, 0), (x1, COUT[out_of[x0]] if x1 else 0)):
            if tensor and out_of[tensor] == block:
                cons += [(f"{name}.conv1.0.weight", off), (f"{name}.residual.0.weight", off)]
    if block == "conv9_1":
        cons.append(("conv_flatten.weight", 0))
    if block == "spec_output_conv.0":
        cons.append(("spec_output_conv.1.weight", 0))
    return cons


def _mul(sd, key, g):
    """sd[key] x g[c] on axis 0, rounded to fp32."""
    a = sd[key].astype(np.float64)
    sd[key] = (a * np.asarray(g, np.float64).reshape(-1, *([1] * (a.ndim - 1)))).astype(F32)


def _div_columns(sd, key, off, g):
    w = sd[key].astype(np.float64)
    n = len(g)
    w[:, off:off + n] /= np.asarray(g, np.float64).reshape(1, n, *([1] * (w.ndim - 2)))
    sd[key] = w.astype(F32)


def _spread(k: float, seed: int):
    sd = synth.make_state_dict(0)
    rng = np.random.Generator(np.random.PCG64(seed))
    for name, _, cout in RESBLOCKS_2D:
        gh = 10.0 ** rng.uniform(-k, k, cout)
        go = 10.0 ** rng.uniform(-k, k, cout)
        for p in ("weight", "bias"):
            _mul(sd, f"{name}.conv1.1.{p}", gh)
            _mul(sd, f"{name}.conv2.1.{p}", go)
            _mul(sd, f"{name}.residual.1.{p}", go)
        _div_columns(sd, f"{name}.conv2.0.weight", 0, gh)
        for key, off in consumers(name):
            _div_columns(sd, key, off, go)
    return sd


def _signs():
    sd = synth.make_state_dict(0)
    rng = np.random.Generator(np.random.PCG64(34))
    for bn in BN_2D:
        neg = rng.uniform(size=sd[bn + ".weight"].shape) < 1.0 / 3.0
        neg[int(rng.integers(len(neg)))] = True                 # (at least one in every BatchNorm)
        sd[bn + ".weight"] = np.where(neg, -sd[bn + ".weight"], sd[bn + ".weight"]).astype(F32)
    return sd


def dead_channels(block: str) -> dict:
    """The four channels of `block` that the `dead` member kills, by kind (seeded by the block's position)."""
    i = [n for n, _, _ in RESBLOCKS_2D].index(block)
    rng = np.random.Generator(np.random.PCG64(100 + i))
    h = rng.choice(COUT[block], 2, replace=False)
    o = rng.choice(COUT[block], 2, replace=False)
    return dict(hidden_zero=int(h[0]), hidden_const=int(h[1]), out_clipped=int(o[0]), out_zero=int(o[1]))


def _dead():
    sd = synth.make_state_dict(0)
    for name, _, _ in RESBLOCKS_2D:
        d = dead_channels(name)
        g1, b1 = sd[f"{name}.conv1.1.weight"], sd[f"{name}.conv1.1.bias"]
        g1[d["hidden_zero"]] = 0; b1[d["hidden_zero"]] = 0
        g1[d["hidden_const"]] = 0; b1[d["hidden_const"]] = abs(b1[d["hidden_const"]]) + F32(0.25)
        for bn in ("conv2.1", "residual.1"):
            g, b = sd[f"{name}.{bn}.weight"], sd[f"{name}.{bn}.bias"]
            g[d["out_clipped"]] = 0; b[d["out_clipped"]] = -abs(b[d["out_clipped"]]) - F32(0.05)
            g[d["out_zero"]] = 0; b[d["out_zero"]] = 0
    return sd


# tinyvar's running_mean.  30 and not 50: the reference's fp32 BatchNorm computes x - mean, whose rounding is half an ulp of the mean
# (2^-19 at 50, 2^-20 at 30) times the channel's scale; with 50 that alone puts the fp32 oracle 2.35e-5 from the float64 one on the
# logits of the pad window, against the 2.5e-5 this suite asks of every member (test_checkpoint_zoo.py); with 30 it is 8.3e-6.
TINYVAR_MEAN = 30.0


def _tinyvar():
    sd = synth.make_state_dict(0)
    for i, bn in enumerate(BN_ALL):
        g, be, mu, var = (sd[bn + k].astype(np.float64) for k in (".weight", ".bias", ".running_mean", ".running_var"))
        n = len(g)
        ch = np.arange((i * 3) % 8, n, 8) if n >= 8 else np.array([i % n])
        for j, c in enumerate(ch):
            vnew = float(F32(0.0 if j % 2 == 0 else 1e-12))
            target = be[c] - mu[c] * g[c] / np.sqrt(var[c] + EPS)           # the folded bias, which stays
            g[c] = float(F32(g[c] / np.sqrt(var[c] + EPS) * np.sqrt(vnew + EPS)))
            var[c] = vnew
            sc = g[c] / np.sqrt(vnew + EPS)                     # the folded scale as the fp32 gamma gives it
            if (j // 2) % 2:
                continue
            # beta = target + mean x scale is ~TINYVAR_MEAN in fp32, so its rounding alone would move the folded bias by up to 2^-20
            # relative to the mean: of the 65 fp32 values from TINYVAR_MEAN upwards take the mean whose beta is nearest an fp32 value.
            # Needed for the member to BE the seed-0 function: with the mean taken as it is, the float64 logits sit 4.0e-6 from
            # seed 0's, the size of the f16x2 error the GPU test measures against them; with the search 2.2e-7, like the spread members
            m, best = F32(TINYVAR_MEAN), None
            for _ in range(65):
                b = target + float(m) * sc
                if best is None or abs(float(F32(b)) - b) < best[0]:
                    best = (abs(float(F32(b)) - b), float(m), float(F32(b)))
                m = np.nextafter(m, F32(np.inf))
            mu[c], be[c] = best[1], best[2]
        for k, a in ((".weight", g), (".bias", be), (".running_mean", mu), (".running_var", var)):
            sd[bn + k] = a.astype(F32)
    return sd


def _runaway():
    sd = synth.make_state_dict(0)
    for i, bn in enumerate(BN_ALL):
        var = sd[bn + ".running_var"]
        if len(var) >= 16:
            var[(i * 11) % 16::16] = 0
    return sd


def members():
    return {"seed7": lambda: synth.make_state_dict(7), "spread3": lambda: _spread(3.0, 3), "spread6": lambda: _spread(6.0, 6),
            "signs": _signs, "dead": _dead, "tinyvar": _tinyvar, "runaway": _runaway}


# the two checkpoints every test had before the zoo, under names (test_gpu_layers.py maps its `hostile` flag to them)
BASE = {"seed0": lambda: synth.make_state_dict(0), "hostile": lambda: synth.make_state_dict(0, hostile=True)}


def build(name: str):
    m = members()
    return (m[name] if name in m else BASE[name])()


# ---- the f16x2 channel exponents of a whole checkpoint (weights.hip build_model / build_resblock), on the host ----------------------
def _log2_est(w, b, s_in):
    """log2 of norm_exponent's estimate, sqrt(0.5 sum (w 2^-s_in)^2 + b^2) (-inf for a zero row with zero bias)."""
    ws = w * torch.pow(2.0, -s_in.to(torch.float64)).view(1, -1, *([1] * (w.dim() - 2)))
    return torch.log2(torch.sqrt(0.5 * (ws * ws).flatten(1).sum(1) + b * b))


def exponent_chain(sd, with_log2: bool = False):
    """{tensor: int64 exponents} for h1 ... hs, c1 ... s9 and flat_part, as weights.hip chooses them: the hidden tensor from conv1's rows on the
    block input's exponents (a concat input: cat[skip's, upsampled half's]), the output from the B launch's row [w2 | wr] -- w2's columns
    on the hidden exponents, wr's on the input's -- and the bias b2 + br.  with_log2: also {tensor: log2 of each channel's estimate}
    (a device exponent may differ only where that lies on a half-integer: the two sides sum in different orders)."""
    exps, logs = {}, {}
    for name, x0, x1, hn, yn in GRAPH:
        W = R.block_weights(sd, name)
        s_in = torch.zeros(1, dtype=torch.int64) if x0 is None else exps[x0]
        if x1:
            s_in = torch.cat([s_in, exps[x1]])
        exps[hn] = R.norm_exponents(W["w1"], W["b1"], s_in)
        logs[hn] = _log2_est(W["w1"], W["b1"], s_in)
        row = torch.cat([W["w2"].flatten(1), W["wr"].flatten(1)], dim=1)
        s_row = torch.cat([exps[hn].repeat_interleave(9), s_in])
        exps[yn] = R.norm_exponents(row, W["b2"] + W["br"], s_row)
        logs[yn] = _log2_est(row, W["b2"] + W["br"], s_row)
    # the common exponent of conv_flatten's partial sums (256 of them per window and row group: one value)
    exps["flat_part"] = torch.full((256,), R.flatten_scale(sd, exps["c9"], "f16x2"), dtype=torch.int64)
    logs["flat_part"] = torch.full((256,), R.flatten_log2_rms(sd, exps["c9"]), dtype=torch.float64)
    return (exps, logs) if with_log2 else exps


EXPONENT_TENSORS = [t for g in GRAPH for t in g[3:]] + ["flat_part"]


def exponent_mismatches(device: dict, sd):
    """Device exponents {tensor: ints} against exponent_chain(sd) -> (mismatches off a rounding tie [(tensor, channel, device, host)],
    number of channels excused because log2(est) lies within 1e-9 of a half-integer)."""
    host, logs = exponent_chain(sd, with_log2=True)
    bad, ties = [], 0
    for t, h in host.items():
        d = torch.as_tensor(np.asarray(device[t]).astype(np.int64))
        assert d.shape == h.shape, (t, d.shape, h.shape)
        for c in torch.nonzero(d != h).flatten().tolist():
            frac = float(logs[t][c]) % 1.0
            if abs(frac - 0.5) <= 1e-9:
                ties += 1
            else:
                bad.append((t, c, int(d[c]), int(h[c])))
    return bad, ties


# ---- the float64 oracle on a member (tests/test_checkpoint_zoo.py on the CPU, tests/test_gpu_checkpoints.py against the device) -------
E2E_WINDOWS = list(range(0, 104, 13))          # eight of the C1 recording's 105 windows: what the end-to-end GPU test runs
SAME_WINDOWS = [0, 20, 50]                     # where the function-preserving members are held to the seed-0 checkpoint


def c1_features(c1: dict, windows):
    """The oracle's fp32 mel features (N, 128, 256) of the given windows of the C1 recording (the conftest fixture's dict)."""
    from oracle import oracle_np as O
    x = torch.stack([torch.from_numpy(c1["padded"][s:s + 66150]) for s in c1["starts"][list(windows)]])
    return O.mel_features(x, torch.from_numpy(synth.hann_window_512()), torch.from_numpy(synth.mel_filterbank()))


def oracle(sd_np, feats: torch.Tensor, dtype=torch.float64):
    """oracle_np.unet_forward in `dtype` on fp32 features -> (logits (N, 1, 256), spec (N, 2, 128, 256)) as float64 numpy."""
    from oracle import oracle_np as O
    sd = {k: torch.as_tensor(np.asarray(v)) for k, v in sd_np.items()}
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        spec, mask = O.unet_forward(sd, feats.to(dtype), want_spec=True)
    return mask.double().numpy(), spec.double().numpy()
