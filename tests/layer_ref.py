"""float64 references of single launches of the network, computed from the tensors the device stored, and the bounds the device's
stored outputs are held to (tests/test_layer_ref.py checks on the CPU that the bounds catch seeded defects; tests/test_gpu_layers.py
holds every launch of the device to them).

Not imported by the library.  Tensors are torch float64, NCHW.  A stored tensor is compared in NORMALISED units: the stored value of
channel c is 2^e[c] x the layer's value (f16x2 channel exponents, weights.hip; e = 0 in fp32 and bf16).  The references are computed in
layer units from the device's own inputs brought back to layer units, with the BatchNorm folded as weights.hip folds it (float64, then
rounded to fp32: the weights the device packs), and scaled to normalised units at the end.

Every reference comes with a MAGNITUDE pass M: the same graph on |w|, |x|, |b| (ReLU the identity).  Bounds, u = 2^-24.  Two kinds of
error are counted separately:

  representation  what the storage formats lose.  Derived worst case, element by element.
  accumulation    fp32 rounding of the running sums.  NOT derived worst case: the worst case D u M (D accumulator roundings per output,
                  up to ~10^3 here) is 2^-14 M, above every bar below, and no real sum approaches it -- each rounding is relative to the
                  running sum, which is far below M, and the roundings have random signs.  The bars below assume it stays under 2^-21 M.
                  That is an assumption, stated here, and what supports it is measurement: the fp32 launches (fp32 weights and inputs,
                  so accumulation is all their error beyond 2 u M) come to at most 0.039 x 2^-17 M = 2^-21.7 M on MI355X (DESIGN.md
                  section 2), and the f16x2 launches use the same fp32 accumulators.

  fp32    2^-17 M: representation 2 u M (the output's rounding; the folded weights are the device's exactly) plus accumulation, with
          headroom of 2^4 over the assumption.
  f16x2   2^-20 M: representation -- the weight pairs hold 23 bits (2^-23 |w|), hi.x_hi + hi.x_lo + lo.x_hi drops lo.x_lo (<= 2^-24
          |w x|), the output pair rounds at 2^-23 |y|: 2^-21.6 M together -- plus accumulation (2^-21 M): 2^-20.2 M.  (2^-17 M, the fp32
          bar, is too wide here: losing every low half of the input moves a 1152-term output by ~2^-12 sqrt(K) |w x|, 1x that bar.)
          Plus an absolute FLOOR in normalised units for the low halves that are f16 subnormals (absolute resolution 2^-24, rounding
          error 2^-25):
            2^-25                       the output's own low half
            2^-25 sum |x|               the weights' low halves (every input the launch multiplies by a split weight)
            |W| (2^-25 (1 + ...))       an intermediate held as a pair inside the launch (conv1_1's h1 and features), propagated
  bf16    the device's output is the round-to-nearest-even bf16 of its fp32 result, which lies within 2^-17 M of the reference (weights as
          packed: f2bf of the fp32 fold; bf16 products are exact in fp32, so this is the fp32 bar).  So the stored value must EQUAL bf16_rn(ref) wherever no bf16 rounding boundary lies within
          2^-17 M of ref; where one does, it may be the neighbour.  Bound: 2^-17 M + |bf16_rn(ref + d) - bf16_rn(ref - d)|, d = 2^-17 M.
          (The issue's starting point 2^-8 |ref| + 2^-17 M lets a truncating store pass at ratio ~2; this one fails it by >> 10.)  Every
          bf16 rounding the form performs inside the launch is repeated by the reference, with the same neighbour allowance propagated
          through |W| (table BF16_INTERNAL below).  A form that rounds something the table does not list fails, on purpose.

Exact checks: pooled tensors equal maxpool2 of the decoded full-resolution tensor in every mode; every stored f16x2 pair is a canonical
split, hi == f16_rn(hi + lo) (ties included: see canonical_split_mismatches).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

TOL = {"fp32": 2.0 ** -17, "bf16": 2.0 ** -17, "f16x2": 2.0 ** -20}
FLOOR = 2.0 ** -25

# bf16 roundings inside a launch, and what the reference does about each (the output's own rounding is always there):
#   "repeat": the reference rounds the same value, with the neighbour allowance 2^-17 M pushed through |W|;
#   "allow":  the reference does not round it but adds the stated allowance.
#   launch               tensor          treatment                what is rounded
BF16_INTERNAL = {
    "A": [],                                                      # h = relu(conv1(x) + b1), stored
    "B.proj": [],                                                 # "projection in B": y = relu(conv2(h) + conv1x1(x) + b2 + br)
    "B.r": [("r", "repeat", "conv1x1(x) + br, written by A as bf16 and added by B")],
    "conv1_1.B conv4": [("feat", "repeat", "the features and the first conv's weights, as that conv's MFMA operands"),
                        ("h1", "repeat", "relu(conv1(feat) + b1), the second conv's operand (in LDS)"),
                        ("wr f", "allow 2^-15 |wr| |f|", "the 1 -> 32 residual as bf16 halves, whi f_hi + whi f_lo + wlo f_hi")],
    "conv1_1.B conv2": [("h1", "repeat", "relu(conv1(feat) + b1) from fp32 features and weights (VALU), the second conv's operand")],
    "conv9_1.B flatten": [("c9", "repeat", "conv9_1's output as the flatten MFMA's operand: the stored bf16 c9 itself"),
                          ("wf", "repeat", "conv_flatten's weights, f2bf")],
}


# ---- number formats -------------------------------------------------------------------------------------------------------------
def bf16_rn(x: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even to bf16 of the fp32 value of x (weights.hip f2bf; the kernels' conversions)."""
    u = x.to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    r = torch.where(r >= 2 ** 31, r - 2 ** 32, r).to(torch.int32)
    return r.view(torch.float32).to(torch.float64)


def bf16_trunc(x: torch.Tensor) -> torch.Tensor:
    u = x.to(torch.float32).contiguous().view(torch.int32)
    return (u & ~0xFFFF).view(torch.float32).to(torch.float64)


def f16_rn(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).to(torch.float16).to(torch.float64)


def split_f16(x: torch.Tensor):
    """The kernels' split of an fp32 value: hi = f16_rn(x), lo = f16_rn(x - hi)."""
    hi = f16_rn(x)
    return hi, f16_rn(x.to(torch.float32).to(torch.float64) - hi)


def neighbour_allowance(pre: torch.Tensor, d, relu: bool = True) -> torch.Tensor:
    """|bf16_rn(relu(pre + d)) - bf16_rn(relu(pre - d))|: nonzero only where a rounding boundary lies within d of pre."""
    act = F.relu if relu else (lambda t: t)
    return (bf16_rn(act(pre + d)) - bf16_rn(act(pre - d))).abs()


def canonical_split_mismatches(hi: np.ndarray, lo: np.ndarray) -> int:
    """Stored f16 pairs (uint16 planes) that are not a round-to-nearest split: hi == f16_rn(hi + lo), i.e. |lo| at most half the gap
    from hi to its neighbour on lo's side.  A tie (|lo| exactly that half) is canonical too: lo = f16_rn(x - hi) may round up to it,
    which subnormal low halves (resolution 2^-24) do often."""
    h = hi.view(np.float16)
    l = lo.view(np.float16).astype(np.float32)
    nb = np.nextafter(h, np.where(l < 0, np.float16(-np.inf), np.float16(np.inf))).astype(np.float32)
    half = np.abs(nb - h.astype(np.float32)) / 2
    return int((np.abs(l) > half).sum())


# ---- weights as the device folds them --------------------------------------------------------------------------------------------
def _t(a) -> torch.Tensor:
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def fold(sd, conv: str, bn: str):
    """weights.hip fold_conv_bn: w * g / sqrt(var + eps) and beta - mean * g / sqrt(var + eps) in float64, rounded to fp32."""
    w = _t(sd[conv + ".weight"]).to(torch.float32).to(torch.float64)
    g, be, mu, var = (_t(sd[bn + k]).to(torch.float32).to(torch.float64) for k in (".weight", ".bias", ".running_mean", ".running_var"))
    sc = g / torch.sqrt(var + 1e-5)
    wf = (w * sc.view(-1, *([1] * (w.dim() - 1)))).to(torch.float32).to(torch.float64)
    bf = (be - mu * sc).to(torch.float32).to(torch.float64)
    return wf, bf


def block_weights(sd, name: str) -> dict:
    w1, b1 = fold(sd, name + ".conv1.0", name + ".conv1.1")
    w2, b2 = fold(sd, name + ".conv2.0", name + ".conv2.1")
    wr, br = fold(sd, name + ".residual.0", name + ".residual.1")
    return dict(w1=w1, b1=b1, w2=w2, b2=b2, wr=wr, br=br)


def as_packed(W: dict, mode: str) -> dict:
    """The weights a mode's launches multiply by: bf16 packs f2bf of the fp32 fold (biases stay fp32)."""
    if mode != "bf16":
        return W
    return {k: (bf16_rn(v) if k.startswith("w") else v) for k, v in W.items()}


def norm_exponents(w: torch.Tensor, b: torch.Tensor, s_in: torch.Tensor) -> torch.Tensor:
    """weights.hip norm_exponent for one conv (or the sum of two rows' sums of squares, given as w = cat along dim 1): for tests that
    emulate the f16x2 storage on the CPU.  -round(log2(sqrt(0.5 sum (w 2^-s_in)^2 + b^2))), clamped to [-60, 60]."""
    ws = w * torch.pow(2.0, -s_in.to(torch.float64)).view(1, -1, *([1] * (w.dim() - 2)))
    est = torch.sqrt(0.5 * (ws * ws).flatten(1).sum(1) + b * b)
    e = -torch.round(torch.log2(est))
    return torch.where(est > 0, e, torch.zeros_like(e)).clamp(-60, 60).to(torch.int64)


def scale(x: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """x (NCHW) times 2^e[c]."""
    return x * torch.pow(2.0, e.to(torch.float64)).view(1, -1, 1, 1)


# ---- launch references ---------------------------------------------------------------------------------------------------------
def up2(t: torch.Tensor) -> torch.Tensor:
    return F.interpolate(t, scale_factor=2, mode="nearest")


def block_input(x0: torch.Tensor, x1: torch.Tensor | None) -> torch.Tensor:
    """The A launch's input, cat[skip, up2(x1)] (pytorch_neural_nets.py:171-180)."""
    return x0 if x1 is None else torch.cat([x0, up2(x1)], dim=1)


def conv(x, w, b=None, pad=1):
    return F.conv2d(x, w, b, padding=pad)


def box3(x: torch.Tensor) -> torch.Tensor:
    """sum over channels and the 3x3 neighbourhood (zero padding): the inputs one output of a 3x3 conv multiplies."""
    s = x.sum(1, keepdim=True)
    return F.conv2d(s, torch.ones(1, 1, 3, 3, dtype=x.dtype), padding=1)


class Ref:
    """pre: the reference before the output's ReLU, layer units; M: the magnitude pass (layer units); floor: f16x2 absolute floor in
    normalised units of the output; allow: allowances of what happens inside the launch (bf16 neighbour flips of internal roundings,
    f16x2 floors of internal pairs), layer units."""

    def __init__(self, pre, M, floor=0.0, allow=0.0):
        self.pre, self.M, self.floor, self.allow = pre, M, floor, allow


def ref_A(W: dict, x: torch.Tensor, mode: str, s_x=None) -> Ref:
    """A launch: h = relu(bn1(conv1(x))), x = cat[skip, up2(x1)] in layer units; s_x: x's exponents (f16x2)."""
    Wp = as_packed(W, mode)
    pre = conv(x, Wp["w1"], Wp["b1"])
    M = conv(x.abs(), Wp["w1"].abs(), Wp["b1"].abs())
    floor = FLOOR * (1.0 + box3(scale(x, s_x).abs())) if mode == "f16x2" else 0.0
    return Ref(pre, M, floor)


def ref_B(W: dict, h: torch.Tensor, x: torch.Tensor, mode: str, r_stored: bool, s_h=None, s_x=None) -> Ref:
    """B launch: y = relu(bn2(conv2(h)) + bnr(convr(x))) from the device's h and block input x (layer units).  r_stored: the pass ran
    the block as A + r / B (bf16 then rounds r; fp32 / f16x2 keep it in fp32)."""
    Wp = as_packed(W, mode)
    r = conv(x, Wp["wr"], Wp["br"], pad=0)
    Mr = conv(x.abs(), Wp["wr"].abs(), Wp["br"].abs(), pad=0)
    allow = 0.0
    if mode == "bf16" and r_stored:
        allow = neighbour_allowance(r, TOL[mode] * Mr, relu=False)
        r = bf16_rn(r)
    pre = conv(h, Wp["w2"], Wp["b2"]) + r
    M = conv(h.abs(), Wp["w2"].abs(), Wp["b2"].abs()) + Mr
    floor = 0.0
    if mode == "f16x2":
        floor = FLOOR * (1.0 + box3(scale(h, s_h).abs()) + scale(x, s_x).abs().sum(1, keepdim=True))
    return Ref(pre, M, floor, allow)


def ref_conv1_1(W: dict, feat: torch.Tensor, mode: str, s_h=None, form: str = "conv4") -> Ref:
    """conv1_1.B as one launch from the features (N, 1, 128, 256): c1 = relu(bn2(conv2(relu(bn1(conv1(f))))) + bnr(convr(f))); h1
    never leaves the launch.  bf16: what is rounded depends on the form (BF16_INTERNAL: conv4.hip rounds the features, the first conv's
    weights and h1; conv2.hip's form computes h1 on the VALU in fp32 and rounds h1 alone); f16x2: features and h1 are held as f16
    pairs.  s_h: h1's exponents (f16x2)."""
    Wp = as_packed(W, mode)
    first = Wp if form == "conv4" else W
    f = bf16_rn(feat) if mode == "bf16" and form == "conv4" else feat
    hpre = conv(f, first["w1"], first["b1"])
    Mh = conv(f.abs(), first["w1"].abs(), first["b1"].abs())
    h = F.relu(hpre)
    if mode == "bf16":
        h = bf16_rn(h)
    r = conv(feat, W["wr"], W["br"], pad=0)
    pre = conv(h, Wp["w2"], Wp["b2"]) + r
    M = conv(Mh, Wp["w2"].abs(), Wp["b2"].abs()) + conv(feat.abs(), W["wr"].abs(), W["br"].abs(), pad=0)
    if mode == "bf16":
        # h1's neighbour flips through |w2|; conv4.hip: the residual as whi f_hi + whi f_lo + wlo f_hi (bf16 halves: 2^-15 |wr f|)
        allow = conv(neighbour_allowance(hpre, TOL[mode] * Mh), Wp["w2"].abs())
        if form == "conv4":
            allow = allow + 2.0 ** -15 * conv(feat.abs(), W["wr"].abs(), pad=0)
        return Ref(pre, M, 0.0, allow)
    if mode == "f16x2":
        # h1 (normalised) as a pair: its own low half, the first weights' low halves (x |f|), the features' low halves (x |w1 2^e_h|);
        # carried to c1 through |w2 2^-e_h| (layer units of c1)
        fh = FLOOR * (1.0 + box3(feat.abs()) + scale_w(W["w1"], s_h, None).abs().flatten(1).sum(1).view(1, -1, 1, 1))
        allow = conv(fh, scale_w(W["w2"], None, s_h).abs())
        return Ref(pre, M, FLOOR * (1.0 + box3(scale(h, s_h).abs())), allow)
    return Ref(pre, M)


def scale_w(w: torch.Tensor, s_out, s_in) -> torch.Tensor:
    """w[co][ci] 2^(s_out[co] - s_in[ci]) (None: 0)."""
    so = torch.zeros(w.shape[0]) if s_out is None else torch.as_tensor(s_out)
    si = torch.zeros(w.shape[1]) if s_in is None else torch.as_tensor(s_in)
    ex = so.to(torch.float64).view(-1, 1) - si.to(torch.float64).view(1, -1)
    return w * torch.pow(2.0, ex).view(*ex.shape, *([1] * (w.dim() - 2)))


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def deviation(ref: Ref, e, mode: str) -> torch.Tensor:
    """How far the device's value before its output rounding may be from ref.pre, in layer units (e: the output's exponents)."""
    floor = ref.floor if torch.is_tensor(ref.floor) else torch.tensor(float(ref.floor))
    return TOL[mode] * ref.M + ref.allow + scale(torch.broadcast_to(floor, ref.M.shape), -torch.as_tensor(e))


def compare(stored: torch.Tensor, ref: Ref, s_y, mode: str) -> dict:
    """stored: decoded device output in normalised units (NCHW).  -> worst ratio |delta| / bound, where it is (n, y, x, c), the count
    over the bound and the largest |delta|."""
    e = torch.zeros(stored.shape[1], dtype=torch.int64) if s_y is None else torch.as_tensor(s_y, dtype=torch.int64)
    pre = scale(ref.pre, e)
    dev = scale(deviation(ref, e, mode), e)
    if mode == "bf16":
        want = bf16_rn(F.relu(pre))
        bound = dev + neighbour_allowance(pre, dev)
    else:
        want = F.relu(pre)
        bound = dev
    return ratio_report(stored, want, bound)


def ratio_report(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> dict:
    d = (got - want).abs()
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bound)         # (0 / 0: exact where nothing is allowed)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    k = int(torch.argmax(ratio))
    idx = np.unravel_index(k, tuple(ratio.shape))
    at = (int(idx[0]), int(idx[2]), int(idx[3]), int(idx[1])) if len(idx) == 4 else tuple(int(i) for i in idx)
    return dict(ratio=float(ratio.flatten()[k]), at=at, over=int((~(d <= bound)).sum()), max_abs=float(d.max()))


def pool_mismatches(full: torch.Tensor, pooled: torch.Tensor) -> int:
    """Pooled tensor vs maxpool2 of the full-resolution one, decoded values (exact in every mode)."""
    return int((F.max_pool2d(full, 2, 2) != pooled).sum())


# ---- heads ----------------------------------------------------------------------------------------------------------------------
def ref_spec_tail(sd, s9: torch.Tensor) -> Ref:
    """spec = relu(conv1x1(s9) + b) (spec_output_conv.1), from the device's s9 in layer units; an fp32 epilogue."""
    w = _t(sd["spec_output_conv.1.weight"]).to(torch.float32).to(torch.float64)
    b = _t(sd["spec_output_conv.1.bias"]).to(torch.float32).to(torch.float64)
    return Ref(conv(s9, w, b, pad=0), conv(s9.abs(), w.abs(), b.abs(), pad=0))


def mask_head(sd, flat: torch.Tensor, absolute: bool = False) -> torch.Tensor:
    """mask_output_conv (ResBlock1D + Conv1d) on flat (N, 4, 256); absolute: the magnitude pass (|w|, |b|, ReLU the identity)."""
    def f1(p):
        w, b = fold(sd, p[0], p[1])
        return (w.abs(), b.abs()) if absolute else (w, b)
    relu = (lambda t: t) if absolute else F.relu
    pfx = "mask_output_conv.0"
    w1, b1 = f1((pfx + ".conv1.0", pfx + ".conv1.1"))
    w2, b2 = f1((pfx + ".conv2.0", pfx + ".conv2.1"))
    wr, br = f1((pfx + ".residual.0", pfx + ".residual.1"))
    idt = F.conv1d(flat, wr, br)
    out = relu(F.conv1d(flat, w1, b1, padding=1))
    out = relu(F.conv1d(out, w2, b2, padding=1) + idt)
    wo = _t(sd["mask_output_conv.1.weight"]).to(torch.float32).to(torch.float64)
    bo = _t(sd["mask_output_conv.1.bias"]).to(torch.float32).to(torch.float64)
    if absolute:
        wo, bo = wo.abs(), bo.abs()
    return F.conv1d(out, wo, bo)


def flatten_weights(sd):
    w = _t(sd["conv_flatten.weight"]).to(torch.float32).to(torch.float64)
    b = _t(sd["conv_flatten.bias"]).to(torch.float32).to(torch.float64)
    return w, b


def flatten_log2_rms(sd, e_c9) -> float:
    """log2 of the rms of conv_flatten's weights with their columns on conv9_1's normalised channels (wf 2^-e[ci])."""
    wf, _ = flatten_weights(sd)
    return float(torch.log2(torch.sqrt((scale_w(wf, None, torch.as_tensor(e_c9, dtype=torch.int64)) ** 2).mean())))


def flatten_scale(sd, e_c9, mode: str) -> int:
    """The common exponent that the flatten partial sums carry (weights.hip s_common): f16x2 puts the rms of the filter, columns on
    normalised inputs, at 2^-4: -round(log2 rms) - 4, clamped to [-60, 60] (0 for an all-zero filter); fp32 and bf16 scale nothing.
    (Until the checkpoint zoo it was the median of conv9_1's exponents, which is the same number while those lie together and says
    nothing about the filter once they do not: weights.hip build_model.)"""
    if mode != "f16x2":
        return 0
    l = flatten_log2_rms(sd, e_c9)
    return int(max(-60, min(60, -round(l) - 4))) if np.isfinite(l) else 0


def ref_flatten(sd, c9n: torch.Tensor, e_c9, mode: str):
    """conv_flatten's sums (before bias and ReLU) from conv9_1's output as the device holds it (normalised units, NCHW; the flatten in
    the B launch's epilogue multiplies exactly these values: fp32, the bf16 rounding, or the stored f16 pair).  -> (ref, bound), both
    (N, 4, W) in the units of the device's partial sums, 2^s_common x layer units.  The filter is the device's: wf 2^(s_common - e[ci])
    (f2bf of it in bf16, an f16 pair in f16x2).  Bound: TOL M over the 4096 products, plus in f16x2 the filter's subnormal low halves
    (2^-25 sum |c9|)."""
    e = torch.as_tensor(e_c9, dtype=torch.int64)
    wf, _ = flatten_weights(sd)
    wfs = scale_w(wf, torch.full((4,), flatten_scale(sd, e, mode)), e).to(torch.float32).to(torch.float64)
    if mode == "bf16":
        wfs = bf16_rn(wfs)
    ref = conv(c9n, wfs, pad=0).squeeze(2)
    bound = TOL[mode] * conv(c9n.abs(), wfs.abs(), pad=0).squeeze(2)
    if mode == "f16x2":
        bound = bound + FLOOR * c9n.abs().sum((1, 2)).unsqueeze(1)
    return ref, bound


def ref_head(sd, parts: torch.Tensor, e_c9, mode: str):
    """mask_head_parts from the device's partial sums parts (N, G, 4, W): sum over the row groups, x 2^-s_common, + conv_flatten's
    bias, ReLU, ResBlock1D + Conv1d -> logits (N, 1, W).  The kernel is fp32 in every mode: bound 2^-17 M, M the head's magnitude
    graph on sum_g |parts| 2^-s_common + |b| (the fixed-order fp32 sum of at most 16 partials included)."""
    fscale = 2.0 ** -flatten_scale(sd, e_c9, mode)
    _, bfl = flatten_weights(sd)
    s = parts.sum(1) * fscale
    logits = mask_head(sd, F.relu(s + bfl.view(1, -1, 1)))
    M = mask_head(sd, parts.abs().sum(1) * fscale + bfl.abs().view(1, -1, 1), absolute=True)
    return logits, TOL["fp32"] * M
