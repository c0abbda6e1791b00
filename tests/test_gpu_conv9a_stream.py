"""conv9_1.A as a row-streaming kernel (csrc/conv9a.hip) against conv4_ups.hip's form of the same launch (development build,
SOFTSPOKEN_C9A=0), on the five-window signal of test_gpu_layers (every strip, both picture edges, the zero-padded tail) with the float64
reference and derived bound of tests/layer_ref.py:
  * both forms: every stored value of h9 within compare()'s bound of ref_A computed from the device's own c1 and c8, its planes a
    canonical split;
  * the streaming form's work units are independent and a row's arithmetic does not depend on how the work is cut: passes of 5,
    2 + 2 + 1, 1 and 2 windows, one workgroup instead of a full grid (a wave then walks 20 units in a row: the state carried between
    units) and 16-row units (band-edge halo rows, the other cut of the six-step role cycle) give the same bits, both planes of h9 and
    the logits;
  * the range test: conv9_1's first BatchNorm gain scaled up (without the channel normalisation, which would take it out) makes the
    pass report SS_ERR_RANGE, which the fp32 mode answers; the unscaled checkpoint does not raise the flag.
One child process per configuration (the switches are read when the library loads); each runs the network once per pass size."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STREAM = "conv3x3_ups_stream16_kernel/conv9_1.A"
TILES = "conv3x3_ups_kernel/conv9_1.A"

_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
torch.set_grad_enabled(False)
from softspoken_amd import native, checkpoint
from oracle import oracle_np as O
import layer_ref as R
import checkpoint_zoo as Z
mode = "f16x2"
sd = Z.build("seed0")
sig = np.load({sig_npy!r})
S = O.plan_windows(len(sig) / 22050.0)[{sel!r}]
ctx = native.Context(checkpoint.pack_state_dict(sd), 0, precision=mode, chunk=5)
fid = ctx.add_f32_22k(sig)
out = {{}}

def get(name, n):
    d = ctx.debug_activation(name, 0, n)
    return torch.from_numpy(d["value"]).permute(0, 3, 1, 2).contiguous(), torch.as_tensor(d["exponents"].astype(np.int64)), d

def run(windows, chunk):
    ctx.set_chunk(chunk)
    ctx.reset_stats()
    _, mask = ctx.infer_windows(fid, windows, want_spec=False)
    n = len(windows) if chunk >= len(windows) else (len(windows) - 1) % chunk + 1
    return mask, np.stack(ctx.debug_activation("h9", 0, n)["planes"])

mask, h9p = run(S, 5)
names = [k["name"] for k in ctx.kernel_stats() if k["name"].endswith("/conv9_1.A")]
print("KERNEL", ";".join(names), flush=True)
out.update(mask5=mask, h9_5=h9p)
# the float64 reference, from the tensors the device stored
c1, e1, _ = get("c1", 5); c8, e8, _ = get("c8", 5); h, e_h, d_h = get("h9", 5)
x, ex = R.block_input(R.scale(c1, -e1), R.scale(c8, -e8)), torch.cat([e1, e8])
rep = R.compare(h, R.ref_A(R.block_weights(sd, "conv9_1"), x, mode, ex), e_h, mode)
print("H9", "%.4g" % rep["ratio"], rep["over"], R.canonical_split_mismatches(d_h["planes"][0], d_h["planes"][1]), flush=True)
if {sizes!r}:
    m, p = run(S, 2);      out.update(mask221=m, h9_221=p)       # passes of 2 + 2 + 1: the last pass holds window 4
    m, p = run(S, 1);      out.update(mask1=m, h9_1=p)           # five passes of one window
    m, p = run(S[1:3], 2); out.update(mask2=m, h9_2=p)           # one pass of two windows (1 and 2)
np.savez({out_npz!r}, **out)
print("CHILD_OK", flush=True)
"""

_RANGE = r"""
import sys, numpy as np
sys.path.insert(0, {root!r})
from softspoken_amd import synth, native, checkpoint
sig = np.load({sig_npy!r})
from oracle import oracle_np as O
S = O.plan_windows(len(sig) / 22050.0)[{sel!r}]
def logits(sd, prec):
    c = native.Context(checkpoint.pack_state_dict(sd), 0, precision=prec, chunk=5)
    fid = c.add_f32_22k(sig)
    try:
        _, m = c.infer_windows(fid, S, want_spec=False)
        names = [k["name"] for k in c.kernel_stats() if k["name"].endswith("/conv9_1.A")]
        assert prec != "f16x2" or names == [{stream!r}], names
        return m
    finally:
        c.close()
sd = synth.make_state_dict(0)
assert np.isfinite(logits(sd, "f16x2")).all()               # the unscaled checkpoint does not raise the flag
# the largest gain under which every packed weight of conv9_1's first conv still has an f16 representation (30000 < 65504) -- the folded
# taps and, on the upsampled half's channels, the pre-summed ones (sums over the row sets x the column sets of the parity classes): the
# weights are accepted, the launch's outputs -- sums of 576 such terms -- are not representable
w = sd["conv9_1.conv1.0.weight"].astype(np.float64)
g = sd["conv9_1.conv1.1.weight"].astype(np.float64) / np.sqrt(sd["conv9_1.conv1.1.running_var"].astype(np.float64) + 1e-5)
wf = w * g.reshape(-1, 1, 1, 1)
sets = ([0], [1, 2], [0, 1], [2])
pre = max(float(np.abs(wf[:, 32:][:, :, r][:, :, :, c].sum((2, 3))).max()) for r in sets for c in sets)
gain = 30000.0 / max(float(np.abs(wf).max()), pre)
big = {{k: v.copy() for k, v in sd.items()}}
big["conv9_1.conv1.1.weight"] = (big["conv9_1.conv1.1.weight"] * np.float32(gain)).astype(np.float32)
try:
    logits(big, "f16x2")
    raise SystemExit("no range error")
except native.NativeError as e:
    assert e.code == 8 == native.SS_ERR_RANGE and "f16 range" in str(e), e
assert np.isfinite(logits(big, "fp32")).all()               # ... and the fp32 re-run answers
print("RANGE_OK")
"""


@pytest.fixture(scope="module")
def signal(tmp_path_factory):
    import test_gpu_layers as TL
    return TL.layer_signal.__wrapped__(tmp_path_factory) if hasattr(TL.layer_signal, "__wrapped__") else TL.layer_signal.__pytest_wrapped__.obj(tmp_path_factory)


@pytest.fixture(scope="module")
def runs(signal, build_all):
    """Each configuration's child, once: its printed checks and its saved bits."""
    from softspoken_amd import build as hip_build
    res = {}
    for tag, env, sizes in (("stream", {}, True), ("tiles", {"SOFTSPOKEN_C9A": "0"}, False), ("grid1", {"SOFTSPOKEN_C9A_GRID": "1"}, False),
                            ("rows16", {"SOFTSPOKEN_C9A_ROWS": "16"}, False)):
        out = os.path.join(signal["dir"], "c9a_" + tag + ".npz")
        code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), sig_npy=signal["sig"], sel=signal["sel"], sizes=sizes, out_npz=out)
        e = dict(os.environ); e.update(env); e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
        r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
        lines = r.stdout.splitlines()
        print(tag, "\n".join(l for l in lines if l.split(" ")[0] in ("KERNEL", "H9")))
        assert r.returncode == 0 and "CHILD_OK" in lines, r.stdout[-2000:] + r.stderr[-3000:]
        res[tag] = dict(lines={l.split()[0]: l.split()[1:] for l in lines if l.split(" ")[0] in ("KERNEL", "H9")}, **np.load(out))
    return res


@pytest.mark.parametrize("tag,kernel", [("stream", STREAM), ("tiles", TILES)])
def test_both_forms_within_the_float64_bound(runs, tag, kernel):
    """Five windows: h9 against ref_A under compare()'s bound, its planes a canonical split -- the project's derived bound, as
    test_gpu_layers holds every launch to."""
    l = runs[tag]["lines"]
    assert l["KERNEL"] == [kernel], l["KERNEL"]
    assert float(l["H9"][0]) <= 1.0 and int(l["H9"][1]) == 0 and int(l["H9"][2]) == 0, l["H9"]


def test_pass_size_does_not_change_a_bit(runs):
    r = runs["stream"]
    assert np.array_equal(r["h9_221"], r["h9_5"][:, 4:5]) and np.array_equal(r["h9_1"], r["h9_5"][:, 4:5]) and np.array_equal(r["h9_2"], r["h9_5"][:, 1:3])
    assert np.array_equal(r["mask221"], r["mask5"]) and np.array_equal(r["mask1"], r["mask5"]) and np.array_equal(r["mask2"], r["mask5"][1:3])


def test_one_workgroup_gives_the_bits_of_the_full_grid(runs):
    """SOFTSPOKEN_C9A_GRID=1: 160 units on eight waves, 20 in a row on each (the full grid never gives a wave a second unit below 65
    windows): what a wave carries from one unit to the next -- the fragment ring's slots, the operand rows -- must not reach the results."""
    a, b = runs["stream"], runs["grid1"]
    assert b["lines"]["KERNEL"] == [STREAM]
    assert np.array_equal(a["h9_5"], b["h9_5"]) and np.array_equal(a["mask5"], b["mask5"])


def test_sixteen_row_units(runs):
    """SOFTSPOKEN_C9A_ROWS=16: eight bands per window instead of four.  A row's arithmetic does not depend on the cut (the halo rows at
    a band's edges are read from c1 and c8 like any other row): the same bits of h9, and so the same logits."""
    a, b = runs["stream"], runs["rows16"]
    assert b["lines"]["KERNEL"] == [STREAM]
    assert np.array_equal(a["h9_5"], b["h9_5"]) and np.array_equal(a["mask5"], b["mask5"])


def test_range_flag(signal, build_all):
    from softspoken_amd import build as hip_build
    e = dict(os.environ); e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB; e["SOFTSPOKEN_NORM"] = "0"
    code = _RANGE.format(root=ROOT, sig_npy=signal["sig"], sel=signal["sel"], stream=STREAM)
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RANGE_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
