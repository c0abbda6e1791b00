"""conv9_1.B as a row-streaming kernel (csrc/conv9s.hip) against conv4.hip's form of the same launch (development build,
SOFTSPOKEN_C9S=0), on the five-window signal of test_gpu_layers (every strip, both picture edges, the zero-padded tail) with the float64
references and derived bounds of tests/layer_ref.py:
  * both forms, spec pass: every stored value of c9 within compare()'s bound of ref_B, the flatten sums within ref_flatten's bound;
  * the streaming form's work units are independent and its arithmetic does not depend on how the work is cut: passes of 5, 2 + 2 + 1
    and 1 windows, and one workgroup instead of a full grid (a wave then walks 22 units in a row: the state carried between units),
    give the same bits, logits and c9 planes; 16-row units give the same c9 planes (band-edge halo rows) and logits within the head's
    bound (the flatten's partial sums are cut differently);
  * the range test: conv9_1's second BatchNorm gain scaled up (without the channel normalisation, which would take it out) makes the
    mask-only pass report SS_ERR_RANGE, which the fp32 mode answers; the unscaled checkpoint does not raise the flag.
One child process per configuration (the switches are read when the library loads); each runs the network once per pass size."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

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
L = native.lib()
out = {{}}

def get(name, n):
    d = ctx.debug_activation(name, 0, n)
    return torch.from_numpy(d["value"]).permute(0, 3, 1, 2).contiguous(), torch.as_tensor(d["exponents"].astype(np.int64)), d

def run(windows, chunk, spec=True):
    ctx.set_chunk(chunk)
    ctx.reset_stats()
    _, mask = ctx.infer_windows(fid, windows, want_spec=spec)
    n = len(windows) if chunk >= len(windows) else (len(windows) - 1) % chunk + 1
    d = ctx.debug_activation("c9", 0, n) if spec else None
    return mask, (np.stack(d["planes"]) if spec else None), ctx.debug_activation("flat_part", 0, n)["planes"][0]

mask, c9p, parts = run(S, 5)
names = [k["name"] for k in ctx.kernel_stats() if k["name"].endswith("/conv9_1.B")]
print("KERNEL", ";".join(names), flush=True)
out.update(mask5=mask, c9_5=c9p, parts5=parts)
# the float64 references, from the tensors the device stored
c1, e1, _ = get("c1", 5); c8, e8, _ = get("c8", 5); h, e_h, _ = get("h9", 5); y, e_y, d_y = get("c9", 5)
x, ex = R.block_input(R.scale(c1, -e1), R.scale(c8, -e8)), torch.cat([e1, e8])
buf = np.zeros(1, np.uint8)
r_stored = L.ss_debug_activation(ctx._h, b"r9", 0, 0, 0, native._ptr(buf), 0, None, None) == native.SS_ERR_ARG
rep = R.compare(y, R.ref_B(R.block_weights(sd, "conv9_1"), R.scale(h, -e_h), x, mode, r_stored, e_h, ex), e_y, mode)
print("C9", "%.4g" % rep["ratio"], rep["over"], R.canonical_split_mismatches(d_y["planes"][0], d_y["planes"][1]), flush=True)
ref, bound = R.ref_flatten(sd, y, e_y, mode)
rep = R.ratio_report(torch.from_numpy(parts.astype(np.float64)).sum(1), ref, bound)
print("FLATTEN", "%.4g" % rep["ratio"], rep["over"], parts.shape[1], flush=True)
lg, bound = R.ref_head(sd, torch.from_numpy(parts.astype(np.float64)), torch.as_tensor(ctx.debug_activation("c9", 0, 0)["exponents"].astype(np.int64)), mode)
rep = R.ratio_report(torch.from_numpy(mask).double(), lg, bound)
print("HEAD", "%.4g" % rep["ratio"], rep["over"], flush=True)
if {sizes!r}:
    m, c, _ = run(S, 2);      out.update(mask221=m, c9_221=c)       # passes of 2 + 2 + 1: the last pass holds window 4
    m, c, _ = run(S, 1);      out.update(mask1=m, c9_1=c)           # five passes of one window
    m, c, _ = run(S[1:3], 2); out.update(mask2=m, c9_2=c)           # one pass of two windows (1 and 2)
    m, _, p = run(S, 5, spec=False); out.update(mask_nospec=m, parts_nospec=p)
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
        _, m = c.infer_windows(fid, S, want_spec=False)      # the mask-only pass: c9 is not stored, its split values feed the flatten
        names = [k["name"] for k in c.kernel_stats() if k["name"].endswith("/conv9_1.B")]
        assert prec != "f16x2" or names == ["conv9_stream16_kernel/conv9_1.B"], names
        return m
    finally:
        c.close()
sd = synth.make_state_dict(0)
assert np.isfinite(logits(sd, "f16x2")).all()               # the unscaled checkpoint does not raise the flag
# the largest gain under which every folded weight of conv9_1's second conv still has an f16 representation (30000 < 65504): the
# weights are accepted, the block's outputs -- sums of 288 such terms -- are not representable
w = sd["conv9_1.conv2.0.weight"].astype(np.float64)
g = sd["conv9_1.conv2.1.weight"].astype(np.float64) / np.sqrt(sd["conv9_1.conv2.1.running_var"].astype(np.float64) + 1e-5)
gain = 30000.0 / float(np.abs(w * g.reshape(-1, 1, 1, 1)).max())
big = {{k: v.copy() for k, v in sd.items()}}
big["conv9_1.conv2.1.weight"] = (big["conv9_1.conv2.1.weight"] * np.float32(gain)).astype(np.float32)
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
    for tag, env, sizes in (("stream", {}, True), ("tiles", {"SOFTSPOKEN_C9S": "0"}, False), ("grid1", {"SOFTSPOKEN_C9S_GRID": "1"}, False),
                            ("rows16", {"SOFTSPOKEN_C9S_ROWS": "16"}, False)):
        out = os.path.join(signal["dir"], "c9s_" + tag + ".npz")
        code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), sig_npy=signal["sig"], sel=signal["sel"], sizes=sizes, out_npz=out)
        e = dict(os.environ); e.update(env); e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
        r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
        lines = r.stdout.splitlines()
        print(tag, "\n".join(l for l in lines if l.split(" ")[0] in ("KERNEL", "C9", "FLATTEN", "HEAD")))
        assert r.returncode == 0 and "CHILD_OK" in lines, r.stdout[-2000:] + r.stderr[-3000:]
        res[tag] = dict(lines={l.split()[0]: l.split()[1:] for l in lines if l.split(" ")[0] in ("KERNEL", "C9", "FLATTEN", "HEAD")}, **np.load(out))
    return res


@pytest.mark.parametrize("tag,kernel,groups", [("stream", "conv9_stream16_kernel/conv9_1.B", 4), ("tiles", None, 8)])
def test_both_forms_within_the_float64_bounds(runs, tag, kernel, groups):
    """Spec pass, five windows: c9 against ref_B under compare()'s bound (and its planes a canonical split), the flatten's group sums
    against ref_flatten, the logits against ref_head -- the project's derived bounds, as test_gpu_layers holds every launch to."""
    l = runs[tag]["lines"]
    assert (l["KERNEL"] == [kernel]) if kernel else ("conv3x3_v4_kernel" in l["KERNEL"][0] and ";" not in " ".join(l["KERNEL"])), l["KERNEL"]
    assert float(l["C9"][0]) <= 1.0 and int(l["C9"][1]) == 0 and int(l["C9"][2]) == 0, l["C9"]
    assert float(l["FLATTEN"][0]) <= 1.0 and int(l["FLATTEN"][1]) == 0 and int(l["FLATTEN"][2]) == groups, l["FLATTEN"]
    assert float(l["HEAD"][0]) <= 1.0 and int(l["HEAD"][1]) == 0, l["HEAD"]


def test_pass_size_does_not_change_a_bit(runs):
    r = runs["stream"]
    assert np.array_equal(r["mask221"], r["mask5"]) and np.array_equal(r["mask1"], r["mask5"]) and np.array_equal(r["mask2"], r["mask5"][1:3])
    assert np.array_equal(r["c9_221"], r["c9_5"][:, 4:5]) and np.array_equal(r["c9_1"], r["c9_5"][:, 4:5]) and np.array_equal(r["c9_2"], r["c9_5"][:, 1:3])
    # the mask-only pass is the same kernel with store_out clear: the same partial sums, the same logits
    assert np.array_equal(r["parts_nospec"], r["parts5"]) and np.array_equal(r["mask_nospec"], r["mask5"])


def test_one_workgroup_gives_the_bits_of_the_full_grid(runs):
    """SOFTSPOKEN_C9S_GRID=1: 180 units on eight waves, 22 or 23 in a row on each (the full grid never gives a wave a second unit below
    57 windows): what a wave carries from one unit to the next must not reach the results."""
    a, b = runs["stream"], runs["grid1"]
    assert b["lines"]["KERNEL"] == ["conv9_stream16_kernel/conv9_1.B"]
    assert np.array_equal(a["mask5"], b["mask5"]) and np.array_equal(a["c9_5"], b["c9_5"]) and np.array_equal(a["parts5"], b["parts5"])


def test_sixteen_row_units(runs):
    """SOFTSPOKEN_C9S_ROWS=16: eight bands per window instead of four.  c9 does not depend on the cut (the halo rows at a band's edges
    are read from h9 like any other row): same bits.  The flatten's partial sums are cut differently, so the logits agree through the
    bounds: both runs' group sums lie within ref_flatten's bound of the flatten of the SAME c9 and each run's logits within ref_head's
    bound of the head of its own sums (asserted per child); what is left between the two is printed."""
    a, b = runs["stream"], runs["rows16"]
    l = b["lines"]
    assert l["KERNEL"] == ["conv9_stream16_kernel/conv9_1.B"] and int(l["FLATTEN"][2]) == 8 and b["parts5"].shape[1] == 8
    assert np.array_equal(a["c9_5"], b["c9_5"])
    assert float(l["C9"][0]) <= 1.0 and int(l["C9"][1]) == 0 and float(l["FLATTEN"][0]) <= 1.0 and int(l["FLATTEN"][1]) == 0
    assert float(l["HEAD"][0]) <= 1.0 and int(l["HEAD"][1]) == 0, l["HEAD"]
    print("max |logits(16-row units) - logits(32-row units)| = %.3g" % float(np.abs(a["mask5"] - b["mask5"]).max()))


def test_range_flag(signal, build_all):
    from softspoken_amd import build as hip_build
    e = dict(os.environ); e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB; e["SOFTSPOKEN_NORM"] = "0"
    code = _RANGE.format(root=ROOT, sig_npy=signal["sig"], sel=signal["sel"])
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RANGE_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
