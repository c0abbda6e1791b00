"""conv1_1.B as the row-streaming kernel on eight 32-column strips (csrc/conv1s.hip, conv1_stream16_kernel) at its SEAMS.  A strip's
taps of dx = -1 / +1 read h1 one column outside the strip, which a third first-conv tile produces (in-picture: the neighbouring strip's
own value; left of strip 0 and right of strip 7: the second conv's zero padding), and a band's first and last row read h1 rows of the
neighbouring band.  On a short signal (a stretch of the synthetic recording, then full-scale white noise: every mel row and every column
differs) and five windows -- the leading pad (zero features), a voiced one, one across the recording's end, one inside the noise, the
last (zero padding inside the image) -- both planes of c1 and p1 are read back and
  (a) held to tests/layer_ref.py's float64 reference and derived bound (ratio <= 1, nothing over), with the worst ratio printed and
      asserted per class of position: strip seams (columns 32 k - 1, 32 k), picture edge columns, band seams (rows 16 k - 1, 16 k),
      edge rows, interior;
  (b) the same bits for passes of 5, 2 + 2 + 1 and 1 windows, for 16-row units (SOFTSPOKEN_C1S_ROWS=16) and with the per-value range
      test (SOFTSPOKEN_C1S_TRACK=1);
  (c) p1 = maxpool2x2 of the stored c1 exactly, both tensors canonically split;
  (d) on the zero-feature window c1 does not depend on the column away from the picture's edges: columns 2 .. 253 of a row hold the
      same bits (a halo that is not the neighbour's value, or a mask on an interior strip, breaks this).
One child process per switch set on the development library (the switches are read when the library loads)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"base": "conv1_stream16_kernel<false>/conv1_1.B", "rows16": "conv1_stream16_kernel<false>/conv1_1.B",
           "track": "conv1_stream16_kernel<true>/conv1_1.B"}
CLASSES = ("strip_seams", "edge_cols", "band_seams", "edge_rows", "interior")

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

def run(windows, chunk):
    # -> the planes [c1 hi, c1 lo, p1 hi, p1 lo] of the LAST pass (the workspace holds one pass)
    ctx.set_chunk(chunk)
    ctx.reset_stats()
    ctx.infer_windows(fid, windows, want_spec=False)
    n = len(windows) if chunk >= len(windows) else (len(windows) - 1) % chunk + 1
    c1, p1 = ctx.debug_activation("c1", 0, n), ctx.debug_activation("p1", 0, n)
    return [np.asarray(c1["planes"][0]), np.asarray(c1["planes"][1]), np.asarray(p1["planes"][0]), np.asarray(p1["planes"][1])]

five = run(S, 5)
print("KERNEL", ";".join(k["name"] for k in ctx.kernel_stats() if k["name"].endswith("/conv1_1.B")), flush=True)
out = {{"five%d" % i: a for i, a in enumerate(five)}}

def get(name, n):
    d = ctx.debug_activation(name, 0, n)
    return torch.from_numpy(d["value"]).permute(0, 3, 1, 2).contiguous(), torch.as_tensor(d["exponents"].astype(np.int64)), d

if {full!r}:
    # (a) the float64 reference: compare()'s want and bound (f16x2: want = relu(pre), bound = the derived deviation), kept per element
    feat, _, _ = get("feat", 5)
    c1, e1, d1 = get("c1", 5)
    p1, _, dp = get("p1", 5)
    e_h = torch.as_tensor(ctx.debug_activation("h1", 0, 0)["exponents"].astype(np.int64))
    ref = R.ref_conv1_1(R.block_weights(sd, "conv1_1"), feat, mode, e_h, "conv4")
    rep = R.compare(c1, ref, e1, mode)
    want = torch.relu(R.scale(ref.pre, e1))
    bound = R.scale(R.deviation(ref, e1, mode), e1)
    d = (c1 - want).abs()
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bound)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    assert float(ratio.max()) == rep["ratio"], (float(ratio.max()), rep["ratio"])
    over = ~(d <= bound)
    H, W = ratio.shape[2], ratio.shape[3]
    col = torch.zeros(W, dtype=torch.bool); row = torch.zeros(H, dtype=torch.bool)
    ecol = torch.zeros(W, dtype=torch.bool); erow = torch.zeros(H, dtype=torch.bool)
    for k in range(1, W // 32): col[32 * k - 1] = col[32 * k] = True
    for k in range(1, H // 16): row[16 * k - 1] = row[16 * k] = True
    ecol[0] = ecol[W - 1] = True; erow[0] = erow[H - 1] = True
    ones = torch.ones(H, W, dtype=torch.bool)
    cls = dict(strip_seams=ones & col[None, :], edge_cols=ones & ecol[None, :], band_seams=ones & row[:, None], edge_rows=ones & erow[:, None])
    cls["interior"] = ~(cls["strip_seams"] | cls["edge_cols"] | cls["band_seams"] | cls["edge_rows"])
    for name, m in cls.items():
        print("CLASS", name, int(m.sum()), "%.4g" % float(ratio[:, :, m].max()), int(over[:, :, m].sum()), flush=True)
    print("ALL", "%.4g" % rep["ratio"], rep["over"], flush=True)
    # (c) the pooled tensor and the splits
    print("EXACT", R.pool_mismatches(c1, p1), R.canonical_split_mismatches(d1["planes"][0], d1["planes"][1]),
          R.canonical_split_mismatches(dp["planes"][0], dp["planes"][1]), flush=True)
    # (d) window 0 has zero features: away from the picture's edge columns a row's pixels are all alike
    assert not feat[0].any(), "window 0 is not the leading pad"
    z = [a[0] for a in five[:2]]
    print("ZERO", sum(int((a[:, 2:254] != a[:, 2:3]).sum()) for a in z), flush=True)
    # (b) the pass cuts: 2 + 2 + 1 (last pass: window 4), 2 + 2 (windows 2, 3), 2 (windows 0, 1); five passes of one window
    for tag, wins, chunk, sl in (("c221", S, 2, slice(4, 5)), ("c22", S[:4], 2, slice(2, 4)), ("c2", S[:2], 2, slice(0, 2))):
        got = run(wins, chunk)
        print("CUT", tag, int(all(np.array_equal(g, f[sl]) for g, f in zip(got, five))), flush=True)
    for k in range(5):
        got = run(S[k:k + 1], 1)
        print("CUT", "one%d" % k, int(all(np.array_equal(g, f[k:k + 1]) for g, f in zip(got, five))), flush=True)
np.savez({out_npz!r}, **out)
print("CHILD_OK", flush=True)
"""


@pytest.fixture(scope="module")
def seam_signal(tmp_path_factory):
    """6 s of the synthetic recording, then 3.2 s of full-scale white noise; five of its windows."""
    from softspoken_amd import synth
    from oracle import oracle_np as O
    pcm = synth.to_pcm16(synth.synth_audio(1001, 6.0, 16000, 1))
    rec, _, _ = O.load_audio_from_bytes(synth.wav_bytes(pcm, 16000))
    noise = np.random.default_rng(11).uniform(-1.0, 1.0, int(3.2 * 22050)).astype(np.float32)
    sig = np.concatenate([rec, noise]).astype(np.float32)
    starts = O.plan_windows(len(sig) / 22050.0)
    padded = O.pad_3s(sig)
    rms = np.array([np.sqrt(np.mean(padded[s:s + 66150].astype(np.float64) ** 2)) for s in starts])
    lead = 66150                                          # the leading pad's samples
    in_rec = np.flatnonzero(starts + 66150 <= lead + len(rec))
    voiced = int(in_rec[np.argmax(rms[in_rec])])
    in_noise = np.flatnonzero((starts >= lead + len(rec)) & (starts + 66150 <= lead + len(sig)))
    across = np.flatnonzero((starts < lead + len(rec)) & (starts + 66150 > lead + len(rec)))
    assert rms[0] == 0.0 and len(in_noise) and len(across)
    sel = sorted({0, voiced, int(across[len(across) // 2]), int(in_noise[0]), len(starts) - 1})
    assert len(sel) == 5 and sel[0] == 0, sel
    d = tmp_path_factory.mktemp("c1s_seams")
    np.save(d / "sig.npy", sig)
    return dict(dir=str(d), sig=str(d / "sig.npy"), sel=sel)


@pytest.fixture(scope="module")
def runs(seam_signal, build_all):
    from softspoken_amd import build as hip_build
    res = {}
    for tag, env in (("base", {}), ("rows16", {"SOFTSPOKEN_C1S_ROWS": "16"}), ("track", {"SOFTSPOKEN_C1S_TRACK": "1"})):
        out = os.path.join(seam_signal["dir"], tag + ".npz")
        code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), sig_npy=seam_signal["sig"], sel=seam_signal["sel"], full=tag == "base",
                             out_npz=out)
        e = dict(os.environ); e.update(env); e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
        r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
        lines = [l.split() for l in r.stdout.splitlines() if l.split(" ")[0] in ("KERNEL", "CLASS", "ALL", "EXACT", "ZERO", "CUT")]
        print(tag, "\n".join(" ".join(l) for l in lines))
        assert r.returncode == 0 and "CHILD_OK" in r.stdout.splitlines(), r.stdout[-2000:] + r.stderr[-3000:]
        res[tag] = dict(lines=lines, **np.load(out))
    return res


def _lines(run, key):
    return [l[1:] for l in run["lines"] if l[0] == key]


def test_the_kernel_under_test(runs):
    for tag, name in KERNELS.items():
        assert _lines(runs[tag], "KERNEL") == [[name]], (tag, _lines(runs[tag], "KERNEL"))


@pytest.mark.parametrize("cls", CLASSES)
def test_float64_bound_per_class(runs, cls):
    """(a) every class of position on its own: a seam's error must not hide behind the maximum over the picture."""
    got = {l[0]: l[1:] for l in _lines(runs["base"], "CLASS")}
    assert sorted(got) == sorted(CLASSES)
    count, ratio, over = int(got[cls][0]), float(got[cls][1]), int(got[cls][2])
    assert count > 0 and ratio <= 1.0 and over == 0, (cls, got[cls])
    (all_ratio, all_over), = _lines(runs["base"], "ALL")
    assert float(all_ratio) <= 1.0 and int(all_over) == 0


def test_pass_cuts_give_the_same_bits(runs):
    """(b) 5 | 2 + 2 + 1 | 1: both planes of c1 and of p1."""
    cuts = {l[0]: int(l[1]) for l in _lines(runs["base"], "CUT")}
    assert sorted(cuts) == sorted(["c221", "c22", "c2"] + ["one%d" % k for k in range(5)]) and all(cuts.values()), cuts


@pytest.mark.parametrize("tag", ["rows16", "track"])
def test_unit_rows_and_range_test_give_the_same_bits(runs, tag):
    """(b) 16-row units: eight bands, every band seam at another row; TRACK: the other instantiation."""
    for i in range(4):
        assert np.array_equal(runs[tag]["five%d" % i], runs["base"]["five%d" % i]), (tag, i)


def test_pool_and_splits_exact(runs):
    """(c)"""
    (l,) = _lines(runs["base"], "EXACT")
    assert [int(x) for x in l] == [0, 0, 0], l


def test_zero_features_do_not_see_the_strips(runs):
    """(d)"""
    (l,) = _lines(runs["base"], "ZERO")
    assert int(l[0]) == 0, l
