"""Every launch of a network pass against a float64 reference computed from the tensors the device stored (tests/layer_ref.py; the
front-end launch: tests/frontend_ref.py, from the padded signal the device holds), and the spec head end to end against the float64
oracle.

The per-launch checks run in child processes on the development build (SOFTSPOKEN_LIB: ss_debug_activation reads the workspace back).
A child prints one line per launch,
    LAUNCH <config> <pass> <launch> <max |delta| / bound> <window,y,x,c of the max> <count over the bound> <exact-check mismatches>
and one COVER line for every plan name of kernel_stats() that has no check; the parent asserts on them.  An f16x2 child also prints
    EXPONENTS <config> <channels whose exponent is not the host emulation's> <channels excused as rounding ties> <the first few>
for the exponents ss_debug_activation reports for h1 ... hs, c1 ... s9 and the flatten's partial sums (tests/checkpoint_zoo.py
exponent_chain).  Every child also prints, per pass,
    PLAN <config> <pass> <JSON: [name, launches, flops, bytes, issued] of every kernel_stats() entry, in order>
and the parent holds these to tests/golden/launch_plan.json: which kernel form served which launch, how often, and what the engine
booked for it (names and counts equal, the three doubles to 1e-9 relative: reassociated double arithmetic moves them by about 1e-15,
a dropped term by far more).

The golden was recorded on an MI355X from the commit BEFORE the engine's block table and runner (0df854f), with only this file's PLAN
print applied there, not from the code under test: it pins the launch order, the form chosen for every launch under every switch set
below and the roofline bookkeeping across that rewrite."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_SPEC = 1e-4          # the fp32 parity bar (BASELINE.json north_star), on every value of the spec head
TOL_SPEC_BF16 = 0.15     # bf16: the throughput mode's stated score tolerance (test_bf16_mode)

# the ResBlocks behind conv1_1 in launch order: block, x0, x1, h, r, y, pool (tests/test_net_table.py holds them to csrc/net.h)
BLOCKS = [("conv2_1", "p1", None, "h2", "r2", "c2", "p2"), ("conv3_1", "p2", None, "h3", "r3", "c3", "p3"),
          ("conv4_1", "p3", None, "h4", "r4", "c4", "p4"), ("conv_bottleneck", "p4", None, "hb", "rb", "bott", None),
          ("encoder_out", "bott", None, "he", "re", "enc", None), ("conv6", "c4", "enc", "h6", "r6", "c6", None),
          ("conv7", "c3", "c6", "h7", "r7", "c7", None), ("conv8", "c2", "c7", "h8", "r8", "c8", None),
          ("conv9_1", "c1", "c8", "h9", "r9", "c9", None), ("spec_output_conv.0", "c9", None, "hs", "rs", "s9", None)]

_CHILD = r"""
import json, sys, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
torch.set_grad_enabled(False)
from softspoken_amd import synth, native, checkpoint
from oracle import oracle_np as O
import layer_ref as R
import frontend_ref as FR
import checkpoint_zoo as Z
tag, mode, ckpt, n_sel, out_npy = {tag!r}, {mode!r}, {ckpt!r}, {n_sel!r}, {out_npy!r}
sd = Z.build(ckpt)
sig = np.load({sig_npy!r})
starts = O.plan_windows(len(sig) / 22050.0)
ctx = native.Context(checkpoint.pack_state_dict(sd), 0, precision=mode, chunk=5)
fid = ctx.add_f32_22k(sig)
sel = {sel!r}[:n_sel] if n_sel == 5 else [{sel!r}[0], {sel!r}[3]]
S = starts[sel]
BLOCKS = {blocks!r}
W = {{b[0]: R.block_weights(sd, b[0]) for b in BLOCKS}}
W["conv1_1"] = R.block_weights(sd, "conv1_1")
L = native.lib()

def exps(name):
    return torch.as_tensor(ctx.debug_activation(name, 0, 0)["exponents"].astype(np.int64))

def get(name, n):
    d = ctx.debug_activation(name, 0, n)
    return torch.from_numpy(d["value"]).permute(0, 3, 1, 2).contiguous(), torch.as_tensor(d["exponents"].astype(np.int64)), d

def status(name):
    # 0: readable; SS_ERR_ARG for an r tensor: the pass wrote it (A + r / B); SS_ERR_STATE: the pass did not write it
    buf = np.zeros(1, np.uint8)
    return L.ss_debug_activation(ctx._h, name.encode(), 0, 0, 0, native._ptr(buf), 0, None, None)

def split_bad(d):
    return R.canonical_split_mismatches(d["planes"][0], d["planes"][1]) if mode == "f16x2" else 0

checked = set()
def report(pname, launch, rep, exact=0):
    checked.add(launch)
    at = rep["at"]
    print("LAUNCH", tag, pname, launch, "%.4g" % rep["ratio"], "%d,%d,%d,%d" % tuple(at[:4]) if len(at) >= 4 else ",".join(map(str, at)),
          rep["over"], exact, flush=True)

saved = {{}}
def check_pass(pname, n, with_spec, spec, logits):
    win = S[-n:]
    feat, _, _ = get("feat", n)
    pad = ctx.read_signal(fid, padded=True)
    # front-end: the float64 reference and interval bound of tests/frontend_ref.py, from the padded signal as the device holds it
    fe = FR.check(feat[:, 0].numpy(), FR.windows_of(pad, win), sd["mel_spectrogram.spectrogram.window"], sd["mel_spectrogram.mel_scale.fb"])
    report(pname, "frontend", dict(ratio=fe["ratio"], at=(fe["at"][0], fe["at"][1], fe["at"][2], 0), over=fe["over"]))
    c1, e_c1, d_c1 = get("c1", n)
    p1, e_p1, d_p1 = get("p1", n)
    form = "conv2" if any(k["name"].startswith("conv3x3_v2") and k["name"].endswith("/conv1_1.B") for k in ctx.kernel_stats()) else "conv4"
    report(pname, "conv1_1.B", R.compare(c1, R.ref_conv1_1(W["conv1_1"], feat, mode, exps("h1"), form), e_c1, mode),
           R.pool_mismatches(c1, p1) + split_bad(d_c1) + split_bad(d_p1))
    have = {{"c1": (c1, e_c1), "p1": (p1, e_p1)}}
    raw = {{"c1": d_c1["planes"]}}
    for blk, x0n, x1n, hn, rn, yn, pn in BLOCKS:
        if blk == "spec_output_conv.0" and not with_spec:
            break
        x0, e0 = have[x0n]
        x, ex = R.scale(x0, -e0), e0
        if x1n:
            x1, e1 = have[x1n]
            x, ex = R.block_input(x, R.scale(x1, -e1)), torch.cat([e0, e1])
        h, e_h, d_h = get(hn, n)
        raw[hn] = d_h["planes"]
        report(pname, blk + ".A", R.compare(h, R.ref_A(W[blk], x, mode, ex), e_h, mode), split_bad(d_h))
        r_stored = status(rn) == native.SS_ERR_ARG
        if yn == "c9" and not with_spec:
            # the flatten-only form: c9 is not stored (refused), the B launch's only output is the flatten's partial sums.  It is the
            # same kernel as the spec pass's (store_out is a run-time flag), so on the same inputs its partial sums must equal that
            # pass's bit for bit -- and those were held to conv_flatten of the stored c9 there.
            assert status("c9") == native.SS_ERR_STATE, "c9 readable after a pass that did not store it"
            parts = ctx.debug_activation("flat_part", 0, n)["planes"][0]
            same_in = all(all(np.array_equal(a, b) for a, b in zip(raw[t], saved[t])) for t in ("c1", "c8", "h9"))
            same = same_in and np.array_equal(parts, saved["flat_part"])
            report(pname, blk + ".B", dict(ratio=0.0 if same else float("inf"), at=(0, 0, 0, 0), over=0 if same else 1))
            break
        y, e_y, d_y = get(yn, n)
        raw[yn] = d_y["planes"]
        exact = split_bad(d_y)
        if pn:
            p, e_p, d_p = get(pn, n)
            exact += R.pool_mismatches(y, p) + split_bad(d_p)
            have[pn] = (p, e_p)
        report(pname, blk + ".B", R.compare(y, R.ref_B(W[blk], R.scale(h, -e_h), x, mode, r_stored, e_h, ex), e_y, mode), exact)
        have[yn] = (y, e_y)
        if yn == "c9":
            # conv_flatten in the same launch's epilogue: its partial sums against the flatten of the c9 it stored
            parts = ctx.debug_activation("flat_part", 0, n)["planes"][0]
            ref, bound = R.ref_flatten(sd, y, e_y, mode)
            got = torch.from_numpy(parts.astype(np.float64)).sum(1)
            report(pname, "conv9_1.B:flatten", R.ratio_report(got, ref, bound))
            if pname == "spec":
                saved.update({{t: raw[t] for t in ("c1", "c8", "h9")}}, flat_part=parts)
    parts = torch.from_numpy(ctx.debug_activation("flat_part", 0, n)["planes"][0].astype(np.float64))
    lg, bound = R.ref_head(sd, parts, exps("c9"), mode)
    report(pname, "mask_head_parts", R.ratio_report(torch.from_numpy(logits[-n:]).double(), lg, bound))
    if with_spec:
        s9, e_s9 = have["s9"]
        ref = R.ref_spec_tail(sd, R.scale(s9, -e_s9))
        report(pname, "spec_tail", R.compare(torch.from_numpy(spec[-n:]).double(), ref, None, "f16x2" if mode == "f16x2" else "fp32"))

def run(pname, with_spec, chunk):
    ctx.set_chunk(chunk)
    ctx.reset_stats()
    spec, mask = ctx.infer_windows(fid, S, want_spec=with_spec)
    n = len(S) if chunk >= len(S) else (len(S) - 1) % chunk + 1
    check_pass(pname, n, with_spec, spec, mask)
    for s in ctx.kernel_stats():
        if s["name"].split("/")[-1] not in checked:
            print("COVER", tag, pname, s["name"], flush=True)
    print("PLAN", tag, pname, json.dumps([[s["name"], s["launches"], s["flops"], s["bytes"], s["issued_flops"]] for s in ctx.kernel_stats()]), flush=True)
    checked.clear()
    return mask

mask = run("spec", True, 5)
np.save(out_npy, mask)
if mode == "f16x2":
    # the exponents the device chose against the stated rule, -round(log2(sqrt(1/2 sum w^2 + b^2))) through the whole graph on the host
    # (checkpoint_zoo.exponent_chain): the bounds above are in the device's own units and would hold for any choice
    bad, ties = Z.exponent_mismatches({{t: ctx.debug_activation(t, 0, 0)["exponents"] for t in Z.EXPONENT_TENSORS}}, sd)
    print("EXPONENTS", tag, len(bad), ties, ";".join("%s[%d]:%d!=%d" % b for b in bad[:8]), flush=True)
run("nospec", False, 5)
if n_sel == 5:
    run("ragged", True, 2)
if mode == "fp32":                                       # (every fp32 block runs as A + r / B: r2 written, refused as such)
    assert status("r2") == native.SS_ERR_ARG
assert L.ss_debug_activation(ctx._h, b"nope", 0, 0, 0, None, 0, None, None) == native.SS_ERR_ARG
buf = np.zeros(16, np.uint8)
assert L.ss_debug_activation(ctx._h, b"c1", 0, 0, 99, native._ptr(buf), 16, None, None) == native.SS_ERR_ARG
print("CHILD_OK", tag, flush=True)
"""


@pytest.fixture(scope="module")
def layer_signal(tmp_path_factory):
    """The C1 recording followed by 2 s of full-scale white noise, and the five windows: the leading pad (zero features), a voiced
    window, the 1e-3 burst (f16x2 low halves subnormal), one inside the noise (every mel row active) and the last (zero padding inside
    the image)."""
    from softspoken_amd import synth
    from oracle import oracle_np as O
    pcm = synth.to_pcm16(synth.synth_audio(1001, 60.0, 16000, 1))
    c1sig, _, _ = O.load_audio_from_bytes(synth.wav_bytes(pcm, 16000))
    noise = np.random.default_rng(7).uniform(-1.0, 1.0, 2 * 22050).astype(np.float32)
    sig = np.concatenate([c1sig, noise]).astype(np.float32)
    starts = O.plan_windows(len(sig) / 22050.0)
    d = tmp_path_factory.mktemp("layers")
    np.save(d / "sig.npy", sig)
    # window choice on the signal itself: the loudest C1 window, the quietest non-silent one (the burst), the first window that starts
    # inside the noise
    padded = O.pad_3s(sig)
    rms = np.array([np.sqrt(np.mean(padded[s:s + 66150].astype(np.float64) ** 2)) for s in starts])
    c1w = len(O.plan_windows(60.0))
    voiced = int(np.argmax(rms[:c1w]))
    nz = np.where(rms[:c1w] > 0, rms[:c1w], np.inf)
    burst = int(np.argmin(nz[1:]) + 1)
    noisew = int(np.argmax(starts >= len(c1sig) + 66150))
    sel = [0, voiced, burst, noisew, len(starts) - 1]
    return dict(dir=str(d), sig=str(d / "sig.npy"), sel=sel, starts=starts)


PLAN_GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plan.json")
PLAN_RTOL = 1e-9


def _check_plan(key, plans):
    """plans: {pass: [[name, launches, flops, bytes, issued], ...]} of one child against the golden's entry `key`."""
    with open(PLAN_GOLDEN) as f:
        want = json.load(f)[key]
    assert sorted(plans) == sorted(want), (key, sorted(plans), sorted(want))
    for pname, got in plans.items():
        w = want[pname]
        assert [g[:2] for g in got] == [x[:2] for x in w], "%s %s: launches differ\n  got  %s\n  want %s" % (key, pname, [g[:2] for g in got], [x[:2] for x in w])
        bad = [(g, x) for g, x in zip(got, w) if any(abs(a - b) > PLAN_RTOL * abs(b) for a, b in zip(g[2:], x[2:]))]
        assert not bad, "%s %s: booked flops / bytes / issued differ, first: got %s want %s" % ((key, pname) + bad[0])


def _child(tag, mode, env, layer_signal, n_sel=5, hostile=False, ckpt=None, plan_key=None):
    """ckpt: a checkpoint of tests/checkpoint_zoo.py by name; without one, `hostile` picks between the two the suite had before it.
    plan_key: the child's entry in tests/golden/launch_plan.json (default: tag)."""
    from softspoken_amd import build as hip_build
    ckpt = ckpt or ("hostile" if hostile else "seed0")
    out_npy = os.path.join(layer_signal["dir"], tag + ".npy")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), tag=tag, mode=mode, ckpt=ckpt, n_sel=n_sel, out_npy=out_npy,
                         sig_npy=layer_signal["sig"], sel=layer_signal["sel"], blocks=BLOCKS)
    e = dict(os.environ); e.update(env); e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=900)
    lines = r.stdout.splitlines()
    print("\n".join(l[:400] for l in lines if l.startswith(("LAUNCH", "COVER", "EXPONENTS", "PLAN"))))
    assert r.returncode == 0 and any(l.startswith("CHILD_OK") for l in lines), r.stdout[-3000:] + r.stderr[-3000:]
    launches = [l.split() for l in lines if l.startswith("LAUNCH")]
    uncovered = [l for l in lines if l.startswith("COVER")]
    assert not uncovered, "launches without a check: " + "; ".join(uncovered)
    bad = [" ".join(l) for l in launches if not (float(l[4]) <= 1.0 and int(l[6]) == 0 and int(l[7]) == 0)]
    assert not bad, "launches over their bound:\n" + "\n".join(bad)
    expo = [l.split() for l in lines if l.startswith("EXPONENTS")]
    assert len(expo) == (1 if mode == "f16x2" else 0), expo
    assert all(int(l[2]) == 0 for l in expo), "device exponents off the rule: " + " ".join(expo[0])
    # the checkpoints are fixed, and none has a channel on a rounding tie: the excuse must not be where a wrong rule hides
    assert all(int(l[3]) == 0 for l in expo), "channels excused as rounding ties: " + " ".join(expo[0])
    plans = {l.split(" ", 3)[2]: json.loads(l.split(" ", 3)[3]) for l in lines if l.startswith("PLAN")}
    assert sorted(plans) == sorted(["spec", "nospec"] + (["ragged"] if n_sel == 5 else [])), sorted(plans)
    _check_plan(plan_key or tag, plans)
    return out_npy


_REFUSALS = r"""
import sys, numpy as np
sys.path.insert(0, {root!r})
from softspoken_amd import synth, native, checkpoint
from oracle import oracle_np as O
L = native.lib()
ctx = native.Context(checkpoint.pack_state_dict(synth.make_state_dict(0)), 0, precision="fp32")
buf = np.zeros(16, np.uint8)
def refused(name, code, words):
    rc = L.ss_debug_activation(ctx._h, name.encode(), 0, 0, 0, native._ptr(buf), 0, None, None)
    msg = L.ss_last_error(ctx._h).decode()
    assert rc == code and words in msg, (name, rc, msg)
refused("c1", native.SS_ERR_STATE, "no workspace")
sig = synth.synth_audio(3, 6.0, 22050, 1, with_silence=False).reshape(-1).astype(np.float32)
fid = ctx.add_f32_22k(sig)
n_win = len(O.plan_windows(len(sig) / 22050.0))
assert n_win >= 2
ctx.set_chunk((n_win + 1) // 2)                         # two passes: the second runs on the second lane (SOFTSPOKEN_LANES=2)
ctx.run_begin()
refused("c1", native.SS_ERR_STATE, "in flight")
ctx.run_end()
refused("c1", native.SS_ERR_STATE, "second lane")
ctx.infer_windows(fid, O.plan_windows(len(sig) / 22050.0)[:1])
assert L.ss_debug_activation(ctx._h, b"c1", 0, 0, 1, None, 0, None, None) == 0
refused("r2", native.SS_ERR_ARG, "fragment order")
refused("h1", native.SS_ERR_STATE, "did not write")
print("REFUSALS_OK")
"""


def test_readback_refusals(build_all):
    """ss_debug_activation refuses: no workspace yet, a run in flight, a last pass on the second lane, an r tensor (fragment order),
    a tensor the pass did not write."""
    from softspoken_amd import build as hip_build
    e = dict(os.environ); e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB; e["SOFTSPOKEN_LANES"] = "2"
    r = subprocess.run([sys.executable, "-c", _REFUSALS.format(root=ROOT)], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "REFUSALS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


PRODUCT = [("fp32", "fp32", False), ("f16x2", "f16x2", False), ("bf16", "bf16", False), ("hostile_f16x2", "f16x2", True),
           ("hostile_fp32", "fp32", True)]


@pytest.mark.parametrize("tag,mode,hostile", PRODUCT)
def test_every_launch_of_the_product_forms(tag, mode, hostile, layer_signal, build_all):
    """Product forms, five windows: a pass with the spec head, one without it (conv9_1.B's flatten-only form: its partial sums equal
    the spec pass's bit for bit), a ragged pass (chunk 2: the last pass holds one window).  The dev library's logits equal the product
    library's."""
    from softspoken_amd import native, synth, checkpoint
    out = _child(tag, mode, {}, layer_signal, hostile=hostile)
    ctx = native.Context(checkpoint.pack_state_dict(synth.make_state_dict(0, hostile=hostile)), 0, precision=mode, chunk=5)
    fid = ctx.add_f32_22k(np.load(layer_signal["sig"]))
    _, mask = ctx.infer_windows(fid, layer_signal["starts"][layer_signal["sel"]], want_spec=True)
    ctx.close()
    assert np.array_equal(mask, np.load(out)), "dev and product libraries disagree"


ALTERNATE = [({"SOFTSPOKEN_CONV4": "0"}, "bf16"), ({"SOFTSPOKEN_CONV4": "0", "SOFTSPOKEN_NW": "4"}, "bf16"), ({"SOFTSPOKEN_NW": "4"}, "fp32"),
             ({"SOFTSPOKEN_UPS32": "0"}, "fp32"), ({"SOFTSPOKEN_UPS32_NT": "2"}, "fp32"), ({"SOFTSPOKEN_UPS32_NT": "3"}, "fp32"),
             ({"SOFTSPOKEN_RPROJ": "0"}, "bf16"), ({"SOFTSPOKEN_RPROJ": "0", "SOFTSPOKEN_PF2": "0"}, "bf16"),
             ({"SOFTSPOKEN_DUO": "0"}, "f16x2"), ({"SOFTSPOKEN_DUO": "2"}, "f16x2"), ({"SOFTSPOKEN_DUO_H8": "0"}, "f16x2"),
             ({"SOFTSPOKEN_UPS": "0"}, "f16x2"), ({"SOFTSPOKEN_UPSR": "0"}, "f16x2"), ({"SOFTSPOKEN_RING": "0"}, "f16x2"),
             ({"SOFTSPOKEN_RING": "2"}, "f16x2"), ({"SOFTSPOKEN_NTB1": "0"}, "f16x2"), ({"SOFTSPOKEN_RPROJ": "0"}, "f16x2"),
             ({"SOFTSPOKEN_RPROJ": "1"}, "f16x2"),
             ({"SOFTSPOKEN_C1S_ROWS": "16"}, "f16x2"), ({"SOFTSPOKEN_C1S_TRACK": "1"}, "f16x2"), ({"SOFTSPOKEN_C1S": "0"}, "f16x2"),
             ({"SOFTSPOKEN_C1S_FORM": "32"}, "f16x2"), ({"SOFTSPOKEN_C1S_FORM": "32", "SOFTSPOKEN_C1S_ROWS": "16"}, "f16x2")]


def _alt_id(env, mode):
    return "-".join(f"{k[11:]}={v}" for k, v in env.items()) + "-" + mode


@pytest.mark.parametrize("env,mode", ALTERNATE, ids=[_alt_id(e, m) for e, m in ALTERNATE])
def test_every_launch_of_the_alternate_forms(env, mode, layer_signal, build_all):
    """The switch sets of test_gpu_parity's test_alternate_kernel_structures and test_conv1_streaming_kernel_variants_agree, whose
    forms are otherwise held only to the score bars: two windows (the pad and the noise)."""
    _child("alt", mode, env, layer_signal, n_sel=2, plan_key="alt-" + _alt_id(env, mode))


ZOO = [(name, mode) for name in ("seed7", "spread3", "spread6", "signs", "dead", "tinyvar") for mode in ("f16x2", "fp32")] + \
      [("spread3", "bf16"), ("dead", "bf16")]


@pytest.mark.parametrize("name,mode", ZOO, ids=[f"{n}-{m}" for n, m in ZOO])
def test_every_launch_on_the_checkpoint_zoo(name, mode, layer_signal, build_all):
    """The checkpoints of tests/checkpoint_zoo.py (another draw, per-channel gains of 10^+-3 and 10^+-6, negative gammas, dead channels,
    variances of zero), two windows (the pad and the noise): the same bounds, unchanged, and in f16x2 the device's exponents against
    the host emulation of the rule.  Dead channels are exact on both sides (0 / 0 counts as exact in ratio_report)."""
    _child("zoo_" + name, mode, {}, layer_signal, n_sel=2, ckpt=name, plan_key=f"zoo_{name}-{mode}")


@pytest.mark.parametrize("mode,hostile", [("fp32", False), ("f16x2", False), ("bf16", False), ("f16x2", True), ("fp32", True)])
def test_spec_head_end_to_end(mode, hostile, c1, build_all):
    """All 105 windows of C1, every value of the 2 x 128 x 256 map, against the float64 oracle (oracle_np.unet_forward on float64
    features of the oracle's front-end): 1e-4 in fp32 and f16x2 (the hostile-scale checkpoint too), bf16 within its score tolerance."""
    import torch
    from softspoken_amd import native, synth, checkpoint
    from oracle import oracle_np as O
    torch.set_grad_enabled(False)
    sd_np = synth.make_state_dict(0, hostile=hostile)
    ctx = native.Context(checkpoint.pack_state_dict(sd_np), 0, precision=mode, chunk=64)
    fid = ctx.add_f32_22k(c1["sig"])
    spec, _ = ctx.infer_windows(fid, c1["starts"], want_spec=True)
    ctx.close()
    sd = {k: torch.as_tensor(np.asarray(v)).to(torch.float64) for k, v in sd_np.items()}
    sd32 = synth.to_torch_state_dict(sd_np)
    worst = 0.0
    for i0 in range(0, len(c1["starts"]), 16):
        x = torch.stack([torch.from_numpy(c1["padded"][s:s + 66150]) for s in c1["starts"][i0:i0 + 16]])
        feats = O.mel_features(x, sd32["mel_spectrogram.spectrogram.window"], sd32["mel_spectrogram.mel_scale.fb"]).to(torch.float64)
        ref, _ = O.unet_forward(sd, feats, want_spec=True)
        worst = max(worst, float(np.abs(spec[i0:i0 + 16] - ref.numpy()).max()))
    print(f"spec head {mode}{' hostile' if hostile else ''}: max |spec - float64 oracle| = {worst:.3g}")
    assert worst < (TOL_SPEC_BF16 if mode == "bf16" else TOL_SPEC), worst
