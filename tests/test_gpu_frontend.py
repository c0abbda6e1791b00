"""The mel front-end kernel (softspoken_amd/csrc/frontend.hip) against the float64 reference and the derived interval bound of
tests/frontend_ref.py, on a real MI355X: every input class with zero values outside the bound, three exact properties (alignment,
batch independence, frame isolation), the tables the loader builds itself, other filterbanks that fit, the loader's refusals; and,
in child processes on the development build, the power spectrum of every bin and the first kernel structure.

A report line per class, as test_gpu_layers prints them:
    FRONTEND <class> worst |delta| / half-width <ratio> at window <w>, mel row <j>, frame <t> (<ratio> where m >= 1); outside <count>"""
import os
import subprocess
import sys

import numpy as np
import pytest

import frontend_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN_KEY, FB_KEY = "mel_spectrogram.spectrogram.window", "mel_spectrogram.mel_scale.fb"


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native
    return native


@pytest.fixture(scope="module")
def ctx(native, blob):
    c = native.Context(blob, 0, precision="fp32")
    yield c
    c.close()


@pytest.fixture(scope="module")
def tables(sd_np):
    return sd_np[WIN_KEY].astype(np.float32), sd_np[FB_KEY].astype(np.float32)


@pytest.fixture(scope="module")
def inputs(c1):
    return {name: (sig, starts) for name, sig, starts in R.input_set(c1["padded"], c1["starts"], R.c5_windows())}


@pytest.fixture(scope="module")
def refs(inputs, tables):
    """Class name -> ReferenceSet for the standard tables, computed when first asked for and kept for the module."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = R.ReferenceSet(R.windows_of(*inputs[name]), *tables)
        return cache[name]
    return get


def device_features(c, sig, starts):
    c.reset()
    fid = c.add_f32_22k(sig, padded=True)
    return c.features(fid, starts)


def assert_inside(reports):
    for name, rep in reports:
        print(R.line(name, rep), flush=True)
    bad = [R.line(name, rep) for name, rep in reports if rep["over"] or not rep["ratio"] <= 1.0]
    assert not bad, "values outside the bound:\n" + "\n".join(bad)


TONES = ["tones_%g" % a for a in R.TONE_AMPS]


# ---- the product kernel against the bound ---------------------------------------------------------------------------------------------
def test_every_input_class_is_inside_the_bound(ctx, inputs, refs):
    """Stepped tones through every bin centre and half-bin point at three amplitudes, impulses at the frame and reflection edges, the
    white-noise amplitude ladder from 1e-30 to 1e12, DC, a full-scale square wave, all C1 windows, the C5 windows: zero values
    outside the interval.  The 1e-30 ladder step gives exactly zero features (1 + m rounds to 1)."""
    reports = []
    for name, (sig, starts) in inputs.items():
        feat = device_features(ctx, sig, starts)
        reports.append((name, refs(name).check(feat)))
        if name == "white_1e-30":
            assert not feat.any(), "features of 1e-30 noise are not exactly zero"
    assert_inside(reports)


# ---- exact properties -----------------------------------------------------------------------------------------------------------------
def test_alignment_is_exact(ctx, inputs):
    """The features of starts + d equal those of the signal shifted by d read at starts, bit for bit (the sample pairs of a frame are
    8-byte reads: every alignment of a window in the arena), and a file behind a first file of odd length gives the same features."""
    sig, _ = inputs["white_1"]
    starts = 13231 * np.arange(6)
    for d in (1, 2, 3, 5, 255, 13229):
        assert starts[-1] + d + R.N_WIN <= len(sig)
        a = device_features(ctx, sig, starts + d)
        b = device_features(ctx, sig[d:], starts)
        assert np.array_equal(a, b), "shift %d" % d
    alone = device_features(ctx, sig, starts)
    ctx.reset()
    ctx.add_f32_22k(np.full(R.N_WIN + 1, 0.25, np.float32), padded=True)
    fid = ctx.add_f32_22k(sig, padded=True)
    assert np.array_equal(ctx.features(fid, starts), alone)
    assert np.array_equal(ctx.features(fid, starts + 1), device_features(ctx, sig, starts + 1))


def test_batch_independence_is_exact(ctx, inputs):
    """A window alone, in a batch of 2 and in a batch of 1 005 (launch_frontend: 64 units a window over at most 8 waves x the CU count,
    so every wave walks about 30 units) has the same features."""
    sig, _ = inputs["white_1"]
    room = len(sig) - R.N_WIN
    starts = (np.arange(1005) * 7919) % room
    ctx.reset()
    fid = ctx.add_f32_22k(sig, padded=True)
    big = ctx.features(fid, starts)
    for i in (0, 1, 502, 1003, 1004):
        assert np.array_equal(ctx.features(fid, starts[i:i + 1])[0], big[i]), i
    for i in (0, 501, 1003):
        assert np.array_equal(ctx.features(fid, starts[i:i + 2]), big[i:i + 2]), i
    assert np.array_equal(ctx.features(fid, starts[[1004, 0]]), big[[1004, 0]])


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_frame_isolation_is_exact(ctx, inputs, value):
    """One NaN (one +inf) sample at position p: exactly the frames that cover p are NaN in all 128 rows, every other value of the
    window equals the clean signal's bit for bit.  Frame t covers samples 256 t - 256 .. 256 t + 255; frame 0 also reads samples
    1 .. 256 as its reflected half; samples from 65 536 on are read by no frame."""
    sig, _ = inputs["white_1"]
    x = sig[777:777 + R.N_WIN].copy()
    clean = device_features(ctx, x, [0])[0]
    assert np.isfinite(clean).all()
    for p in (0, 1, 100, 255, 256, 257, 1000, 33075, 65279, 65280, 65535, 65536, 66149):
        want = [t for t in range(256) if 256 * t - 256 <= p <= 256 * t + 255 or (t == 0 and 1 <= p <= 256)]
        y = x.copy(); y[p] = value
        assert np.nonzero(R.Reference(y[None], np.ones(512, np.float32), np.zeros((1025, 128), np.float32)).bad[0])[0].tolist() == want
        got = device_features(ctx, y, [0])[0]
        hit = np.zeros(256, bool); hit[want] = True
        assert np.isnan(got[:, hit]).all(), "p = %d: frames %s are not NaN in every row" % (p, want)
        assert np.array_equal(got[:, ~hit], clean[:, ~hit]), "p = %d: a frame that does not cover it changed" % p


# ---- tables the loader builds, other filterbanks, refusals ---------------------------------------------------------------------------
def _context_with(native, sd_np, drop=(), **replace):
    from softspoken_amd import checkpoint
    sd = {k: v for k, v in sd_np.items() if k not in drop}
    sd.update(replace)
    return native.Context(checkpoint.pack_state_dict(sd), 0, precision="fp32")


def test_tables_built_by_the_loader(native, sd_np, inputs, tables, refs):
    """A checkpoint without the two torchaudio buffers: the loader's float32 recipes (weights.hip build_tables) give features within
    the bound computed from torch's own hann_window(512) and the filterbank recipe of softspoken_amd.layout."""
    from softspoken_amd import layout
    win, fb = R.hann_periodic_f32(), layout.mel_filterbank().astype(np.float32)
    same = np.array_equal(win, tables[0]) and np.array_equal(fb, tables[1])
    print("FRONTEND loader tables: torch's window and the layout filterbank %s the checkpoint's buffers" % ("equal" if same else "differ from"))
    c = _context_with(native, sd_np, drop=(WIN_KEY, FB_KEY))
    reports = []
    for name in TONES + ["c1"]:
        feat = device_features(c, *inputs[name])
        ref = refs(name) if same else R.ReferenceSet(R.windows_of(*inputs[name]), win, fb)
        reports.append(("no-buffers:" + name, ref.check(feat)))
    c.close()
    assert_inside(reports)


def _supports(fb):
    return [np.nonzero(fb[:, j])[0] for j in range(128)]


def other_filterbanks(fb):
    """The standard supports with seeded weights in [0.25, 1]; every filter's support shortened from the left by 1, 2 and 3 bins (all
    four alignments of a run's first bin inside its group of four; a filter keeps at least one tap)."""
    rng = np.random.default_rng(99)
    out = []
    a = np.zeros_like(fb)
    for j, nz in enumerate(_supports(fb)):
        a[nz, j] = rng.uniform(0.25, 1.0, len(nz)).astype(np.float32)
    out.append(("seeded-weights", a))
    for d in (1, 2, 3):
        b = fb.copy()
        for j, nz in enumerate(_supports(fb)):
            b[nz[:min(d, len(nz) - 1)], j] = 0.0
        out.append(("left-%d" % d, b))
    return out


def test_other_filterbanks_that_fit(native, sd_np, inputs, tables):
    """Filterbanks other than the standard one, on the tone and white-noise classes, within the bound computed from that filterbank:
    the permuted, padded weight image and the alignment slot for run starts the standard filterbank never produces."""
    win, fb = tables
    starts_mod4 = set()
    reports = []
    for tag, fbx in other_filterbanks(fb):
        starts_mod4 |= {int(nz[0]) % 4 for nz in _supports(fbx) if len(nz)}
        c = _context_with(native, sd_np, **{FB_KEY: fbx})
        for name in ("tones_0.5", "white_1"):
            feat = device_features(c, *inputs[name])
            reports.append((tag + ":" + name, R.ReferenceSet(R.windows_of(*inputs[name]), win, fbx).check(feat)))
        c.close()
    assert starts_mod4 == {0, 1, 2, 3}
    assert_inside(reports)


def refused_filterbanks(fb):
    a = fb.copy(); a[768, 127] = 0.5
    b = fb.copy(); lo = int(np.nonzero(fb[:, 10])[0][0]); b[lo:lo + 11, 10] = 0.5
    c = fb.copy()
    for j, nz in enumerate(_supports(fb)):
        c[nz[0]:nz[0] + (10 if j < 64 else 32), j] = 0.5
    assert (c != 0).sum() > 1536 and np.nonzero(c.any(1))[0].max() < 768
    return [(a, "mel filterbank has weight above bin 767"), (b, "mel filterbank: a filter is wider than the front-end kernel's fixed trip counts"),
            (c, "mel filterbank has more than 1536 non-zero weights")]


def test_filterbanks_that_do_not_fit_are_refused(native, sd_np, inputs, tables, refs):
    """A weight at bin 768, a narrow filter of 11 taps, more than 1 536 non-zero weights: SS_ERR_FORMAT with the loader's message and
    no context (host-side checks of the table: no kernel ever runs with a table that does not fit).  A context made afterwards works."""
    for fbx, words in refused_filterbanks(tables[1]):
        with pytest.raises(native.NativeError) as e:
            _context_with(native, sd_np, **{FB_KEY: fbx})
        assert e.value.code == native.SS_ERR_FORMAT and words in str(e.value), str(e.value)
    c = _context_with(native, sd_np)
    feat = device_features(c, *inputs["square_74"])
    c.close()
    assert_inside([("after-refusals:square_74", refs("square_74").check(feat))])


# ---- development build: the power spectrum, the first kernel structure ---------------------------------------------------------------
_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r})
from softspoken_amd import synth, native, checkpoint
d = np.load({in_npz!r})
ctx = native.Context(checkpoint.pack_state_dict(synth.make_state_dict(0)), 0, precision="fp32")
out = {{}}
for name in {names!r}:
    ctx.reset()
    fid = ctx.add_f32_22k(d[name + ".sig"], padded=True)
    out[name] = ctx.features(fid, d[name + ".starts"])
ctx.close()
np.savez({out_npz!r}, **out)
print("CHILD_OK", flush=True)
"""


def _dev_child(tmp, inputs, names, fedbg):
    """One child process on the development build with SOFTSPOKEN_FEDBG set: what ss_features returns for the classes named."""
    from softspoken_amd import build as hip_build
    in_npz = os.path.join(tmp, "in.npz")
    if not os.path.exists(in_npz):
        arrays = {}
        for name, (sig, starts) in inputs.items():
            arrays[name + ".sig"] = sig; arrays[name + ".starts"] = np.asarray(starts, dtype=np.int64)
        np.savez(in_npz, **arrays)
    out_npz = os.path.join(tmp, "out_%d.npz" % fedbg)
    code = _CHILD.format(root=ROOT, in_npz=in_npz, out_npz=out_npz, names=list(names))
    env = dict(os.environ, SOFTSPOKEN_LIB=hip_build.DEV_LIB, SOFTSPOKEN_FEDBG=str(fedbg))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, "FEDBG=%d: %s %s" % (fedbg, r.stdout[-2000:], r.stderr[-2000:])
    return np.load(out_npz)


def test_power_spectrum_of_every_bin(build_all, inputs, tables, tmp_path):
    """Development build, SOFTSPOKEN_FEDBG = 512 + 1024 sel (sel = 0 .. 5: 128 bins a run): |X[k]|^2 of all 768 bins of every frame
    of the tone, impulse, full-scale-noise and DC windows within 2 |X[k]| eps + eps^2 + 2^-22 P[k] of the float64 spectrum.  Printed:
    the worst |delta| / bound per quarter pass r = k mod 4 and per frame of the unit t mod 4.  (The only check that sees bin 0.)"""
    names = TONES + ["impulses", "white_1", "dc_0.999"]
    dumps = [_dev_child(str(tmp_path), inputs, names, 512 + 1024 * sel) for sel in range(6)]
    by_r, by_t, over, worst = np.zeros(4), np.zeros(4), 0, (0.0, None)
    for name in names:
        x = R.windows_of(*inputs[name])
        got = np.concatenate([d[name] for d in dumps], axis=1).transpose(0, 2, 1).astype(np.float64)      # (B, 256, 768)
        assert got.shape == (len(x), 256, 768)
        ref = R.ReferenceSet(x, tables[0], tables[1], keep_spectrum=True)
        for j, part in enumerate(ref.parts):
            p64, bound = part.power_bound()
            g = got[j * ref.chunk:(j + 1) * ref.chunk]
            d = np.abs(g - p64[..., :768])
            ratio = np.where(d == 0, 0.0, d / bound[..., :768])
            ratio = np.where(np.isnan(ratio), np.inf, ratio)
            over += int((~(d <= bound[..., :768])).sum())
            for r in range(4):
                by_r[r] = max(by_r[r], ratio[..., r::4].max()); by_t[r] = max(by_t[r], ratio[:, r::4].max())
            if ratio.max() > worst[0]:
                at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
                worst = (float(ratio.max()), (name, int(at[0]) + j * ref.chunk, int(at[1]), int(at[2])))
    print("FRONTEND power spectrum: worst |delta| / bound per quarter pass r = k mod 4:", " ".join("%.4g" % v for v in by_r))
    print("FRONTEND power spectrum: worst |delta| / bound per frame of the unit t mod 4:", " ".join("%.4g" % v for v in by_t))
    print("FRONTEND power spectrum: worst %.4g at (class, window, frame, bin) %s; outside %d" % (worst[0], worst[1], over))
    assert over == 0 and worst[0] <= 1.0


def test_first_structure_is_inside_the_bound(build_all, inputs, refs, tmp_path):
    """Development build, SOFTSPOKEN_FEDBG = 256: the first kernel structure (log10f / sqrtf where the product kernel uses the
    hardware's log2 and sqrt) on the tone, white-noise and C1 classes.  The two kernels' features may differ; each is inside the bound."""
    names = TONES + ["white_1", "c1"]
    dump = _dev_child(str(tmp_path), inputs, names, 256)
    assert_inside([("first-structure:" + name, refs(name).check(dump[name])) for name in names])
