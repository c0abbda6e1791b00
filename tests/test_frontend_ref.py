"""CPU tests of tests/frontend_ref.py, the float64 reference and bound the device's mel front-end is held to: correct float32
implementations are inside it with no exception on the whole input set, seeded defects are outside it, the one known blind spot
stays written down.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import frontend_ref as R
from oracle import oracle_np as O

torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def tables(sd_np):
    return sd_np["mel_spectrogram.spectrogram.window"].astype(np.float32), sd_np["mel_spectrogram.mel_scale.fb"].astype(np.float32)


@pytest.fixture(scope="module")
def classes(c1):
    return {name: R.windows_of(sig, starts) for name, sig, starts in R.input_set(c1["padded"], c1["starts"], R.c5_windows())}


# ---- the two float32 front-ends K is fixed against, and the plain-C oracle ----------------------------------------------------------
def torch_features(x, win, fb):
    return O.mel_features(torch.from_numpy(x), torch.from_numpy(win), torch.from_numpy(fb)).numpy()


def fft_r2_f32(a):
    """a (..., 2048) complex64: radix-2 decimation in time, float32 twiddles, every operation rounded to float32."""
    n = 2048
    rev = np.array([int(format(i, "011b")[::-1], 2) for i in range(n)])
    a = a[..., rev].astype(np.complex64)
    length = 2
    while length <= n:
        tw = np.exp(-2j * np.pi * np.arange(length // 2) / length).astype(np.complex64)
        a = a.reshape(a.shape[:-1] + (n // length, length))
        ev, od = a[..., :length // 2], a[..., length // 2:] * tw
        a = np.concatenate([ev + od, ev - od], axis=-1).reshape(a.shape[:-2] + (n,))
        length *= 2
    return a


def r2_features(x, win, fb):
    out = np.empty((len(x), 128, 256), np.float32)
    for i in range(len(x)):
        fr = (R.frame_samples(x[i:i + 1])[0] * win).astype(np.float32)
        buf = np.zeros((256, 2048), np.complex64); buf[:, :512] = fr
        X = fft_r2_f32(buf)[:, :1025]
        P = (X.real * X.real + X.imag * X.imag).astype(np.float32)
        m = (P @ fb).astype(np.float32)
        out[i] = np.sqrt(np.log10(m + np.float32(1))).astype(np.float32).T
    return out


def c_features(x, win, fb):
    from oracle import oracle_c
    oracle_c.build()
    return oracle_c.mel_features(x, win, fb)


def test_radix2_fft_is_an_fft():
    z = np.random.default_rng(0).standard_normal((3, 2048)).astype(np.complex64)
    assert np.abs(fft_r2_f32(z) - np.fft.fft(z.astype(np.complex128))).max() < 1e-3


def test_float32_front_ends_are_inside_the_bound(classes, tables):
    """torch's float32 stft, the radix-2 float32 FFT above and the plain-C oracle: zero values outside the interval at K on every
    input class; the two float32 ones reach zero at K / 4 already (that is how K was fixed: frontend_ref's docstring)."""
    win, fb = tables
    impls = dict(torch=torch_features, radix2=r2_features, c_oracle=c_features)
    need = {k: 1 for k in impls}
    bad = []
    for name, x in classes.items():
        for i0 in range(0, len(x), 16):
            xs = x[i0:i0 + 16]
            ref = R.Reference(xs, win, fb)
            for impl, fn in impls.items():
                f = fn(xs, win, fb)
                rep = ref.check(f)
                mk = ref.min_k(f)
                need[impl] = max(need[impl], mk if mk is not None else 1 << 30)
                if rep["over"]:
                    bad.append((impl, name, i0, rep))
        print("FRONTEND_REF", name, len(x), "windows; minimum K so far", need, flush=True)
    print("FRONTEND_REF minimum K per implementation:", need)
    assert not bad, bad
    assert need["c_oracle"] == 1
    assert 4 * max(need["torch"], need["radix2"]) <= R.K, need


# ---- seeded defects -------------------------------------------------------------------------------------------------------------------
def _tap(fb, j, which):
    nz = np.nonzero(fb[:, j])[0]
    return int(nz[0] if which == "first" else nz[-1])


def defective(x, win, fb, kind):
    """A float64 front-end with one seeded defect, rounded to float32 at the end (and at m + 1, as every implementation rounds there)."""
    x64 = x.astype(np.float64)
    w = win.astype(np.float64)
    fbd = fb.astype(np.float64).copy()
    xp = np.concatenate([x64[:, 256:0:-1], x64], axis=1)
    idx = 256 * np.arange(256)[:, None] + np.arange(512)[None, :]
    if kind == "frame0_zero_padded":
        xp[:, :256] = 0.0
    if kind == "one_sample_late":
        idx = idx + 1
    if kind == "symmetric_hann":
        w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(512) / 511.0)
    P = np.abs(np.fft.rfft(xp[:, idx] * w, n=2048, axis=-1)) ** 2
    if kind == "quarter_pass_r3_2e-5":
        P[..., 3::4] *= 1 + 2e-5
    if kind == "all_power_1e-5":
        P *= 1 + 1e-5
    if kind == "bins_513_514_swapped":
        P[..., [513, 514]] = P[..., [514, 513]]
    if kind == "bin_512_x1.001":
        P[..., 512] *= 1.001
    if kind == "bin_743_dropped":
        P[..., 743] = 0.0
    if kind == "group_300_unpermuted":                     # the buffer's (0, 2, 1, 3) order read as (0, 1, 2, 3)
        P[..., [301, 302]] = P[..., [302, 301]]
    if kind == "bin_0_halved":
        P[..., 0] *= 0.5
    if kind.startswith("tap_"):
        _, which, j = kind.split("_")
        fbd[_tap(fb, int(j), which), int(j)] = 0.0
    m = P @ fbd
    f = R.g((1.0 + m).astype(np.float32).astype(np.float64))
    if kind == "feature_2e-6":
        f = f * (1 + 2e-6)
    return f.astype(np.float32).transpose(0, 2, 1)


WIDE, NARROW = 100, 5
# defect -> the input class that must catch it (and the windows of it that are looked at; None: the tone window of the bin named)
DEFECTS = [("quarter_pass_r3_2e-5", "c1", None), ("quarter_pass_r3_2e-5", "white_1", None), ("quarter_pass_r3_2e-5", "square_74", None),
           ("all_power_1e-5", "c1", None), ("all_power_1e-5", "white_1", None), ("all_power_1e-5", "square_74", None),
           ("feature_2e-6", "c1", None), ("feature_2e-6", "white_1", None), ("feature_2e-6", "square_74", None),
           ("tap_last_%d" % WIDE, "tones_0.5", ("last", WIDE)), ("tap_first_%d" % WIDE, "tones_0.5", ("first", WIDE)),
           ("tap_last_%d" % NARROW, "tones_0.5", ("last", NARROW)), ("tap_first_%d" % NARROW, "tones_0.5", ("first", NARROW)),
           ("bins_513_514_swapped", "tones_0.5", 513), ("bin_512_x1.001", "tones_0.5", 512), ("bin_743_dropped", "tones_0.5", 743),
           ("bin_743_dropped", "white_1", None),
           ("frame0_zero_padded", "impulses", None), ("frame0_zero_padded", "white_1", None),
           ("one_sample_late", "impulses", None), ("one_sample_late", "white_1", None), ("one_sample_late", "c1", None),
           ("symmetric_hann", "white_1", None), ("symmetric_hann", "tones_0.5", 300),
           ("group_300_unpermuted", "tones_0.5", 301)]


def _pick(classes, fb, cls, where):
    x = classes[cls]
    if where is None and cls == "impulses":
        return x
    if where is None:
        return x[::max(1, len(x) // 4)][:5] if cls != "c1" else x[[20, 40, 60, 80]]
    k = _tap(fb, where[1], where[0]) if isinstance(where, tuple) else where
    return x[R.tone_window_of_bin(k):R.tone_window_of_bin(k) + 1]


@pytest.mark.parametrize("kind,cls,where", DEFECTS, ids=["%s-%s" % (d[0], d[1]) for d in DEFECTS])
def test_seeded_defect_is_outside_the_bound(kind, cls, where, classes, tables):
    win, fb = tables
    x = _pick(classes, fb, cls, where)
    ref = R.Reference(x, win, fb)
    clean = ref.check(defective(x, win, fb, "none"))
    rep = ref.check(defective(x, win, fb, kind))
    print("FRONTEND_REF defect", kind, "on", cls, "->", rep["over"], "of", x.shape[0] * 32768, "values outside, worst ratio %.3g" % rep["ratio"],
          "(clean: %d outside, %.3g)" % (clean["over"], clean["ratio"]))
    assert clean["over"] == 0
    assert rep["over"] > 0


def test_bin_0_is_a_blind_spot_of_the_features(classes, tables):
    """Bin 0 carries no mel weight: halving P[0] changes no feature, bit for bit (DC input included).  The power-spectrum read-back of
    test_gpu_frontend is the only check that sees bin 0; its bound does see this defect."""
    win, fb = tables
    assert not fb[0].any()
    for cls in ("dc_0.999", "tones_0.5", "white_1"):
        x = classes[cls][:1]
        assert np.array_equal(defective(x, win, fb, "bin_0_halved"), defective(x, win, fb, "none"))
    x = classes["dc_0.999"][:1]
    ref = R.Reference(x, win, fb, keep_spectrum=True)
    p64, bound = ref.power_bound()
    half = p64.copy(); half[..., 0] *= 0.5
    assert (np.abs(half - p64) > bound)[..., 0].all() and not (np.abs(half - p64) > bound)[..., 1:].any()


def test_non_finite_frames(tables):
    """A NaN or an infinity in a frame's samples: the reference wants NaN in all 128 rows of exactly the frames that cover it."""
    win, fb = tables
    x = np.random.default_rng(5).uniform(-1, 1, (1, R.N_WIN)).astype(np.float32)
    x[0, 1000] = np.inf
    ref = R.Reference(x, win, fb)
    assert np.nonzero(ref.bad[0])[0].tolist() == [3, 4]
    f = torch_features(np.where(np.isfinite(x), x, 0).astype(np.float32), win, fb)
    assert ref.check(f)["over"] == 2 * 128                # finite values in the two frames are refused
    f[0, :, 3:5] = np.nan
    assert ref.check(f)["over"] == 0
    f[0, 7, 9] = np.nan
    assert ref.check(f)["over"] == 1                      # and a NaN elsewhere is outside


def test_loader_band_edges_give_the_reference_filterbank(gold):
    """weights.hip's kMelEdgesHz (the loader's filterbank for a checkpoint without the `fb` buffer) equals layout.mel_edges_hz(), and
    the loader's recipe on those edges, restated here operation for operation in float32, gives the reference-made fixture's 1 469
    weights bit for bit.  (With a C library's correctly rounded powf in place of the table 19 edges and 416 weights differ from
    layout's, which every checkpoint and fixture of the project is built on.)"""
    from softspoken_amd import layout
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "softspoken_amd", "csrc", "weights.hip")).read()
    body = re.search(r"kMelEdgesHz\[130\] = \{(.*?)\};", src, re.S).group(1)
    edges = np.array([float.fromhex(t.rstrip("f")) if "x" in t else float(t.rstrip("f")) for t in re.findall(r"[0-9a-fx.+p-]+f", body)])
    assert len(edges) == 130 and np.array_equal(edges.astype(np.float32), edges)
    edges = edges.astype(np.float32)
    assert np.array_equal(edges, layout.mel_edges_hz())
    f32 = np.float32
    allf = (11025.0 * np.arange(1025) / 1024.0).astype(f32)
    fb = np.zeros((1025, 128), f32)
    for j in range(128):
        down = (f32(-1.0) * (edges[j] - allf)) / f32(edges[j + 1] - edges[j])
        up = (edges[j + 2] - allf) / f32(edges[j + 2] - edges[j + 1])
        fb[:, j] = np.maximum(f32(0), np.minimum(down, up))
    g = gold["mel_tables"]
    r, c = np.nonzero(fb)
    assert np.array_equal(r, g["rows"]) and np.array_equal(c, g["cols"]) and np.array_equal(fb[r, c], g["vals"])
