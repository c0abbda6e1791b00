"""Float64 reference of the mel front-end and the bound its float32 implementations are held to (tests only: numpy, no GPU, not
imported by the library).  tests/test_frontend_ref.py tests this module on the CPU; tests/test_gpu_frontend.py, test_gpu_layers.py,
test_gpu_parity.py and test_gpu_c3.py hold the device to it; tools/fe_spectrum_check.py prints from it.

Reference.  Everything in float64, from the float32 samples x, the float32 window w (512) and the float32 filterbank fb (1025 x 128)
that the context was given:
    frame t (t = 0 .. 255) = x[256 t - 256 .. 256 t + 255], x[-k] = x[k] (only frame 0 reflects), times w, zero-padded to 2048;
    X = rFFT_2048(frame),  P[k] = |X[k]|^2,  m[j] = sum_k fb[k, j] P[k],  feature[j, t] = g(1 + m[j]),  g(y) = sqrt(log10(y)).
A window has 66 150 samples; frame 255 ends at sample 65 535 and the rest is not read.

Bound.  u = 2^-24 (float32 unit roundoff), per frame e2 = sqrt(sum_n (x_n w_n)^2):
  * spectrum: every bin of a float32 FFT of the frame is off by at most eps = K u e2 (K: below);
  * power: |dP[k]| <= 2 |X[k]| eps + eps^2 + 2^-22 P[k]   (the last term: the two squares, their sum and the 0.25 factor);
  * mel: dm[j] = sum_k fb[k, j] (2 |X[k]| eps + eps^2) + 2^-21 m[j]   (squares and factors as above, plus the float32 sum of at most
    40 non-negative terms, accumulated by fma: 40 u < 2^-21 - 2^-22 ... the terms are non-negative, so the sum's relative error is
    bounded by the number of additions times u);
  * feature: it must lie in [g(y_lo) (1 - 2^-21), g(y_hi) (1 + 2^-21)], y_lo / y_hi = float32(1 + m -/+ dm) moved TWO float32
    neighbours outward (one for the rounding of the mel sum m, one for the rounding of m + 1), y_lo not below 1.
    2^-21 is derived, not measured: a 1-ulp logarithm (2^-23 relative, halved by the root: 2^-24), the rounded constant log10(2) and
    the rounded product (2^-24 + 2^-25 after halving ... both enter under the root), a 1-ulp square root (2^-23): together about
    2^-22.3; 2^-21 leaves a factor 2.4.  The interval form is what makes quiet bins checkable: where 1 + m sits on the coarse
    float32 grid next to 1 the interval is one or two grid steps wide (3.2e-4 ... 5e-4 in feature units) and nowhere wider than it
    must be (median width 1e-6 ... 2e-6 on speech-like input and white noise).
  * non-finite input: a frame whose 512 samples hold a NaN or an infinity must be NaN in all 128 rows; every other frame of the
    window is judged as above.

Assumptions, and what supports them:
  * K.  The one number that is not derived: the rigorous bound for an 11-stage float32 FFT (Higham, Accuracy and Stability, 24.1) is
    about 3 000 u e2 per bin and would hide every defect tests/test_frontend_ref.py seeds.  K is an ASSUMPTION about well-behaved
    float32 FFTs, fixed against CPU float32 implementations and never against the device: the smallest power of two at which two
    independent float32 front-ends have zero values outside the interval over the whole input set below, times 4 for a different
    factorisation (radix-16 passes, table twiddles rounded to float32, the untangle butterfly of the packed real FFT).
    Measured on the whole input set (input_set() with the C5 windows: 294 windows, 9.6 M values):
        oracle_np.mel_features (torch's float32 stft):          zero outside at K = 4 (39 values outside at K = 2)
        radix-2 DIT FFT in complex64, float32 twiddles (test):  zero outside at K = 8 (4 values outside at K = 4, all of them in the
                                                                0.5-amplitude stepped tones; 73 at K = 2)
        oracle_c.mel_features (FFT in double; does not count):  zero outside at K = 1
    hence K = 4 x 8 = 32.  (On a subset of the tones -- every 16th bin -- both reach zero at K = 4, which would give 16; the rule is
    stated on the whole set, and the whole set gives 8.)  test_frontend_ref.py asserts all three at K, asserts that the two float32
    ones are inside at K / 4, and prints each implementation's minimum.  The device is never used to set K: a device value outside
    the interval is a finding to be explained from the power-spectrum read-back, not a reason to raise K.
  * the filterbank's weights are non-negative (asserted): the mel sum then has no cancellation;
  * a filter has at most 40 non-zero taps (asserted against the filterbank given; the standard one has 32 at most).

Blind spot (asserted in test_frontend_ref.py so that it stays written down): bin 0 carries no mel weight in the standard filterbank,
so an error in P[0] changes no feature.  Only the power-spectrum read-back (power_bound) sees it."""
import numpy as np

U = 2.0 ** -24
K = 32                  # see the docstring: 4 x the larger of the two float32 implementations' minima
REL_G = 2.0 ** -21      # log2 x log10(2), sqrt: derived above
REL_MEL = 2.0 ** -21
REL_POW = 2.0 ** -22
N_WIN, N_FRAMES, N_MELS = 66150, 256, 128


def g(y):
    return np.sqrt(np.log10(np.maximum(y, 1.0)))


def windows_of(sig, starts):
    sig = np.asarray(sig, dtype=np.float32)
    return np.stack([sig[int(s):int(s) + N_WIN] for s in starts])


def frame_samples(x):
    """x (B, 66150) -> (B, 256, 512): the samples of every frame, reflected at the left edge, same dtype."""
    xp = np.concatenate([x[:, 256:0:-1], x], axis=1)
    idx = 256 * np.arange(N_FRAMES)[:, None] + np.arange(512)[None, :]
    return xp[:, idx]


def frames64(x, win):
    return frame_samples(np.asarray(x, dtype=np.float32).astype(np.float64)) * np.asarray(win, dtype=np.float64)


def hann_periodic_f32():
    import torch
    return torch.hann_window(512, periodic=True, dtype=torch.float32).numpy()


class Reference:
    """The float64 quantities of a batch of windows x (B, 66150) that the bounds need; keep_spectrum also keeps |X| and P (B, 256, nb)."""

    def __init__(self, x, win, fb, keep_spectrum=False):
        x = np.asarray(x, dtype=np.float32)
        fb = np.asarray(fb, dtype=np.float32).astype(np.float64)
        assert x.ndim == 2 and x.shape[1] == N_WIN and fb.shape == (1025, N_MELS)
        assert (fb >= 0).all() and int((fb != 0).sum(0).max()) <= 40, "the bound assumes non-negative weights, at most 40 taps a filter"
        nb = int(np.nonzero(fb.any(1))[0].max()) + 1 if fb.any() else 1          # bins above the last weighted one play no part
        self.nb = nb if not keep_spectrum else max(nb, 768)
        sf = fb.sum(0)
        B = len(x)
        self.m = np.empty((B, N_FRAMES, N_MELS)); self.s1 = np.empty_like(self.m); self.e2 = np.empty((B, N_FRAMES))
        self.bad = np.empty((B, N_FRAMES), bool)
        self.sf = sf
        if keep_spectrum:
            self.A = np.empty((B, N_FRAMES, self.nb)); self.P = np.empty_like(self.A)
        for i in range(B):
            fs = frame_samples(x[i:i + 1].astype(np.float64))[0]
            self.bad[i] = ~np.isfinite(fs).all(-1)
            fr = np.where(self.bad[i][:, None], 0.0, fs * np.asarray(win, dtype=np.float64))
            A = np.abs(np.fft.rfft(fr, n=2048, axis=-1))[:, :self.nb]
            self.e2[i] = np.sqrt((fr ** 2).sum(-1))
            self.m[i] = (A * A) @ fb[:self.nb]
            self.s1[i] = A @ fb[:self.nb]
            if keep_spectrum:
                self.A[i] = A; self.P[i] = A * A

    def features(self):
        """(B, 128, 256) float64."""
        return g(1.0 + self.m).transpose(0, 2, 1)

    def interval(self, k=K):
        """-> lo, hi (B, 128, 256) float64: where a feature may lie."""
        eps = k * U * self.e2[..., None]
        dm = 2 * self.s1 * eps + self.sf * eps ** 2 + REL_MEL * self.m
        one, inf = np.float32(1), np.float32(np.inf)
        with np.errstate(over="ignore"):
            ylo = np.maximum((1 + self.m - dm), 1.0).astype(np.float32)
            yhi = (1 + self.m + dm).astype(np.float32)
        for _ in range(2):
            ylo = np.nextafter(ylo, one); yhi = np.nextafter(yhi, inf)
        lo = g(ylo.astype(np.float64)) * (1 - REL_G)
        hi = g(yhi.astype(np.float64)) * (1 + REL_G)
        return lo.transpose(0, 2, 1), hi.transpose(0, 2, 1)

    def outside(self, feat, k=K):
        """feat (B, 128, 256) -> bool (B, 128, 256): outside the interval, or not NaN in a frame that holds a non-finite sample."""
        f = np.asarray(feat, dtype=np.float64)
        lo, hi = self.interval(k)
        bad = np.broadcast_to(self.bad[:, None, :], f.shape)
        return np.where(bad, ~np.isnan(f), ~((f >= lo) & (f <= hi)))

    def check(self, feat, k=K):
        """-> dict(over: values outside, ratio: worst |feature - interval midpoint| / half-width over the finite frames (1: on the
        interval's edge), at: (window, mel row, frame) of it, ratio_loud: the worst over the values with m >= 1, width_max, width_median)."""
        f = np.asarray(feat, dtype=np.float64)
        assert f.shape == (len(self.m), N_MELS, N_FRAMES), f.shape
        lo, hi = self.interval(k)
        bad = np.broadcast_to(self.bad[:, None, :], f.shape)
        out = np.where(bad, ~np.isnan(f), ~((f >= lo) & (f <= hi)))
        half = 0.5 * (hi - lo)
        with np.errstate(invalid="ignore"):
            # (where the interval starts at 0, the feature of m + 1 = 1, nothing can lie below it: the distance from 0 over the width)
            r = np.where(lo == 0, f / (hi - lo), np.abs(f - 0.5 * (hi + lo)) / half)
        r = np.where(bad, np.where(np.isnan(f), 0.0, np.inf), np.where(np.isnan(r), np.inf, r))
        at = np.unravel_index(int(np.argmax(r)), r.shape)
        # the same over the values with m >= 1 alone: there the float32 grid of 1 + m is finer than the allowance and the ratio shows
        # the arithmetic, not on which side of a grid step a quiet bin fell
        loud = r[np.broadcast_to((self.m >= 1.0).transpose(0, 2, 1), r.shape)]
        return dict(over=int(out.sum()), ratio=float(r[at]), at=tuple(int(i) for i in at), ratio_loud=float(loud.max()) if loud.size else 0.0,
                    width_max=float((hi - lo).max()), width_median=float(np.median(hi - lo)))

    def min_k(self, feat, ks=(1, 2, 4, 8, 16, 32, 64)):
        """The smallest K of ks with zero values outside (None: none)."""
        for k in ks:
            if not self.outside(feat, k).any():
                return k
        return None

    def power_bound(self, k=K):
        """-> P64, bound (B, 256, nb) for the power-spectrum read-back (needs keep_spectrum)."""
        eps = k * U * self.e2[..., None]
        return self.P, 2 * self.A * eps + eps ** 2 + REL_POW * self.P


class ReferenceSet:
    """Reference of many windows, held in chunks of 8 (memory) and computed on up to 8 threads (numpy's FFT releases the lock)."""

    def __init__(self, x, win, fb, keep_spectrum=False, chunk=8, threads=8):
        from concurrent.futures import ThreadPoolExecutor
        self.chunk, self.n = chunk, len(x)
        with ThreadPoolExecutor(max_workers=threads) as ex:
            self.parts = list(ex.map(lambda i: Reference(x[i:i + chunk], win, fb, keep_spectrum), range(0, len(x), chunk)))

    def check(self, feat, k=K):
        assert len(feat) == self.n, (len(feat), self.n)
        rep = None
        for j, part in enumerate(self.parts):
            i = j * self.chunk
            r = part.check(feat[i:i + self.chunk], k)
            r["at"] = (r["at"][0] + i,) + r["at"][1:]
            if rep is None:
                rep = r
            else:
                rep = dict(over=rep["over"] + r["over"], ratio_loud=max(rep["ratio_loud"], r["ratio_loud"]), width_max=max(rep["width_max"], r["width_max"]), width_median=rep["width_median"],
                           **({"ratio": r["ratio"], "at": r["at"]} if r["ratio"] > rep["ratio"] else {"ratio": rep["ratio"], "at": rep["at"]}))
        return rep


def check(feat, x, win, fb, k=K):
    return ReferenceSet(x, win, fb).check(feat, k)


def line(name, rep):
    return "FRONTEND %s worst |delta| / half-width %.4g at window %d, mel row %d, frame %d (%.4g where m >= 1); outside %d" % (
        (name, rep["ratio"]) + tuple(rep["at"]) + (rep["ratio_loud"], rep["over"]))


# ---- the input set (every class one seeded signal and its window starts, for add_f32_22k(..., padded=True)) -------------------------
TONE_AMPS = (0.5, 1e-2, 1e-4)
LADDER = (1e-30, 1e-6, 1e-3, 1.0, 1e3, 1e12)
IMPULSES = (0, 1, 255, 256, 257, 511, 33075, 66149)
TONE_HOP = 32 * 2048                # a window holds 32 tone segments and 614 samples of the 33rd


def stepped_tones(amp):
    """The tone steps every 2048 samples through k = 0, 0.5, 1, ... 767.5 bins of the 2048-point FFT (segment s: k = s / 2): every bin
    centre, hence every tap of every filter, is the dominant term of the frames inside its segment.  48 windows; window i holds the
    bins 16 i .. 16 i + 15, and starts 37 i mod 256 samples into its first segment (arbitrary alignments)."""
    k = np.arange(1536) / 2.0
    n = np.arange(2048, dtype=np.float64)
    seg = amp * np.cos(2 * np.pi * k[:, None] / 2048.0 * n[None, :] + 0.3 * k[:, None])
    sig = np.concatenate([seg.reshape(-1), seg[0]]).astype(np.float32)
    starts = TONE_HOP * np.arange(48) + (37 * np.arange(48)) % 256
    return sig, starts


def tone_window_of_bin(k):
    return int(k) // 16


def input_set(c1_padded, c1_starts, c5=None):
    """-> list of (class name, float32 signal, starts).  c5: (padded signal, starts) of test_gpu_c3's C5 windows, where at hand."""
    rng = np.random.default_rng(20261)
    out = []
    for a in TONE_AMPS:
        out.append(("tones_%g" % a,) + stepped_tones(a))
    imp = np.zeros(len(IMPULSES) * N_WIN, np.float32)
    for i, p in enumerate(IMPULSES):
        imp[i * N_WIN + p] = 0.9
    out.append(("impulses", imp, N_WIN * np.arange(len(IMPULSES))))
    for a in LADDER:
        nw = 8 if a == 1.0 else 4
        sig = (rng.uniform(-1.0, 1.0, N_WIN + 13231 * (nw - 1)) * a).astype(np.float32)
        assert np.isfinite(sig).all()
        out.append(("white_%g" % a, sig, 13231 * np.arange(nw)))
    out.append(("dc_0.999", np.full(N_WIN, 0.999, np.float32), np.array([0])))
    out.append(("square_74", np.where((np.arange(N_WIN) // 37) % 2 == 0, 1.0, -1.0).astype(np.float32), np.array([0])))
    out.append(("c1", np.asarray(c1_padded, dtype=np.float32), np.asarray(c1_starts)))
    if c5 is not None:
        out.append(("c5", np.asarray(c5[0], dtype=np.float32), np.asarray(c5[1])))
    return out


C5_PICK = (0, 5, 400, 401, 777, 1000, 1004)


def c5_windows():
    """The C5 windows of test_gpu_c3 (10 min of 48 kHz stereo PCM16 through the plain-C oracle's mixdown and resampler, which the device
    equals bit for bit there) -> (padded signal, the seven picked starts)."""
    from softspoken_amd import synth, native
    from oracle import oracle_c, oracle_np as O
    oracle_c.build()
    x2 = synth.to_pcm16(synth.synth_audio(5000, 60.0, 48000, 2, with_silence=False))
    x = np.ascontiguousarray(np.concatenate([x2] * 10))
    sig = oracle_c.decode_resample(x.view(np.uint8).reshape(-1), native.PCM_S16, 2, x.shape[0], 48000)
    return O.pad_3s(sig), O.plan_windows(600.0)[list(C5_PICK)]
