"""The recordings of the source-output tests (tests/test_source_out_host.py without a GPU, tests/test_gpu_source_out.py with one): one
definition, so that the CPU test shows the reference inside its own bound on exactly the cases the GPU test holds the device to."""
import numpy as np

import source_out_ref as S

FMT = dict(u8=1, pcm16=2, pcm24=3, pcm32=4, f32=5, f64=6, s8=7, s16be=8, s24be=9, s32be=10, f32be=11, f64be=12)

# (name, rate, channels): the separation bound's cases, 2.5 s each under test_gpu_separation.B1_REGIONS and the spread head, fp32
SEP_CASES = [("u8", 8000, 1), ("pcm16", 16000, 3), ("f32", 22050, 2), ("pcm24", 44100, 1), ("pcm32", 96000, 5), ("f64", 16000, 2),
             ("s16be", 16000, 2), ("s24be", 22050, 1), ("f32be", 8000, 2)]
F16_CASE = ("pcm24", 48000, 2)                 # the one f16x2 context; also the each-channel case
LINK_CASES = [("f32", 22050, 2), ("f32be", 8000, 2), ("f64", 16000, 2)]          # exact link to the 16-bit path, scale 0.5

_RECS = {}


def pack(x: np.ndarray, name: str, sr: int):
    """(data bytes uint8, format code, decoded float32 (frames, ch)) of samples x float32 (frames, ch) in the encoding `name`: the WAV
    encodings through test_gpu_separation._pack (synth.wav_bytes), the AIFF ones through synth.aiff_bytes and the library's header walk,
    f64 / s8 / s32be / f64be as raw sample bytes."""
    import test_gpu_separation as T
    from softspoken_amd import native, synth
    fmt, ch = FMT[name], x.shape[1]
    if name in ("u8", "pcm16", "pcm24", "pcm32", "f32"):
        data, info, dec, _ = T._pack(x, name, sr)
        assert info.format == fmt
        return np.ascontiguousarray(data), fmt, dec
    if name in ("s16be", "s24be", "f32be"):
        if name == "f32be":
            img = synth.aiff_bytes(x, sr, compression=b"fl32")
        else:
            bits = 16 if name == "s16be" else 24
            S_ = float(1 << (bits - 1))
            img = synth.aiff_bytes(np.clip(np.rint(x.astype(np.float64) * S_), -S_, S_ - 1).astype(np.int64), sr, bits)
        info = native.wav_parse(img)
        assert info.format == fmt and info.channels == ch and info.frames == len(x)
        data = np.frombuffer(img, dtype=np.uint8, count=info.data_bytes, offset=info.data_offset).copy()
    elif name in ("f64", "f64be"):
        data = np.frombuffer(np.ascontiguousarray(x).astype("<f8" if name == "f64" else ">f8").tobytes(), dtype=np.uint8).copy()
    else:
        data = S.encode(x.reshape(-1), fmt)
    return data, fmt, S.decode(data, fmt).reshape(-1, ch)


def rec(name: str, sr: int, ch: int, seconds: float = 2.5, seed: int = 51, scale: float = 0.5):
    """A seeded recording (test_gpu_separation._make's audio) in the encoding `name`, cached: pack()'s tuple."""
    from softspoken_amd import synth
    key = (name, sr, ch, seconds, seed, scale)
    if key not in _RECS:
        x = synth.synth_audio(seed, seconds, sr, ch, with_silence=False).T.reshape(-1, ch)
        _RECS[key] = pack((x * scale).astype(np.float32), name, sr)
    return _RECS[key]


def check_bound(label: str, got: np.ndarray, data, fmt: int, ch: int, m: np.ndarray, y64: np.ndarray, e32: float, n_fft: int) -> float:
    """Hold output bytes `got` (frames, fb) to source_out_ref.separation_bound inside the mask m and to the input's bytes outside it;
    prints the case's line and returns the largest excess over the tolerance (<= 0 when the case passes; asserted here)."""
    frames = len(m)
    src = np.frombuffer(np.ascontiguousarray(data), dtype=np.uint8)[: got.size].reshape(got.shape)
    assert np.array_equal(got[~m], src[~m]), label
    ref, tol = S.separation_bound(y64[m], e32, fmt)
    inside = np.ascontiguousarray(got[m]).reshape(-1)
    val = (S.codes(inside, fmt) if fmt in S.BITS else S.decode(inside, fmt)).astype(np.float64).reshape(-1, ch)
    over = np.abs(val - ref) - tol
    worst = float(over.max()) if over.size else 0.0
    print(f"SRCBOUND {label}: N={n_fft} ch={ch} fmt={fmt} e32={e32:.5f} tol={float(tol.max()) if over.size else 0.0:.6g} "
          f"largest |got - ref| - tol={worst:.6g} samples={over.size} frames={frames}")
    assert worst <= 0.0, (label, worst, int((over > 0).sum()))
    return worst
