"""Reference of "source output" (include/softspoken.h) in numpy: silenced audio in the recording's own sample
encoding.  fmt is the recording's enum ss_pcm_format (1-6 little endian U8 S16 S24 S32 F32 F64; 7-12 big endian S8 S16 S24 S32 F32 F64),
fb = channels x bytes per sample the frame size; the merged frame ranges of a region table are ss_silence_pcm's (Python round, clamped
to the file, merged: separation_ref.merged_intervals).

Zeroing: a byte whose frame lies in no range is the input byte (nothing is decoded); a byte whose frame lies in a range is the encoding's
zero, 0x80 for U8 and 0x00 for the other eleven.

Encode of a float32 y: an integer format of b bits has S = 2^(b-1), q = rint(y x S) with the product in float32 (exact, a power of two)
rounded to nearest even, saturated to [-S, S - 1], NaN -> 0; U8 stores q + 128, S8 q; F32 stores y's bits, F64 (double)y; the big-endian
formats the same value with its bytes reversed.

Separation: separation_ref's y = x + w (p - x) inside a merged interval, encoded; outside, the input's bytes."""
import numpy as np

import separation_ref as R

BPS = {1: 1, 2: 2, 3: 3, 4: 4, 5: 4, 6: 8, 7: 1, 8: 2, 9: 3, 10: 4, 11: 4, 12: 8}
BITS = {1: 8, 2: 16, 3: 24, 4: 32, 7: 8, 8: 16, 9: 24, 10: 32}           # the integer formats
ZERO_BYTE = {f: (0x80 if f == 1 else 0x00) for f in BPS}
BIG_ENDIAN = {7, 8, 9, 10, 11, 12}


def _samples_le(data: np.ndarray, fmt: int) -> np.ndarray:
    """(n, bytes per sample) uint8, every sample's bytes in little-endian order."""
    b = np.frombuffer(np.ascontiguousarray(data), dtype=np.uint8).reshape(-1, BPS[fmt])
    return b[:, ::-1] if fmt in BIG_ENDIAN else b


def codes(data, fmt: int) -> np.ndarray:
    """The integer code of every sample of an integer format (U8: the stored byte - 128), int64."""
    b = _samples_le(data, fmt).astype(np.int64)
    bits = BITS[fmt]
    v = sum(b[:, i] << (8 * i) for i in range(bits // 8))
    if fmt == 1:
        return v - 128
    return np.where(v >= 1 << (bits - 1), v - (1 << bits), v)


def decode(data, fmt: int) -> np.ndarray:
    """PCM bytes -> float32, as the library's loader decodes (x / 2^(bits-1); 32-bit through double; F64 rounded to float32)."""
    if fmt in BITS:
        k, S = codes(data, fmt), float(1 << (BITS[fmt] - 1))
        return (k.astype(np.float64) / S).astype(np.float32)
    le = np.ascontiguousarray(_samples_le(data, fmt))
    if BPS[fmt] == 4:
        return le.view("<f4").reshape(-1).copy()
    with np.errstate(over="ignore"):
        return le.view("<f8").reshape(-1).astype(np.float32)


def quantize(y, bits: int) -> np.ndarray:
    """q of the definition, int64."""
    y = np.asarray(y, dtype=np.float32)
    S = np.float32(1 << (bits - 1))
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.rint(y * S).astype(np.float64)                 # the float32 product, rounded to nearest even
    q = np.where(np.isnan(q), 0.0, q)
    return np.clip(q, -float(S), float(S) - 1.0).astype(np.int64)


def encode(y, fmt: int) -> np.ndarray:
    """float32 samples -> the bytes of `fmt`, uint8 (n x bytes per sample)."""
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    if fmt in BITS:
        q = quantize(y, BITS[fmt])
        if fmt == 1:
            q = q + 128
        le = np.stack([(q >> (8 * i)) & 255 for i in range(BPS[fmt])], axis=1).astype(np.uint8)
    elif BPS[fmt] == 4:
        le = y.astype("<f4").view(np.uint8).reshape(-1, 4)
    else:
        le = y.astype("<f8").view(np.uint8).reshape(-1, 8)
    return np.ascontiguousarray(le[:, ::-1] if fmt in BIG_ENDIAN else le).reshape(-1)


def frame_mask(frames: int, sr: int, regions) -> np.ndarray:
    m = np.zeros(frames, dtype=bool)
    for a, b in R.merged_intervals(regions, sr, frames):
        m[a:b] = True
    return m


def silence_source(data, fmt: int, sr: int, channels: int, frames: int, regions) -> np.ndarray:
    """ss_silence_pcm_source: uint8 (frames, fb)."""
    fb = channels * BPS[fmt]
    out = np.frombuffer(np.ascontiguousarray(data), dtype=np.uint8)[: frames * fb].reshape(frames, fb).copy()
    out[frame_mask(frames, sr, regions)] = ZERO_BYTE[fmt]
    return out


def separate_source(data, fmt: int, sr: int, channels: int, frames: int, regions, y: np.ndarray) -> np.ndarray:
    """ss_separate_pcm_source given the blend y (frames, channels) in unit scale (float32): the input's bytes outside the merged
    intervals, encode(y) inside."""
    fb = channels * BPS[fmt]
    out = np.frombuffer(np.ascontiguousarray(data), dtype=np.uint8)[: frames * fb].reshape(frames, fb).copy()
    m = frame_mask(frames, sr, regions)
    out[m] = encode(np.asarray(y, dtype=np.float32)[m].reshape(-1), fmt).reshape(-1, fb)
    return out


def ulp32(v) -> np.ndarray:
    """The spacing of float32 at |v| (float64 in, float64 out)."""
    a = np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)
    return np.spacing(a).astype(np.float64)


def separation_bound(y64_lsb: np.ndarray, e32_lsb: float, fmt: int):
    """(reference, tolerance) of a separated output in the units the output is compared in: integer codes for the integer formats, unit
    scale for the float ones.  y64_lsb: the unrounded float64 output of separation_ref.separate(..., unrounded=True), in units of
    1 / 32767; e32_lsb: max |separate_f32 - y64| of the case in the same units.  |got - y64 u| <= r + 4 e32 u with u = S / 32767 and
    r = max(0.5, 0.5 ulp_float32(y) S), the output rounding of a float32 value; the float formats: u = 1 / 32767, r = 0.5 ulp_float32(y).
    The reference is clipped to the codes, which cannot widen the bound."""
    y = np.asarray(y64_lsb, dtype=np.float64) / 32767.0
    if fmt in BITS:
        S = float(1 << (BITS[fmt] - 1))
        ref = np.clip(y * S, -S, S - 1.0)
        r = np.maximum(0.5, 0.5 * ulp32(y) * S)
        return ref, r + 4.0 * e32_lsb * S / 32767.0
    return y, 0.5 * ulp32(y) + 4.0 * e32_lsb / 32767.0
