"""The byte order of the 16-bit activation tensors (csrc/kernels.h: ActStride, act_stride, act_offset), compiled for the host and
enumerated for every tensor shape of the network: the five resolutions 128 x 256 ... 8 x 16, 32 / 64 / 96 / 128 channels, and the
half-resolution source of an upsampled input.

  * pixel-major ([window][H][W][C]) and chunk-planar ([window][C / 32][H][W][32]) are both bijections of (y, x, c) onto the same
    H W C 2 bytes of a window; pixel-major is ((y W + x) C + c) 2, chunk-planar the formula of kernels.h; for 32 channels they are
    the same order; chunk-planar, a chunk's patch row is contiguous;
  * every 16-byte piece a patch load can address -- offsets formed as the loaders of conv4.hip and conv4_ups.hip form them: a piece's
    pixel index from the patch origin times the pixel pitch, plus the tile's origin offset (mod 2^32), or 0 (the zero header) when the
    piece's halo side is a picture border -- stays inside header + tensor and is the piece it should be: the 10 x 18 and 18 x 18 patches
    at every tile origin, their nearest-upsampled form on a half-resolution source, and the 6 x 10 low-resolution patch."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SRC = r"""
#include "kernels.h"
#include <vector>
using ss::ActStride;
static constexpr uint32_t kHdr = 256;
extern "C" {
void al_stride(int H, int W, int C, int planar, uint32_t* out) { const ActStride s = ss::act_stride(H, W, C, planar != 0); out[0] = s.pix; out[1] = s.chunk; }
uint32_t al_offset(int H, int W, int C, int planar, int n, int y, int x, int c) {
    return ss::act_offset(ss::act_stride(H, W, C, planar != 0), H, W, C, n, y, x, c);
}
// offsets of every (y, x, c) of window n, minus the window's first byte: out[(y W + x) C + c]
void al_window(int H, int W, int C, int planar, int n, int64_t* out) {
    const ActStride s = ss::act_stride(H, W, C, planar != 0);
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) for (int c = 0; c < C; ++c)
        out[((int64_t)y * W + x) * C + c] = (int64_t)ss::act_offset(s, H, W, C, n, y, x, c) - (int64_t)n * ss::act_window_bytes(H, W, C);
}
// The patch loads of a launch over an [N][H][W] picture in tiles of TH x 16 pixels, every 32-channel chunk of the source tensor, every
// 16-byte part.  mode 0: the source has the picture's resolution, patch (TH + 2) x 18 from (y0 - 1, x0 - 1) (conv4.hip pix_full,
// conv4_ups.hip's skip patch); mode 1: the source [N][H/2][W/2] nearest-upsampled, the same patch (conv4.hip pix_half); mode 2: the
// source [N][H/2][W/2] at its own resolution, patch (TH/2 + 2) x 10 from (y0/2 - 1, x0/2 - 1) (conv4_ups.hip's low-resolution patch).
// Returns the number of pieces that are wrong: outside [0, header + tensor), or not the piece (n, y, x, chunk, part) / the header.
int64_t al_patch_walk(int N, int H, int W, int C, int planar, int TH, int mode, int64_t* n_pieces) {
    const int Hs = mode ? H >> 1 : H, Ws = mode ? W >> 1 : W;
    const ActStride s = ss::act_stride(Hs, Ws, C, planar != 0);
    const uint64_t end = (uint64_t)kHdr + (uint64_t)N * Hs * Ws * C * 2;
    const int PR = mode == 2 ? TH / 2 + 2 : TH + 2, PC = mode == 2 ? 10 : 18;
    int64_t bad = 0, count = 0;
    for (int n = 0; n < N; ++n) for (int y0 = 0; y0 < H; y0 += TH) for (int x0 = 0; x0 < W; x0 += 16) for (int ch = 0; ch < C; ch += 32) {
        const uint32_t tm = (y0 == 0 ? 1u : 0u) | (y0 + TH == H ? 2u : 0u) | (x0 == 0 ? 4u : 0u) | (x0 + 16 == W ? 8u : 0u);
        const uint32_t toff = kHdr + (mode ? ss::act_offset(s, Hs, Ws, C, n, (y0 >> 1) - 1, (x0 >> 1) - 1, ch)
                                           : ss::act_offset(s, H, W, C, n, y0 - 1, x0 - 1, ch));
        for (int pyy = 0; pyy < PR; ++pyy) for (int pxx = 0; pxx < PC; ++pxx) for (int part = 0; part < 4; ++part) {
            const uint32_t f = (pyy == 0 ? 1u : 0u) | (pyy == PR - 1 ? 2u : 0u) | (pxx == 0 ? 4u : 0u) | (pxx == PC - 1 ? 8u : 0u);
            const uint32_t pix = mode == 0 ? pyy * W + pxx : mode == 1 ? ((pyy + 1) >> 1) * Ws + ((pxx + 1) >> 1) : pyy * Ws + pxx;
            uint32_t off = pix * s.pix + (toff + part * 16u);                 // mod 2^32, as the loaders
            if (f & tm) off = 0;
            ++count;
            // where the piece lies in the source
            const int sy = mode == 0 ? y0 - 1 + pyy : mode == 1 ? (y0 >> 1) - 1 + ((pyy + 1) >> 1) : (y0 >> 1) - 1 + pyy;
            const int sx = mode == 0 ? x0 - 1 + pxx : mode == 1 ? (x0 >> 1) - 1 + ((pxx + 1) >> 1) : (x0 >> 1) - 1 + pxx;
            const bool inside = sy >= 0 && sy < Hs && sx >= 0 && sx < Ws;
            if ((uint64_t)off + 16 > end) { ++bad; continue; }
            if (inside != !(f & tm)) { ++bad; continue; }                      // the flags name exactly the pieces outside the picture
            if (inside) {
                const uint64_t want = (uint64_t)kHdr + (uint64_t)n * Hs * Ws * C * 2 +
                                      (planar && C > 32 ? (uint64_t)(ch / 32) * Hs * Ws * 64 + ((uint64_t)sy * Ws + sx) * 64
                                                        : (((uint64_t)sy * Ws + sx) * C + ch) * 2) + part * 16;
                if (off != want) ++bad;
            }
        }
    }
    *n_pieces = count;
    return bad;
}
}
"""

LEVELS = [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)]
CHANNELS = [32, 64, 96, 128]


@pytest.fixture(scope="module")
def al(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    d = tmp_path_factory.mktemp("act_layout")
    src = d / "act_layout.hip"
    src.write_text(_SRC)
    lib = d / "libact_layout.so"
    cmd = [hipcc, "-O1", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "softspoken_amd", "csrc"), str(src), "-o", str(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    L = ctypes.CDLL(str(lib))
    L.al_offset.restype = ctypes.c_uint32
    L.al_patch_walk.restype = ctypes.c_int64
    L.al_patch_walk.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
    return L


def _window(al, H, W, C, planar, n):
    out = np.empty(H * W * C, np.int64)
    al.al_window(H, W, C, planar, n, out.ctypes.data_as(ctypes.c_void_p))
    return out.reshape(H, W, C)


def _stride(al, H, W, C, planar):
    s = (ctypes.c_uint32 * 2)()
    al.al_stride(H, W, C, planar, s)
    return int(s[0]), int(s[1])


@pytest.mark.parametrize("H,W", LEVELS)
@pytest.mark.parametrize("C", CHANNELS)
def test_orders_are_bijections_with_the_stated_formulas(al, H, W, C):
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    nhwc_want = ((y * W + x) * C + c) * 2
    planar_want = (c // 32) * (H * W * 64) + (y * W + x) * 64 + (c % 32) * 2
    assert _stride(al, H, W, C, 0) == (2 * C, 64)
    assert _stride(al, H, W, C, 1) == ((64, H * W * 64) if C > 32 else (2 * C, 64))
    for n in (0, 3):                                   # (the window stride is H W C 2 in both orders: al_window subtracts it)
        nhwc = _window(al, H, W, C, 0, n)
        planar = _window(al, H, W, C, 1, n)
        assert np.array_equal(nhwc, nhwc_want)
        assert np.array_equal(planar, planar_want)
        for offs in (nhwc, planar):                    # every 2-byte slot of the window's H W C 2 bytes exactly once
            assert np.array_equal(np.sort(offs.ravel()), np.arange(H * W * C) * 2)
        if C == 32:
            assert np.array_equal(nhwc, planar)
    # a chunk's patch row (18 pixels of one row, one chunk) is 18 x 64 contiguous bytes; its last byte's successor is the row's next pixel
    planar = _window(al, H, W, C, 1, 0)
    for k in range(C // 32):
        rows = planar[:, :, 32 * k:32 * k + 32].reshape(H, W * 32)
        assert np.array_equal(np.diff(rows, axis=1), np.full((H, W * 32 - 1), 2))
        assert np.array_equal(np.diff(rows[:, 0]), np.full(H - 1, W * 64))         # and the rows of a chunk follow each other


def test_offsets_of_a_large_pass_stay_32_bit(al):
    # 1016 windows of the largest tensors: the last element's offset, computed mod 2^32, is the true one (below 4 GB)
    for (H, W, C) in [(128, 256, 32), (64, 128, 64), (32, 64, 96), (16, 32, 128)]:
        n = 1015
        true = n * H * W * C * 2 + ((C - 1) // 32) * H * W * 64 + ((H - 1) * W + W - 1) * 64 + ((C - 1) % 32) * 2
        assert true < 2 ** 32
        assert al.al_offset(H, W, C, 1, n, H - 1, W - 1, C - 1) == true


# (H, W) of the launch, rows of its tiles, mode (see al_patch_walk), channels of the source
def _patch_cases():
    cases = []
    for (H, W) in LEVELS:
        for C in CHANNELS:
            for TH in (8, 16):
                if H % TH:
                    continue
                cases.append((H, W, C, TH, 0))
                if H >= 16:                              # a half-resolution source exists down to 8 x 16
                    cases.append((H, W, C, TH, 1))
            if H >= 16:
                cases.append((H, W, C, 8, 2))
    return cases


@pytest.mark.parametrize("planar", [0, 1])
def test_every_patch_piece_stays_inside_header_and_tensor(al, planar):
    total = 0
    for (H, W, C, TH, mode) in _patch_cases():
        for N in (1, 2):
            cnt = ctypes.c_int64(0)
            bad = al.al_patch_walk(N, H, W, C, planar, TH, mode, ctypes.byref(cnt))
            assert bad == 0, (N, H, W, C, planar, TH, mode, bad)
            PR, PC = (TH // 2 + 2, 10) if mode == 2 else (TH + 2, 18)
            assert cnt.value == N * (H // TH) * (W // 16) * (C // 32) * PR * PC * 4
            total += cnt.value
    assert total > 0
