"""The work order of the four-tile ring kernels (csrc/kernels.h: ring_item, ring_items, ring_group0, ring_group_step), compiled for the
host and enumerated: which (position, channel group) each tile of each workgroup takes in each item, for both orders -- side by side
(the product: a quad's groups on neighbouring workgroups of one XCD at the same time) and sequential (the development build's
alternative: a workgroup walks a quad's groups one after the other)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SRC = r"""
#include "kernels.h"
extern "C" {
int wo_item(int xcd, int wg, int G, int item, int tile, int total_pos, int ngroups, int seq, int* g) {
    const ss::RingItem r = ss::ring_item(xcd, wg, G, item, tile, total_pos, ngroups, seq != 0);
    *g = r.g;
    return r.pos;
}
int wo_items(int xcd, int wg, int G, int tile, int total_pos, int ngroups, int seq) { return ss::ring_items(xcd, wg, G, tile, total_pos, ngroups, seq != 0); }
int wo_group0(int wg, int ngroups, int seq) { return ss::ring_group0(wg, ngroups, seq != 0); }
int wo_group_step(int G, int ngroups, int seq) { return ss::ring_group_step(G, ngroups, seq != 0); }
// the whole walk of a launch: out[(pos * ngroups + g)] += 1 per visit; rec[((xcd * G + wg) * max_items + item) * 4 + tile] = pos * ngroups + g
// or -1 - g (no work); returns the largest item count of a tile
int wo_walk(int G, int total_pos, int ngroups, int seq, int max_items, int* visits, int* rec) {
    int most = 0;
    for (int xcd = 0; xcd < 8; ++xcd)
        for (int wg = 0; wg < G; ++wg)
            for (int tile = 0; tile < 4; ++tile) {
                const int n = ss::ring_items(xcd, wg, G, tile, total_pos, ngroups, seq != 0);
                if (n > most) most = n;
                for (int item = 0; item < max_items; ++item) {
                    const ss::RingItem r = ss::ring_item(xcd, wg, G, item, tile, total_pos, ngroups, seq != 0);
                    if (r.pos >= 0) visits[r.pos * ngroups + r.g] += 1;
                    if ((r.pos >= 0) != (item < n)) return -1;                     // work is a prefix of the items, as long as ring_items says
                    rec[(((long)xcd * G + wg) * max_items + item) * 4 + tile] = r.pos >= 0 ? r.pos * ngroups + r.g : -1 - r.g;
                }
            }
    return most;
}
}
"""


@pytest.fixture(scope="module")
def wo(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    d = tmp_path_factory.mktemp("work_order")
    src = d / "work_order.hip"
    src.write_text(_SRC)
    lib = d / "libwork_order.so"
    # the host pass alone: the map is a __host__ __device__ function, and this is the code the launch functions and tools would run
    cmd = [hipcc, "-O1", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "softspoken_amd", "csrc"), str(src), "-o", str(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    L = ctypes.CDLL(str(lib))
    ip = ctypes.POINTER(ctypes.c_int)
    L.wo_item.argtypes = [ctypes.c_int] * 8 + [ip]
    L.wo_walk.argtypes = [ctypes.c_int] * 5 + [ip, ip]
    return L


# (tiles_x, tiles_y, ngroups) of the launches the engine sends through the ring kernels (8 x 16-pixel tiles of a 128 x 256 window's levels):
# conv3_1.A/B, conv4_1.A/B, conv_bottleneck / encoder_out A/B, conv6.A/B, conv7.A/B, conv8.A -- and each tiling with every group count
ENGINE_SHAPES = [(4, 4, 3), (2, 2, 4), (1, 1, 4), (2, 2, 3), (4, 4, 2), (8, 8, 1)]
SHAPES = sorted(set(ENGINE_SHAPES) | {(tx, ty, g) for (tx, ty, _) in ENGINE_SHAPES for g in (1, 2, 3, 4)})
WINDOWS = [1, 2, 5, 105, 1005, 1016]
GRIDS = [1, 19, 32, 38]                                # workgroups per XCD (grid = 8 x this)


def _walk(wo, G, total_pos, ngroups, seq):
    # an upper bound of the items of a workgroup, plus a few past the end (which must be without work)
    quads = ((total_pos + 7) // 8 + 3) // 4
    max_items = max((quads * ngroups + G - 1) // G, (quads + G - 1) // G * ngroups) + 3
    visits = np.zeros(total_pos * ngroups, np.int32)
    rec = np.full(8 * G * max_items * 4, -99, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    most = wo.wo_walk(G, total_pos, ngroups, int(seq), max_items, visits.ctypes.data_as(ip), rec.ctypes.data_as(ip))
    assert most >= 0, "a tile has work behind an item without, or ring_items disagrees with ring_item"
    assert most <= max_items - 3
    return visits, rec.reshape(8, G, max_items, 4)


def _reference_sequential(G, total_pos, ngroups, max_items):
    """The map the kernels used before (conv4.hip tile_of's RING branch, conv4_ups.hip count_pos / compute_next), written out in numpy."""
    per_pos = (total_pos + 7) >> 3
    xcd, wg, it, tile = np.meshgrid(np.arange(8), np.arange(G), np.arange(max_items), np.arange(4), indexing="ij")
    loc, gper = wg * 4 + tile, G * 4
    idx = loc + (it // ngroups) * gper
    pos = xcd * per_pos + idx
    ok = (idx < per_pos) & (pos < total_pos)
    return np.where(ok, pos * ngroups + it % ngroups, -1 - it % ngroups)


@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_every_position_and_group_exactly_once(wo, shape, G):
    tx, ty, ngroups = shape
    for n in WINDOWS:
        total_pos = n * tx * ty
        for seq in (False, True):
            visits, rec = _walk(wo, G, total_pos, ngroups, seq)
            assert (visits == 1).all(), (shape, n, G, seq, np.flatnonzero(visits != 1)[:8])
            # the four tiles of a workgroup carry the same group in every item, with or without work
            g = np.where(rec >= 0, rec % ngroups, -1 - rec)
            assert (g == g[..., :1]).all(), (shape, n, G, seq)
            # ... and take the four consecutive positions of one quad
            pos = np.where(rec >= 0, rec // ngroups, -1)
            have = pos >= 0
            assert (have[..., 1:] <= have[..., :-1]).all()                      # a tile without work: only behind the tiles that have
            assert ((pos - pos[..., :1] == np.arange(4)) | ~have).all()
            # the group sequence of a workgroup is g0 + i * step, as the bank rings' cursors count it
            for w in range(G):
                g0, st = wo.wo_group0(w, ngroups, int(seq)), wo.wo_group_step(G, ngroups, int(seq))
                assert (g[0, w, :, 0] == (g0 + st * np.arange(g.shape[2])) % ngroups).all()


@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_groups_of_a_quad_on_consecutive_workgroups_of_one_xcd(wo, shape, G):
    """Side by side: per XCD the items are (quad, group), group fastest, dealt to the workgroups in turn -- item j runs on workgroup j mod G
    as that workgroup's item j div G.  So the groups of a quad sit on consecutive workgroups (mod G) of ONE XCD, and where they share an
    item index they run at the same time."""
    tx, ty, ngroups = shape
    for n in WINDOWS:
        total_pos = n * tx * ty
        _, rec = _walk(wo, G, total_pos, ngroups, False)
        per_pos = (total_pos + 7) >> 3
        for xcd in range(8):
            r = rec[xcd, :, :, 0]                                               # tile 0 = the quad's first position
            w, it = np.nonzero(r >= 0)
            quad = (r[w, it] // ngroups - xcd * per_pos) // 4
            g = r[w, it] % ngroups
            j = quad * ngroups + g
            assert (w == j % G).all() and (it == j // G).all(), (shape, n, G, xcd)


@pytest.mark.parametrize("G", GRIDS)
def test_one_group_is_the_former_map(wo, G):
    """ngroups = 1: both orders are the map the kernels had; the sequential order is that map for every group count."""
    for tx, ty, _ in ENGINE_SHAPES:
        for n in WINDOWS:
            total_pos = n * tx * ty
            for ngroups in (1, 2, 3, 4):
                _, rec = _walk(wo, G, total_pos, ngroups, True)
                want = _reference_sequential(G, total_pos, ngroups, rec.shape[2])
                assert (rec == want).all(), (tx, ty, n, G, ngroups)
            _, rec = _walk(wo, G, total_pos, 1, False)
            assert (rec == _reference_sequential(G, total_pos, 1, rec.shape[2])).all(), (tx, ty, n, G)

