"""The work order "one group per workgroup" (csrc/kernels.h: gres_item, gres_items, gres_group, gres_grid, gres_grid_ok), compiled for the
host and enumerated: workgroup w of an XCD carries channel group w mod ngroups for its whole life (its banks stay in LDS), the
G / ngroups slots deal the XCD's positions among themselves, NH consecutive ones per item, and the workgroups of a slot walk the same
position sequence."""
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
int gr_grid_ok(int grid, int ngroups) { return ss::gres_grid_ok(grid, ngroups) ? 1 : 0; }
int gr_grid(int num_cus, int total_pos, int ngroups, int nh) { return ss::gres_grid(num_cus, total_pos, ngroups, nh); }
int gr_group(int wg, int ngroups) { return ss::gres_group(wg, ngroups); }
// the whole walk of a launch: visits[pos * ngroups + g] += 1; rec[((xcd * G + wg) * max_items + item) * nh + tile] = pos * ngroups + g,
// or -1 - g (no work); returns the largest item count of a tile, -1 when gres_items disagrees with gres_item
int gr_walk(int G, int total_pos, int ngroups, int nh, int max_items, int* visits, int* rec) {
    int most = 0;
    for (int xcd = 0; xcd < 8; ++xcd)
        for (int wg = 0; wg < G; ++wg)
            for (int tile = 0; tile < nh; ++tile) {
                const int n = ss::gres_items(xcd, wg, G, tile, total_pos, ngroups, nh);
                if (n > most) most = n;
                for (int item = 0; item < max_items; ++item) {
                    const ss::RingItem r = ss::gres_item(xcd, wg, G, item, tile, total_pos, ngroups, nh);
                    if (r.pos >= 0) visits[r.pos * ngroups + r.g] += 1;
                    if ((r.pos >= 0) != (item < n)) return -1;                     // work is a prefix of the items, as long as gres_items says
                    rec[(((long)xcd * G + wg) * max_items + item) * nh + tile] = r.pos >= 0 ? r.pos * ngroups + r.g : -1 - r.g;
                }
            }
    return most;
}
}
"""


@pytest.fixture(scope="module")
def gr(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    d = tmp_path_factory.mktemp("group_resident_order")
    src = d / "group_resident_order.hip"
    src.write_text(_SRC)
    lib = d / "libgroup_resident_order.so"
    # the host pass alone: the map is a __host__ __device__ function, and this is the code the chooser runs
    cmd = [hipcc, "-O1", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "softspoken_amd", "csrc"), str(src), "-o", str(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    L = ctypes.CDLL(str(lib))
    ip = ctypes.POINTER(ctypes.c_int)
    L.gr_walk.argtypes = [ctypes.c_int] * 5 + [ip, ip]
    return L


NGROUPS = 2
POSITIONS = [16, 32, 64]              # per window: conv7.B (4 x 4 tiles of 8 x 16), conv2_1.B as 16-row (4 x 8) and 8-row (8 x 8) tiles
WINDOWS = [1, 2, 5, 105, 1005]
GRIDS = [2, 4, 16, 32]                # workgroups per XCD (grid = 8 x this)
TILES = [2, 4]                        # NH


def _walk(gr, G, total_pos, ngroups, nh):
    S = G // ngroups
    units = ((total_pos + 7) // 8 + nh - 1) // nh
    max_items = (units + S - 1) // S + 3           # an upper bound of a workgroup's items, plus a few past the end (without work)
    visits = np.zeros(total_pos * ngroups, np.int32)
    rec = np.full(8 * G * max_items * nh, -99, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    most = gr.gr_walk(G, total_pos, ngroups, nh, max_items, visits.ctypes.data_as(ip), rec.ctypes.data_as(ip))
    assert most >= 0, "a tile has work behind an item without, or gres_items disagrees with gres_item"
    assert most <= max_items - 3
    return visits, rec.reshape(8, G, max_items, nh)


@pytest.mark.parametrize("nh", TILES)
@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("ppw", POSITIONS)
def test_every_position_and_group_exactly_once(gr, ppw, G, nh):
    for n in WINDOWS:
        total_pos = n * ppw
        visits, rec = _walk(gr, G, total_pos, NGROUPS, nh)          # (also: work is a prefix of a tile's items, gres_items of them)
        assert (visits == 1).all(), (ppw, n, G, nh, np.flatnonzero(visits != 1)[:8])
        # a workgroup's group never changes, with or without work, and is w mod ngroups
        g = np.where(rec >= 0, rec % NGROUPS, -1 - rec)
        want = np.array([gr.gr_group(w, NGROUPS) for w in range(G)])
        assert (want == np.arange(G) % NGROUPS).all()
        assert (g == want[None, :, None, None]).all(), (ppw, n, G, nh)
        # the tiles of an item take consecutive positions of the workgroup's XCD; a tile without work only behind the tiles that have
        pos = np.where(rec >= 0, rec // NGROUPS, -1)
        have = pos >= 0
        assert (have[..., 1:] <= have[..., :-1]).all()
        assert ((pos - pos[..., :1] == np.arange(nh)) | ~have).all()
        per_pos = (total_pos + 7) >> 3
        xcd = np.arange(8)[:, None, None, None]
        assert (((pos >= xcd * per_pos) & (pos < (xcd + 1) * per_pos)) | ~have).all()


@pytest.mark.parametrize("nh", TILES)
@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("ppw", POSITIONS)
def test_siblings_walk_the_same_positions(gr, ppw, G, nh):
    """The workgroups of a slot (w = slot * ngroups + g) see the same position in every item and tile: a position's patches are read by
    neighbouring workgroups of one XCD at the same time."""
    for n in WINDOWS:
        _, rec = _walk(gr, G, n * ppw, NGROUPS, nh)
        pos = np.where(rec >= 0, rec // NGROUPS, -1).reshape(8, G // NGROUPS, NGROUPS, rec.shape[2], nh)
        assert (pos == pos[:, :, :1]).all(), (ppw, n, G, nh)
        # slot s takes the items s, s + S, s + 2 S, ... of the XCD, nh positions each
        S = G // NGROUPS
        first = pos[:, :, 0, :, 0]
        s, i = np.meshgrid(np.arange(S), np.arange(rec.shape[2]), indexing="ij")
        per_pos = (n * ppw + 7) >> 3
        want = np.arange(8)[:, None, None] * per_pos + (s + i * S)[None] * nh
        assert ((first == want) | (first < 0)).all(), (ppw, n, G, nh)


def test_grid_predicate_and_grid_size(gr):
    # the chooser takes the form only on grids that are a multiple of 8 x ngroups
    for ngroups in (2, 3, 4):
        for grid in range(0, 400):
            assert bool(gr.gr_grid_ok(grid, ngroups)) == (grid > 0 and grid % (8 * ngroups) == 0), (grid, ngroups)
    for nh in TILES:
        for num_cus in (16, 32, 128, 256):
            for ppw in POSITIONS:
                for n in WINDOWS:
                    grid = gr.gr_grid(num_cus, n * ppw, NGROUPS, nh)
                    assert gr.gr_grid_ok(grid, NGROUPS) and grid <= num_cus, (num_cus, ppw, n, nh, grid)
                    # a small pass shrinks the grid to the slots that have an item on the busiest XCD, never below one slot
                    units = ((n * ppw + 7) // 8 + nh - 1) // nh
                    assert grid == 8 * NGROUPS * max(1, min(num_cus // 8 // NGROUPS, units)), (num_cus, ppw, n, nh, grid)
                    visits, _ = _walk(gr, grid // 8, n * ppw, NGROUPS, nh)
                    assert (visits == 1).all()
    # workgroups per XCD that are no multiple of the group count: refused
    for num_cus in (8, 24, 40, 120, 248):
        grid = gr.gr_grid(num_cus, 1005 * 64, NGROUPS, 4)
        assert grid == 0 and not gr.gr_grid_ok(grid, NGROUPS), num_cus
    assert gr.gr_grid(256, 1005 * 64, 3, 4) == 0                 # 32 workgroups per XCD, three groups
