"""The network's graph as csrc/net.h states it (kActs, kBlocks), compiled for the host into a small program that prints the two tables:
the tables agree with themselves, and the tests' own copies of the graph (test_gpu_layers.BLOCKS, checkpoint_zoo.GRAPH,
test_v4_forms.LAYERS) say the same graph."""
import json
import os
import shutil
import subprocess

import pytest

import checkpoint_zoo
import test_gpu_layers
import test_v4_forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the unit under test: the host-only header, no kernel and no HIP call in it
_SRC = r"""
#include "net.h"
#include <cstdio>
using namespace ss;
static void act(const char* key, Act t, const char* end) {
    if (t == kNoAct) printf("\"%s\": null%s", key, end); else printf("\"%s\": \"%s\"%s", key, kActs[t].name, end);
}
int main() {
    printf("{\"count\": %d, \"acts\": [", (int)kActCount);
    for (int i = 0; i < kActCount; ++i)
        printf("%s[\"%s\", %d, %d, %d, %d]", i ? ", " : "", kActs[i].name, kActs[i].H, kActs[i].W, kActs[i].C, kActs[i].frag_order ? 1 : 0);
    printf("], \"blocks\": [");
    for (int i = 0; i < kBlockCount; ++i) {
        const Block& k = kBlocks[i];
        printf("%s{\"name\": \"%s\", \"c0\": %d, \"c1\": %d, \"cout\": %d, \"H\": %d, \"W\": %d, ", i ? ", " : "", k.name, k.c0, k.c1, k.cout, k.H, k.W);
        act("x0", k.x0, ", "); act("x1", k.x1, ", "); act("h", k.h, ", "); act("r", k.r, ", "); act("y", k.y, ", "); act("pool", k.pool, ", ");
        printf("\"first_in_loader\": %d, \"flat_in_b\": %d, \"spec_only\": %d}", k.first_in_loader, k.flat_in_b, k.spec_only);
    }
    printf("]}\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def net(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    d = tmp_path_factory.mktemp("net_table")
    src, exe = d / "net_table.hip", d / "net_table"
    src.write_text(_SRC)
    r = subprocess.run([hipcc, "-O1", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-I", os.path.join(ROOT, "softspoken_amd", "csrc"),
                        str(src), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    t = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    t["shape"] = {a[0]: tuple(a[1:4]) for a in t["acts"]}
    return t


def test_the_tables_agree_with_themselves(net):
    acts, blocks, shape = net["acts"], net["blocks"], net["shape"]
    assert len(acts) == net["count"] == 36 and len(blocks) == 11
    assert len(shape) == len(acts) and len({b["name"] for b in blocks}) == len(blocks)        # names are unique
    written = set()                                      # the y and pool tensors of the blocks so far
    for b in blocks:
        H, W, co = b["H"], b["W"], b["cout"]
        if b["first_in_loader"]:                         # conv1_1: the single feature channel, no input tensor, no r
            assert (b["name"], b["x0"], b["x1"], b["r"], b["c0"], b["c1"]) == ("conv1_1", None, None, None, 1, 0)
        else:
            assert b["x0"] in written and shape[b["x0"]] == (H, W, b["c0"]), b
            assert shape[b["r"]] == (H, W, co), b
        if b["x1"]:
            assert b["x1"] in written and shape[b["x1"]] == (H // 2, W // 2, b["c1"]), b
        else:
            assert b["c1"] == 0, b
        assert shape[b["h"]] == shape[b["y"]] == (H, W, co), b
        if b["pool"]:
            assert shape[b["pool"]] == (H // 2, W // 2, co), b
        written |= {b["y"], b["pool"]} - {None}
    # every tensor belongs to exactly one block, in exactly one role
    roles = [b[k] for b in blocks for k in ("h", "r", "y", "pool") if b[k]]
    assert sorted(roles) == sorted(shape)
    assert {a[0] for a in acts if a[4]} == {b["r"] for b in blocks if b["r"]}                  # exactly the r tensors are frag_order
    assert len([a for a in acts if a[4]]) == 10
    assert [b["name"] for b in blocks if b["flat_in_b"]] == ["conv9_1"]
    assert [b["name"] for b in blocks if b["spec_only"]] == ["spec_output_conv.0"] and blocks[-1]["spec_only"]


def test_the_tests_say_the_same_graph(net):
    blocks = net["blocks"]
    # test_gpu_layers.BLOCKS: the blocks behind conv1_1 with their tensors
    assert test_gpu_layers.BLOCKS == [tuple(b[k] for k in ("name", "x0", "x1", "h", "r", "y", "pool")) for b in blocks[1:]]
    assert (blocks[0]["name"], blocks[0]["y"], blocks[0]["pool"]) == ("conv1_1", "c1", "p1")       # (what its check_pass reads of conv1_1)
    # checkpoint_zoo.GRAPH names a block's inputs by the producing block's OUTPUT y, whether the consumer reads y or its pooled copy
    unpooled = {b["pool"]: b["y"] for b in blocks if b["pool"]}
    assert checkpoint_zoo.GRAPH == [(b["name"], unpooled.get(b["x0"], b["x0"]), b["x1"], b["h"], b["y"]) for b in blocks]
    assert checkpoint_zoo.COUT == {b["name"]: b["cout"] for b in blocks}
    # test_v4_forms.LAYERS: name, H, W, C0, C1, Cout, the block pools
    assert test_v4_forms.LAYERS == [(b["name"], b["H"], b["W"], b["c0"], b["c1"], b["cout"], b["pool"] is not None) for b in blocks]
