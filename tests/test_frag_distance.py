"""The f16x2 conv kernels' operand reads stay ahead of their matrix products IN THE BINARY (tools/frag_distance.py): the multiply loops
are written as software prefetch, and hipcc sinks every ds_read to just in front of the v_mfma that consumes it unless fences hold
the order (csrc/mfma_util.h frag_fence).  A compiler update that collapses the prefetch again, or a change that makes one of these
kernels spill, fails here.

Checked on the product build's listing of conv4.hip and conv4_ups.hip, for the f16x2 forms the network's launches take (and every
other NT = 1 f16x2 form the launches recorded in tests/golden/v4_forms.json take in the product library), and for both sub-pixel kernels:
  * no scratch;
  * past the first LEAD products of a burst (the products between two barriers or block labels: one multiply loop and what rides on
    it; the first depth - 1 steps of a loop cannot have their reads ahead), no product has its operands' read closer than FLOOR
    products in front of it.  FLOOR = 2 is what ships: two waves multiply per SIMD, so two products are about one LDS round trip.
conv3x3_upsr_kernel ships with the scheduler's order (fenced it measured 1.3 - 2 % slower): no floor, no scratch."""
import json
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import frag_distance as FD  # noqa: E402

LEAD = 2          # products: two steps of a one-product loop, one step of the merged loop (two products a step), part of a projection step
FLOOR = 2

ASM = """
\t.text
_Z4demov:                               ; @_Z4demov
; %bb.0:
\tds_read_b128 v[0:3], v40
\tds_read_b128 v[4:7], v41 offset:1024
\tds_read_b128 v[8:11], v40 offset:32
\tds_read_b128 v[12:15], v41 offset:2048
\ts_waitcnt lgkmcnt(2)
\tv_mfma_f32_32x32x16_f16 v[16:31], v[4:7], v[0:3], v[16:31]
\tds_read_b128 v[0:3], v40 offset:64
\tds_read2_b64 v[4:7], v41 offset1:1
\tv_mfma_f32_32x32x16_f16 v[16:31], v[12:15], v[8:11], v[16:31]
\tv_mfma_f32_32x32x16_f16 v[16:31], v[4:7], v[0:3], v[16:31]
\tv_mov_b32_e32 v0, v50
\tv_mfma_f32_32x32x16_f16 v[16:31], v[4:7], v[0:3], v[16:31]
\tglobal_load_dwordx4 v[4:7], v[60:61], off
\tv_mfma_f32_32x32x16_f16 v[16:31], v[4:7], v[0:3], v[16:31]
\ts_barrier
\tds_read_b128 v[0:3], v40
\tv_mfma_f32_32x32x16_f16 v[16:31], v[4:7], v[0:3], v[16:31]
.LBB0_2:
\tv_mfma_f32_32x32x16_f16 v[16:31], v[8:11], v[0:3], v[16:31]
\ts_endpgm
_Z5emptyv:
\ts_endpgm
\t.amdgpu_metadata
    .name:           _Z4demov
    .private_segment_fixed_size: 12
    .vgpr_count:     62
"""


def test_parser_on_a_hand_written_listing():
    ks = FD.parse_asm(ASM)
    assert list(ks) == ["_Z4demov"]                       # a function without products is left out
    k = ks["_Z4demov"]
    # product 0: both operands read before any product -> 0.  product 1: read before product 0 -> 1.  product 2: its operands
    # were read between products 0 and 1 (ds_read2 counts) -> 1.  product 3: v0 rewritten by a v_mov -> only v[4:7] counts: read
    # before product 1, products 1 and 2 in between -> 2.  product 4: v[4:7] now from memory, v[1:3] still from the LDS -> 3
    assert [d for _, _, d in k.products[:5]] == [0, 1, 1, 2, 3]
    # the barrier starts a burst, the block label another; the last product's operands: v[1:3]... read right before product 5 -> 1
    assert [(b, i) for b, i, _ in k.products] == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (2, 0)]
    assert [d for _, _, d in k.products[5:]] == [0, 1]
    assert k.bursts() == [5, 1, 1]
    assert (k.vgprs, k.scratch) == (62, 12)
    assert k.min_distance() == 0 and k.min_distance(lead=1) == 1
    assert k.histogram(lead=1) == {1: 2, 2: 1, 3: 1}
    assert FD.parse_remarks("remark: Function Name: _Z4demov\nremark:     VGPRs: 62\nremark:     AGPRs: 0\n"
                            "remark:     ScratchSize [bytes/lane]: 12\n") == {"_Z4demov": (62, 0, 12)}


def _hipcc():
    from softspoken_amd import build as B
    h = B._hipcc()
    return h if os.path.exists(h) or shutil.which(h) else None


needs_hipcc = pytest.mark.skipif(_hipcc() is None, reason="no hipcc")


@pytest.fixture(scope="module")
def listings():
    out = {}
    for unit in ("conv4_ups.hip", "conv4.hip"):
        ks = FD.compile_unit(unit)
        names = FD.demangle(list(ks))
        for sym, k in ks.items():
            out[re.sub(r"^(void )?ss::", "", names[sym]).split("(")[0]] = k
    return out


# the forms the network's f16x2 launches take (tools/layers.py prints them per launch)
T = "conv3x3_v4_kernel<1, %s>"
NETWORK_FORMS = [T % a for a in (
    "4, true, false, false, false, 0, false, false, false, true, false, 4, false",     # conv2_1.A
    "4, true, false, false, true, 1, false, false, false, true, false, 4, true",       # conv2_1.B
    "4, false, true, false, false, 0, false, false, false, true, false, 4, false",     # conv3_1.A, conv4_1.A, conv_bottleneck.A, encoder_out.A
    "4, false, false, true, true, 0, false, false, false, true, false, 4, false",      # conv3_1.B, conv4_1.B
    "4, false, false, true, false, 0, false, false, false, true, false, 4, false",     # conv_bottleneck.B, encoder_out.B, conv6.B
    "4, true, false, true, false, 0, false, false, false, true, false, 4, true",       # conv7.B
    "4, true, false, true, false, 0, false, false, false, true, false, 4, false",      # conv8.B
    "8, true, false, false, false, 4, false, true, false, true, false, 1, false")]     # conv9_1.B


def _product_f16x2_forms():
    """One-tile-wide (NT = 1) f16x2 forms of the product library in the recorded launches: the network's and those of other shapes.
    (The NT = 3 forms hold two slots under their register cap and restart the rotation for the second bank; no launch of the
    network takes them.)"""
    j = json.load(open(os.path.join(ROOT, "tests", "golden", "v4_forms.json")))
    used = sorted({j["rows"][i][0] for i in j["product"] if i >= 0})
    args = lambda n: n.rstrip(">").split("<")[1].split(", ")
    return [j["names"][n] for n in used if args(j["names"][n])[10] == "true" and args(j["names"][n])[0] == "1"]      # SPLIT, NT = 1


@needs_hipcc
def test_f16x2_kernels_keep_their_reads_ahead_and_do_not_spill(listings):
    forms = _product_f16x2_forms()
    assert set(NETWORK_FORMS) <= set(forms), set(NETWORK_FORMS) - set(forms)
    bad = []
    for name in forms + ["conv3x3_ups_kernel"]:
        k = listings[name]
        print(name, "vgpr", k.vgprs, "scratch", k.scratch, "min distance past the lead", k.min_distance(LEAD), dict(k.histogram(LEAD)))
        if k.scratch != 0 or k.min_distance(LEAD) is None or k.min_distance(LEAD) < FLOOR or k.histogram(LEAD).get(0):
            bad.append((name, k.scratch, k.min_distance(LEAD)))
    assert not bad, bad


@needs_hipcc
def test_ring_sub_pixel_kernel_does_not_spill(listings):
    k = listings["conv3x3_upsr_kernel"]
    print("conv3x3_upsr_kernel vgpr", k.vgprs, "scratch", k.scratch, dict(k.histogram()))
    assert k.scratch == 0 and len(k.products) == 90
