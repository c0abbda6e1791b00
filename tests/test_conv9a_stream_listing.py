"""conv9a.hip in the BINARY (tools/frag_distance.py on the product build's listing, as tests/test_conv9_stream_listing.py does for
conv9s.hip):
  * no scratch, at most 256 registers (two waves per SIMD);
  * a row step is 108 + 48 = 156 products with no block label inside it -- a request behind a branch would make the compiler wait for
    every outstanding load.  The six copies of the row step (row parity x the two role cycles) may follow one
    another without a label, so a burst is a whole number of row steps;
  * past the first LEAD products of a burst no product has its fragments' LDS read closer than 12 products in front of it: a tap's set
    of the skip half is read a tap ahead, a six-product set of the upsampled half two sets ahead, the next row step's first set in front
    of the last twelve products (csrc/stream16.h S16Ring3), and the fences hold that order against the scheduler."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import frag_distance as FD  # noqa: E402

STEP = 108 + 48   # products of a row step
COPIES = 6        # row steps in the unrolled loop
LEAD = 12         # products: one tap group
FLOOR = 12


def _hipcc():
    from softspoken_amd import build as B
    h = B._hipcc()
    return h if os.path.exists(h) or shutil.which(h) else None


needs_hipcc = pytest.mark.skipif(_hipcc() is None, reason="no hipcc")


@needs_hipcc
def test_conv9a_stream_kernel_listing():
    ks = FD.compile_unit("conv9a.hip")
    names = FD.demangle(list(ks))
    by_name = {re.sub(r"^(void )?ss::", "", names[sym]).split("(")[0]: k for sym, k in ks.items()}
    assert list(by_name) == ["conv3x3_ups_stream16_kernel"], list(by_name)
    k = by_name["conv3x3_ups_stream16_kernel"]
    print("conv3x3_ups_stream16_kernel vgpr", k.vgprs, "agpr", k.agprs, "scratch", k.scratch, "bursts", k.bursts(), dict(k.histogram(LEAD)))
    assert k.scratch == 0 and k.vgprs + (k.agprs or 0) <= 256
    assert all(b % STEP == 0 for b in k.bursts()) and sum(k.bursts()) == COPIES * STEP, k.bursts()
    assert k.min_distance(LEAD) >= FLOOR and not k.histogram(LEAD).get(0) and not k.histogram(LEAD).get("other")
