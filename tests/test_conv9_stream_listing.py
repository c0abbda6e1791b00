"""conv9s.hip in the BINARY (tools/frag_distance.py on the product build's listing, as tests/test_frag_distance.py does for conv4.hip):
  * no scratch, at most 256 registers (two waves per SIMD);
  * a row step is one burst of 24 + 108 + 6 products with no block label inside it -- a request behind a branch would make the
    compiler wait for every outstanding load (csrc/conv9s.hip, "Every request of the loop is unconditional");
  * past the first LEAD products of a row step (the c1 half of the projection, whose fragments the step has only just asked for) no
    product has its fragments' LDS read closer than one tap group (12 products) in front of it: the tap loop of csrc/stream16.h
    reads a tap ahead, and the fences hold that order against the scheduler.
The same floor holds for the other kernel on that core, conv1s.hip's 16-pixel form."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import frag_distance as FD  # noqa: E402

LEAD = 12         # products: one tap group
FLOOR = 12


def _hipcc():
    from softspoken_amd import build as B
    h = B._hipcc()
    return h if os.path.exists(h) or shutil.which(h) else None


needs_hipcc = pytest.mark.skipif(_hipcc() is None, reason="no hipcc")


def _listing(unit):
    ks = FD.compile_unit(unit)
    names = FD.demangle(list(ks))
    return {re.sub(r"^(void )?ss::", "", names[sym]).split("(")[0]: k for sym, k in ks.items()}


@needs_hipcc
def test_conv9_stream_kernel_listing():
    k = _listing("conv9s.hip")["conv9_stream16_kernel"]
    print("conv9_stream16_kernel vgpr", k.vgprs, "agpr", k.agprs, "scratch", k.scratch, "bursts", k.bursts(), dict(k.histogram(LEAD)))
    assert k.scratch == 0 and k.vgprs + (k.agprs or 0) <= 256
    assert set(k.bursts()) == {24 + 108 + 6}, k.bursts()
    assert k.min_distance(LEAD) >= FLOOR and not k.histogram(LEAD).get(0)


@needs_hipcc
def test_conv1_stream_kernel_keeps_the_floor_on_the_shared_core():
    ks = _listing("conv1s.hip")
    for name in ("conv1_stream16_kernel<true>", "conv1_stream16_kernel<false>"):
        k = ks[name]
        print(name, "vgpr", k.vgprs, "scratch", k.scratch, dict(k.histogram(LEAD)))
        assert k.scratch == 0 and k.vgprs + (k.agprs or 0) <= 256
        assert k.min_distance(LEAD) >= FLOOR
