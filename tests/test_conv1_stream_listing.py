"""conv1s.hip's product form in the BINARY (tools/frag_distance.py on the product build's listing, as tests/test_conv9a_stream_listing.py
does for conv9a.hip), for both instantiations of conv1_stream16_kernel:
  * no scratch, at most 256 registers (two waves per SIMD);
  * the row loop holds three copies of the row step (the h1 rows change roles), the tail two more; a row step is 12 + 4 + 108
    products: the three first-conv tiles (two pixel tiles and the halo tile), the rank-1 / bias products that start the accumulators,
    the nine taps.  The taps' 108 products lie in ONE burst, no block label inside: a request behind a branch would make the compiler
    wait for every outstanding read.  The only labels of a row step are the wave-uniform "row outside the
    picture" test around the first conv and the row-pair test of the pooling;
  * past the first LEAD products of a burst no product has its fragments' LDS read closer than 12 products in front of it: a tap's
    set is read a tap ahead, tap 0's in front of the 16 products before the taps (csrc/stream16.h S16Ring3), and the fences hold
    that order against the scheduler."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import frag_distance as FD  # noqa: E402

FIRST, RANK1, TAPS = 12, 4, 108
COPIES = 5        # row steps in the listing: three in the loop, two behind it
LEAD = 12         # products: one tap group
FLOOR = 12
NAMES = ("conv1_stream16_kernel<true>", "conv1_stream16_kernel<false>")


def _hipcc():
    from softspoken_amd import build as B
    h = B._hipcc()
    return h if os.path.exists(h) or shutil.which(h) else None


needs_hipcc = pytest.mark.skipif(_hipcc() is None, reason="no hipcc")


@pytest.fixture(scope="module")
def listing():
    ks = FD.compile_unit("conv1s.hip")
    names = FD.demangle(list(ks))
    return {re.sub(r"^(void )?ss::", "", names[sym]).split("(")[0]: k for sym, k in ks.items()}


@needs_hipcc
def test_both_instantiations_are_in_the_product_build(listing):
    assert sorted(listing) == sorted(NAMES), sorted(listing)


@needs_hipcc
@pytest.mark.parametrize("name", NAMES)
def test_conv1_stream_kernel_listing(listing, name):
    k = listing[name]
    print(name, "vgpr", k.vgprs, "agpr", k.agprs, "scratch", k.scratch, "bursts", k.bursts(), dict(k.histogram(LEAD)))
    assert k.scratch == 0 and k.vgprs + (k.agprs or 0) <= 256
    # the unit's prologue makes two h1 rows; every row step one more
    assert len(k.products) == 2 * FIRST + COPIES * (FIRST + RANK1 + TAPS), len(k.products)
    # the taps in one burst: the bursts that hold more than the first conv's products are the row steps', each with its 108 taps whole
    # (the rank-1 products in front of them may share the burst, nothing else does)
    big = [b for b in k.bursts() if b > FIRST + RANK1]
    assert len(big) == COPIES and all(b in (TAPS, RANK1 + TAPS) for b in big), k.bursts()
    assert k.min_distance(LEAD) >= FLOOR and not k.histogram(LEAD).get(0) and not k.histogram(LEAD).get("other")
