"""The two byte orders of the f16x2 activation tensors (csrc/kernels.h ActStride; development build: SOFTSPOKEN_LAYOUT=1 chunk-planar for
the tensors wider than 32 channels, 0 every tensor [window][H][W][C]) compute the same bits: the order decides where a value lies, nothing
about what is computed.  Checked on five windows of the C1 signal with the spec head on, in a pass of 5 windows and in passes of 2
(the last one holds 1 window: a grid smaller than the chip), on the logits, the spec map and both planes of every stored tensor
(ss_debug_activation returns [n][H][W][C] whatever the stored order).  These passes hold border tiles (the zero header), tensors of 2, 3
and 4 chunks, pooled outputs, upsampled sources, the sub-pixel ring kernel and the group-resident and ring forms.  The product library
gives the development library's logits, and bf16 (one order only) does not see the switch."""
import functools
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDE = ("h2", "c2", "p2", "h3", "c3", "p3", "h4", "c4", "p4", "hb", "bott", "he", "enc", "h6", "c6", "h7", "c7")
CANDIDATES = ("h1", "c1", "p1") + WIDE + ("h8", "c8", "h9", "c9", "hs", "s9")

_CHILD = r"""
import sys, hashlib, numpy as np
sys.path.insert(0, {root!r})
from softspoken_amd import synth, native, checkpoint
from oracle import oracle_np as O
def h(a): return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]
dev, mode = {dev!r}, {mode!r}
pcm = synth.to_pcm16(synth.synth_audio(1001, 60.0, 16000, 1))
sig, _, _ = O.load_audio_from_bytes(synth.wav_bytes(pcm, 16000))
starts = O.plan_windows(60.0)[[0, 17, 41, 77, 104]]
blob = checkpoint.pack_state_dict(synth.make_state_dict(0))
L = native.lib()
for case, chunk, last in (("five", 5, 5), ("two", 2, 1)):        # last: windows of the last pass, the one ss_debug_activation sees
    ctx = native.Context(blob, 0, precision=mode, chunk=chunk)
    fid = ctx.add_f32_22k(sig)
    spec, m = ctx.infer_windows(fid, starts, want_spec=True)
    print("LOGITS", case, h(m), flush=True)
    print("SPEC", case, h(spec), flush=True)
    if dev and mode == "f16x2":
        buf = np.zeros(1, np.uint8)
        for name in {cands!r}:
            if L.ss_debug_activation(ctx._h, name.encode(), 0, 0, 0, native._ptr(buf), 0, None, None) != 0: continue
            d = ctx.debug_activation(name, 0, last)
            assert len(d["planes"]) == 2
            print("TENSOR", case, name, h(d["planes"][0]), h(d["planes"][1]), flush=True)
    ctx.close()
print("CHILD_OK", flush=True)
"""


@functools.lru_cache(maxsize=None)
def _run(layout, dev=True, mode="f16x2"):
    from softspoken_amd import build as hip_build
    e = dict(os.environ)
    e.pop("SOFTSPOKEN_LAYOUT", None)
    if layout is not None:
        e["SOFTSPOKEN_LAYOUT"] = str(layout)
    if dev:
        e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
    else:
        e.pop("SOFTSPOKEN_LIB", None)
    code = _CHILD.format(root=ROOT, dev=dev, mode=mode, cands=CANDIDATES)
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for l in r.stdout.splitlines():
        p = l.split()
        if p and p[0] in ("LOGITS", "SPEC"):
            out[(p[0].lower(), p[1])] = p[2]
        elif p and p[0] == "TENSOR":
            out[(p[2], p[1], "hi")] = p[3]
            out[(p[2], p[1], "lo")] = p[4]
    return out


def test_both_orders_give_the_same_bits(build_all):
    planar = _run(1)
    nhwc = _run(0)
    for case in ("five", "two"):
        assert ("logits", case) in planar and ("spec", case) in planar
        for name in WIDE + ("hs", "s9"):
            assert (name, case, "hi") in planar and (name, case, "lo") in planar, (name, case)
    assert set(planar) == set(nhwc)
    diff = sorted(k for k in planar if planar[k] != nhwc[k])
    assert not diff, diff


def test_product_library_equals_the_development_library(build_all):
    prod = _run(None, dev=False)
    devl = _run(1)
    nhwc = _run(0)
    for case in ("five", "two"):
        for what in ("logits", "spec"):
            assert prod[(what, case)] == devl[(what, case)] == nhwc[(what, case)], (what, case)


def test_bf16_does_not_see_the_switch(build_all):
    a = _run(1, mode="bf16")
    b = _run(0, mode="bf16")
    assert a == b and ("logits", "five") in a and ("logits", "two") in a
