"""The ring kernels' two work orders (csrc/kernels.h; development build: SOFTSPOKEN_ORDER=1 side by side, 0 sequential) compute the same
bits: the order decides which tile of which workgroup takes a (position, channel group) and when, nothing about what is computed for it.
Checked on the C1 file (105 windows in one pass: the XCDs' position ranges end ragged) and on a 5-window pass (fewer quads than
workgroups), on the logits and on both stored planes of every activation tensor of the pass; and with waves put to sleep at the
stages' synchronisation points (ConvArgs::dbg bit 10, as tests/test_gpu_parity.py's timing test does) against the product library."""
import functools
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tensors behind the launches that go through the ring kernels (A launches write h*, B launches c* / p* and the 8 x 16 level's outputs)
RING_TENSORS = ("h3", "c3", "p3", "h4", "c4", "p4", "hb", "bott", "he", "enc", "h6", "c6", "h7", "c7")
CANDIDATES = ("h1", "c1", "p1", "h2", "c2", "p2", "h3", "c3", "p3", "h4", "c4", "p4", "hb", "bott", "he", "enc",
              "h6", "c6", "h7", "c7", "h8", "c8", "h9", "c9")

_CHILD = r"""
import sys, hashlib, numpy as np
sys.path.insert(0, {root!r})
from softspoken_amd import synth, native, checkpoint
from oracle import oracle_np as O
def h(a): return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]
dev = {dev!r}
pcm = synth.to_pcm16(synth.synth_audio(1001, 60.0, 16000, 1))
sig, _, _ = O.load_audio_from_bytes(synth.wav_bytes(pcm, 16000))
ctx = native.Context(checkpoint.pack_state_dict(synth.make_state_dict(0)), 0, precision="f16x2")
fid = ctx.add_f32_22k(sig)
L = native.lib()
def dump(case, n):
    if not dev: return
    buf = np.zeros(1, np.uint8)
    for name in {cands!r}:
        if L.ss_debug_activation(ctx._h, name.encode(), 0, 0, 0, native._ptr(buf), 0, None, None) != 0: continue
        d = ctx.debug_activation(name, 0, n)
        assert len(d["planes"]) == 2
        print("TENSOR", case, name, h(d["planes"][0]), h(d["planes"][1]), flush=True)
assert ctx.run()                                           # 105 windows, one pass
lg = ctx.window_logits(fid)
assert lg.shape[0] == 105
print("LOGITS c1", h(lg), flush=True)
dump("c1", 105)
starts = O.plan_windows(60.0)[[0, 17, 41, 77, 104]]
_, m = ctx.infer_windows(fid, starts)                      # a 5-window pass
print("LOGITS five", h(m), flush=True)
dump("five", 5)
ctx.close()
"""


def _run(env, dev=True):
    return _run_cached(tuple(sorted(env.items())), dev)


@functools.lru_cache(maxsize=None)
def _run_cached(env, dev):
    from softspoken_amd import build as hip_build
    e = dict(os.environ); e.update(dict(env))
    if dev:
        e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
    else:
        e.pop("SOFTSPOKEN_LIB", None)
    code = _CHILD.format(root=ROOT, dev=dev, cands=CANDIDATES)
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for l in r.stdout.splitlines():
        p = l.split()
        if p and p[0] == "LOGITS":
            out[("logits", p[1])] = p[2]
        elif p and p[0] == "TENSOR":
            out[(p[2], p[1], "hi")] = p[3]
            out[(p[2], p[1], "lo")] = p[4]
    return out


def test_both_orders_give_the_same_bits(build_all):
    new = _run({"SOFTSPOKEN_ORDER": "1"})
    old = _run({"SOFTSPOKEN_ORDER": "0"})
    for case in ("c1", "five"):
        assert ("logits", case) in new
        for name in RING_TENSORS:
            assert (name, case, "hi") in new and (name, case, "lo") in new, (name, case)
    assert set(new) == set(old)
    diff = sorted(k for k in new if new[k] != old[k])
    assert not diff, diff


@pytest.mark.parametrize("dbg", [1024, 1024 + 2048, 1024 + 4096, 1024 + 6144])
def test_side_by_side_order_under_wave_jitter_equals_the_product(build_all, dbg):
    """Chosen waves sleep about a microsecond at every synchronisation point of a stage (a rotating wave, wave 0 only, all but wave 0, the
    odd waves): sibling workgroups drift apart and the bank rings' cursors are exercised off the beat.  Same logits as the product library."""
    plain = _run({}, dev=False)
    jit = _run({"SOFTSPOKEN_ORDER": "1", "SOFTSPOKEN_DBG": str(dbg)})
    for case in ("c1", "five"):
        assert jit[("logits", case)] == plain[("logits", case)], case
