"""conv7.B and conv2_1.B with one channel group per workgroup and that group's banks resident in LDS (csrc/conv4.hip GRES, csrc/kernels.h
gres_item; development build: SOFTSPOKEN_GRES=1 on, 0 the former forms) compute the same bits as the forms they replace: per output
pixel the sequence of matrix products into the accumulator is the same, and neither the tile shape nor the wave that owns a pixel
enters the arithmetic.  Checked on the C1 file (105 windows in one pass: the XCDs' position ranges end ragged), on a 5-window pass and
on a 1-window pass (conv7.B has 16 positions: most workgroups are without work), on the logits and on both stored planes of every
activation tensor of the pass; and with waves put to sleep at the stages' synchronisation points (ConvArgs::dbg bit 10, as
tests/test_gpu_parity.py's timing test does) against the product library."""
import functools
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tensors the two launches write
GRES_TENSORS = ("c2", "p2", "c7")
CANDIDATES = ("h1", "c1", "p1", "h2", "c2", "p2", "h3", "c3", "p3", "h4", "c4", "p4", "hb", "bott", "he", "enc",
              "h6", "c6", "h7", "c7", "h8", "c8", "h9", "c9")
CASES = ("c1", "five", "one")
TILES = (4,)                                               # tiles per workgroup of the forms that are built (four 4-wave tiles)

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
plan = O.plan_windows(60.0)
_, m = ctx.infer_windows(fid, plan[[0, 17, 41, 77, 104]])  # a 5-window pass
print("LOGITS five", h(m), flush=True)
dump("five", 5)
_, m = ctx.infer_windows(fid, plan[[41]])                  # a 1-window pass
print("LOGITS one", h(m), flush=True)
dump("one", 1)
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


@pytest.mark.parametrize("nh", TILES)
def test_resident_groups_give_the_same_bits(build_all, nh):
    new = _run({"SOFTSPOKEN_GRES": "1"})
    old = _run({"SOFTSPOKEN_GRES": "0"})
    for case in CASES:
        assert ("logits", case) in new
        for name in GRES_TENSORS:
            assert (name, case, "hi") in new and (name, case, "lo") in new, (name, case)
    assert set(new) == set(old)
    diff = sorted(k for k in new if new[k] != old[k])       # the two launches' tensors, and nothing else moves either
    assert not diff, diff


@pytest.mark.parametrize("dbg", [1024, 1024 + 2048, 1024 + 4096, 1024 + 6144])
@pytest.mark.parametrize("nh", TILES)
def test_resident_groups_under_wave_jitter_equal_the_product(build_all, nh, dbg):
    """Chosen waves sleep about a microsecond at every synchronisation point of a stage (a rotating wave, wave 0 only, all but wave 0, the
    odd waves): the tiles of a workgroup and the sibling workgroups drift apart.  Same logits as the product library."""
    plain = _run({}, dev=False)
    jit = _run({"SOFTSPOKEN_GRES": "1", "SOFTSPOKEN_DBG": str(dbg)})
    for case in CASES:
        assert jit[("logits", case)] == plain[("logits", case)], case
