"""The f16x2 conv kernels keep their operand reads ahead of their matrix products with scheduling fences (csrc/mfma_util.h
frag_fence): product order, operands, accumulators, barriers and LDS layout are untouched, so the arithmetic must not notice -- nor
may it notice the register allocation, which differs between the product and the development build of the same sources.

C1 recording (60 s, seed 1001), f16x2, passes of 105, 5 and 1 windows (5 and 1 have fewer quads than workgroups: tiles keep the beat
without work): the product library's logits equal the development library's bit for bit, and are within 1e-4 of
tests/golden/c1_logits.npz (the reference's own logits; the f16x2 mode's stated bound, tests/test_gpu_parity.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "c1_logits.npz")
PICK = {"c1": list(range(105)), "five": [0, 17, 41, 77, 104], "one": [41]}
TOL = 1e-4

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r})
from softspoken_amd import synth, native, checkpoint
from oracle import oracle_np as O
pcm = synth.to_pcm16(synth.synth_audio(1001, 60.0, 16000, 1))
sig, _, _ = O.load_audio_from_bytes(synth.wav_bytes(pcm, 16000))
ctx = native.Context(checkpoint.pack_state_dict(synth.make_state_dict(0)), 0, precision="f16x2")
fid = ctx.add_f32_22k(sig)
plan = O.plan_windows(60.0)
out = {{}}
for case, idx in {pick!r}.items():
    _, m = ctx.infer_windows(fid, plan[idx])
    assert m.shape[0] == len(idx), (case, m.shape)
    out[case] = np.ascontiguousarray(m, dtype=np.float32)
ctx.close()
np.savez({dst!r}, **out)
"""


@functools.lru_cache(maxsize=None)
def _logits(dev, tmp):
    from softspoken_amd import build as hip_build
    e = dict(os.environ)
    if dev:
        e["SOFTSPOKEN_LIB"] = hip_build.DEV_LIB
    else:
        e.pop("SOFTSPOKEN_LIB", None)
    dst = os.path.join(tmp, "dev.npz" if dev else "product.npz")
    code = _CHILD.format(root=ROOT, pick=PICK, dst=dst)
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(np.load(dst))


@pytest.fixture(scope="module")
def runs(build_all, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("frag_prefetch"))
    return _logits(False, tmp), _logits(True, tmp)


@pytest.mark.parametrize("case", list(PICK))
def test_product_and_dev_builds_give_the_same_bits(runs, case):
    prod, dev = runs
    assert prod[case].shape == dev[case].shape
    assert prod[case].tobytes() == dev[case].tobytes(), float(np.abs(prod[case] - dev[case]).max())


@pytest.mark.parametrize("case", list(PICK))
def test_logits_within_the_stated_bound_of_the_reference(runs, case):
    gold = np.load(GOLD)["logits"]
    want = gold[PICK[case]].reshape(len(PICK[case]), -1)
    for lib in runs:
        got = lib[case].reshape(len(PICK[case]), -1)
        err = float(np.abs(got - want).max())
        print(case, "max |logit - reference| =", err)
        assert got.shape == want.shape and err < TOL, (case, err)
