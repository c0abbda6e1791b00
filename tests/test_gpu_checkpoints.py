"""The network end to end on the checkpoint zoo (tests/checkpoint_zoo.py) against the float64 oracle: eight windows of the C1 recording
(every 13th), logits and every value of the spec maps.  Reference: oracle_np.unet_forward in float64 on the oracle's mel features, as in
test_gpu_layers.py's test_spec_head_end_to_end; tests/test_checkpoint_zoo.py holds the reference's own fp32 arithmetic to a quarter of the
bars used here, on these windows.

Bars: the project's 1e-4 (fp32 and f16x2), times max |ref| where that exceeds 1 (signs; runaway, whose logits are ~1e33); bf16 its
stated 0.15.  Every member except runaway must RUN in f16x2: a refusal (SS_ERR_RANGE) there is a failure of the channel normalisation's
claim.  runaway (BatchNorm scales of 316 compounding through the blocks, channel exponents at the -60 clamp) may be refused in f16x2, or
answered within the bar; anything else -- non-finite values, finite values outside the bar -- is what that member exists to catch."""
import numpy as np
import pytest

import checkpoint_zoo as Z

pytestmark = pytest.mark.gpu

TOL_FP32 = 1e-4          # the fp32 parity bar (BASELINE.json north_star)
TOL_BF16 = 0.15          # bf16: the throughput mode's stated score tolerance (test_bf16_mode)


@pytest.fixture(scope="module")
def native(build_all):
    from softspoken_amd import native as n
    return n


@pytest.fixture(scope="module")
def ref64(c1):
    """name -> float64 oracle (logits, spec) on the eight windows, computed once per member."""
    feats = Z.c1_features(c1, Z.E2E_WINDOWS)
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Z.oracle(Z.build(name), feats)
        return cache[name]
    return get


def _device(native, c1, name, mode, chunk=8):
    """-> (logits, spec) of the eight windows from a fresh context on member `name`."""
    from softspoken_amd import checkpoint
    ctx = native.Context(checkpoint.pack_state_dict(Z.build(name)), 0, precision=mode, chunk=chunk)
    try:
        fid = ctx.add_f32_22k(c1["sig"])
        spec, mask = ctx.infer_windows(fid, c1["starts"][Z.E2E_WINDOWS], want_spec=True)
    finally:
        ctx.close()
    return mask, spec


@pytest.fixture(scope="module")
def seed0_f16x2(native, c1):
    return _device(native, c1, "seed0", "f16x2")[0]


def _deltas(got, ref):
    """max |got - ref| of logits and spec, each relative to max(1, max |ref|)."""
    return tuple(float(np.abs(g.astype(np.float64) - r).max() / max(1.0, np.abs(r).max())) for g, r in zip(got, ref))


CASES = [(n, m) for n in ("seed7", "spread3", "spread6", "signs", "dead", "tinyvar") for m in ("f16x2", "fp32")] + [("spread3", "bf16")]


@pytest.mark.parametrize("name,mode", CASES, ids=[f"{n}-{m}" for n, m in CASES])
def test_member_end_to_end(name, mode, native, c1, ref64, seed0_f16x2):
    got = _device(native, c1, name, mode)                    # (creating the f16x2 context must succeed: a NativeError fails the test)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    dm, ds = _deltas(got, ref64(name))
    print(f"zoo {name} {mode}: max |logits - float64 oracle| = {dm:.3g}, spec {ds:.3g} (x max(1, max |ref|) = "
          f"{max(1.0, np.abs(ref64(name)[0]).max()):.3g}, {max(1.0, np.abs(ref64(name)[1]).max()):.3g})")
    tol = TOL_BF16 if mode == "bf16" else TOL_FP32
    assert dm <= tol and ds <= tol, (dm, ds)
    if mode == "f16x2" and name in ("spread3", "spread6", "tinyvar"):
        # the same function as the seed-0 checkpoint: the device's own f16x2 answers must agree too
        d0 = float(np.abs(got[0].astype(np.float64) - seed0_f16x2).max())
        print(f"zoo {name} f16x2: max |logits - the device's f16x2 logits on seed 0| = {d0:.3g}")
        assert d0 <= TOL_FP32, d0


def test_runaway(native, c1, ref64):
    from softspoken_amd import checkpoint
    ref = ref64("runaway")
    assert np.abs(ref[0]).max() > 1e30                       # (the member is what it says)
    dm, ds = _deltas(_device(native, c1, "runaway", "fp32"), ref)
    print(f"zoo runaway fp32: max |logits - float64 oracle| / max |ref| = {dm:.3g}, spec {ds:.3g}")
    assert dm <= TOL_FP32 and ds <= TOL_FP32, (dm, ds)
    blob = checkpoint.pack_state_dict(Z.build("runaway"))
    try:
        ctx = native.Context(blob, 0, precision="f16x2", chunk=8)
    except native.NativeError as e:
        assert e.code == native.SS_ERR_RANGE == 8, e
        print("zoo runaway f16x2: refused at creation:", e)
        return
    try:
        fid = ctx.add_f32_22k(c1["sig"])
        starts = c1["starts"][Z.E2E_WINDOWS]
        try:
            spec, mask = ctx.infer_windows(fid, starts, want_spec=True)
        except native.NativeError as e:
            assert e.code == native.SS_ERR_RANGE == 8, e
            print("zoo runaway f16x2: refused at the first infer_windows:", e)
            assert ctx.features(fid, starts[:2]).shape == (2, 128, 256)          # the context stays usable
            with pytest.raises(native.NativeError) as e2:                        # ... and answers the same way again
                ctx.infer_windows(fid, starts[:1])
            assert e2.value.code == 8
            return
        assert np.isfinite(mask).all() and np.isfinite(spec).all(), "f16x2 returned non-finite values instead of refusing"
        dm, ds = _deltas((mask, spec), ref)
        print(f"zoo runaway f16x2: answered; max |logits - float64 oracle| / max |ref| = {dm:.3g}, spec {ds:.3g}")
        assert dm <= TOL_FP32 and ds <= TOL_FP32, (dm, ds)
    finally:
        ctx.close()


def test_chunking_invariance_on_a_heterogeneous_member(native, c1):
    """spread6 (channel exponents over 2^40 inside one tensor), f16x2: chunks of 1, 3 and 8 over the eight windows, bit-identical logits."""
    out = [_device(native, c1, "spread6", "f16x2", chunk=k)[0] for k in (1, 3, 8)]
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
