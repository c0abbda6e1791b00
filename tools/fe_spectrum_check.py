"""Dev build only: the front-end kernel's power spectrum |X[k]|^2 (k < 768) against the float64 reference and per-bin bound of
tests/frontend_ref.py, 128 bins per run (SOFTSPOKEN_FEDBG = 512 + 1024 sel).  tests/test_gpu_frontend.py asserts the same on its whole
input set; this prints the worst |delta| / bound per quarter pass for one noise signal."""
import os, sys, subprocess, json
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) > 1:
    sel = int(sys.argv[1])
    import frontend_ref as R
    from softspoken_amd import synth, native, checkpoint
    sd = synth.make_state_dict(0)
    rng = np.random.default_rng(3)
    sig = (rng.standard_normal(66150 + 13230) * 0.1).astype(np.float32)
    starts = np.array([0, 13230])
    c = native.Context(checkpoint.pack_state_dict(sd), 0, precision="bf16")
    fid = c.add_f32_22k(sig, padded=True)
    got = c.features(fid, starts).transpose(0, 2, 1).astype(np.float64)      # [2][256 frames][128 bins of the selection]
    ref = R.Reference(R.windows_of(sig, starts), sd["mel_spectrogram.spectrogram.window"], sd["mel_spectrogram.mel_scale.fb"], keep_spectrum=True)
    p64, bound = ref.power_bound()
    ks = slice(128 * sel, 128 * sel + 128)
    ratio = np.abs(got - p64[..., ks]) / bound[..., ks]
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(json.dumps(dict(sel=sel, worst=float(ratio.max()), by_r=[float(ratio[..., r::4].max()) for r in range(4)],
                          at=dict(window=int(at[0]), frame=int(at[1]), bin=int(at[2]) + 128 * sel), over=int((ratio > 1).sum()))))
else:
    from softspoken_amd import build
    for sel in range(6):
        e = dict(os.environ, SOFTSPOKEN_LIB=build.DEV_LIB, SOFTSPOKEN_FEDBG=str(512 + 1024 * sel))
        r = subprocess.run([sys.executable, __file__, str(sel)], env=e, capture_output=True, text=True, timeout=300)
        print([l for l in r.stdout.splitlines() if l.startswith("{")] or r.stderr[-500:])
        if r.returncode != 0:
            break
