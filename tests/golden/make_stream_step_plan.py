"""Record tests/golden/stream_step_plan.json: what every step of tests/test_gpu_stream_bands.py's chunk-4 case launches
([kernel, launches, bytes] per step, from ss_get_kernel_stats on a profiling context).  Needs the GPU.

    python tests/golden/make_stream_step_plan.py [output path]

The table is the record of the step's launches: regenerate it only for a change that is meant to alter them."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import separation_ref as R                    # noqa: E402
import test_gpu_separation as T               # noqa: E402
import test_gpu_stream_bands as B             # noqa: E402
from softspoken_amd import native, synth      # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else B.STEP_PLAN_GOLDEN
    ctx = T._head_ctx(native, R.spread_head(synth.make_state_dict(0)), "fp32", chunk=4, profile=True)
    _, table = B.step_plan_run(native, ctx, B.step_plan_threshold(native, ctx))
    ctx.close()
    with open(out, "w") as f:
        json.dump(dict(case="test_step_structure_chunk_4", columns=["kernel", "launches", "bytes"], steps=table), f, indent=0)
        f.write("\n")
    print("wrote", out, len(table), "steps")


if __name__ == "__main__":
    main()
