"""How far ahead of its matrix product is an operand fragment read from the LDS -- in the BINARY, not in the source?

usage: python tools/frag_distance.py conv4_ups.hip [substring of a kernel's name ...]      (a csrc/ unit: compiled here, product flags)
       python tools/frag_distance.py listing.s [substring ...]                             (assembly from hipcc -S --cuda-device-only)

For every v_mfma* of a kernel: the number of v_mfma* issued between the latest ds_read* into one of its A / B operand registers and
the product itself ("distance").  0 = the product waits for a whole LDS round trip; with two waves multiplying per SIMD about two
products' worth of matrix cycles hide one.  Only ds_read* and v_mfma* are counted; any other instruction that writes a register
forgets the register's read (a product with no operand straight from the LDS shows as "other").  The listing is walked
in text order (the multiply loops are fully unrolled).  A "burst" is the products between two s_barrier or block labels: one stage's multiply phase;
`lead` products at the head of a burst are its prologue (their reads cannot be far ahead: the patch was published by the barrier).

Per kernel: VGPRs, AGPRs and scratch (from -Rpass-analysis=kernel-resource-usage when the tool compiles; else from the listing's
.vgpr_count / .private_segment_fixed_size metadata), the histogram over all products and the one past the first `--lead N` of a burst.
The parsing (parse_asm) is importable: tests/test_frag_distance.py feeds it text."""
from __future__ import annotations

import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_REG = re.compile(r"v(?:\[(\d+):(\d+)\]|(\d+))")
_FUNC = re.compile(r"^([A-Za-z_][\w$.]*):\s*(?:;.*)?$")
_NO_DST = ("ds_write", "ds_store", "global_store", "buffer_store", "flat_store", "scratch_store", "global_atomic", "buffer_atomic",
           "ds_add", "ds_or", "ds_max", "ds_min", "v_cmp", "v_cmpx", "v_readfirstlane", "v_readlane", "v_accvgpr_write", "v_nop")


def _regs(operand: str):
    """VGPR numbers of one operand ('v[4:7]' -> 4..7, 'v9' -> 9; anything else -> nothing)."""
    m = _REG.fullmatch(operand.strip())
    if not m:
        return []
    if m.group(3) is not None:
        return [int(m.group(3))]
    return list(range(int(m.group(1)), int(m.group(2)) + 1))


def _operands(rest: str):
    out, depth, cur = [], 0, ""
    for ch in rest:
        if ch == "[":
            depth += 1
        elif ch == "]":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip()); cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


class Kernel:
    """One kernel's products: `products` is a list of (burst, index in burst, distance or None) in text order."""

    def __init__(self, name):
        self.name = name
        self.products = []
        self.vgprs = self.agprs = self.scratch = None

    def histogram(self, lead: int = 0):
        h = collections.Counter()
        for _, i, d in self.products:
            if i >= lead:
                h["other" if d is None else d] += 1
        return h

    def min_distance(self, lead: int = 0):
        """Smallest distance past the first `lead` products of every burst (None: no such product reads the LDS)."""
        ds = [d for _, i, d in self.products if i >= lead and d is not None]
        return min(ds) if ds else None

    def bursts(self):
        c = collections.Counter(b for b, _, _ in self.products)
        return [c[b] for b in sorted(c)]


def parse_asm(text: str):
    """{kernel symbol: Kernel} of an AMDGPU assembly listing (functions without products are left out)."""
    kernels, k = {}, None
    last_read, n_mfma, burst, in_burst = {}, 0, 0, 0
    meta_name = None
    for line in text.splitlines():
        m = _FUNC.match(line)
        if m and not line.startswith(".L"):
            k = kernels.setdefault(m.group(1), Kernel(m.group(1)))
            last_read, n_mfma, burst, in_burst = {}, 0, 0, 0
            continue
        t = line.strip()
        if line.startswith(".LBB") and in_burst:          # a basic block's head ends a burst as a barrier does
            burst += 1
            in_burst = 0
        # metadata at the end of the listing (.amdhsa_kernel blocks are not needed: the YAML carries the same)
        mm = re.match(r"\.name:\s+(\S+)", t)
        if mm:
            meta_name = mm.group(1)
        for key, attr in ((".vgpr_count:", "vgprs"), (".agpr_count:", "agprs"), (".private_segment_fixed_size:", "scratch")):
            if t.startswith(key) and meta_name in kernels:
                setattr(kernels[meta_name], attr, int(t.split()[1]))
        if k is None or not line[:1].isspace() or not t or t[0] in ".;":
            continue
        t = t.split(";")[0].strip()
        parts = t.split(None, 1)
        op, rest = parts[0], (parts[1] if len(parts) > 1 else "")
        if op == "s_endpgm":
            k = None
            continue
        if op.startswith("s_barrier"):
            if in_burst:
                burst += 1
                in_burst = 0
            continue
        ops = _operands(rest)
        if op.startswith("ds_read") or op.startswith("ds_load"):
            for r in _regs(ops[0]) if ops else []:
                last_read[r] = n_mfma
        elif op.startswith("v_mfma") or op.startswith("v_smfmac"):
            srcs = [r for o in ops[1:3] for r in _regs(o)]
            marks = [last_read[r] for r in srcs if r in last_read]      # (an operand from memory or from arithmetic has no mark)
            d = n_mfma - max(marks) if marks else None
            k.products.append((burst, in_burst, d))
            in_burst += 1
            n_mfma += 1
            for r in _regs(ops[0]) if ops else []:
                last_read.pop(r, None)
        elif ops and not op.startswith(_NO_DST) and not op.startswith("s_"):
            for r in _regs(ops[0]):
                last_read.pop(r, None)
    return {n: kk for n, kk in kernels.items() if kk.products}


def parse_remarks(stderr: str):
    """{kernel symbol: (VGPRs, AGPRs, scratch bytes per lane)} from -Rpass-analysis=kernel-resource-usage."""
    out, name, vg, ag = {}, None, None, None
    for l in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", l)
        if m: name, vg, ag = m.group(1), None, None
        m = re.search(r" VGPRs: (\d+)", l)
        if m: vg = int(m.group(1))
        m = re.search(r"AGPRs: (\d+)", l)
        if m: ag = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", l)
        if m and name: out[name] = (vg, ag, int(m.group(1)))
    return out


def compile_unit(unit: str, dev: bool = False):
    """Assembly and resource remarks of csrc/<unit> with the flags of softspoken_amd/build.py; returns {symbol: Kernel}."""
    from softspoken_amd import build as B
    src = unit if os.path.exists(unit) else os.path.join(B.CSRC, unit)
    base = os.path.basename(src)
    cmd = [B._hipcc()] + B.FLAGS + B.EXTRA_FLAGS.get(base, []) + (["-DSS_DEVBUILD"] if dev else []) + \
          ["-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", src, "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    ks = parse_asm(r.stdout)
    for name, (vg, ag, sc) in parse_remarks(r.stderr).items():
        if name in ks:
            ks[name].vgprs, ks[name].agprs, ks[name].scratch = vg, ag, sc
    return ks


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    d = r.stdout.splitlines() if r.returncode == 0 else list(names)
    return dict(zip(names, d))


def _fmt(h):
    keys = sorted(k for k in h if k != "other")
    return "  ".join(f"{k}: {h[k]}" for k in keys) + (f"  other: {h['other']}" if h.get("other") else "")


def main(argv):
    lead, dev, args = 0, False, []
    it = iter(argv)
    for x in it:
        if x == "--lead": lead = int(next(it))
        elif x == "--dev": dev = True
        else: args.append(x)
    if not args:
        print(__doc__); return 2
    ks = parse_asm(open(args[0]).read()) if args[0].endswith(".s") else compile_unit(args[0], dev)
    names = demangle(list(ks))
    for sym, k in ks.items():
        dn = re.sub(r"^void ss::", "", names[sym]).split("(")[0]
        if args[1:] and not any(p in dn for p in args[1:]):
            continue
        print(dn)
        print(f"   vgpr {k.vgprs} agpr {k.agprs} scratch {k.scratch}   products {len(k.products)} in bursts {k.bursts()}")
        print(f"   all products:      {_fmt(k.histogram())}")
        if lead:
            print(f"   past the first {lead}:  {_fmt(k.histogram(lead))}   min {k.min_distance(lead)}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
