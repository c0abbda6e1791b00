"""Per-launch fabric reads and L2 hit rate of the multi-group ring launches from rocprofv3 --pmc passes (each with --kernel-trace only) on
tools/run_chunks.py f16x2 <windows> 2: one pass with FETCH_SIZE, one with TCC_HIT_sum TCC_MISS_sum GRBM_GUI_ACTIVE.
Several launches of a pass share an instantiation; they are told apart by their dispatch order within the (second, warm) repetition.
FETCH_SIZE is in KiB and counts wide streaming reads at half on gfx950 (x 2, calibrated on conv2_1.A / conv9_1.A whose fetch equals their
input; not calibrated for 64-byte slices of wider pixels: compare orders of the same launch, and launches with their one-group sibling).
usage: python tools/fetch_order_summary.py <windows> <label=fetch_dir:hit_dir> ...      -> markdown on stdout"""
import collections, csv, glob, os, sys

# launches of a pass in dispatch order per instantiation: (layer, H, W, C0, C1 (upsampled, at H/2 x W/2), Cout, B launch)
RING_A = "conv3x3_v4_kernel<1, 4, false, true, false, false, 0, false, false, false, true, false, 4, false>"
RING_BP = "conv3x3_v4_kernel<1, 4, false, false, true, true, 0, false, false, false, true, false, 4, false>"
RING_B = "conv3x3_v4_kernel<1, 4, false, false, true, false, 0, false, false, false, true, false, 4, false>"
RES_B = "conv3x3_v4_kernel<1, 4, true, false, true, false, 0, false, false, false, true, false, 4, false>"
GRES_B = "conv3x3_v4_kernel<1, 4, true, false, true, false, 0, false, false, false, true, false, 4, true>"     # one group per workgroup, banks resident
LAUNCHES = {
    "conv3x3_upsr_kernel": [("conv6.A", 16, 32, 128, 128, 96, False), ("conv7.A", 32, 64, 96, 96, 64, False), ("conv8.A", 64, 128, 64, 64, 32, False)],
    RING_A: [("conv3_1.A", 32, 64, 64, 0, 96, False), ("conv4_1.A", 16, 32, 96, 0, 128, False), ("conv_bottleneck.A", 8, 16, 128, 0, 128, False),
             ("encoder_out.A", 8, 16, 128, 0, 128, False)],
    RING_BP: [("conv3_1.B", 32, 64, 96, 0, 96, True), ("conv4_1.B", 16, 32, 128, 0, 128, True)],
    RING_B: [("conv_bottleneck.B", 8, 16, 128, 0, 128, True), ("encoder_out.B", 8, 16, 128, 0, 128, True), ("conv6.B", 16, 32, 96, 0, 96, True)],
    GRES_B: [("conv7.B", 32, 64, 64, 0, 64, True)],
    RES_B: [("conv8.B", 64, 128, 32, 0, 32, True)],
}


def short(k):
    k = k.replace("void ", "").replace("ss::", "")
    depth = 0
    for i, ch in enumerate(k):
        if ch == "<": depth += 1
        elif ch == ">": depth -= 1
        elif ch == "(" and depth == 0: return k[:i]
    return k


def per_launch(d, counter):
    """{kernel: [value per launch of the second repetition, in dispatch order]}"""
    rows = collections.defaultdict(dict)
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == counter:
                k = short(r["Kernel_Name"])
                rows[k][int(r["Dispatch_Id"])] = rows[k].get(int(r["Dispatch_Id"]), 0.0) + float(r["Counter_Value"])
    return {k: [v[i] for i in sorted(v)][len(v) // 2:] for k, v in rows.items()}


def durations(d):
    rows = collections.defaultdict(dict)
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows[short(r["Kernel_Name"])][int(r["Dispatch_Id"])] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    return {k: [v[i] for i in sorted(v)][len(v) // 2:] for k, v in rows.items()}


def algorithmic(n, H, W, C0, C1, Cout, b):
    # what the launch has to read once: both f16 planes of its 3x3 input; a B launch also the block's r (fp32 fragments)
    return n * (H * W * C0 * 4 + (H // 2) * (W // 2) * C1 * 4 + (H * W * Cout * 4 if b else 0))


nwin = int(sys.argv[1])
runs = []
for spec in sys.argv[2:]:
    label, dirs = spec.split("=")
    fd, hd = dirs.split(":")
    runs.append((label, per_launch(fd, "FETCH_SIZE"), per_launch(hd, "TCC_HIT_sum"), per_launch(hd, "TCC_MISS_sum"), per_launch(hd, "GRBM_GUI_ACTIVE"), durations(hd)))
print("| launch | groups | algorithmic MB | " + " | ".join("%s: fetch MB (x alg.) · L2 hit · µs · GHz" % r[0] for r in runs) + " |")
print("|---|---|---|" + "---|" * len(runs))
for kern, ls in LAUNCHES.items():
    for i, (layer, H, W, C0, C1, Cout, b) in enumerate(ls):
        alg = algorithmic(nwin, H, W, C0, C1, Cout, b)
        cells = []
        for label, fe, hit, miss, act, dur in runs:
            try:
                f = fe[kern][i] * 1024 * 2
                h, m = hit[kern][i], miss[kern][i]
                us = dur[kern][i]
                cells.append("%.0f (%.2f) · %.3f · %.0f · %.2f" % (f / 1e6, f / alg, h / max(h + m, 1.0), us, act[kern][i] / 8 / us / 1e3))          # (the counter sums the 8 XCDs)
            except (KeyError, IndexError):           # an instantiation name rocprofv3 did not print, or fewer launches than listed: the table above is stale
                raise SystemExit("fetch_order_summary: no launch %d of %s in run %s (kernels seen: %s)" % (i, kern, label, sorted(fe)))
        print("| %s | %d | %.0f | %s |" % (layer, Cout // 32, alg / 1e6, " | ".join(cells)))
