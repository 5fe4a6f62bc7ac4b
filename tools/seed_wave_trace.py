#!/usr/bin/env python
"""Medians of the seed route's launches from rocprofv3 kernel traces (no GPU: reads the CSV files).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python bench.py --gpus 1 --steps 30 --warmup 3
    python tools/seed_wave_trace.py NAME=DIR/t_kernel_trace.csv [NAME=...]

Per trace: median (min-max) in microseconds of the coarse bound kernel (the control), of seed_park_kernel,
sweep_fold_kernel and sweep_finish_kernel, and of the two seed launches of a call taken apart: the launches of the
row-part instantiation of sweep2_kernel come in pairs, first wave then second wave, and the first wave's is the longer
one of a pair."""
import collections
import csv
import re
import statistics
import sys

WANT = ("prune_bound_mm32_kernel", "seed_park_kernel", "sweep_fold_kernel", "sweep_finish_kernel")


def fmt(v):
    return "n=%d  median %.1f  (%.1f-%.1f)" % (len(v), statistics.median(v), min(v), max(v))


def main():
    for arg in sys.argv[1:]:
        name, path = arg.split("=", 1)
        by = collections.defaultdict(list)
        for r in csv.DictReader(open(path)):
            t0 = int(r["Start_Timestamp"])
            by[re.sub(r"^void |\(.*$", "", r["Kernel_Name"])].append((t0, (int(r["End_Timestamp"]) - t0) / 1e3))
        print("== %s" % name)
        for k in sorted(by):
            us = [d for _, d in sorted(by[k])]
            # the row-part instantiations: sweep2_kernel<Dpad, false, 0, true, true[, true]>
            if re.match(r"sweep2_kernel<\d+, (false|true), 0, true, true", k):
                pairs = [us[i:i + 2] for i in range(0, len(us) - 1, 2)]
                print("  %-52s first wave   %s" % (k, fmt([max(p) for p in pairs])))
                print("  %-52s second wave  %s" % ("", fmt([min(p) for p in pairs])))
            elif any(w in k for w in WANT):
                print("  %-52s %s" % (k, fmt(us)))


if __name__ == "__main__":
    main()
