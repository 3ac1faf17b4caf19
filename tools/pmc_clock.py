#!/usr/bin/env python3
"""Per-kernel clock and instruction counts out of one rocprofv3 --pmc pass (counter_collection.csv, no tracing beside it):
    python tools/pmc_clock.py <dir with *_counter_collection.csv> [kernel-name regex]
Counters: GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_INSTS_VALU.  Per kernel (demangled name up to its template arguments):
launches, median duration, effective clock = GRBM_GUI_ACTIVE / 8 XCDs / duration, mfma_busy = SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs *
GRBM_GUI_ACTIVE / 8), and the median SQ_INSTS_MFMA / SQ_INSTS_VALU per launch (medians over launches)."""
import collections
import csv
import glob
import os
import re
import statistics
import sys

root = sys.argv[1]
flt = re.compile(sys.argv[2]) if len(sys.argv) > 2 else None
per = collections.defaultdict(dict)          # (name, dispatch) -> {counter: value, "ns": duration}
for f in glob.glob(os.path.join(root, "**", "*_counter_collection.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        name = re.sub(r"\(.*$", "", r["Kernel_Name"]).replace("void ", "").replace("c3r::", "")
        if flt and not flt.search(name):
            continue
        d = per[(name, f, r["Dispatch_Id"])]
        d[r["Counter_Name"]] = float(r["Counter_Value"])
        d["ns"] = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
by = collections.defaultdict(list)
for (name, _f, _d), v in per.items():
    by[name].append(v)
print("%-40s %6s %9s %9s %10s %14s %14s" % ("kernel", "n", "ms", "clock_GHz", "mfma_busy", "INSTS_MFMA", "INSTS_VALU"))
for name, vs in sorted(by.items()):
    vs = [v for v in vs if v["ns"] > 0 and "GRBM_GUI_ACTIVE" in v]
    if not vs:
        continue
    med = lambda xs: statistics.median(xs)
    ms = med([v["ns"] * 1e-6 for v in vs])
    clk = med([v["GRBM_GUI_ACTIVE"] / 8 / v["ns"] for v in vs])
    busy = med([v.get("SQ_VALU_MFMA_BUSY_CYCLES", 0) / (1024 * v["GRBM_GUI_ACTIVE"] / 8) for v in vs])
    print("%-40s %6d %9.3f %9.3f %10.3f %14.4g %14.4g" % (name[:40], len(vs), ms, clk, busy, med([v.get("SQ_INSTS_MFMA", 0) for v in vs]),
                                                        med([v.get("SQ_INSTS_VALU", 0) for v in vs])))
