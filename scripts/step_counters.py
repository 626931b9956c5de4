"""Per-dispatch hardware counters of the headline step kernel from rocprofv3
--pmc passes (run_counter_collection.csv), as JSON.

    python scripts/step_counters.py PASS_DIR [PASS_DIR ...] > counters.json

Each pass directory is the -d of one `rocprofv3 --pmc ... -o run
--output-format csv -- python bench.py` run (counters only, no tracing in the
same run).  Per counter: median and mean over the dispatches of
vecenv_step_kernel<2, 0, false, true, false, ...> at 4096 worlds, summed over
the counter's instances by rocprofv3."""
import csv
import glob
import json
import os
import statistics
import sys

KERNEL = "vecenv_step_kernel<2, 0, false, true, false"


def main():
    out = {"kernel": KERNEL, "counters": {}}
    for d in sys.argv[1:]:
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            vals = {}
            for r in csv.DictReader(open(path)):
                grid = r.get("Grid_Size") or r.get("Grid_Size_X")
                # 4096 worlds: 64 blocks of 64 threads, or of 128 with the helper wave
                if KERNEL in r["Kernel_Name"] and (not grid or int(grid) in (4096, 8192)):
                    vals.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
            for name, v in sorted(vals.items()):
                out["counters"][name] = {"dispatches": len(v), "median": statistics.median(v),
                                         "mean": round(statistics.mean(v), 2), "min": min(v), "max": max(v)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
