#!/usr/bin/env python3
"""The flat probe's launches, call by call, out of a rocprofv3 kernel trace (csv) of bench.py: per call its kernels with their
durations and the gaps between them, then min / mean / max per kernel over the calls after the first `skip` (the warm-up).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o main -- python3 bench.py --no-cpu --no-queries
    python3 tools/probe_step_trace.py DIR/main_kernel_trace.csv [skip=3]"""
import csv
import sys

SHORT = {"probe_domain_kernel": "sample", "NoRoot, 1>": "build", "NoRoot, 2>": "answer", "NoRoot, 0>": "plain"}


def short(name):
    for key, s in SHORT.items():
        if key in name and ("probe_kernel" in name or key == "probe_domain_kernel"):
            return s
    return None


def main():
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    rows = []
    with open(sys.argv[1]) as f:
        for r in csv.DictReader(f):
            s = short(r["Kernel_Name"])
            if s:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), s, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])))
    rows.sort()
    calls = []  # a call ends with its answer (or is one plain launch)
    cur = []
    for r in rows:
        cur.append(r)
        if r[2] in ("answer", "plain"):
            calls.append(cur)
            cur = []
    per = {}
    prev_end = None
    for i, c in enumerate(calls):
        parts = []
        for j, (s, e, name, wgs) in enumerate(c):
            if j:
                parts.append("gap %.1f" % ((s - c[j - 1][1]) / 1e3))
            parts.append("%s %.1f us (%d blocks)" % (name, (e - s) / 1e3, wgs))
            if i >= skip:
                per.setdefault(name, []).append((e - s) / 1e3)
        span = (c[-1][1] - c[0][0]) / 1e3
        since = "" if prev_end is None else "  [%.1f us after the call before]" % ((c[0][0] - prev_end) / 1e3)
        if i >= skip:
            per.setdefault("first start to last end", []).append(span)
            if prev_end is not None:
                per.setdefault("idle before the call", []).append((c[0][0] - prev_end) / 1e3)
        prev_end = c[-1][1]
        print("call %2d: %d launch(es), %.1f us first start to last end: %s%s" % (i, len(c), span, ", ".join(parts), since))
    print("calls %d.. (steady state):" % skip)
    for name, v in per.items():
        print("  %-24s n %3d  min %8.1f  mean %8.1f  max %8.1f us  (spread %.2f %%)" % (name, len(v), min(v), sum(v) / len(v), max(v), 100 * (max(v) - min(v)) / min(v)))


if __name__ == "__main__":
    main()
