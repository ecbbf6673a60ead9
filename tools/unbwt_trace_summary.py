"""Per-block summary of the inverse BWT's kernels in a kernel trace of tools/tail_pipe_probe.py:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o tail -- python tools/tail_pipe_probe.py 8 768 --settings=default --trials=1
    python tools/unbwt_trace_summary.py DIR/**/tail_kernel_trace.csv [blocks per decode = 768]
A pass is what lies between a k_ub_hist and the next k_ub_tail on the stream (one block, or a run of blocks through the batched kernels; the
run's size is read off the k_ub_tail grid).  Printed per BLOCK, over the last decode of the trace (the ones before it are warm-up): the span
from the first to the last kernel, the time inside k_ub_walk, k_ub_walk_long, the jump rounds and all other kernels of the pass, and the gaps
(span minus kernel time), with launches per block."""
import csv
import sys


def main():
    path = sys.argv[1]
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 768
    names = ("k_ub_", "k_rs_", "k_scan_", "k_add_last")
    rows = [r for r in csv.DictReader(open(path)) if any(n in r["Kernel_Name"] for n in names)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    passes, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "k_ub_hist" in name:
            cur = []
        if cur is None:
            continue  # (a sorter kernel of the encoder)
        cur.append(r)
        if "k_ub_tail" in name:
            per_pass = int(r.get("Grid_Size_Y", r.get("Grid_Size_y", "1")) or 1)
            passes.append((max(1, per_pass), cur))
            cur = None
    # the last decode: passes from the end until `blocks` blocks are covered
    take, got = [], 0
    for p in reversed(passes):
        if got >= blocks:
            break
        take.append(p)
        got += p[0]
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    tot = {"span": 0.0, "walk": 0.0, "walk_long": 0.0, "jump": 0.0, "other": 0.0, "launches": 0}
    for _, p in take:
        tot["span"] += (int(p[-1]["End_Timestamp"]) - int(p[0]["Start_Timestamp"])) / 1e3
        tot["launches"] += len(p)
        for r in p:
            n = r["Kernel_Name"]
            key = "walk_long" if "k_ub_walk_long" in n else "walk" if "k_ub_walk" in n else "jump" if "k_ub_jump" in n else "other"
            tot[key] += us(r)
    kernels = tot["walk"] + tot["walk_long"] + tot["jump"] + tot["other"]
    print(f"{path}: {len(take)} passes, {got} blocks (last decode), {got / max(1, len(take)):.2f} blocks per pass")
    print("per block, us: span %.1f = k_ub_walk %.1f + k_ub_walk_long %.1f + jump rounds %.1f + other kernels %.1f + gaps %.1f; launches %.1f"
          % tuple(x / max(1, got) for x in (tot["span"], tot["walk"], tot["walk_long"], tot["jump"], tot["other"], tot["span"] - kernels, tot["launches"])))


if __name__ == "__main__":
    main()
