"""Per-block summary of the forward BWT's kernels in a kernel trace of the benchmark:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o front -- python bench.py --gpus 1 --steps 1 --warmup 0 --no-cpu-baseline
    python tools/bwt_trace_summary.py DIR/**/front_kernel_trace.csv
A transform is what lies between a k_bwt_sym_hist and the next k_bwt_finish on the same queue (one block, or a run of blocks through the
job-table kernels: the run's size is the y extent of the k_bwt_sym_hist grid).  Only the sorter's own kernels, the shared sort / scan
kernels and the runtime's fills and copies on that queue are counted.  Printed per BLOCK: the span from the first to the last kernel, the
time inside kernels, the gaps (span minus kernel time), launches, and the time of each kernel family by the phase it was launched in."""
import csv
import statistics
import sys

OWN = ("k_bwt_", "k_vlc_", "k_big_", "k_bg_", "k_isa_", "k_rs_", "k_scan_", "k_add_last", "fillBuffer", "copyBuffer")
FAMILIES = ("vlc build", "keys / hist / outside", "round-0 passes", "heads / spines", "route / wide / tail", "big-round passes", "big-round other",
            "isa build", "doubling passes", "doubling other", "scans", "fills and copies", "finish")


def family(name, phase):
    if "fillBuffer" in name or "copyBuffer" in name:
        return "fills and copies"
    if "k_scan_" in name or "k_add_last" in name:
        return "scans"
    if "k_rs_" in name:
        return {"round0": "round-0 passes", "big": "big-round passes", "isa": "isa build", "doubling": "doubling passes"}.get(phase, "round-0 passes")
    if "k_vlc_" in name:
        return "vlc build"
    if any(x in name for x in ("k_bwt_route", "k_bwt_wide", "k_bwt_tail")):
        return "route / wide / tail"
    if any(x in name for x in ("k_bwt_heads", "k_bwt_reduce_heads", "k_bwt_spine", "k_bwt_reset_words")):
        return "heads / spines"
    if "k_bwt_finish" in name:
        return "finish"
    if "k_big_" in name:
        return "big-round other"
    if "k_bwt_doubling" in name or (phase == "doubling" and "k_bg_" in name):
        return "doubling other"
    if "k_bg_" in name or "k_isa_" in name:
        return "isa build"
    return "keys / hist / outside"


def next_phase(name, phase):
    if "k_bwt_vlc_keys" in name:
        return "round0"
    if "k_big_keys" in name:
        return "big"
    if "k_bg_reduce" in name and phase not in ("isa", "doubling"):
        return "isa"
    if "k_bwt_doubling" in name:
        return "doubling"
    if any(x in name for x in ("k_bwt_heads", "k_bwt_route", "k_bwt_reduce_heads")):
        return "resolve"
    return phase


def main():
    path = sys.argv[1]
    rows = [r for r in csv.DictReader(open(path)) if any(n in r["Kernel_Name"] for n in OWN)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    qkey = "Queue_Id" if rows and "Queue_Id" in rows[0] else None
    runs, open_runs = [], {}
    for r in rows:
        name = r["Kernel_Name"]
        q = r[qkey] if qkey else 0
        if "k_bwt_sym_hist" in name:
            b = int(r.get("Grid_Size_Y", r.get("Grid_Size_y", "1")) or 1)
            open_runs[q] = {"blocks": max(1, b), "rows": [], "phase": "codes"}
        run = open_runs.get(q)
        if run is None:
            continue
        run["phase"] = next_phase(name, run["phase"])
        run["rows"].append((r, family(name, run["phase"])))
        if "k_bwt_finish" in name:
            runs.append(run)
            del open_runs[q]
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    blocks = sum(x["blocks"] for x in runs)
    span = busy = 0.0
    launches = 0
    fam = {f: 0.0 for f in FAMILIES}
    fam_n = {f: 0 for f in FAMILIES}
    spans = []
    for x in runs:
        rs = x["rows"]
        sp = (max(int(r["End_Timestamp"]) for r, _ in rs) - int(rs[0][0]["Start_Timestamp"])) / 1e3
        span += sp
        spans.append(sp / x["blocks"])
        launches += len(rs)
        for r, f in rs:
            busy += us(r)
            fam[f] += us(r)
            fam_n[f] += 1
    nb = max(1, blocks)
    print(f"{path}: {len(runs)} runs, {blocks} forward BWTs, {blocks / max(1, len(runs)):.2f} blocks per run")
    if not runs:
        return
    print("per block (mean, us): span first..last kernel %.1f, kernels busy %.1f, gaps %.1f, launches %.1f" % (span / nb, busy / nb, (span - busy) / nb, launches / nb))
    print("span per block over the runs: median %.1f us, min %.1f, max %.1f; sum of spans %.3f s" % (statistics.median(spans), min(spans), max(spans), span / 1e6))
    print("per block by family (mean us, launches):")
    for f in FAMILIES:
        if fam_n[f]:
            print("  %-24s %9.1f %8.1f" % (f, fam[f] / nb, fam_n[f] / nb))


if __name__ == "__main__":
    main()
