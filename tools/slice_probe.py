#!/usr/bin/env python3
"""Measurements behind the strided range calls ("Strided range decode"), in the manner of tools/range_probe.py.  One process,
the variants alternate, --repeats rounds after a warm-up round.

1. Default, profiler off, end to end:
   case 1: one eighth of the columns (dimension 1) of --matrices float32 matrices of --matrix-mib MiB in one
           unpack_state_dict(slices=) call, against unpack_state_dict followed by narrow(...).contiguous(): time and
           torch.cuda.max_memory_allocated above what is allocated before the call.
   case 2: one eighth of the middle dimension of one float32 tensor of --shape, against the full unpack: chunks of the frame, CM
           launches and time.
2. --kernels-only: the strided merge (k = 1, 2, 4, 8, with and without a base) on --slots x --slot-mib MiB slots, for every period of
   PERIODS, alternating in one process with its yardstick: what a range call launches to move the SAME NUMBER of destination bytes per
   slot as one clipped contiguous segment (k_range_segments for k = 2, 4, 8; a k = 1 clip is a plain copy, k_copy_segments, or with a
   base k_delta_segments).  Kernel times come from
   `rocprofv3 --kernel-trace --stats -f csv -d DIR -o slice -- python tools/slice_probe.py --kernels-only`, then
   `python tools/slice_probe.py --from-trace DIR/slice_kernel_trace.csv`, which assigns the trace's dispatches of the segment kernels
   to the variants in launch order (fixed: see kernel_order) and adds them to --out under "kernels".  The rule: a variant's
   worst repeat per destination byte lies within its yardstick's own best-to-worst spread plus 25 % of the yardstick's best; it is
   applied to the periods of RULE_PERIODS, the others are reported.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bzip3_amd  # noqa: E402

NO_BASE = 2 ** 64 - 1
PERIODS = {"run4k_stride32k": (4 << 10, 32 << 10), "run64k_stride512k": (64 << 10, 512 << 10), "run64_stride512": (64, 512), "run8_stride64": (8, 64)}
RULE_PERIODS = ("run4k_stride32k", "run64k_stride512k")
KERNELS = ("k_copy_segments", "k_move_segments", "k_delta_segments", "k_range_segments", "k_strided_segments")
# (name, kernel, yardstick, element size, base, period)
VARIANTS = []
for _k in (1, 2, 4, 8):
    for _b in (0, 1):
        for _p in PERIODS:
            _tag = f"k{_k}{'_base' if _b else ''}_{_p}"
            # (a k = 1 clip without a base is a plain copy and one with a base a delta copy: what the range call launches for it)
            VARIANTS.append((f"clip_{_tag}", "k_range_segments" if _k > 1 else "k_delta_segments" if _b else "k_copy_segments", None, _k, _b, _p))
            VARIANTS.append((f"strided_{_tag}", "k_strided_segments", f"clip_{_tag}", _k, _b, _p))


def kernel_order(repeats):
    return [(rep - 1, v) for rep in range(repeats + 1) for v in VARIANTS]


def dest_bytes(slot_bytes, period):
    run, stride = PERIODS[period]
    return slot_bytes // stride * run


def from_trace(path, slots, slot_bytes, repeats, out):
    import csv

    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    order = kernel_order(repeats)
    assert len(rows) == len(order), (len(rows), len(order))
    times = {}
    for r, (rep, (name, kernel, *_)) in zip(rows, order):
        assert kernel in r["Kernel_Name"], (r["Kernel_Name"], name)
        if rep >= 0:
            times.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    res = {}
    for name, kernel, yard, k, has_base, period in VARIANTS:
        v = times[name]
        nbytes = slots * dest_bytes(slot_bytes, period)
        e = {"kernel": kernel, "destination_bytes": nbytes, "kernel_ms": [round(x, 4) for x in v], "best_ms": round(min(v), 4), "worst_ms": round(max(v), 4),
             "dest_gb_per_s_best": round(nbytes / (min(v) * 1e-3) / 1e9, 1)}
        if yard:
            y = times[yard]
            e.update({"yardstick": yard, "worst_over_yardstick_best": round(max(v) / min(y), 3), "best_over_yardstick_best": round(min(v) / min(y), 3),
                      "yardstick_spread": round(max(y) / min(y) - 1, 4)})
            if period in RULE_PERIODS:
                e["within_rule"] = max(v) / min(y) <= max(y) / min(y) + 0.25
        res[name] = e
    kernels = {"slots": slots, "slot_bytes": slot_bytes, "periods": {k: list(v) for k, v in PERIODS.items()}, "rule_periods": list(RULE_PERIODS),
               "source": "rocprofv3 --kernel-trace, run of its own", "kernels": res}
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["kernels"] = kernels
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(kernels))


def kernel_probe(lib, slots, slot_bytes, repeats):
    import torch

    pitch = slot_bytes + 256
    src = torch.randint(0, 256, (slots * pitch + 64,), dtype=torch.uint8, device="cuda:0")
    base = torch.randint(0, 256, (slots * pitch + 64,), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(slots * pitch + 64, dtype=torch.uint8, device="cuda:0")
    calls = {}
    for name, _, yard, k, has_base, period in VARIANTS:
        run, stride = PERIODS[period]
        n = dest_bytes(slot_bytes, period)
        if yard:  # the runs from the slot's first byte on
            t = (C.c_uint64 * (10 * slots))(*[v for i in range(slots) for v in (i * pitch, i * pitch if has_base else NO_BASE, i * pitch, slot_bytes, k | 0x100, 0, run, run, stride, n)])
            calls[name] = (lambda t=t: lib.bz3_hip_debug_strided(src.data_ptr(), base.data_ptr(), dst.data_ptr(), t, slots))
        else:  # as many bytes from the middle of the slot, one clipped segment
            a = (slot_bytes - n) // 2 // 16 * 16
            t = (C.c_uint64 * (7 * slots))(*[v for i in range(slots) for v in (i * pitch, i * pitch if has_base else NO_BASE, i * pitch, slot_bytes, k | 0x100, a, a + n)])
            calls[name] = (lambda t=t: lib.bz3_hip_debug_range(src.data_ptr(), base.data_ptr(), dst.data_ptr(), t, slots))
    times = {name: [] for name in calls}
    for rep in range(repeats + 1):  # the first round warms up
        for name, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = call()
            dt = time.perf_counter() - t0
            assert rc == 0, (name, rc)
            if rep:
                times[name].append(dt)
    return {name: {"ms": [round(1e3 * x, 4) for x in v], "best_ms": round(1e3 * min(v), 4)} for name, v in times.items()}


def _stats(v):
    return {"s": [round(x, 5) for x in v], "median_s": round(statistics.median(v), 5), "best_s": round(min(v), 5), "worst_s": round(max(v), 5)}


def _alternate(torch, variants, repeats):
    """variants: {name: call -> result}.  Per name the times, the peaks of allocated memory above the level before the call, the last result."""
    t, peak, last = {k: [] for k in variants}, {k: [] for k in variants}, {}
    for rep in range(repeats + 1):  # the first round warms up
        for name, call in variants.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            got = call()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                t[name].append(dt)
                peak[name].append(torch.cuda.max_memory_allocated() - before)
            if rep == repeats:
                last[name] = got
            del got
    return t, peak, last


def columns_probe(matrices, matrix_bytes, repeats):
    import torch

    rows = 2048
    cols = matrix_bytes // 4 // rows
    g = torch.Generator(device="cuda:0").manual_seed(5)
    sd = {f"w{i}": torch.randn(rows, cols, generator=g, device="cuda:0") * 0.02 for i in range(matrices)}
    packed = bzip3_amd.pack_state_dict(sd)
    lo, hi = cols // 8 * 3, cols // 8 * 4
    slices = {k: (1, lo, hi) for k in sd}
    variants = {"slices": lambda: bzip3_amd.unpack_state_dict(packed, slices=slices),
                "full_then_narrow": lambda: {k: v.narrow(1, lo, hi - lo).contiguous() for k, v in bzip3_amd.unpack_state_dict(packed).items()}}
    t, peak, last = _alternate(torch, variants, repeats)
    for name, got in last.items():
        assert all(torch.equal(got[k], sd[k][:, lo:hi]) for k in sd), name
    return {"matrices": matrices, "shape": [rows, cols], "dtype": "float32", "columns": [lo, hi], "frame_bytes": sum(p.frame.numel() for p in packed.values()),
            "tensor_bytes": matrices * matrix_bytes, "slice_bytes": matrices * rows * (hi - lo) * 4, "times": {k: _stats(v) for k, v in t.items()},
            "peak_allocated_bytes_above_start": {k: v for k, v in peak.items()}}


def middle_probe(lib, shape, repeats):
    import torch

    g = torch.Generator(device="cuda:0").manual_seed(6)
    x = torch.randn(*shape, generator=g, device="cuda:0") * 0.02
    p = bzip3_amd.pack_tensor(x)
    lo, hi = shape[1] // 8 * 3, shape[1] // 8 * 4
    launches = {}

    def counted(name, call):
        def f():
            lib.bz3_hip_debug_cm_launches(1)
            got = call()
            launches[name] = lib.bz3_hip_debug_cm_launches(1)
            return got
        return f

    variants = {"slice": counted("slice", lambda: bzip3_amd.unpack_tensor_slice(p, 1, lo, hi)), "full": counted("full", lambda: bzip3_amd.unpack_tensor(p))}
    t, peak, last = _alternate(torch, variants, repeats)
    assert torch.equal(last["slice"], x[:, lo:hi]) and torch.equal(last["full"], x)
    inner = shape[2] * 4
    runs = [(i * shape[1] * inner + lo * inner, i * shape[1] * inner + hi * inner) for i in range(shape[0])]
    needed = len({c for a, z in runs for c in range(a // p.block_size, (z - 1) // p.block_size + 1)})
    return {"shape": list(shape), "dtype": "float32", "middle": [lo, hi], "block_size": p.block_size, "chunks": -(-p.nbytes // p.block_size), "chunks_needed": needed,
            "run_bytes": (hi - lo) * inner, "stride_bytes": shape[1] * inner, "cm_launches": launches, "times": {k: _stats(v) for k, v in t.items()},
            "peak_allocated_bytes_above_start": {k: v for k, v in peak.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrices", type=int, default=32)
    ap.add_argument("--matrix-mib", type=int, default=16)
    ap.add_argument("--shape", type=int, nargs=3, default=(64, 4096, 1024))
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--slot-mib", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--from-trace", help="a rocprofv3 kernel trace (csv) of a --kernels-only run: add its kernel times to --out and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slice_probe.json"))
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace, a.slots, a.slot_mib << 20, a.repeats, a.out)
    lib = bzip3_amd.load()
    if a.kernels_only:  # (the times that count are the trace's: the wall clock around the hooks is printed, not recorded)
        print(json.dumps({"kernels_host_wall_clock": kernel_probe(lib, a.slots, a.slot_mib << 20, a.repeats)}))
        return
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["columns"] = columns_probe(a.matrices, a.matrix_mib << 20, a.repeats)
    doc["middle"] = middle_probe(lib, tuple(a.shape), a.repeats)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
