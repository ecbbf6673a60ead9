#!/usr/bin/env python3
"""Measurements behind the index decode calls ("Index decode"), in the manner of tools/slice_probe.py.  One process, the
variants alternate, --repeats rounds after a warm-up round.

1. Default, profiler off, end to end: --pick of the --shape[0] experts (dimension 0) of one float32 tensor of --shape, once spread evenly
   and once in neighbouring pairs that share chunks, through
     index: unpack_tensor_index,
     full:  unpack_tensor followed by index_select,
     rows:  one unpack_tensor_rows entry per expert in ONE bz3_hip_decompress_device_range_many call (unpack_state_dict(rows=) over a
            dict that names the same PackedTensor once per expert):
   time, torch.cuda.max_memory_allocated above what is allocated before the call, CM launches, and the chunks each variant decodes
   (from the layout).  Every one of these calls takes one block's serial CM decode whatever it decodes -- about 15 s at the default
   16 MiB block -- so a case is 3 x (--repeats + 1) such calls, some five minutes at five repeats: --cases runs one case per invocation,
   and the result file is written after every case.
2. --kernels-only: the select merge (k = 1, 2, 4, 8, with and without a base) on --slots x --slot-mib MiB slots, for every period of
   slice_probe.PERIODS as a uniform piece list of m = 2, 64 and 4096 pieces per period through bz3_hip_debug_select, alternating in one
   process with its yardstick, k_strided_segments gathering the SAME BYTE SET through bz3_hip_debug_strided.  Kernel times come from
   `rocprofv3 --kernel-trace --stats -f csv -d DIR -o select -- python tools/select_probe.py --kernels-only`, then
   `python tools/select_probe.py --from-trace DIR/select_kernel_trace.csv`, which assigns the trace's dispatches of the segment kernels
   to the variants in launch order and adds them to --out under "kernels".  The rule ("Strided range decode"): a variant's
   worst repeat lies within its yardstick's own best-to-worst spread plus 25 % of the yardstick's best; it is applied to the periods of
   slice_probe.RULE_PERIODS, the others are reported.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bzip3_amd  # noqa: E402
from slice_probe import NO_BASE, PERIODS, RULE_PERIODS, _alternate, _stats, dest_bytes  # noqa: E402

PIECES = (2, 64, 4096)
KERNELS = ("k_strided_segments", "k_select_segments")
# (name, kernel, yardstick, element size, base, period, pieces per period)
VARIANTS = []
for _k in (1, 2, 4, 8):
    for _b in (0, 1):
        for _p in PERIODS:
            _tag = f"k{_k}{'_base' if _b else ''}_{_p}"
            VARIANTS.append((f"strided_{_tag}", "k_strided_segments", None, _k, _b, _p, 0))
            for _m in PIECES:
                VARIANTS.append((f"select_m{_m}_{_tag}", "k_select_segments", f"strided_{_tag}", _k, _b, _p, _m))


def kernel_order(repeats):
    return [(rep - 1, v) for rep in range(repeats + 1) for v in VARIANTS]


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
    for name, kernel, yard, k, has_base, period, m in VARIANTS:
        v = times[name]
        nbytes = slots * dest_bytes(slot_bytes, period)
        e = {"kernel": kernel, "destination_bytes": nbytes, "kernel_ms": [round(x, 4) for x in v], "best_ms": round(min(v), 4), "worst_ms": round(max(v), 4),
             "dest_gb_per_s_best": round(nbytes / (min(v) * 1e-3) / 1e9, 1)}
        if yard:
            y = times[yard]
            e.update({"yardstick": yard, "pieces_per_period": m, "worst_over_yardstick_best": round(max(v) / min(y), 3), "best_over_yardstick_best": round(min(v) / min(y), 3),
                      "yardstick_spread": round(max(y) / min(y) - 1, 4)})
            if period in RULE_PERIODS:
                e["within_rule"] = max(v) / min(y) <= max(y) / min(y) + 0.25
        res[name] = e
    kernels = {"slots": slots, "slot_bytes": slot_bytes, "periods": {k: list(v) for k, v in PERIODS.items()}, "rule_periods": list(RULE_PERIODS), "pieces_per_period": list(PIECES),
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
    for name, _, yard, k, has_base, period, m in VARIANTS:
        run, stride = PERIODS[period]
        n = dest_bytes(slot_bytes, period)
        if not yard:  # the runs from the slot's first byte on
            t = (C.c_uint64 * (10 * slots))(*[v for i in range(slots) for v in (i * pitch, i * pitch if has_base else NO_BASE, i * pitch, slot_bytes, k | 0x100, 0, run, run, stride, n)])
            calls[name] = (lambda t=t: lib.bz3_hip_debug_strided(src.data_ptr(), base.data_ptr(), dst.data_ptr(), t, slots))
        else:  # the same bytes as m uniform pieces per period of m strides; every slot reads the one list
            pc = (C.c_uint64 * (2 * m))(*[v for j in range(m) for v in (j * stride, run)])
            t = (C.c_uint64 * (12 * slots))(*[v for i in range(slots) for v in (i * pitch, i * pitch if has_base else NO_BASE, i * pitch, slot_bytes, k | 0x100, 0, m * stride, 0, 0, n, 0, m)])
            calls[name] = (lambda t=t, pc=pc, m=m: lib.bz3_hip_debug_select(src.data_ptr(), base.data_ptr(), dst.data_ptr(), t, slots, pc, m))
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


def experts_probe(lib, shape, experts, repeats):
    import torch

    g = torch.Generator(device="cuda:0").manual_seed(6)
    x = torch.randn(*shape, generator=g, device="cuda:0") * 0.02
    p = bzip3_amd.pack_tensor(x)
    launches = {}

    def counted(name, call):
        def f():
            lib.bz3_hip_debug_cm_launches(1)
            got = call()
            launches[name] = lib.bz3_hip_debug_cm_launches(1)
            return got
        return f

    index = torch.tensor(experts, device="cuda:0")
    many = {f"e{i}": p for i in experts}  # the same frame once per expert: n independent range entries of one _many call
    rows = {f"e{i}": (i, i + 1) for i in experts}
    variants = {"index": counted("index", lambda: bzip3_amd.unpack_tensor_index(p, 0, experts)),
                "full": counted("full", lambda: bzip3_amd.unpack_tensor(p).index_select(0, index)),
                "rows": counted("rows", lambda: list(bzip3_amd.unpack_state_dict(many, rows=rows).values()))}
    t, peak, last = _alternate(torch, variants, repeats)
    want = x.index_select(0, index)
    assert torch.equal(last["index"], want) and torch.equal(last["full"], want) and torch.equal(torch.cat(last["rows"]), want)
    e = p.nbytes // shape[0]
    per_expert = [set(range(i * e // p.block_size, ((i + 1) * e - 1) // p.block_size + 1)) for i in experts]
    chunks = -(-p.nbytes // p.block_size)
    # (a CM launch is a window of up to 256 chunks, so the chunks each variant decodes are counted from the layout: the index call the union of
    # the experts' chunks, the rows call every entry's chunks, the full call all of them)
    decoded = {"index": len(set().union(*per_expert)), "full": chunks, "rows": sum(len(c) for c in per_expert)}
    return {"shape": list(shape), "dtype": "float32", "experts": list(experts), "block_size": p.block_size, "chunks": chunks, "chunks_decoded": decoded,
            "expert_bytes": e, "cm_launches": launches, "times": {k: _stats(v) for k, v in t.items()}, "peak_allocated_bytes_above_start": {k: v for k, v in peak.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(64, 1024, 1024))
    ap.add_argument("--pick", type=int, default=8)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--slot-mib", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", nargs="*", choices=["experts_spread", "experts_paired"], help="the end-to-end cases to run (default: both)")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--from-trace", help="a rocprofv3 kernel trace (csv) of a --kernels-only run: add its kernel times to --out and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_probe.json"))
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace, a.slots, a.slot_mib << 20, a.repeats, a.out)
    lib = bzip3_amd.load()
    if a.kernels_only:  # (the times that count are the trace's: the wall clock around the hooks is printed, not recorded)
        print(json.dumps({"kernels_host_wall_clock": kernel_probe(lib, a.slots, a.slot_mib << 20, a.repeats)}))
        return
    n, pick = a.shape[0], a.pick
    # evenly spread; then neighbouring pairs, placed so that a pair lies inside one chunk wherever a chunk holds two experts or more
    cases = {"experts_spread": [i * (n // pick) for i in range(pick)], "experts_paired": sorted(i * (n // (pick // 2)) + d for i in range(pick // 2) for d in (0, 1))}
    for name in a.cases or list(cases):  # (a call with a 16 MiB block takes one block's decode time, about 15 s, whatever it decodes: the file is written after every case)
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc[name] = experts_probe(lib, tuple(a.shape), cases[name], a.repeats)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
        print(json.dumps({name: doc[name]}), flush=True)


if __name__ == "__main__":
    main()
