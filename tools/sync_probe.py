#!/usr/bin/env python3
"""Measurements behind the sync ("Sync"), in the manner of tools/update_probe.py.

1. Default, profiler off: a state dict of --tensors float32 tensors of N(0, 0.02) of --chunks-per-tensor chunks of --block-mib MiB each (a short
   last one), 1024 chunks at the defaults, so that a fresh pack takes ceil(1024 / 256) = 4 encode windows.  For each of --dirty per cent of the
   chunks (0, 1, 10, 100; spread evenly over the dict, one element changed in each) sync_state_dict against pack_state_dict of the new tensors, the
   path a user has without it on the same library, alternating in one process, --repeats times after a warm-up round in which every synced frame is
   compared with the packed one.  The model to compare with: a sync of d dirty chunks costs ceil(d / 256) encode windows and one pass over 2 T
   bytes (plus the checksums, which both paths compute), the pack ceil(n / 256) windows; `model` records the counts, the CM launches of each path
   are counted (bz3_hip_debug_cm_launches) and the medians and ranges go to --out.
2. --kernels-only: k_diff_segments on --slots segments of --slot-mib MiB, both sides aligned and `a` 7 and / or `b` 9 bytes off, alternating in one
   process with k_copy_segments moving the same bytes at the same alignments through bz3_hip_debug_copy_segments (its yardstick: both move two
   bytes per byte of a segment).  Kernel times come from `rocprofv3 --kernel-trace --stats -f csv -d DIR -o sync -- python tools/sync_probe.py
   --kernels-only`, then `python tools/sync_probe.py --from-trace DIR/.../sync_kernel_trace.csv`, which assigns the trace's dispatches of the two
   kernels to the variants in launch order and adds best to worst, bytes per second and the ratios to --out under "kernels".  The expectation a
   variant is held against is its yardstick's best time plus the yardstick's own spread plus 25 %, the margin of the delta section.
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
import bzip3_amd  # noqa: E402

OFFSETS = [("aligned", 0, 0), ("a7", 7, 0), ("b9", 0, 9), ("a7_b9", 7, 9)]  # (name, first side's bytes off a 16-byte boundary, second side's)
# (name, kernel, yardstick, offsets): a copy's first side is its destination, the side its tiles follow, as a diff's tiles follow `a`
VARIANTS = [(f"copy_{n}", "k_copy_segments", None, (x, y)) for n, x, y in OFFSETS] + [(f"diff_{n}", "k_diff_segments", f"copy_{n}", (x, y)) for n, x, y in OFFSETS]
KERNELS = ("k_copy_segments", "k_diff_segments")
MARGIN = 0.25


def _stats(v):
    return {"s": [round(x, 5) for x in v], "median_s": round(statistics.median(v), 5), "best_s": round(min(v), 5), "worst_s": round(max(v), 5)}


def from_trace(path, slots, slot_bytes, repeats, out):
    import csv

    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    order = [(rep - 1, v) for rep in range(repeats + 1) for v in VARIANTS]
    assert len(rows) == len(order), (len(rows), len(order))
    times = {}
    for r, (rep, (name, kernel, *_)) in zip(rows, order):
        assert kernel in r["Kernel_Name"], (r["Kernel_Name"], name)
        if rep >= 0:
            times.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    res = {}
    moved = 2 * slots * slot_bytes  # a copy reads and writes every byte, a diff reads it on both sides
    for name, kernel, yard, offs in VARIANTS:
        v = times[name]
        e = {"kernel": kernel, "offsets_mod_16": list(offs), "kernel_ms": [round(x, 4) for x in v], "best_ms": round(min(v), 4), "worst_ms": round(max(v), 4),
             "tb_per_s_best": round(moved / (min(v) * 1e-3) / 1e12, 3), "tb_per_s_worst": round(moved / (max(v) * 1e-3) / 1e12, 3)}
        if yard:
            y = times[yard]
            spread = max(y) / min(y) - 1
            e.update({"yardstick": yard, "worst_over_yardstick_best": round(max(v) / min(y), 3), "best_over_yardstick_best": round(min(v) / min(y), 3),
                      "yardstick_spread": round(spread, 4), "expected_at_most": round(1 + spread + MARGIN, 3), "within_expectation": max(v) / min(y) <= 1 + spread + MARGIN})
        res[name] = e
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["kernels"] = {"slots": slots, "slot_bytes": slot_bytes, "bytes_moved_per_launch": moved, "source": "rocprofv3 --kernel-trace, run of its own", "kernels": res}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["kernels"]))


def kernel_probe(lib, slots, slot_bytes, repeats):
    import torch

    pitch = slot_bytes + 256
    room = slots * pitch + 64
    a = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")
    b = a.clone()  # equal runs: every tile reads all its bytes whatever the kernel does once it has found a difference
    at = [i * pitch for i in range(slots)]
    flags = (C.c_uint32 * slots)()
    calls = {}
    for name, kernel, _, (x, y) in VARIANTS:
        if kernel == "k_copy_segments":  # (src_off, dst_off, len): the destination at the first offset, the source at the second
            t = (C.c_uint64 * (3 * slots))(*[v for o in at for v in (o + y, o + x, slot_bytes)])
            calls[name] = (lambda t=t: lib.bz3_hip_debug_copy_segments(a.data_ptr(), b.data_ptr(), t, slots))
        else:
            t = (C.c_uint64 * (3 * slots))(*[v for o in at for v in (o + x, o + y, slot_bytes)])
            calls[name] = (lambda t=t: lib.bz3_hip_debug_diff(a.data_ptr(), b.data_ptr(), t, slots, flags))
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


def frame_probe(lib, tensors, per_tensor, block_bytes, dirty_percents, repeats):
    import torch

    cols = 1024
    per_block = block_bytes // (cols * 4)  # rows in a block
    rows = per_tensor * per_block - 1  # a short last block
    g = torch.Generator(device="cuda:0").manual_seed(tensors + per_tensor)
    prev = {f"t{i:04d}": torch.randn(rows, cols, generator=g, device="cuda:0") * 0.02 for i in range(tensors)}
    names = list(prev)
    packed = bzip3_amd.pack_state_dict(prev, block_bytes, lib=lib)
    chunks = tensors * per_tensor
    assert all(p.block_size == block_bytes and p.planes == 4 for p in packed.values())
    total = sum(p.nbytes for p in packed.values())
    out = {"dtype": "float32", "planes": 4, "tensors": tensors, "chunks": chunks, "block_bytes": block_bytes, "input_bytes": total,
           "frame_bytes": sum(p.frame.numel() for p in packed.values()), "data": "N(0, 0.02)", "cases": {}}
    for pc in dirty_percents:
        d = chunks * pc // 100 if pc else 0
        which = sorted({(j * chunks) // d for j in range(d)}) if d else []
        sd = {k: v.clone() for k, v in prev.items()}
        for c in which:  # one element in the middle of the chunk
            sd[names[c // per_tensor]][(c % per_tensor) * per_block + per_block // 2, 7] += 1.0
        t = {"sync": [], "pack": []}
        launches, recoded = {}, None
        for rep in range(repeats + 1):  # the first round warms up and checks
            frames = {}
            for path in t:
                stats = {}
                lib.bz3_hip_debug_cm_launches(1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                q = bzip3_amd.sync_state_dict(packed, sd, prev, stats=stats, lib=lib) if path == "sync" else bzip3_amd.pack_state_dict(sd, block_bytes, lib=lib)
                torch.cuda.synchronize()
                dt_s = time.perf_counter() - t0
                launches[path] = lib.bz3_hip_debug_cm_launches(1)
                print(f"{pc} % dirty, round {rep}: {path} {dt_s:.3f} s, {launches[path]} CM launches", file=sys.stderr, flush=True)
                if rep:
                    t[path].append(dt_s)
                else:
                    frames[path] = q
                    if path == "sync":
                        recoded = sum(r for r, _ in stats.values())
                del q
            if not rep:
                assert recoded == len(which), (recoded, len(which))
                for k in names:
                    assert torch.equal(frames["sync"][k].frame, frames["pack"][k].frame) and frames["sync"][k].crc == frames["pack"][k].crc, ("the synced frame is not the packed one", pc, k)
        e = {"dirty_chunks": len(which), "cm_launches": launches,
             "model": {"sync_encode_windows": -(-len(which) // 256), "pack_encode_windows": -(-chunks // 256), "sync_bytes_compared": 2 * total},
             "times": {k: _stats(v) for k, v in t.items()}}
        e["pack_over_sync_median"] = round(e["times"]["pack"]["median_s"] / e["times"]["sync"]["median_s"], 2)
        e["pack_best_over_sync_worst"] = round(e["times"]["pack"]["best_s"] / e["times"]["sync"]["worst_s"], 2)
        out["cases"][f"{pc}_percent"] = e
        del sd
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tensors", type=int, default=128)
    ap.add_argument("--chunks-per-tensor", type=int, default=8)
    ap.add_argument("--block-mib", type=int, default=1)
    ap.add_argument("--dirty", type=int, nargs="+", default=[0, 1, 10, 100])
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--slot-mib", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--from-trace", help="a rocprofv3 kernel trace (csv) of a --kernels-only run: add its kernel times to --out and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_probe.json"))
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace, a.slots, a.slot_mib << 20, a.repeats, a.out)
    lib = bzip3_amd.load()
    if a.kernels_only:  # (the times that count are the trace's: the wall clock around the hooks is printed, not recorded)
        print(json.dumps({"kernels_host_wall_clock": kernel_probe(lib, a.slots, a.slot_mib << 20, a.repeats)}))
        return
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["frames"] = frame_probe(lib, a.tensors, a.chunks_per_tensor, a.block_mib << 20, a.dirty, a.repeats)
    doc["repeats"] = a.repeats
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
