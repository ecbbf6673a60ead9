#!/usr/bin/env python3
"""Measurements behind the range update ("Range update"), in the manner of tools/range_probe.py.

1. Default, profiler off: per dtype (float32, bfloat16) and chunk count (--chunks, default 64 and 256) one tensor of N(0, 0.02) whose frame has
   that many chunks of --block-mib MiB (a short last one).  update_tensor_rows of 1 row, of one block's worth of rows and of 8 blocks' worth, at
   an interior row that starts in the middle of a chunk, against the path a user has without it on the same library -- unpack_tensor, slice
   assign, pack_tensor --, alternating in one process, --repeats times after a warm-up round.  Every update is checked once, in the warm-up round:
   its frame is the full path's frame.  The model to compare with: an update of w bytes costs 2 decodes and w / bs + 2 encodes and one copy of
   the frame, the full path n of each; `chunks_coded` records the counts.
2. --kernels-only: the clipped split (k = 2, 4, 8, with and without a base) on --slots x --slot-mib MiB slots, each clipped by 7 bytes at both
   ends, alternating in one process with the whole-block split of the same bytes (its yardstick), both through bz3_hip_debug_patch.  Kernel times
   come from `rocprofv3 --kernel-trace --stats -f csv -d DIR -o update -- python tools/update_probe.py --kernels-only`, then
   `python tools/update_probe.py --from-trace DIR/.../update_kernel_trace.csv`, which assigns the trace's dispatches of the three segment kernels to
   the variants in launch order and adds bytes per second to --out under "kernels".
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

NO_BASE = 2 ** 64 - 1
CLIP = 7
# (name, kernel, yardstick, element size, base)
VARIANTS = [(f"split{k}", "k_move_segments", None, k, 0) for k in (2, 4, 8)]
VARIANTS += [(f"delta_split{k}", "k_delta_segments", None, k, 1) for k in (2, 4, 8)]
VARIANTS += [(f"clip_split{k}", "k_patch_segments", f"split{k}", k, 0) for k in (2, 4, 8)]
VARIANTS += [(f"clip_delta_split{k}", "k_patch_segments", f"delta_split{k}", k, 1) for k in (2, 4, 8)]
KERNELS = ("k_move_segments", "k_delta_segments", "k_patch_segments")


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
    for name, kernel, yard, _, has_base in VARIANTS:
        v = times[name]
        clip = 2 * CLIP if yard else 0
        moved = (3 if has_base else 2) * slots * (slot_bytes - clip)  # bytes read and written: source (and base) and slot
        e = {"kernel": kernel, "kernel_ms": [round(x, 4) for x in v], "best_ms": round(min(v), 4), "worst_ms": round(max(v), 4),
             "tb_per_s_best": round(moved / (min(v) * 1e-3) / 1e12, 3), "tb_per_s_worst": round(moved / (max(v) * 1e-3) / 1e12, 3)}
        if yard:
            y = times[yard]
            e.update({"yardstick": yard, "worst_over_yardstick_best": round(max(v) / min(y), 3), "best_over_yardstick_best": round(min(v) / min(y), 3),
                      "yardstick_spread": round(max(y) / min(y) - 1, 4)})
        res[name] = e
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["kernels"] = {"slots": slots, "slot_bytes": slot_bytes, "clip_bytes_each_end": CLIP, "source": "rocprofv3 --kernel-trace, run of its own", "kernels": res}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["kernels"]))


def kernel_probe(lib, slots, slot_bytes, repeats):
    import torch

    room = slots * (slot_bytes + 256) + 64
    src = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")
    base = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(room, dtype=torch.uint8, device="cuda:0")
    at = [i * (slot_bytes + 256) for i in range(slots)]
    calls = {}
    for name, _, yard, k, has_base in VARIANTS:
        a, b = (CLIP, slot_bytes - CLIP) if yard else (0, slot_bytes)
        t = (C.c_uint64 * (7 * slots))(*[v for o in at for v in (o + a, o + a + 2 if has_base else NO_BASE, o, slot_bytes, k, a, b)])
        calls[name] = (lambda t=t: lib.bz3_hip_debug_patch(src.data_ptr(), base.data_ptr(), dst.data_ptr(), t, slots))
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


def _coded(start, v, per_block, chunks):
    """The chunks an update of rows [start, start + v) decodes and encodes, and the full path's, from the definition in bz3_hip.h."""
    first, last = start // per_block, (start + v - 1) // per_block
    cut = {first} if start % per_block else set()
    if (start + v) % per_block:
        cut.add(last)
    return {"update_decodes": len(cut), "update_encodes": last - first + 1, "full_path_decodes": chunks, "full_path_encodes": chunks}


def frame_probe(lib, dtype, chunks, block_bytes, repeats):
    import torch

    dt = getattr(torch, dtype)
    es = torch.empty(0, dtype=dt).element_size()
    cols = 4096
    per_block = block_bytes // (cols * es)  # rows in a block
    rows = chunks * per_block - 3  # a short last block
    g = torch.Generator(device="cuda:0").manual_seed(chunks + es)
    x = (torch.randn(rows, cols, generator=g, device="cuda:0") * 0.02).to(dt)
    p = bzip3_amd.pack_tensor(x, block_bytes, lib=lib)
    n_chunks = int.from_bytes(bytes(p.frame[9:13].cpu().numpy()), "little")
    assert n_chunks == chunks and p.block_size == block_bytes, (n_chunks, p.block_size)
    start = (chunks // 3) * per_block + per_block // 2  # an interior row in the middle of a chunk
    spans = {"1_row": 1, "1_block": per_block, "8_blocks": 8 * per_block}
    spans = {k: v for k, v in spans.items() if start + v + per_block < rows}
    values = {k: (torch.randn(v, cols, generator=g, device="cuda:0") * 0.02).to(dt) for k, v in spans.items()}
    out = {"dtype": dtype, "planes": p.planes, "chunks": chunks, "block_bytes": block_bytes, "input_bytes": p.nbytes, "frame_bytes": p.frame.numel(), "row_bytes": cols * es,
           "data": "N(0, 0.02)", "chunks_coded": {k: _coded(start, v, per_block, chunks) for k, v in spans.items()}}
    t = {f"{path}_{k}": [] for k in spans for path in ("update", "full_path")}
    for rep in range(repeats + 1):  # the first round warms up and checks
        frames = {}
        for name in t:
            path, k = name.split("_", 1) if name.startswith("update") else ("full_path", name[len("full_path_") :])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if path == "update":
                q = bzip3_amd.update_tensor_rows(p, start, values[k], lib=lib)
            else:
                y = bzip3_amd.unpack_tensor(p, lib=lib)
                y[start : start + spans[k]] = values[k]
                q = bzip3_amd.pack_tensor(y, block_bytes, planes=p.planes, lib=lib, checksum=False)
                del y
            torch.cuda.synchronize()
            dt_s = time.perf_counter() - t0
            print(f"{dtype} {chunks} chunks, round {rep}: {name} {dt_s:.3f} s", file=sys.stderr, flush=True)
            if rep:
                t[name].append(dt_s)
            else:
                frames[name] = q.frame
            del q
        for k in spans if not rep else ():
            assert torch.equal(frames[f"update_{k}"], frames[f"full_path_{k}"]), ("the update's frame is not the full path's", dtype, chunks, k)
    out["times"] = {k: _stats(v) for k, v in t.items()}
    out["full_over_update_median"] = {k: round(out["times"][f"full_path_{k}"]["median_s"] / out["times"][f"update_{k}"]["median_s"], 2) for k in spans}
    out["full_best_over_update_worst"] = {k: round(out["times"][f"full_path_{k}"]["best_s"] / out["times"][f"update_{k}"]["worst_s"], 2) for k in spans}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunks", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--block-mib", type=int, default=16)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--slot-mib", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--from-trace", help="a rocprofv3 kernel trace (csv) of a --kernels-only run: add its kernel times to --out and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_probe.json"))
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace, a.slots, a.slot_mib << 20, a.repeats, a.out)
    lib = bzip3_amd.load()
    if a.kernels_only:  # (the times that count are the trace's: the wall clock around the hooks is printed, not recorded)
        print(json.dumps({"kernels_host_wall_clock": kernel_probe(lib, a.slots, a.slot_mib << 20, a.repeats)}))
        return
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["frames"] = [frame_probe(lib, d, c, a.block_mib << 20, a.repeats) for d in a.dtypes for c in a.chunks]
    doc["repeats"] = a.repeats
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
