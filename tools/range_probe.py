#!/usr/bin/env python3
"""Measurements behind the range calls ("Range decode"), in the manner of tools/delta_probe.py.

1. Default, profiler off: one frame of --blocks x --block-mib MiB of the benchmark's text (bench.py gen_text_piece at datagen.ENWIK_NOISE).
   decompress_tensor_range for 1, 16 and 64 chunks' worth of bytes at an interior offset, the full decompress_tensor and
   bz3_hip_frame_decoded_size_device (the same header walk, the yardstick of the fixed cost) on the same frame in one process,
   alternating, --repeats times after a warm-up round; every range is compared with the slice of the input.  The model to test is
   time = fixed + per_chunk * chunks: `fit` is the least-squares line through the medians.  Then the walk's skip rate: a range call at
   offset 0 on a frame of --empty empty chunks in front of one real chunk, against the same call on the real chunk's frame alone.
2. --kernels-only: the clipped merge (k = 2, 4, 8, with and without a base) on --slots x --slot-mib MiB slots, each clipped by 7 bytes
   at both ends, alternating in one process with the unclipped merge (its yardstick: the same bytes to within 14 per slot), the split
   and the plain copy, user side aligned and 7 bytes off.  Kernel times come from
   `rocprofv3 --kernel-trace --stats -f csv -d DIR -o range -- python tools/range_probe.py --kernels-only`, then
   `python tools/range_probe.py --from-trace DIR/range_kernel_trace.csv`, which assigns the trace's dispatches of the four segment
   kernels to the variants in launch order (fixed: see kernel_order) and adds them to --out under "kernels".
"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bzip3_amd  # noqa: E402

NO_BASE = 2 ** 64 - 1
CLIP = 7
# (name, kernel, yardstick, element size, base)
VARIANTS = [("copy_out", "k_copy_segments", None, 1, 0)]
VARIANTS += [(f"split{k}", "k_move_segments", None, k, 0) for k in (2, 4, 8)]
VARIANTS += [(f"merge{k}", "k_move_segments", None, k, 0) for k in (2, 4, 8)]
VARIANTS += [(f"delta_out{k}", "k_delta_segments", None, k, 1) for k in (2, 4, 8)]
VARIANTS += [(f"clip_merge{k}", "k_range_segments", f"merge{k}", k, 0) for k in (2, 4, 8)]
VARIANTS += [(f"clip_delta_out{k}", "k_range_segments", f"delta_out{k}", k, 1) for k in (2, 4, 8)]
SHIFTS = (0, 7)
KERNELS = ("k_copy_segments", "k_move_segments", "k_delta_segments", "k_range_segments")


def kernel_order(repeats):
    return [(shift, rep - 1, v) for shift in SHIFTS for rep in range(repeats + 1) for v in VARIANTS]


def from_trace(path, slots, slot_bytes, repeats, out):
    import csv

    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    order = kernel_order(repeats)
    assert len(rows) == len(order), (len(rows), len(order))
    times = {}
    for r, (shift, rep, (name, kernel, *_)) in zip(rows, order):
        assert kernel in r["Kernel_Name"], (r["Kernel_Name"], name)
        if rep >= 0:
            times.setdefault(f"user_shift_{shift}", {}).setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    res = {}
    for sh, d in times.items():
        res[sh] = {}
        for name, kernel, yard, _, has_base in VARIANTS:
            v = d[name]
            moved = (3 if has_base else 2) * slots * slot_bytes
            e = {"kernel": kernel, "kernel_ms": [round(x, 4) for x in v], "best_ms": round(min(v), 4), "worst_ms": round(max(v), 4),
                 "tb_per_s_best": round(moved / (min(v) * 1e-3) / 1e12, 3)}
            if yard:
                y = d[yard]
                e.update({"yardstick": yard, "worst_over_yardstick_best": round(max(v) / min(y), 3), "best_over_yardstick_best": round(min(v) / min(y), 3),
                          "yardstick_spread": round(max(y) / min(y) - 1, 4), "within_rule": max(v) / min(y) <= (max(y) / min(y)) * 1.25})
            res[sh][name] = e
    kernels = {"slots": slots, "slot_bytes": slot_bytes, "clip_bytes_each_end": CLIP, "source": "rocprofv3 --kernel-trace, run of its own", "kernels": res}
    old_path = os.path.join(ROOT, "profiles", "planes_probe_kernels.json")
    if os.path.exists(old_path):  # the existing kernels against the ranges recorded for them, each widened by its own spread on both sides
        old = json.load(open(old_path))
        if old.get("slots") == slots and old.get("slot_bytes") == slot_bytes:
            chk = {}
            for sh, d in old["kernels"].items():
                for name, o in d.items():
                    if name not in res.get(sh, {}):
                        continue
                    sp = o["worst_ms"] / o["best_ms"] - 1
                    lo, hi = o["best_ms"] * (1 - sp), o["worst_ms"] * (1 + sp)
                    n = res[sh][name]
                    chk[f"{sh}/{name}"] = {"recorded_range_ms": [round(lo, 4), round(hi, 4)], "now_ms": [n["best_ms"], n["worst_ms"]], "inside": lo <= n["best_ms"] and n["worst_ms"] <= hi}
            kernels["against_planes_probe_kernels"] = chk
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["kernels"] = kernels
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(kernels))


def kernel_probe(lib, slots, slot_bytes, repeats):
    import torch

    room = slots * (slot_bytes + 256) + 64
    src = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")
    base = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(room, dtype=torch.uint8, device="cuda:0")
    res = {}
    for shift in SHIFTS:
        user = [shift + i * (slot_bytes + 256) for i in range(slots)]
        slot = [i * (slot_bytes + 256) for i in range(slots)]
        ubase = [u + (2 if shift else 0) for u in user]
        calls = {}
        for name, _, yard, k, has_base in VARIANTS:
            if name.startswith("split"):
                t = (C.c_uint64 * (4 * slots))(*[v for u, s in zip(user, slot) for v in (u, s, slot_bytes, k)])
                calls[name] = (lambda t=t: lib.bz3_hip_debug_planes(src.data_ptr(), dst.data_ptr(), t, slots))
            else:
                a, b = (CLIP, slot_bytes - CLIP) if yard else (0, slot_bytes)
                t = (C.c_uint64 * (7 * slots))(*[v for u, ub, s in zip(user, ubase, slot) for v in (s, ub + a if has_base else NO_BASE, u + a, slot_bytes, k | 0x100, a, b)])
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
        res[f"user_shift_{shift}"] = {name: {"ms": [round(1e3 * x, 4) for x in v], "best_ms": round(1e3 * min(v), 4)} for name, v in times.items()}
    return res


def _stats(v):
    return {"s": [round(x, 5) for x in v], "median_s": round(statistics.median(v), 5), "best_s": round(min(v), 5), "worst_s": round(max(v), 5)}


def frame_probe(lib, blocks, block_bytes, repeats, chunk_counts=(1, 16, 64)):
    import torch

    import bench
    import datagen

    bench.seed_text_source(lib)
    piece = 128 << 20
    total = blocks * block_bytes - 12345  # a short last block, so that the byte API drops nothing
    x = torch.cat([bench.gen_text_piece(torch, min(piece, total - o), 7 + o // piece, "cuda:0", datagen.ENWIK_NOISE) for o in range(0, total, piece)])
    frame = bzip3_amd.compress_tensor(x, block_bytes).clone()
    out = {"blocks": blocks, "block_bytes": block_bytes, "input_bytes": total, "frame_bytes": frame.numel(), "text": "bench.py gen_text_piece, datagen.ENWIK_NOISE"}
    first = blocks // 3  # an interior offset, in the middle of a chunk
    spans = {n: (first * block_bytes + block_bytes // 2, n * block_bytes) for n in chunk_counts if n < blocks - first - 1}
    need = C.c_size_t(0)
    t = {"full": [], "decoded_size": [], **{f"range_{n}": [] for n in spans}}
    for rep in range(repeats + 1):  # the first round warms up
        for name in t:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "full":
                got, want = bzip3_amd.decompress_tensor(frame), x
            elif name == "decoded_size":
                assert lib.bz3_hip_frame_decoded_size_device(C.c_void_p(frame.data_ptr()), frame.numel(), C.byref(need)) == 0 and need.value == total
                got = want = None
            else:
                o, w = spans[int(name[6:])]
                got, want = bzip3_amd.decompress_tensor_range(frame, o, w), x[o : o + w]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert got is None or torch.equal(got, want), name
            if rep:
                t[name].append(dt)
            del got
    out["times"] = {k: _stats(v) for k, v in t.items()}
    # a range of n chunks' worth of bytes from the middle of a chunk touches n + 1 chunks
    pts = [(n + 1, out["times"][f"range_{n}"]["median_s"]) for n in spans] + [(blocks, out["times"]["full"]["median_s"])]
    mx, my = sum(p[0] for p in pts) / len(pts), sum(p[1] for p in pts) / len(pts)
    slope = sum((a - mx) * (b - my) for a, b in pts) / sum((a - mx) ** 2 for a, _ in pts)
    out["fit"] = {"points_chunks_decoded_median_s": pts, "per_chunk_s": round(slope, 6), "fixed_s": round(my - slope * mx, 6),
                  "residuals_s": [round(b - (my - slope * mx + slope * a), 6) for a, b in pts],
                  "walk_yardstick_median_s": out["times"]["decoded_size"]["median_s"]}
    return out


def skip_probe(lib, empty, repeats):
    import torch

    payload = torch.arange(3000, device="cuda:0").to(torch.uint8)
    one = bytes(bzip3_amd.compress_tensor(payload, 65 << 10).cpu().numpy())
    assert struct.unpack("<I", one[9:13])[0] == 1
    frames = {"one_chunk": one, "skipping": one[:9] + struct.pack("<I", empty + 1) + bytes(8 * empty) + one[13:]}
    t = {k: [] for k in frames}
    dev = {k: torch.frombuffer(bytearray(v), dtype=torch.uint8).to("cuda:0") for k, v in frames.items()}
    for rep in range(repeats + 1):
        for name, f in dev.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = bzip3_amd.decompress_tensor_range(f, 0, 3000)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert torch.equal(got, payload)
            if rep:
                t[name].append(dt)
    res = {"empty_chunks": empty, **{k: _stats(v) for k, v in t.items()}}
    res["us_per_skipped_chunk_median"] = round(1e6 * (res["skipping"]["median_s"] - res["one_chunk"]["median_s"]) / empty, 3)
    res["us_per_skipped_chunk_best_and_worst"] = [round(1e6 * (res["skipping"]["best_s"] - res["one_chunk"]["worst_s"]) / empty, 3),
                                                  round(1e6 * (res["skipping"]["worst_s"] - res["one_chunk"]["best_s"]) / empty, 3)]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--block-mib", type=int, default=8)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--slot-mib", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--empty", type=int, default=65536)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--from-trace", help="a rocprofv3 kernel trace (csv) of a --kernels-only run: add its kernel times to --out and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_probe.json"))
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace, a.slots, a.slot_mib << 20, a.repeats, a.out)
    lib = bzip3_amd.load()
    if a.kernels_only:  # (the times that count are the trace's: the wall clock around the hooks is printed, not recorded)
        print(json.dumps({"kernels_host_wall_clock": kernel_probe(lib, a.slots, a.slot_mib << 20, a.repeats)}))
        return
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["frame"] = frame_probe(lib, a.blocks, a.block_mib << 20, a.repeats)
    doc["walk_skip"] = skip_probe(lib, a.empty, a.repeats)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
