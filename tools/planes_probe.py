#!/usr/bin/env python3
"""Measurements behind the byte-plane frames ("Typed tensors"); one JSON file.

1. The split / merge kernel (planes.hpp k_move_segments) against the plain segment copy (frame.hpp k_copy_segments) on the same
   window of --slots x --slot-mib MiB, user side aligned and misaligned by 7 bytes, alternating, --repeats times after a warm-up.
   Times are host wall-clock around the test hooks (bz3_hip_debug_copy_segments / bz3_hip_debug_planes: a table upload, one launch,
   one synchronisation), so they include a launch's fixed cost.  Kernel times alone: run
   `rocprofv3 --kernel-trace --stats -f csv -d DIR -o planes -- python tools/planes_probe.py --kernels-only`, then
   `python tools/planes_probe.py --from-trace DIR/planes_kernel_trace.csv`, which assigns the trace's dispatches of the two segment
   kernels to the variants in launch order (the order is fixed: see kernel_order).  Bytes moved = 2 x window bytes.
2. End to end: pack_state_dict + unpack_state_dict (default planes) against compress_tensors + decompress_tensors (planes=1) on the
   same dict of --tensors fp32 N(0, 0.02) tensors of --slot-mib MiB, with the frame sizes of both.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bzip3_amd  # noqa: E402


VARIANTS = ["copy_in", "copy_out"] + [f"{d}{k}" for k in (2, 4, 8) for d in ("split", "merge")]
SHIFTS = (0, 7)


def kernel_order(repeats):
    """The launches of kernel_probe in order: (user shift, repeat or -1 for the warm-up round, variant)."""
    return [(shift, rep - 1, name) for shift in SHIFTS for rep in range(repeats + 1) for name in VARIANTS]


def from_trace(path, slots, slot_bytes, repeats, out):
    """Kernel times of a --kernels-only run from rocprofv3's kernel trace (csv)."""
    import csv

    rows = [r for r in csv.DictReader(open(path)) if "k_copy_segments" in r["Kernel_Name"] or "k_move_segments" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    order = kernel_order(repeats)
    assert len(rows) == len(order), (len(rows), len(order))
    moved = 2 * slots * slot_bytes
    res = {}
    for r, (shift, rep, name) in zip(rows, order):
        assert ("k_copy_segments" in r["Kernel_Name"]) == name.startswith("copy"), (r["Kernel_Name"], name)
        if rep >= 0:
            res.setdefault(f"user_shift_{shift}", {}).setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    res = {sh: {name: {"kernel_ms": [round(x, 4) for x in v], "best_ms": round(min(v), 4), "worst_ms": round(max(v), 4), "tb_per_s_best": round(moved / (min(v) * 1e-3) / 1e12, 3)}
                for name, v in d.items()} for sh, d in res.items()}
    res = {"slots": slots, "slot_bytes": slot_bytes, "source": "rocprofv3 --kernel-trace, run of its own", "kernels": res}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def kernel_probe(lib, slots, slot_bytes, repeats):
    import torch

    room = slots * (slot_bytes + 256) + 64
    src = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(room, dtype=torch.uint8, device="cuda:0")
    res = {}
    for shift in SHIFTS:
        # split: user side (source) at `shift`, slots (destination) 256-byte aligned; merge: the mirror image
        user = [shift + i * (slot_bytes + 256) for i in range(slots)]
        slot = [i * (slot_bytes + 256) for i in range(slots)]
        variants = {"copy_in": (3, [(u, s, slot_bytes) for u, s in zip(user, slot)]), "copy_out": (3, [(s, u, slot_bytes) for u, s in zip(user, slot)])}
        for k in (2, 4, 8):
            variants[f"split{k}"] = (4, [(u, s, slot_bytes, k) for u, s in zip(user, slot)])
            variants[f"merge{k}"] = (4, [(s, u, slot_bytes, k | 0x100) for u, s in zip(user, slot)])
        assert list(variants) == VARIANTS
        tables = {name: (w, (C.c_uint64 * (w * slots))(*[v for seg in segs for v in seg])) for name, (w, segs) in variants.items()}
        times = {name: [] for name in tables}
        for rep in range(repeats + 1):  # the first round warms up
            for name, (w, t) in tables.items():
                fn = lib.bz3_hip_debug_copy_segments if w == 3 else lib.bz3_hip_debug_planes
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = fn(src.data_ptr(), dst.data_ptr(), t, slots)
                dt = time.perf_counter() - t0
                assert rc == 0, (name, rc)
                if rep:
                    times[name].append(dt)
        moved = 2 * slots * slot_bytes
        res[f"user_shift_{shift}"] = {name: {"ms": [round(1e3 * x, 4) for x in v], "best_ms": round(1e3 * min(v), 4), "tb_per_s_best": round(moved / min(v) / 1e12, 3)}
                                      for name, v in times.items()}
    return res


def dict_probe(tensors, tensor_bytes):
    import torch

    g = torch.Generator().manual_seed(1)
    sd = {f"w{i}": (torch.randn(tensor_bytes // 4, generator=g) * 0.02).to("cuda:0") for i in range(tensors)}
    raws = [v.view(torch.uint8) for v in sd.values()]
    bs = bzip3_amd._lossless_block_size(tensor_bytes, 16 << 20, 4)
    out = {"tensors": tensors, "tensor_bytes": tensor_bytes, "block_size": bs}
    for rep in range(2):  # the first round warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        packed = bzip3_amd.pack_state_dict(sd, 16 << 20)
        t1 = time.perf_counter()
        back = bzip3_amd.unpack_state_dict(packed)
        t2 = time.perf_counter()
        frames = bzip3_amd.compress_tensors(raws, bs, planes=1)
        t3 = time.perf_counter()
        plain = bzip3_amd.decompress_tensors(frames, planes=1)
        t4 = time.perf_counter()
    assert all(torch.equal(back[k], sd[k]) for k in sd) and all(torch.equal(a, b) for a, b in zip(plain, raws))
    total = tensors * tensor_bytes
    out["planes"] = {"pack_s": round(t1 - t0, 3), "unpack_s": round(t2 - t1, 3), "frame_bytes": sum(p.frame.numel() for p in packed.values()),
                     "ratio": round(sum(p.frame.numel() for p in packed.values()) / total, 4)}
    out["interleaved"] = {"compress_s": round(t3 - t2, 3), "decompress_s": round(t4 - t3, 3), "frame_bytes": sum(f.numel() for f in frames),
                          "ratio": round(sum(f.numel() for f in frames) / total, 4)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--slot-mib", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tensors", type=int, default=256)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--from-trace", help="a rocprofv3 kernel trace (csv) of a --kernels-only run: write its kernel times to --out and exit")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "planes_probe.json"))
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace, a.slots, a.slot_mib << 20, a.repeats, a.out)
    lib = bzip3_amd.load()
    res = {"slots": a.slots, "slot_bytes": a.slot_mib << 20, "kernels": kernel_probe(lib, a.slots, a.slot_mib << 20, a.repeats)}
    if not a.kernels_only:
        res["state_dict"] = dict_probe(a.tensors, a.slot_mib << 20)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
