#!/usr/bin/env python3
"""Measurements behind the delta frames ("Delta frames"), in the manner of tools/planes_probe.py.

1. --kernels-only: every delta variant (k = 1, 2, 4, 8, in and out) of planes.hpp k_delta_segments on a window of --slots x --slot-mib
   MiB, the user side (source or destination, and the base) aligned and 7 bytes off, alternating in one process with the unchanged
   k_copy_segments, split and merge (the yardsticks), --repeats times after a warm-up round.  Kernel times come from
   `rocprofv3 --kernel-trace --stats -f csv -d DIR -o delta -- python tools/delta_probe.py --kernels-only`, then
   `python tools/delta_probe.py --from-trace DIR/delta_kernel_trace.csv`, which assigns the trace's dispatches of the three segment
   kernels to the variants in launch order (fixed: see kernel_order).  Bytes moved = 3 x window bytes for a delta variant, 2 x for a
   yardstick, so 1.5 x the yardstick's time is the floor of its delta variant.
2. Without --kernels-only, profiler off: pack_state_dict + unpack_state_dict of --tensors fp32 N(0, 0.02) tensors of --slot-mib MiB
   against a base at a step of 1e-3 sigma, beside the same calls without a base in the same process, second of two rounds; times and
   frame sizes.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bzip3_amd  # noqa: E402

NO_BASE = 2 ** 64 - 1
# (name, kernel, yardstick): the yardstick of a delta variant is the base-less launch that moves the same bytes the same way
VARIANTS = [("copy_in", "k_copy_segments", None), ("copy_out", "k_copy_segments", None)]
VARIANTS += [(f"{d}{k}", "k_move_segments", None) for k in (2, 4, 8) for d in ("split", "merge")]
VARIANTS += [(f"delta_{d}{k}", "k_delta_segments", ("copy_" + d) if k == 1 else (("split" if d == "in" else "merge") + str(k))) for k in (1, 2, 4, 8) for d in ("in", "out")]
SHIFTS = (0, 7)


def kernel_order(repeats):
    return [(shift, rep - 1, v) for shift in SHIFTS for rep in range(repeats + 1) for v in VARIANTS]


def from_trace(path, slots, slot_bytes, repeats, out):
    import csv

    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Kernel_Name"] for k in ("k_copy_segments", "k_move_segments", "k_delta_segments"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    order = kernel_order(repeats)
    assert len(rows) == len(order), (len(rows), len(order))
    times = {}
    for r, (shift, rep, (name, kernel, _)) in zip(rows, order):
        assert kernel in r["Kernel_Name"], (r["Kernel_Name"], name)
        if rep >= 0:
            times.setdefault(f"user_shift_{shift}", {}).setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    res = {}
    for sh, d in times.items():
        res[sh] = {}
        for name, kernel, yard in VARIANTS:
            v = d[name]
            moved = (3 if yard else 2) * slots * slot_bytes
            e = {"kernel": kernel, "kernel_ms": [round(x, 4) for x in v], "best_ms": round(min(v), 4), "worst_ms": round(max(v), 4),
                 "tb_per_s_best": round(moved / (min(v) * 1e-3) / 1e12, 3)}
            if yard:
                y = d[yard]
                e.update({"yardstick": yard, "worst_over_yardstick_best": round(max(v) / min(y), 3), "best_over_yardstick_best": round(min(v) / min(y), 3),
                          "yardstick_spread": round(max(y) / min(y) - 1, 4)})
            res[sh][name] = e
    res = {"slots": slots, "slot_bytes": slot_bytes, "source": "rocprofv3 --kernel-trace, run of its own", "kernels": res}
    # the planes-only variants share functions with the delta tiles: their times against the ranges recorded before the delta tiles existed,
    # each range widened by its own spread (worst / best - 1) on both sides
    old_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "planes_probe_kernels.json")
    if os.path.exists(old_path):
        old = json.load(open(old_path))
        if old.get("slots") == slots and old.get("slot_bytes") == slot_bytes:
            chk = {}
            for sh, d in old["kernels"].items():
                for name, o in d.items():
                    sp = o["worst_ms"] / o["best_ms"] - 1
                    lo, hi = o["best_ms"] * (1 - sp), o["worst_ms"] * (1 + sp)
                    n = res["kernels"][sh][name]
                    chk[f"{sh}/{name}"] = {"recorded_range_ms": [round(lo, 4), round(hi, 4)], "now_ms": [n["best_ms"], n["worst_ms"]],
                                           "inside": lo <= n["best_ms"] and n["worst_ms"] <= hi}
            res["against_planes_probe_kernels"] = chk
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def kernel_probe(lib, slots, slot_bytes, repeats):
    import torch

    room = slots * (slot_bytes + 256) + 64
    src = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")
    base = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(room, dtype=torch.uint8, device="cuda:0")
    res = {}
    for shift in SHIFTS:
        user = [shift + i * (slot_bytes + 256) for i in range(slots)]  # the caller's side and the base; the slots are 256-byte aligned
        slot = [i * (slot_bytes + 256) for i in range(slots)]
        ubase = [u + (2 if shift else 0) for u in user]  # the base: aligned with an aligned user side, else at an alignment of its own (9 mod 16)
        tables = {}
        for name, _, yard in VARIANTS:
            inward = name.endswith("_in") or name.startswith(("split", "delta_in"))
            k = int(name[-1]) if name[-1].isdigit() else 1
            mode = k | (0 if inward else 0x100)
            segs = [(u if inward else s, b if yard else NO_BASE, s if inward else u, slot_bytes, mode) for u, b, s in zip(user, ubase, slot)]
            tables[name] = (C.c_uint64 * (5 * slots))(*[v for seg in segs for v in seg])
        times = {name: [] for name in tables}
        for rep in range(repeats + 1):  # the first round warms up
            for name, t in tables.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = lib.bz3_hip_debug_delta(src.data_ptr(), base.data_ptr(), dst.data_ptr(), t, slots)
                dt = time.perf_counter() - t0
                assert rc == 0, (name, rc)
                if rep:
                    times[name].append(dt)
        res[f"user_shift_{shift}"] = {name: {"ms": [round(1e3 * x, 4) for x in v], "best_ms": round(1e3 * min(v), 4)} for name, v in times.items()}
    return res


def reference_sizes(sd, base, packed, plain, count):
    """The first `count` tensors' frames against the reference library on the same bytes (S(D(x, b)) and S(x) on the host): sizes must be equal."""
    import numpy as np

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from oracle_lib import require_ref

    ref = require_ref().lib

    def ref_size(raw, bs, k):
        parts = []
        for off in range(0, len(raw), bs):
            b = raw[off : off + bs]
            m = len(b) // k
            parts.append(np.concatenate([b[: m * k].reshape(m, k).T.reshape(-1), b[m * k :]]))
        data = np.concatenate(parts).tobytes()
        dst = (C.c_uint8 * (ref.bz3_bound(len(data)) + 64))()
        osz = C.c_size_t(len(dst))
        assert ref.bz3_compress(bs, data, dst, len(data), C.byref(osz)) == 0
        return osz.value

    done = []
    for name in list(sd)[:count]:
        x, b = sd[name].cpu().numpy().view(np.uint8), base[name].cpu().numpy().view(np.uint8)
        d = (x.astype(np.int16) - b).astype(np.uint8)
        got = (packed[name].frame.numel(), plain[name].frame.numel())
        want = (ref_size(d, packed[name].block_size, packed[name].planes), ref_size(x, plain[name].block_size, plain[name].planes))
        assert got == want, (name, got, want)
        done.append({"tensor": name, "delta_frame_bytes": got[0], "no_base_frame_bytes": got[1]})
    return done


def dict_probe(tensors, tensor_bytes, ref_check=4):
    import torch

    g = torch.Generator().manual_seed(1)
    base = {f"w{i}": (torch.randn(tensor_bytes // 4, generator=g) * 0.02).to("cuda:0") for i in range(tensors)}
    sd = {k: v + (torch.randn(v.numel(), generator=g) * 2e-5).to("cuda:0") for k, v in base.items()}
    out = {"tensors": tensors, "tensor_bytes": tensor_bytes, "step_sigma": 1e-3}
    for rep in range(2):  # the first round warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        packed = bzip3_amd.pack_state_dict(sd, 16 << 20, base=base)
        t1 = time.perf_counter()
        back = bzip3_amd.unpack_state_dict(packed, base=base)
        t2 = time.perf_counter()
        plain = bzip3_amd.pack_state_dict(sd, 16 << 20)
        t3 = time.perf_counter()
        pback = bzip3_amd.unpack_state_dict(plain)
        t4 = time.perf_counter()
    assert all(torch.equal(back[k], sd[k]) and torch.equal(pback[k], sd[k]) for k in sd)
    out["reference_sizes_checked"] = reference_sizes(sd, base, packed, plain, ref_check)
    total = tensors * tensor_bytes
    for name, ps, a, b in (("delta", packed, t1 - t0, t2 - t1), ("no_base", plain, t3 - t2, t4 - t3)):
        n = sum(p.frame.numel() for p in ps.values())
        out[name] = {"pack_s": round(a, 3), "unpack_s": round(b, 3), "planes": next(iter(ps.values())).planes, "frame_bytes": n, "ratio": round(n / total, 4),
                     "first_frame_bytes": next(iter(ps.values())).frame.numel()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--slot-mib", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tensors", type=int, default=256)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--from-trace", help="a rocprofv3 kernel trace (csv) of a --kernels-only run: write its kernel times to --out and exit")
    ap.add_argument("--out", help="default: profiles/delta_probe.json (end to end), profiles/delta_probe_kernels.json (--from-trace), "
                                  "profiles/delta_probe_wall.json (--kernels-only: host wall-clock around the hooks)")
    a = ap.parse_args()
    if not a.out:
        name = "delta_probe_kernels.json" if a.from_trace else "delta_probe_wall.json" if a.kernels_only else "delta_probe.json"
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", name)
    if a.from_trace:
        return from_trace(a.from_trace, a.slots, a.slot_mib << 20, a.repeats, a.out)
    lib = bzip3_amd.load()
    res = {"slots": a.slots, "slot_bytes": a.slot_mib << 20}
    if a.kernels_only:
        res["kernels_host_wall_clock"] = kernel_probe(lib, a.slots, a.slot_mib << 20, a.repeats)
    else:
        res["state_dict"] = dict_probe(a.tensors, a.slot_mib << 20)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
