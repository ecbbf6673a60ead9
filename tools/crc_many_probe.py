#!/usr/bin/env python3
"""Measurements behind the batched checksum ("Checkpoint files and batched checksums"), in the manner of tools/delta_probe.py:
one process on one GPU, --repeats rounds after a warm-up round, the candidates alternating inside every round.

(a) crc32c_tensors against a loop of base_crc over 256 x 16 MiB and 1024 x 64 KiB uint8 tensors (views of one allocation, 7 bytes off
    a 16-byte boundary).  In this tree base_crc is the n = 1 case of the batched call; with --parent-lib the loop is also timed on the
    parent commit's library, whose single call fetches the head bytes to the host first.
(b) --kernels-only: the batched call on 256 x 16 MiB beside the block codec's crc32c_device on ONE buffer of the same 4 GiB (the single
    call of --parent-lib, else bz3_hip_stage_crc32c on host bytes).  Kernel times come from
    `rocprofv3 --kernel-trace --stats -f csv -d DIR -o crc -- python tools/crc_many_probe.py --kernels-only`, then
    `python tools/crc_many_probe.py --from-trace DIR/crc_kernel_trace.csv`.
(c) pack_state_dict + unpack_state_dict with a base on the 256 fp32 tensors of tools/delta_probe.py: this tree (content checksum
    recorded, one batched call per pack or unpack call) against --parent-lib driven as the parent commit drove it (no content checksum,
    one bz3_hip_crc32c_device call per tensor with a base).
Writes profiles/crc_many_probe.json; a part that was not run is recorded as "not measured"."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bzip3_amd  # noqa: E402

MiB = 1 << 20


def _summary(v):
    return {"s": [round(x, 5) for x in v], "best_s": round(min(v), 5), "worst_s": round(max(v), 5), "spread": round(max(v) / min(v) - 1, 4)}


def _timed(f):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def _views(count, size):
    import torch

    pitch = (size + 7 + 255) & ~255
    buf = torch.randint(0, 256, (count * pitch + 64,), dtype=torch.uint8, device="cuda:0")
    return buf, [buf[7 + i * pitch : 7 + i * pitch + size] for i in range(count)]


def part_a(repeats, parent):
    out = {}
    for count, size in ((256, 16 * MiB), (1024, 64 << 10)):
        buf, ts = _views(count, size)
        cands = {"crc32c_tensors": lambda: bzip3_amd.crc32c_tensors(ts), "loop_of_base_crc": lambda: [bzip3_amd.base_crc(t) for t in ts]}
        if parent is not None:
            cands["loop_of_base_crc_parent_lib"] = lambda: [bzip3_amd.base_crc(t, parent) for t in ts]
        times = {k: [] for k in cands}
        want = None
        for rep in range(repeats + 1):  # the first round warms up
            for k, f in cands.items():
                dt, got = _timed(f)
                want = got if want is None else want
                assert got == want, k
                if rep:
                    times[k].append(dt)
        e = {k: _summary(v) for k, v in times.items()}
        for k in e:
            e[k]["gb_per_s_best"] = round(count * size / e[k]["best_s"] / 1e9, 1)
        e["loop_best_over_batched_best"] = round(e["loop_of_base_crc"]["best_s"] / e["crc32c_tensors"]["best_s"], 2)
        out[f"{count}x{size}"] = e
        del buf, ts
    return out


def part_b(lib, repeats, parent):
    """Under rocprofv3: repeats + 1 rounds of (batched call on 256 x 16 MiB, the existing kernels on one 4 GiB buffer)."""
    import torch

    count, size = 256, 16 * MiB
    buf = torch.randint(0, 256, (count * size,), dtype=torch.uint8, device="cuda:0")
    ts = [buf[i * size : (i + 1) * size] for i in range(count)]
    host = None if parent is not None else buf.cpu().numpy().tobytes()
    crc = C.c_uint32(0)
    wall = {"batched": [], "single_buffer": []}
    for rep in range(repeats + 1):
        dt, _ = _timed(lambda: bzip3_amd.crc32c_tensors(ts))
        if parent is not None:
            du, rc = _timed(lambda: parent.bz3_hip_crc32c_device(C.c_void_p(buf.data_ptr()), buf.numel(), 1, C.byref(crc)))
            assert rc == 0
        else:
            du, _ = _timed(lambda: lib.bz3_hip_stage_crc32c(host, len(host), 1))
        if rep:
            wall["batched"].append(dt)
            wall["single_buffer"].append(du)
    return {"bytes": count * size, "single_buffer_through": "parent library's bz3_hip_crc32c_device" if parent is not None else "bz3_hip_stage_crc32c",
            "host_wall_clock_under_the_profiler": {k: _summary(v) for k, v in wall.items()}}


def from_trace(path, repeats, out_path):
    import csv

    rows = [r for r in csv.DictReader(open(path)) if "k_crc_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6  # noqa: E731
    per = {}
    for name in ("k_crc_many_segments", "k_crc_many_finish", "k_crc_segments", "k_crc_finish"):
        v = [ms(r) for r in rows if name in r["Kernel_Name"]]  # (neither name of the batched kernels contains one of the others)
        per[name] = v[-repeats:] if len(v) >= repeats else v  # the warm-up round comes first
    res = {"source": "rocprofv3 --kernel-trace, run of its own", "kernel_ms": {k: [round(x, 4) for x in v] for k, v in per.items()}}
    if per["k_crc_many_segments"] and per["k_crc_segments"]:
        new = [a + b for a, b in zip(per["k_crc_many_segments"], per["k_crc_many_finish"])]
        old = [a + b for a, b in zip(per["k_crc_segments"], per["k_crc_finish"])]
        bound = max(old) * 1.25
        res.update({"batched_ms": [round(x, 4) for x in new], "single_buffer_ms": [round(x, 4) for x in old], "yardstick_spread": round(max(old) / min(old) - 1, 4),
                    "bound_ms_yardstick_worst_plus_25_percent": round(bound, 4), "batched_worst_inside_the_bound": max(new) <= bound,
                    "batched_best_over_single_best": round(min(new) / min(old), 3)})
    merged = json.load(open(out_path)) if os.path.exists(out_path) else {}
    merged["b_kernels"] = res
    with open(out_path, "w") as f:
        json.dump(merged, f, indent=1)
    print(json.dumps(res))


def part_c(repeats, parent, tensors, tensor_bytes):
    import torch

    g = torch.Generator().manual_seed(1)
    base = {f"w{i}": (torch.randn(tensor_bytes // 4, generator=g) * 0.02).to("cuda:0") for i in range(tensors)}
    sd = {k: v + (torch.randn(v.numel(), generator=g) * 2e-5).to("cuda:0") for k, v in base.items()}
    batched = bzip3_amd.crc32c_tensors

    def loop(ts, inits=None, lib=None):  # what the parent commit did: one single call per tensor
        return [bzip3_amd.base_crc(t, lib) for t in ts]

    def this_tree():
        bzip3_amd.crc32c_tensors = batched
        a, packed = _timed(lambda: bzip3_amd.pack_state_dict(sd, 16 << 20, base=base))
        b, back = _timed(lambda: bzip3_amd.unpack_state_dict(packed, base=base))
        return a, b, packed, back

    def parent_lib():
        bzip3_amd.crc32c_tensors = loop
        try:
            a, packed = _timed(lambda: bzip3_amd.pack_state_dict(sd, 16 << 20, base=base, lib=parent, checksum=False))
            b, back = _timed(lambda: bzip3_amd.unpack_state_dict(packed, base=base, lib=parent))
        finally:
            bzip3_amd.crc32c_tensors = batched
        return a, b, packed, back

    cands = {"this_tree": this_tree}
    if parent is not None:
        cands["parent_lib"] = parent_lib
    times = {k: {"pack": [], "unpack": []} for k in cands}
    frames = {}
    for rep in range(repeats + 1):
        for k, f in cands.items():
            a, b, packed, back = f()
            assert all(torch.equal(back[n], sd[n]) for n in sd), k
            frames[k] = sum(p.frame.numel() for p in packed.values())
            if rep:
                times[k]["pack"].append(a)
                times[k]["unpack"].append(b)
            del packed, back
    out = {"tensors": tensors, "tensor_bytes": tensor_bytes, "frame_bytes": frames}
    for k, d in times.items():
        out[k] = {"pack": _summary(d["pack"]), "unpack": _summary(d["unpack"])}
    if parent is not None:
        for w in ("pack", "unpack"):
            out[f"{w}_this_best_over_parent_best"] = round(out["this_tree"][w]["best_s"] / out["parent_lib"][w]["best_s"], 4)
    else:
        out["parent_lib"] = "not measured"
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tensors", type=int, default=256)
    ap.add_argument("--tensor-mib", type=int, default=16)
    ap.add_argument("--parent-lib", help="libbzip3.so of the parent commit (tools/build_variant.py, or a build of a checkout of it)")
    ap.add_argument("--parts", default="ac", help="which of a, c to run (b is --kernels-only)")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--from-trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crc_many_probe.json"))
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace, a.repeats, a.out)
    lib = bzip3_amd.load()
    parent = bzip3_amd.load(a.parent_lib) if a.parent_lib else None
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.kernels_only:
        res["b_calls"] = part_b(lib, a.repeats, parent)
    else:
        if "a" in a.parts:
            res["a_tensors_against_loop"] = part_a(a.repeats, parent)
        if "c" in a.parts:
            res["c_state_dict"] = part_c(a.repeats, parent, a.tensors, a.tensor_mib << 20)
    for k in ("a_tensors_against_loop", "b_calls", "b_kernels", "c_state_dict"):
        res.setdefault(k, "not measured")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
