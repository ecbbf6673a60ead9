#!/usr/bin/env python3
"""Measurements behind the resize ("Resize"), in the manner of tools/update_probe.py and tools/update_select_probe.py.

(a) Default, profiler off: float32 tensors of N(0, 0.02) with 256 columns (rows of 1 KiB) whose frames have --chunks chunks of --block-mib MiB (a short last
    one).  append_tensor_rows of r rows, r such that the appended bytes are 1 KiB, one chunk and eight chunks, against the path a user has
    without it on the same library: unpack_tensor, torch.cat, pack_tensor(checksum=False).  Then a dict of --dict-tensors tensors of
    --dict-chunks chunks each: append_state_dict_rows of 1 KiB per tensor against unpack_state_dict, torch.cat, pack_state_dict.  The two paths
    alternate in one process, --repeats times after a warm-up round in which their frames are checked equal.
(b) --kernels-only: the replane segment through bz3_hip_debug_replane against k_copy_segments moving the same bytes through
    bz3_hip_debug_copy_segments (its yardstick), on --slots x --slot-mib MiB slots that keep all but 1000 bytes and grow by 4 KiB + 3 bytes, at
    k = 2, 4, 8, alternating after a warm-up round.  Kernel times come from
    `rocprofv3 --kernel-trace --stats -f csv -d DIR -o resize -- python tools/resize_probe.py --kernels-only`, then
    `python tools/resize_probe.py --from-trace DIR/.../resize_kernel_trace.csv`, which assigns the trace's dispatches of the two kernels to the
    variants in launch order and adds them to --out under "kernels".  Without a trace the wall clock around the hooks is printed, not recorded.
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

COLS = 256  # a row of float32 is 1 KiB
KERNELS = ("k_copy_segments", "k_replane_segments")
VARIANTS = [(f"{kind}_k{k}", kernel, k) for k in (2, 4, 8) for kind, kernel in (("copy", "k_copy_segments"), ("replane", "k_replane_segments"))]


def _stats(v):
    return {"s": [round(x, 5) for x in v], "median_s": round(statistics.median(v), 5), "best_s": round(min(v), 5), "worst_s": round(max(v), 5)}


def _timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _tensor(torch, chunks, block_bytes, seed):
    per_block = block_bytes // (COLS * 4)  # rows in a block
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    return torch.randn(chunks * per_block - 3, COLS, generator=g, device="cuda:0") * 0.02  # a short last block


def frame_probe(lib, chunks, block_bytes, repeats):
    import torch

    x = _tensor(torch, chunks, block_bytes, chunks)
    p = bzip3_amd.pack_tensor(x, block_bytes, lib=lib)
    assert p.block_size == block_bytes and int.from_bytes(bytes(p.frame[9:13].cpu().numpy()), "little") == chunks
    row = COLS * 4
    widths = {"1KiB": max(1, 1024 // row), "one_chunk": block_bytes // row, "eight_chunks": 8 * block_bytes // row}
    g = torch.Generator(device="cuda:0").manual_seed(7)
    out = {"dtype": "float32", "planes": p.planes, "chunks": chunks, "block_bytes": block_bytes, "input_bytes": p.nbytes, "frame_bytes": p.frame.numel(), "data": "N(0, 0.02)",
           "rows_appended": widths, "times": {}}
    for name, rows in widths.items():
        values = torch.randn(rows, COLS, generator=g, device="cuda:0") * 0.02
        t = {"append": [], "full_path": []}

        def full():
            y = torch.cat([bzip3_amd.unpack_tensor(p, lib=lib), values])
            return bzip3_amd.pack_tensor(y, block_bytes, planes=p.planes, lib=lib, checksum=False)

        for rep in range(repeats + 1):  # the first round warms up and checks
            da, qa = _timed(torch, lambda: bzip3_amd.append_tensor_rows(p, values, lib=lib))
            df, qf = _timed(torch, full)
            print(f"{chunks} chunks, + {name}, round {rep}: append {da:.3f} s, full path {df:.3f} s", file=sys.stderr, flush=True)
            if rep:
                t["append"].append(da)
                t["full_path"].append(df)
            else:
                assert qa.block_size == qf.block_size and torch.equal(qa.frame, qf.frame), ("the frames differ", chunks, name)
            del qa, qf
        out["times"][name] = {k: _stats(v) for k, v in t.items()}
        out["times"][name]["full_over_append_median"] = round(statistics.median(t["full_path"]) / statistics.median(t["append"]), 2)
    return out


def dict_probe(lib, tensors, chunks, block_bytes, repeats):
    import torch

    sd = {f"t{i}": _tensor(torch, chunks, block_bytes, 1000 + i) for i in range(tensors)}
    packed = bzip3_amd.pack_state_dict(sd, block_bytes, lib=lib)
    g = torch.Generator(device="cuda:0").manual_seed(8)
    rows = {k: torch.randn(max(1, 1024 // (COLS * 4)), COLS, generator=g, device="cuda:0") * 0.02 for k in sd}
    t = {"append": [], "full_path": []}

    def full():
        back = bzip3_amd.unpack_state_dict(packed, lib=lib)
        return bzip3_amd.pack_state_dict({k: torch.cat([back[k], rows[k]]) for k in back}, block_bytes, lib=lib, checksum=False)

    for rep in range(repeats + 1):
        da, qa = _timed(torch, lambda: bzip3_amd.append_state_dict_rows(packed, rows, lib=lib))
        df, qf = _timed(torch, full)
        print(f"dict of {tensors} x {chunks} chunks, round {rep}: append {da:.3f} s, full path {df:.3f} s", file=sys.stderr, flush=True)
        if rep:
            t["append"].append(da)
            t["full_path"].append(df)
        else:
            assert all(torch.equal(qa[k].frame, qf[k].frame) for k in sd), "the frames differ"
        del qa, qf
    res = {"tensors": tensors, "chunks_each": chunks, "block_bytes": block_bytes, "rows_appended_each": next(iter(rows.values())).shape[0], "times": {k: _stats(v) for k, v in t.items()}}
    res["full_over_append_median"] = round(statistics.median(t["full_path"]) / statistics.median(t["append"]), 2)
    return res


def kernel_probe(lib, slots, slot_bytes, repeats):
    import torch

    grown = slot_bytes + 4096 + 3
    room = slots * (grown + 256) + 64
    src = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")
    dst = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")
    at = [i * (grown + 256) for i in range(slots)]
    a = slot_bytes - 1000
    calls = {}
    for name, kernel, k in VARIANTS:
        if kernel == "k_copy_segments":  # the same k runs of a / k bytes, as plain segments
            m, mn = slot_bytes // k, grown // k
            t = (C.c_uint64 * (3 * slots * k))(*[v for o in at for q in range(k) for v in (o + 1 + q * m, o + 5 + q * mn, a // k)])
            calls[name] = (lambda t=t, k=k: lib.bz3_hip_debug_copy_segments(src.data_ptr(), dst.data_ptr(), t, slots * k))
        else:
            t = (C.c_uint64 * (6 * slots))(*[v for o in at for v in (o + 1, o + 5, slot_bytes, grown, k, a)])
            calls[name] = (lambda t=t: lib.bz3_hip_debug_replane(src.data_ptr(), dst.data_ptr(), t, slots))
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


def from_trace(path, slots, slot_bytes, repeats, out):
    import csv

    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    order = [(rep - 1, v) for rep in range(repeats + 1) for v in VARIANTS]
    assert len(rows) == len(order), (len(rows), len(order))
    times = {}
    for r, (rep, (name, kernel, _)) in zip(rows, order):
        assert kernel in r["Kernel_Name"], (r["Kernel_Name"], name)
        if rep >= 0:
            times.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    res = {}
    for name, kernel, k in VARIANTS:
        v = times[name]
        moved = slots * (slot_bytes - 1000) // k * k
        e = {"kernel": kernel, "kernel_ms": [round(x, 4) for x in v], "best_ms": round(min(v), 4), "worst_ms": round(max(v), 4), "bytes_moved": moved,
             "ps_per_byte_best": round(min(v) * 1e9 / moved, 3), "ps_per_byte_worst": round(max(v) * 1e9 / moved, 3)}
        if kernel == "k_replane_segments":
            y = times[f"copy_k{k}"]
            e.update({"yardstick": f"copy_k{k}", "worst_over_yardstick_best": round(max(v) / min(y), 3), "best_over_yardstick_best": round(min(v) / min(y), 3),
                      "yardstick_spread": round(max(y) / min(y) - 1, 4)})
        res[name] = e
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["kernels"] = {"slots": slots, "slot_bytes": slot_bytes, "source": "rocprofv3 --kernel-trace, run of its own", "kernels": res}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["kernels"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunks", default="16,256")
    ap.add_argument("--block-mib", type=int, default=16)
    ap.add_argument("--dict-tensors", type=int, default=256)
    ap.add_argument("--dict-chunks", type=int, default=16)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--slot-mib", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--from-trace", help="a rocprofv3 kernel trace (csv) of a --kernels-only run: add its kernel times to --out and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_probe.json"))
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace, a.slots, a.slot_mib << 20, a.repeats, a.out)
    lib = bzip3_amd.load()
    if a.kernels_only:  # (the times that count are the trace's: the wall clock around the hooks is printed, not recorded)
        print(json.dumps({"kernels_host_wall_clock": kernel_probe(lib, a.slots, a.slot_mib << 20, a.repeats)}))
        return
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["frames"] = [frame_probe(lib, int(c), a.block_mib << 20, a.repeats) for c in a.chunks.split(",")]
    if a.dict_tensors:
        doc["dict"] = dict_probe(lib, a.dict_tensors, a.dict_chunks, a.block_mib << 20, a.repeats)
    doc["repeats"] = a.repeats
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
