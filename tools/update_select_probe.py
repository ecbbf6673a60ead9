#!/usr/bin/env python3
"""Measurements behind the index update ("Index update"), in the manner of tools/update_probe.py and tools/select_probe.py.

(a) Default, profiler off: one float32 tensor of N(0, 0.02) with 4096 columns whose frame has --chunks chunks of --block-mib MiB (a short last one).
    update_tensor_index of --runs scattered runs of --run-rows rows each (dimension 0; `chunks_touched` records how many chunks they cut) and of a block of --cols columns (dimension 1, which cuts
    every chunk), against the two paths a user has without it on the same library: one update_tensor_rows call per run, chained (scattered rows
    alone: a run of a column block is no whole row), and unpack_tensor, index_copy_, pack_tensor(checksum=False).  The three alternate in one
    process, --repeats times after a warm-up round in which their frames are checked equal.
(b) --kernels-only: the select split through bz3_hip_debug_patch_select against the select merge moving the same bytes through
    bz3_hip_debug_select (its yardstick, the parent commit's kernel), on --slots x --slot-mib MiB slots with uniform piece tables of 64 pieces per
    period that want every second piece-length of the chunk; piece lengths 1, 4, 16, 64 and 4096 elements at k = 2, 4, 8, with and without a base,
    alternating after a warm-up round.  Kernel times come from
    `rocprofv3 --kernel-trace --stats -f csv -d DIR -o usel -- python tools/update_select_probe.py --kernels-only`, then
    `python tools/update_select_probe.py --from-trace DIR/.../usel_kernel_trace.csv`, which assigns the trace's dispatches of the two kernels to the
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

NO_BASE = 2 ** 64 - 1
PIECES = 64
LENGTHS = (1, 4, 16, 64, 4096)
# (name, kernel, yardstick, element size, base, piece length in elements, inverse)
VARIANTS = []
for _k in (2, 4, 8):
    for _b in (0, 1):
        for _pl in LENGTHS:
            _tag = f"k{_k}_{'base' if _b else 'plain'}_{_pl}"
            VARIANTS.append((f"merge_{_tag}", "k_select_segments", None, _k, _b, _pl, 1))
            VARIANTS.append((f"split_{_tag}", "k_patch_select_segments", f"merge_{_tag}", _k, _b, _pl, 0))
KERNELS = ("k_select_segments", "k_patch_select_segments")


def _stats(v):
    return {"s": [round(x, 5) for x in v], "median_s": round(statistics.median(v), 5), "best_s": round(min(v), 5), "worst_s": round(max(v), 5)}


def _table(k, pl, slot_bytes):
    """(pieces, stride, nbytes): 64 pieces of pl elements, every second piece-length of the period, as many whole periods as the slot holds."""
    pieces = [(2 * j * pl * k, pl * k) for j in range(PIECES)]
    stride = 2 * PIECES * pl * k
    return pieces, stride, (slot_bytes // stride) * PIECES * pl * k


def from_trace(path, slots, slot_bytes, repeats, out):
    import csv

    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Kernel_Name"] for k in KERNELS)]  # (neither name is a part of the other)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    order = [(rep - 1, v) for rep in range(repeats + 1) for v in VARIANTS]
    assert len(rows) == len(order), (len(rows), len(order))
    times = {}
    for r, (rep, (name, kernel, *_)) in zip(rows, order):
        assert kernel in r["Kernel_Name"], (r["Kernel_Name"], name)
        if rep >= 0:
            times.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    res = {}
    for name, kernel, yard, k, has_base, pl, _ in VARIANTS:
        v = times[name]
        moved = (3 if has_base else 2) * slots * _table(k, pl, slot_bytes)[2]  # bytes read and written: the contiguous side (and base) and the slot's share
        e = {"kernel": kernel, "kernel_ms": [round(x, 4) for x in v], "best_ms": round(min(v), 4), "worst_ms": round(max(v), 4),
             "gb_per_s_best": round(moved / (min(v) * 1e-3) / 1e9, 1), "gb_per_s_worst": round(moved / (max(v) * 1e-3) / 1e9, 1)}
        if yard:
            y = times[yard]
            e.update({"yardstick": yard, "worst_over_yardstick_best": round(max(v) / min(y), 3), "best_over_yardstick_best": round(min(v) / min(y), 3),
                      "yardstick_spread": round(max(y) / min(y) - 1, 4)})
        res[name] = e
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["kernels"] = {"slots": slots, "slot_bytes": slot_bytes, "pieces_per_period": PIECES, "source": "rocprofv3 --kernel-trace, run of its own", "kernels": res}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["kernels"]))


def kernel_probe(lib, slots, slot_bytes, repeats):
    import torch

    room = slots * (slot_bytes + 256) + 64
    planes = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")  # the slots: split form
    flat = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")  # the contiguous side
    base = torch.randint(0, 256, (room,), dtype=torch.uint8, device="cuda:0")
    at = [i * (slot_bytes + 256) for i in range(slots)]
    calls = {}
    for name, _, _, k, has_base, pl, inverse in VARIANTS:
        pieces, stride, nbytes = _table(k, pl, slot_bytes)
        pc = (C.c_uint64 * (2 * PIECES))(*[v for p in pieces for v in p])
        if inverse:
            t = (C.c_uint64 * (12 * slots))(*[v for o in at for v in (o, o + 2 if has_base else NO_BASE, o, slot_bytes, k | 0x100, 0, stride, 0, 0, nbytes, 0, PIECES)])
            calls[name] = (lambda t=t, pc=pc: lib.bz3_hip_debug_select(planes.data_ptr(), base.data_ptr(), flat.data_ptr(), t, slots, pc, PIECES))
        else:
            t = (C.c_uint64 * (12 * slots))(*[v for o in at for v in (o, o + 2 if has_base else NO_BASE, o, slot_bytes, k, 0, stride, 0, 0, nbytes, 0, PIECES)])
            calls[name] = (lambda t=t, pc=pc: lib.bz3_hip_debug_patch_select(flat.data_ptr(), base.data_ptr(), planes.data_ptr(), t, slots, pc, PIECES))
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


def frame_probe(lib, chunks, block_bytes, runs, run_rows, cols_block, repeats):
    import torch

    cols = 4096
    per_block = block_bytes // (cols * 4)  # rows in a block
    rows = chunks * per_block - 3  # a short last block
    g = torch.Generator(device="cuda:0").manual_seed(chunks)
    x = torch.randn(rows, cols, generator=g, device="cuda:0") * 0.02
    p = bzip3_amd.pack_tensor(x, block_bytes, lib=lib)
    n_chunks = int.from_bytes(bytes(p.frame[9:13].cpu().numpy()), "little")
    assert n_chunks == chunks and p.block_size == block_bytes, (n_chunks, p.block_size)
    starts = [(2 * i + 1) * rows // (2 * runs) for i in range(runs)]  # scattered over the whole tensor (with the defaults every run straddles a chunk boundary: two cut chunks per run)
    row_idx = [s + j for s in starts for j in range(run_rows)]
    col_idx = list(range(cols // 3, cols // 3 + cols_block))
    cases = {"scattered_rows": (0, row_idx, (torch.randn(len(row_idx), cols, generator=g, device="cuda:0") * 0.02)),
             "column_block": (1, col_idx, (torch.randn(rows, cols_block, generator=g, device="cuda:0") * 0.02))}
    touched = {"scattered_rows": len({r // per_block for r in row_idx}), "column_block": chunks}
    out = {"dtype": "float32", "planes": p.planes, "chunks": chunks, "block_bytes": block_bytes, "input_bytes": p.nbytes, "frame_bytes": p.frame.numel(), "data": "N(0, 0.02)",
           "runs": runs, "run_rows": run_rows, "column_block": cols_block, "chunks_touched": touched}
    names = ["index_scattered_rows", "chained_rows_scattered_rows", "full_path_scattered_rows", "index_column_block", "full_path_column_block"]
    t = {name: [] for name in names}
    for rep in range(repeats + 1):  # the first round warms up and checks
        frames = {}
        for name in names:
            path, case = next((pth, name[len(pth) + 1 :]) for pth in ("index", "chained_rows", "full_path") if name.startswith(pth + "_"))
            dim, idx, values = cases[case]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if path == "index":
                q = bzip3_amd.update_tensor_index(p, dim, idx, values, lib=lib)
            elif path == "chained_rows":
                q = p
                for i, s in enumerate(starts):
                    q = bzip3_amd.update_tensor_rows(q, s, values[i * run_rows : (i + 1) * run_rows], lib=lib)
            else:
                y = bzip3_amd.unpack_tensor(p, lib=lib)
                y.index_copy_(dim, torch.tensor(idx, device=y.device), values)
                q = bzip3_amd.pack_tensor(y, block_bytes, planes=p.planes, lib=lib, checksum=False)
                del y
            torch.cuda.synchronize()
            dt_s = time.perf_counter() - t0
            print(f"{chunks} chunks, round {rep}: {name} {dt_s:.3f} s", file=sys.stderr, flush=True)
            if rep:
                t[name].append(dt_s)
            else:
                frames[name] = q.frame.clone()
            del q
        if not rep:
            for name in names:
                case = "scattered_rows" if name.endswith("scattered_rows") else "column_block"
                assert torch.equal(frames[name], frames[f"full_path_{case}"]), ("the frames differ", name)
    out["times"] = {k: _stats(v) for k, v in t.items()}
    med = lambda n: out["times"][n]["median_s"]  # noqa: E731
    out["over_index_median"] = {"chained_rows_scattered_rows": round(med("chained_rows_scattered_rows") / med("index_scattered_rows"), 2),
                                "full_path_scattered_rows": round(med("full_path_scattered_rows") / med("index_scattered_rows"), 2),
                                "full_path_column_block": round(med("full_path_column_block") / med("index_column_block"), 2)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunks", type=int, default=16)
    ap.add_argument("--block-mib", type=int, default=4)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--run-rows", type=int, default=4)
    ap.add_argument("--cols", type=int, default=128)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--slot-mib", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--from-trace", help="a rocprofv3 kernel trace (csv) of a --kernels-only run: add its kernel times to --out and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_select_probe.json"))
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace, a.slots, a.slot_mib << 20, a.repeats, a.out)
    lib = bzip3_amd.load()
    if a.kernels_only:  # (the times that count are the trace's: the wall clock around the hooks is printed, not recorded)
        print(json.dumps({"kernels_host_wall_clock": kernel_probe(lib, a.slots, a.slot_mib << 20, a.repeats)}))
        return
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["frames"] = [frame_probe(lib, a.chunks, a.block_mib << 20, a.runs, a.run_rows, a.cols, a.repeats)]
    doc["repeats"] = a.repeats
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
