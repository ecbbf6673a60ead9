#!/usr/bin/env python3
"""The size table behind the delta frames ("Delta frames"), with the reference library alone (oracle/_ref/libbz3ref.so), on
the CPU: compressed / original for x and for D(x, base) = (x - base) mod 256 byte-wise, interleaved and split into byte planes per
block.  1 Mi seeded elements of N(0, 0.02) (the Adam `v` row: their squares), x = base + N(0, step) rounded to the dtype, blocks of
1 MiB - 4.  Prints a markdown table; --json FILE also writes the numbers."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle_lib import require_ref  # noqa: E402

N, BS, SIGMA = 1 << 20, (1 << 20) - 4, 0.02


def ratio(ref, data):
    out = (C.c_uint8 * (ref.bz3_bound(len(data)) + 64))()
    osz = C.c_size_t(len(out))
    assert ref.bz3_compress(BS, data, out, len(data), C.byref(osz)) == 0
    return osz.value / len(data)


def planes(raw, k):
    """S_k: split_k of every block of BS bytes (BS % k == 0 and len(raw) % BS != 0 here, so every block is whole elements but the last's tail)."""
    out = []
    for off in range(0, len(raw), BS):
        b = np.frombuffer(raw[off : off + BS], dtype=np.uint8)
        m = len(b) // k
        out.append(np.concatenate([b[: m * k].reshape(m, k).T.reshape(-1), b[m * k :]]))
    return np.concatenate(out).tobytes()


def as_bytes(a, dtype):
    if dtype == "bfloat16":  # round to nearest even from float32, as torch does
        u = a.astype("<f4").view("<u4").astype(np.uint64)
        return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype("<u2")).tobytes()
    return a.astype({"float32": "<f4", "float64": "<f8", "float16": "<f2"}[dtype]).tobytes()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json")
    a = ap.parse_args()
    ref = require_ref().lib
    rows = [(dt, st, False) for dt in ("float32", "float64", "bfloat16", "float16") for st in (1e-2, 1e-3, 1e-4)] + [("float32", 1e-3, True)]
    res = []
    print("| dtype, step | `x` interleaved | `x` byte planes | `D(x, base)` interleaved | `D` byte planes | planes / interleaved after `D` |")
    print("|---|---|---|---|---|---|")
    for dtype, step, squares in rows:
        rng = np.random.default_rng(2025)
        base = rng.standard_normal(N) * SIGMA
        x = base + rng.standard_normal(N) * (SIGMA * step)
        if squares:  # Adam's second moment: v' = 0.999 v + 0.001 g^2
            base, x = base ** 2, 0.999 * base ** 2 + 0.001 * (rng.standard_normal(N) * SIGMA) ** 2
        k = {"float32": 4, "float64": 8, "bfloat16": 2, "float16": 2}[dtype]
        xb, bb = as_bytes(x, dtype), as_bytes(base, dtype)
        d = ((np.frombuffer(xb, dtype=np.uint8).astype(np.int16) - np.frombuffer(bb, dtype=np.uint8)) % 256).astype(np.uint8).tobytes()
        r = [ratio(ref, xb), ratio(ref, planes(xb, k)), ratio(ref, d), ratio(ref, planes(d, k))]
        name = f"{dtype}, Adam `v` one step on" if squares else f"{dtype}, {step:g} sigma"
        res.append({"dtype": dtype, "step": step, "adam_v": squares, "k": k, "x": r[0], "x_planes": r[1], "d": r[2], "d_planes": r[3]})
        print(f"| {name} | {r[0]:.4f} | {r[1]:.4f} | {r[2]:.4f} | {r[3]:.4f} | {r[3] / r[2]:.3f} |", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"elements": N, "block_size": BS, "rows": res}, f, indent=1)


if __name__ == "__main__":
    main()
