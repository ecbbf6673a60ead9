"""The forward BWT alone through bz3_hip_debug_bwt_many with the run length forced: `count` text blocks of `MiB` each in one call, `reps` times per
forced length B (bz3_hip_debug_set_bwt_batch), the lengths alternating.  Prints per (MiB, B) the transform's wall time per BLOCK
(bz3_hip_stage_last_ms / count): every repetition and the median.  With --single (any build) the same blocks go one by one through
bz3_hip_stage_bwt instead -- the figure of a build without the hook, and of the metric's 256 MiB blocks.
    python tools/bwt_batch_probe.py <MiB> [count=4] [--batch=1,2,3,4] [--reps=5] [--single] [--lib=<another build>]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402  (first: shared HIP runtime)

import bzip3_amd  # noqa: E402
from bench import gen_text_device  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = {a[2:].split("=")[0]: (a.split("=", 1)[1] if "=" in a else "1") for a in sys.argv[1:] if a.startswith("--")}
    mib = float(args[0]) if args else 8.0
    count = int(args[1]) if len(args) > 1 else 4
    reps = int(opt.get("reps", "5"))
    n = int(mib * (1 << 20))
    lib = bzip3_amd.load(opt["lib"]) if "lib" in opt else bzip3_amd.load()
    g = bzip3_amd.StageApi(lib)
    blocks = [bytes(gen_text_device(torch, n, 7 + k, torch.device("cuda", 0)).cpu().numpy()) for k in range(count)]
    if "single" in opt or not hasattr(lib, "bz3_hip_debug_bwt_many"):
        ms = []
        for rep in range(reps + 1):
            t = 0.0
            for b in blocks:
                g.bwt(b)
                t += lib.bz3_hip_stage_last_ms()
            if rep:  # (the first repetition pays the workspace's first touch)
                ms.append(round(t / count, 3))
        print(json.dumps({"mib": mib, "form": "bz3_hip_stage_bwt", "ms_per_block": ms, "median": statistics.median(ms)}), flush=True)
        return
    batches = [int(x) for x in opt.get("batch", "1,2,3,4").split(",")]
    want = None
    ms = {b: [] for b in batches}
    for rep in range(reps + 1):
        for b in batches:
            lib.bz3_hip_debug_set_bwt_batch(b)
            rc, got = g.bwt_many(blocks)
            assert rc == 0
            want = want or got
            assert got == want, "output depends on the run length"
            if rep:
                ms[b].append(round(lib.bz3_hip_stage_last_ms() / count, 3))
    lib.bz3_hip_debug_set_bwt_batch(-1)
    for b in batches:
        print(json.dumps({"mib": mib, "B": b, "ms_per_block": ms[b], "median": statistics.median(ms[b])}), flush=True)


if __name__ == "__main__":
    main()
