"""The encoder's front end at the benchmark's shape, with the forward BWT's run length forced and left to the rule (api_encode.hip encode_group
sends the blocks of a window through bwt_forward_batch in runs of bwt_batch_size's choosing; bz3_hip_debug_set_bwt_batch forces the length).
One batch of `blocks` text blocks of `MiB` each is encoded in device memory `trials` times under every setting given (-1 = the rule), the
settings alternating.  --duo=0,1 alternates the two-thread front end the same way (bz3_hip_set_front_end_duo; -1 = the library's default), inside
every run-length setting.  Prints t_enc, the CM launch and what is left (the front end and the finish) per trial.  Device memory as in
tools/tail_pipe_probe.py.  A build without the hook (--lib=<older build>) takes the setting "none" only.
    python tools/front_pipe_probe.py [MiB=8] [blocks=768] [--batch=1,-1] [--duo=-1] [--trials=3] [--lib=<another build>] [--emu]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import bzip3_amd  # noqa: E402
import datagen  # noqa: E402
from tail_pipe_probe import HipMem, HostMem  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = {a[2:].split("=")[0]: (a.split("=", 1)[1] if "=" in a else "1") for a in sys.argv[1:] if a.startswith("--")}
    emu = "emu" in opt
    mib = float(args[0]) if args else 8.0
    nblk = int(args[1]) if len(args) > 1 else 768
    trials = int(opt.get("trials", "3"))
    if emu:
        sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
        from build_emu import build as build_emu

        lib = bzip3_amd.load(build_emu())
        mem = HostMem()
    else:
        if "lib" in opt:
            bzip3_amd._share_hip_runtime_with_torch()
            lib = bzip3_amd.load(opt["lib"])
        else:
            lib = bzip3_amd.load()
        assert lib.bz3_hip_device_count() > 0
        mem = HipMem()
    hook = hasattr(lib, "bz3_hip_debug_set_bwt_batch")
    settings = [int(x) for x in opt.get("batch", "1,-1").split(",")] if hook else [None]
    duos = [int(x) for x in opt["duo"].split(",")] if "duo" in opt else [None]
    lib.bz3_hip_bind_device(0)
    lib.bz3_hip_set_lean_states(1)
    bs = int(mib * (1 << 20))
    cap = lib.bz3_bound(bs) + 4096
    base = np.frombuffer(datagen.text(bs, seed=1, noise=0.0 if emu else datagen.ENWIK_NOISE), dtype=np.uint8)
    bufs = [mem.alloc(cap) for _ in range(nblk)]
    states = (C.c_void_p * nblk)(*[lib.bz3_new(bs) for _ in range(nblk)])
    assert all(states)
    ptrs = (C.c_void_p * nblk)(*bufs)
    tm = (C.c_float * 8)()
    first = None

    def encode(setting, duo=None):
        nonlocal first
        for k in range(nblk):
            mem.h2d(bufs[k], np.roll(base, k * 4099))
        mem.sync()
        if setting is not None:
            lib.bz3_hip_debug_set_bwt_batch(setting)
        if duo is not None:
            lib.bz3_hip_set_front_end_duo(duo)
        sizes = (C.c_int32 * nblk)(*[bs] * nblk)
        t0 = time.perf_counter()
        lib.bz3_hip_encode_blocks_device(states, ptrs, sizes, nblk)
        t = time.perf_counter() - t0
        assert min(sizes) > 0
        if first is None:
            first = list(sizes)
        assert list(sizes) == first, "coded sizes differ between settings"
        lib.bz3_hip_last_timings(states[0], tm)
        cm = tm[bzip3_amd.T_NAMES.index("cm")] * 1e-3
        ring = lib.bz3_hip_debug_front_end_ring()
        return {"batch": "none" if setting is None else setting, "duo": "lib" if duo is None else duo, "two_threads": (ring >> 29) & 1, "t_enc_s": round(t, 3), "cm_s": round(cm, 3), "front_s": round(t - cm, 3),
                "bwt_ms_block0": round(tm[bzip3_amd.T_NAMES.index("bwt")], 3)}

    encode(settings[0], duos[-1])  # warm-up: allocations (the two-thread form's arena is the larger one)
    for _ in range(trials):
        for s in settings:
            for d in duos:
                print(json.dumps(encode(s, d)), flush=True)
    if duos != [None]:
        lib.bz3_hip_set_front_end_duo(-1)
    if hook:
        lib.bz3_hip_debug_set_bwt_batch(-1)


if __name__ == "__main__":
    main()
