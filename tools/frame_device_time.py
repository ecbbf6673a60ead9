"""Times the device-resident frame API (bz3_hip_compress_device / bz3_hip_decompress_device through bzip3_amd.compress_tensor /
decompress_tensor) against the host path a torch user has without it (.cpu() + bz3_compress, bz3_decompress + .to(device)),
the segment copy kernel against a torch device-to-device copy of the same bytes, and the chunk-header walk per chunk.

    python tools/frame_device_time.py --steps frame,copy,walk --blocks 256 --block-mib 8 --json out.json

One process; the library is loaded (bzip3_amd.load(), which shares torch's HIP runtime without importing torch) before torch is
imported.  Each step can be run on its own (--steps) so that a job script can put a time limit on each.  Results are merged into
--json (one object, one key per step)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bzip3_amd  # noqa: E402

LIB = bzip3_amd.load()
import numpy as np  # noqa: E402
import torch  # noqa: E402


def text_batch(nbytes):
    import datagen

    t = datagen.shakespeare()
    return (t * (nbytes // len(t) + 1))[:nbytes]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def step_frame(a):
    bs = a.block_mib << 20
    data = text_batch(a.blocks * bs - 4096)  # not an exact multiple: the reference's frame would drop the last block (src/libbz3.c:914)
    mib = len(data) / 2**20
    x = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")

    def host_compress():
        h = x.cpu().numpy()
        out = np.empty(LIB.bz3_bound(h.size), dtype=np.uint8)
        osz = C.c_size_t(out.size)
        assert LIB.bz3_compress(bs, h.ctypes.data, out.ctypes.data, h.size, C.byref(osz)) == 0
        return torch.from_numpy(out[: osz.value]).to("cuda:0")

    def host_decompress(frame):
        f = frame.cpu().numpy()
        out = np.empty(len(data), dtype=np.uint8)
        osz = C.c_size_t(out.size)
        assert LIB.bz3_decompress(f.ctypes.data, out.ctypes.data, f.size, C.byref(osz)) == 0
        return torch.from_numpy(out[: osz.value]).to("cuda:0")

    res = {"blocks": a.blocks, "block_bytes": bs, "input_mib": mib, "runs": []}
    for rep in range(a.reps):  # alternate the two paths: the host is shared with other work
        td_c, fd = wall(lambda: bzip3_amd.compress_tensor(x, bs))
        th_c, fh = wall(host_compress)
        assert torch.equal(fd, fh), "device and host frames differ"
        td_d, bd = wall(lambda: bzip3_amd.decompress_tensor(fd))
        th_d, bh = wall(lambda: host_decompress(fh))
        assert torch.equal(bd, x) and torch.equal(bh, x)
        run = {"device_compress_s": td_c, "host_compress_s": th_c, "device_decompress_s": td_d, "host_decompress_s": th_d,
               "frame_bytes": fd.numel()}
        res["runs"].append(run)
        print("frame rep %d: compress device %.3f s (%.1f MiB/s) host %.3f s (%.1f MiB/s); decompress device %.3f s (%.1f MiB/s) host %.3f s (%.1f MiB/s)"
              % (rep, td_c, mib / td_c, th_c, mib / th_c, td_d, mib / td_d, th_d, mib / th_d), flush=True)
        del fd, fh, bd, bh
    return res


def copy_call(src, dst, table):
    t = (C.c_uint64 * len(table))(*table)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    assert LIB.bz3_hip_debug_copy_segments(src.data_ptr(), dst.data_ptr(), t, len(table) // 3) == 0
    return time.perf_counter() - t0


def step_copy(a):
    """Each call copies ~2 GiB.  The library call's wall time includes its table upload, a small hipMalloc and a stream: the time
    of a call that copies 16 bytes is reported beside it and subtracted in the *_net figures."""
    total = 2 << 30
    src = torch.randint(0, 256, (total + (1 << 20),), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)
    reps = 5
    empty = min(copy_call(src, dst, [0, 0, 16]) for _ in range(20))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def torch_copy(n_bytes):
        best = 1e9
        for _ in range(reps):
            ev0.record()
            dst[:n_bytes].copy_(src[:n_bytes])
            ev1.record()
            ev1.synchronize()
            best = min(best, ev0.elapsed_time(ev1) / 1e3)
        return best

    def layout(seg, count, s_align, d_align, stride_pad=4096):
        table, so, do = [], 0, 0
        for _ in range(count):
            so += (s_align - (src.data_ptr() + so)) % 16
            do += (d_align - (dst.data_ptr() + do)) % 16
            table += [so, do, seg]
            so += seg + stride_pad
            do += seg + stride_pad
        assert so <= src.numel() and do <= dst.numel()
        return table

    res = {"empty_call_s": empty, "torch_copy_2GiB_s": torch_copy(total), "slots_8MiB": [], "chunks_65KiB": None}
    seg8 = 8 << 20
    n8 = total // (seg8 + 4096 + 32)
    for s_al, d_al in [(s, 0) for s in range(16)] + [(0, d) for d in range(1, 16)] + [(5, 11), (13, 7)]:
        tab = layout(seg8, n8, s_al, d_al)
        t = min(copy_call(src, dst, tab) for _ in range(reps))
        nbytes = seg8 * n8
        res["slots_8MiB"].append({"src_mod16": s_al, "dst_mod16": d_al, "bytes": nbytes, "call_s": t, "GBps_net": nbytes / max(t - empty, 1e-9) / 1e9})
        print("copy 8 MiB x %d src%%16=%2d dst%%16=%2d: %.3f ms  %.0f GB/s net of the empty call" % (n8, s_al, d_al, t * 1e3, nbytes / max(t - empty, 1e-9) / 1e9), flush=True)
    rng = np.random.default_rng(5)
    seg = 65 * 1024
    n = total // (seg + 64 + 16)
    table, so, do = [], 0, 0
    for _ in range(n):
        so += int(rng.integers(0, 16))
        do += int(rng.integers(0, 16))
        table += [so, do, seg]
        so += seg + 32
        do += seg + 32
    t = min(copy_call(src, dst, table) for _ in range(reps))
    res["chunks_65KiB"] = {"segments": n, "bytes": seg * n, "call_s": t, "GBps_net": seg * n / max(t - empty, 1e-9) / 1e9}
    res["torch_copy_GBps"] = total / res["torch_copy_2GiB_s"] / 1e9
    print("copy 65 KiB x %d random alignments: %.3f ms  %.0f GB/s net; torch copy_ of 2 GiB: %.3f ms  %.0f GB/s (bytes copied per second)"
          % (n, t * 1e3, res["chunks_65KiB"]["GBps_net"], res["torch_copy_2GiB_s"] * 1e3, res["torch_copy_GBps"]), flush=True)
    return res


def step_walk(a):
    """bz3_hip_frame_decoded_size_device over a frame of n empty chunks (a header walk and nothing else): time per chunk,
    read-backs (one per 256 chunks) included."""
    res = []
    for n in (256, 4096, 65536):
        frame = bytearray(b"BZ3v1") + (1 << 20).to_bytes(4, "little") + n.to_bytes(4, "little") + bytes(8 * n)
        f = torch.frombuffer(frame, dtype=torch.uint8).to("cuda:0")
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(3):
            size = C.c_size_t(0)
            t0 = time.perf_counter()
            assert LIB.bz3_hip_frame_decoded_size_device(f.data_ptr(), f.numel(), C.byref(size)) == 0
            best = min(best, time.perf_counter() - t0)
        res.append({"chunks": n, "call_s": best, "us_per_chunk": best / n * 1e6})
        print("walk %6d chunks: %.3f ms, %.2f us per chunk" % (n, best * 1e3, best / n * 1e6), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="frame,copy,walk")
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--block-mib", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert LIB.bz3_hip_device_count() > 0, "no HIP device: this tool measures the GPU and has no CPU mode"
    LIB.bz3_hip_bind_device(0)
    out = {}
    if a.json and os.path.exists(a.json):
        out = json.load(open(a.json))
    out["device"] = torch.cuda.get_device_name(0)
    for s in a.steps.split(","):
        out[s] = {"frame": step_frame, "copy": step_copy, "walk": step_walk}[s](a)
        if a.json:
            json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
