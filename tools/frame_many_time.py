"""Times the batched frame calls (bz3_hip_compress_device_many / bz3_hip_decompress_device_many through bzip3_amd.compress_tensors /
decompress_tensors) against a loop of single-frame calls (compress_tensor / decompress_tensor) over the same tensors and against one
single frame of the same total bytes, for three shapes:

    many_1m    256 x 1 MiB text, single-block frames (block size 16 MiB > the tensor: each frame's block size is bz3_bound(1 MiB))
    many_64k   1024 x 64 KiB text, the effective block size falls to 65 KiB
    few_64m    16 x 64 MiB text at 8 MiB blocks, 128 blocks (each frame's last chunk is the empty one of src/libbz3.c:914)

    python tools/frame_many_time.py --shapes many_1m,many_64k,few_64m --json profiles/frame_many_time.json

A loop of single-frame calls costs one CM launch per frame (minutes for 256 frames), so the loop is timed over the first
frames of a shape given in SHAPES (--loop-frames caps it) and its full time is that mean per frame times the frame count (`loop_*_s_est`; the number timed is
recorded).  The library is loaded before torch is imported (bzip3_amd.load() shares torch's HIP runtime).  Results are merged into
--json, one key per shape."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bzip3_amd  # noqa: E402

LIB = bzip3_amd.load()
import torch  # noqa: E402

# frames, bytes per frame, block size of the batch, block size of the one frame, frames of the timed loop
SHAPES = {"many_1m": (256, 1 << 20, 16 << 20, 1 << 20, 16), "many_64k": (1024, 64 << 10, 16 << 20, 65 << 10, 64),
          "few_64m": (16, 64 << 20, 8 << 20, 8 << 20, 2)}


def text_bytes(nbytes):
    import datagen

    t = datagen.shakespeare()
    return (t * (nbytes // len(t) + 1))[:nbytes]


def kept(nbytes, bs):
    """Bytes a frame of nbytes at block size bs decodes to: an exact multiple of the (effective) block size loses its last block to
    the empty last chunk of src/libbz3.c:914."""
    if bs > nbytes:
        return nbytes
    return nbytes if nbytes % bs else nbytes - bs


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def step(name, a):
    n, per, bs_batch, bs_one, k = SHAPES[name]
    data = text_bytes(n * per + 4096)[: n * per]
    x = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    xs = [x[i * per : (i + 1) * per] for i in range(n)]
    mib = len(data) / 2**20
    res = {"frames": n, "frame_bytes": per, "block_size": bs_batch, "one_frame_block_size": bs_one, "input_mib": mib, "runs": []}
    k = min(k, a.loop_frames)
    for rep in range(a.reps):
        LIB.bz3_hip_debug_cm_launches(1)
        tb_c, frames = wall(lambda: bzip3_amd.compress_tensors(xs, bs_batch))
        cm_c = LIB.bz3_hip_debug_cm_launches(1)
        tb_d, backs = wall(lambda: bzip3_amd.decompress_tensors(frames))
        cm_d = LIB.bz3_hip_debug_cm_launches(1)
        assert all(torch.equal(b, xi[: kept(per, bs_batch)]) for b, xi in zip(backs, xs)), "batched round trip differs"
        tl_c, singles = wall(lambda: [bzip3_amd.compress_tensor(xs[i], bs_batch) for i in range(k)])
        assert all(torch.equal(s, f) for s, f in zip(singles, frames)), "batched frame differs from the single-frame call"
        tl_d, _ = wall(lambda: [bzip3_amd.decompress_tensor(frames[i]) for i in range(k)])
        to_c, one = wall(lambda: bzip3_amd.compress_tensor(x, bs_one))
        to_d, back = wall(lambda: bzip3_amd.decompress_tensor(one))
        assert torch.equal(back, x[: kept(x.numel(), bs_one)])
        run = {"batch_compress_s": tb_c, "batch_decompress_s": tb_d, "batch_cm_launches_compress": cm_c, "batch_cm_launches_decompress": cm_d,
               "loop_frames_timed": k, "loop_compress_s_est": tl_c / k * n, "loop_decompress_s_est": tl_d / k * n,
               "one_frame_compress_s": to_c, "one_frame_decompress_s": to_d,
               "batch_frame_bytes": sum(f.numel() for f in frames), "one_frame_bytes": one.numel()}
        res["runs"].append(run)
        print("%s rep %d: batch %.3f / %.3f s (%d / %d CM launches); loop (est. from %d) %.2f / %.2f s; one frame %.3f / %.3f s  [compress / decompress]"
              % (name, rep, tb_c, tb_d, cm_c, cm_d, k, run["loop_compress_s_est"], run["loop_decompress_s_est"], to_c, to_d), flush=True)
        del frames, backs, singles, one, back
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--loop-frames", type=int, default=1 << 30)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "frame_many_time.json"))
    a = ap.parse_args()
    out = {}
    if os.path.exists(a.json):
        with open(a.json) as f:
            out = json.load(f)
    out["device"] = torch.cuda.get_device_name(0)
    for name in a.shapes.split(","):
        out[name] = step(name, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
