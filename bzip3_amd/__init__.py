"""bzip3_amd -- MI355X-native bzip3 block codec behind the libbz3.h C ABI.

The product is `bzip3_amd/lib/libbzip3.so` (hand-written HIP kernels for gfx950, built by
`bzip3_amd/build.py`).  This module is only the Python-side loader / thin mirror of the C API used by
the tests and bench.py; it contains no compute and NO fallback: if the shared object is missing or no
HIP device is usable, it raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libbzip3.so")

BZ3_OK = 0
BZ3_ERR_OUT_OF_BOUNDS = -1
BZ3_ERR_BWT = -2
BZ3_ERR_CRC = -3
BZ3_ERR_MALFORMED_HEADER = -4
BZ3_ERR_TRUNCATED_DATA = -5
BZ3_ERR_DATA_TOO_BIG = -6
BZ3_ERR_INIT = -7
BZ3_ERR_DATA_SIZE_TOO_SMALL = -8

T_NAMES = ["crc", "rle", "lzp", "bwt", "cm", "copy", "_6", "_7"]

_lib = None


def _declare(L, strict=True):
    vp, i32, u32, sz = C.c_void_p, C.c_int32, C.c_uint32, C.c_size_t
    sig = {
        "bz3_version": (C.c_char_p, []),
        "bz3_last_error": (C.c_int8, [vp]),
        "bz3_strerror": (C.c_char_p, [vp]),
        "bz3_new": (vp, [i32]),
        "bz3_free": (None, [vp]),
        "bz3_bound": (sz, [sz]),
        "bz3_compress": (C.c_int, [u32, vp, vp, sz, C.POINTER(sz)]),
        "bz3_decompress": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
        "bz3_min_memory_needed": (sz, [i32]),
        "bz3_encode_block": (i32, [vp, vp, i32]),
        "bz3_decode_block": (i32, [vp, vp, sz, i32, i32]),
        "bz3_encode_blocks": (None, [vp, vp, vp, i32]),
        "bz3_decode_blocks": (None, [vp, vp, vp, vp, vp, i32]),
        "bz3_orig_size_sufficient_for_decode": (C.c_int, [vp, sz, i32]),
        # bz3_hip.h
        "bz3_hip_device_count": (C.c_int, []),
        "bz3_hip_bind_device": (C.c_int, [C.c_int]),
        "bz3_hip_state_device": (C.c_int, [vp]),
        "bz3_hip_set_cm_mode": (C.c_int, [C.c_int]),
        "bz3_hip_cm_blocks_given_up": (C.c_uint, []),
        "bz3_hip_cm_blocks_routed_full": (C.c_uint, []),
        "bz3_hip_debug_bwt_big_rounds": (None, [C.c_int]),
        "bz3_hip_debug_peak_concurrent_groups": (C.c_int, [C.c_int]),
        "bz3_hip_debug_front_end_ring": (C.c_int, []),
        "bz3_hip_debug_arena_swap_buffers": (C.c_int, [C.c_int]),
        "bz3_hip_cm_variant_for": (C.c_int, [C.c_int, C.c_int, C.c_int]),
        "bz3_hip_set_lean_states": (C.c_int, [C.c_int]),
        "bz3_hip_release_cached_memory": (None, []),
        "bz3_hip_set_keep_workspace": (C.c_int, [C.c_int]),
        "bz3_hip_set_front_end_duo": (C.c_int, [C.c_int]),
        "bz3_hip_set_workspace_headroom": (None, [C.c_longlong]),
        "bz3_hip_workspace_headroom": (sz, []),
        "bz3_hip_debug_headroom_events": (C.c_uint, [C.c_int, C.POINTER(C.c_uint)]),
        "bz3_hip_debug_ring_contexts": (sz, [sz, sz, sz, sz, sz, sz, C.c_int, sz]),
        "bz3_hip_debug_arena_slack": (sz, [sz]),
        "bz3_hip_debug_cm_launches": (C.c_uint, [C.c_int]),
        "bz3_hip_debug_workspace_bytes": (sz, [sz, C.c_int]),
        "bz3_hip_debug_cached_bytes": (sz, [C.c_int]),
        "bz3_hip_encode_block_device": (i32, [vp, vp, i32]),
        "bz3_hip_decode_block_device": (i32, [vp, vp, sz, i32, i32]),
        "bz3_hip_encode_blocks_device": (None, [vp, vp, vp, i32]),
        "bz3_hip_decode_blocks_device": (None, [vp, vp, vp, vp, vp, i32]),
        "bz3_hip_compress_device": (C.c_int, [u32, vp, vp, sz, C.POINTER(sz)]),
        "bz3_hip_decompress_device": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
        "bz3_hip_frame_decoded_size_device": (C.c_int, [vp, sz, C.POINTER(sz)]),
        "bz3_hip_compress_device_many": (C.c_int, [u32, i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_decompress_device_many": (C.c_int, [i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_frame_decoded_sizes_device": (C.c_int, [i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_debug_copy_segments": (i32, [vp, vp, C.POINTER(C.c_uint64), i32]),
        "bz3_hip_last_timings": (None, [vp, C.POINTER(C.c_float)]),
        "bz3_hip_last_bwt_stats": (None, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_uint64)]),
        "bz3_hip_stage_crc32c": (u32, [vp, sz, u32]),
        "bz3_hip_stage_mrle_encode": (i32, [vp, i32, vp]),
        "bz3_hip_stage_mrle_decode": (C.c_int, [vp, vp, i32, i32]),
        "bz3_hip_stage_lzp_encode": (i32, [vp, i32, vp]),
        "bz3_hip_stage_lzp_decode": (i32, [vp, i32, vp, i32]),
        "bz3_hip_stage_bwt": (i32, [vp, vp, i32]),
        "bz3_hip_stage_unbwt": (i32, [vp, vp, i32, i32]),
        "bz3_hip_stage_last_ms": (C.c_float, []),
        "bz3_hip_debug_sort_u32": (i32, [vp, u32, C.c_int, C.c_int, vp, vp]),
        "bz3_hip_debug_scan_u32": (i32, [vp, u32, vp]),
        "bz3_hip_debug_cu_masks": (i32, [C.c_int, C.c_int, vp, vp]),
        "bz3_hip_set_collect_window_us": (None, [C.c_int]),
        "bz3_hip_debug_collected_batches": (C.c_uint, [C.c_int, C.POINTER(C.c_uint)]),
        "bz3_hip_stage_cm_encode": (i32, [vp, i32, vp]),
        "bz3_hip_stage_cm_decode": (None, [vp, i32, vp, i32]),
        "bz3_hip_stage_cm_decode_many": (C.c_float, [vp, i32, vp, i32, i32, vp]),
        "bz3_hip_stage_cm_encode_many": (C.c_float, [vp, i32, vp, C.POINTER(i32), i32]),
        "bz3_hip_encode_stream": (C.c_int, [C.c_int, C.c_int, i32, i32]),
        "bz3_hip_decode_stream": (C.c_int, [C.c_int, C.c_int, i32]),
    }
    for name, (res, args) in sig.items():
        if not strict and not hasattr(L, name):  # an OLDER build loaded for a same-box A/B (load(path)): symbols added since are absent
            continue
        fn = getattr(L, name)  # AttributeError here = the library does not export what include/*.h declares
        fn.restype = res
        fn.argtypes = args
    return L


EXPORTED_SYMBOLS = None


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.7; two HIP runtimes in one process do not both see
    the GPU.  If torch is installed, load ITS runtime first (without importing torch) so that libbzip3.so --
    which only asks for the soname libamdhip64.so.7 -- and a later `import torch` share one runtime.
    Set BZ3_HIP_SYSTEM_RUNTIME=1 to keep the system ROCm runtime instead."""
    if os.environ.get("BZ3_HIP_SYSTEM_RUNTIME") == "1":
        return
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def load(path=None):
    """Load libbzip3.so (building nothing, falling back to nothing)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    if path is None:
        _share_hip_runtime_with_torch()
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} is missing: the HIP extension has not been built (python -m bzip3_amd.build). "
            "bzip3_amd has no CPU or PyTorch fallback by design."
        )
    L = _declare(C.CDLL(p), strict=path is None)
    if path is None:
        _lib = L
    return L


def _cbuf(data, cap):
    cap = max(1, cap)
    if len(data) == cap:
        return (C.c_uint8 * cap).from_buffer_copy(data)
    buf = (C.c_uint8 * cap)()
    if len(data):
        C.memmove(buf, data if isinstance(data, bytes) else bytes(data), len(data))
    return buf


class StageApi:
    """Per-stage hooks on host buffers (bz3_hip_stage_*), same call shapes as the CPU checker used by the tests."""

    def __init__(self, lib=None):
        self.lib = lib or load()

    def crc32c(self, data, init=1):
        return self.lib.bz3_hip_stage_crc32c(_cbuf(data, len(data)), len(data), init)

    def mrle_encode(self, data):
        out = (C.c_uint8 * (len(data) + 64))()
        n = self.lib.bz3_hip_stage_mrle_encode(_cbuf(data, len(data)), len(data), out)
        return C.string_at(out, n)

    def mrle_decode(self, data, outlen, maxin=None):
        maxin = len(data) if maxin is None else maxin
        out = (C.c_uint8 * max(1, outlen))()
        rc = self.lib.bz3_hip_stage_mrle_decode(_cbuf(data, len(data)), out, outlen, maxin)
        return rc, C.string_at(out, outlen)

    def lzp_encode(self, data):
        out = (C.c_uint8 * (len(data) + 64))()
        n = self.lib.bz3_hip_stage_lzp_encode(_cbuf(data, len(data)), len(data), out)
        return n, (C.string_at(out, n) if n > 0 else b"")

    def lzp_decode(self, data, maxout):
        out = (C.c_uint8 * max(8, maxout))()
        n = self.lib.bz3_hip_stage_lzp_decode(_cbuf(data, len(data)), len(data), out, maxout)
        return n, (C.string_at(out, n) if n > 0 else b"")

    def bwt(self, data):
        out = (C.c_uint8 * max(1, len(data)))()
        idx = self.lib.bz3_hip_stage_bwt(_cbuf(data, len(data)), out, len(data))
        return idx, C.string_at(out, len(data))

    def unbwt(self, data, idx):
        out = (C.c_uint8 * max(1, len(data)))()
        rc = self.lib.bz3_hip_stage_unbwt(_cbuf(data, len(data)), out, len(data), idx)
        return rc, C.string_at(out, len(data))

    def cm_encode(self, data):
        out = (C.c_uint8 * (len(data) + len(data) // 50 + 64))()
        n = self.lib.bz3_hip_stage_cm_encode(_cbuf(data, len(data)), len(data), out)
        return C.string_at(out, n)

    def cm_decode(self, data, n):
        out = (C.c_uint8 * max(1, n))()
        self.lib.bz3_hip_stage_cm_decode(_cbuf(data, len(data)), len(data), out, n)
        return C.string_at(out, n)


class State:
    """RAII wrapper of `struct bz3_state` (bz3_new / bz3_free)."""

    def __init__(self, block_size, lib=None):
        self.lib = lib or load()
        self.block_size = block_size
        self.ptr = self.lib.bz3_new(block_size)
        if not self.ptr:
            raise RuntimeError(f"bz3_new({block_size}) returned NULL (invalid size, no HIP device, or out of device memory)")

    def close(self):
        if self.ptr:
            self.lib.bz3_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def last_error(self):
        return self.lib.bz3_last_error(self.ptr)

    def strerror(self):
        return self.lib.bz3_strerror(self.ptr).decode()

    def timings(self):
        t = (C.c_float * 8)()
        self.lib.bz3_hip_last_timings(self.ptr, t)
        return {T_NAMES[i]: t[i] for i in range(6)}

    def bwt_stats(self):
        r, p, e = C.c_int32(), C.c_int32(), C.c_uint64()
        self.lib.bz3_hip_last_bwt_stats(self.ptr, C.byref(r), C.byref(p), C.byref(e))
        return {"rounds": r.value, "radix_passes": p.value, "sorted_elements": e.value}

    # host-buffer API ------------------------------------------------------------------------
    def encode_block(self, data):
        cap = self.lib.bz3_bound(max(len(data), self.block_size)) + 64
        buf = _cbuf(data, cap)
        n = self.lib.bz3_encode_block(self.ptr, buf, len(data))
        return n, self.last_error, (C.string_at(buf, n) if n > 0 else b"")

    def decode_block(self, data, orig_size, buffer_size=None, comp_size=None):
        cap = self.lib.bz3_bound(self.block_size) + 64
        buffer_size = cap if buffer_size is None else buffer_size
        comp_size = len(data) if comp_size is None else comp_size
        buf = _cbuf(data, max(cap, buffer_size, len(data) + 1))
        n = self.lib.bz3_decode_block(self.ptr, buf, buffer_size, comp_size, orig_size)
        return n, self.last_error, (C.string_at(buf, n) if n > 0 else b"")


def encode_block(data, block_size, lib=None):
    with State(block_size, lib) as st:
        return st.encode_block(data)


def decode_block(data, orig_size, block_size, lib=None, **kw):
    with State(block_size, lib) as st:
        return st.decode_block(data, orig_size, **kw)


class Bz3Error(RuntimeError):
    """A libbz3 call returned an error code: `.code` is the BZ3_ERR_* value; `.out` (decompress_tensor only) the bytes the call
    committed before the error, as a view of the output tensor.  The batched calls (compress_tensors / decompress_tensors) also set
    `.index` (the lowest failing frame, whose code `.code` is), `.codes` (every frame's code) and `.outs` (per frame, a view of the
    bytes the call committed for it)."""

    def __init__(self, code, what, out=None, index=None, codes=None, outs=None):
        super().__init__(f"{what} failed with {code} ({_ERR_NAMES.get(code, 'unknown error')})" + ("" if index is None else f" at frame {index}"))
        self.code = code
        self.out = out
        self.index = index
        self.codes = codes
        self.outs = outs


_ERR_NAMES = {v: k for k, v in globals().items() if k.startswith("BZ3_ERR_")}


def _device_u8(x, what):
    import torch

    if not isinstance(x, torch.Tensor) or x.device.type != "cuda" or x.dtype != torch.uint8 or not x.is_contiguous():
        raise TypeError(f"{what} must be a contiguous torch.uint8 tensor on a GPU")
    return x


def compress_tensor(x, block_size=16 << 20, lib=None):
    """The .bz3 frame of the bytes of `x` (a contiguous torch.uint8 GPU tensor; view a tensor of another dtype with
    .view(torch.uint8).flatten()), computed on x's GPU: a uint8 tensor on the same device holding exactly the frame bytes of
    bz3_compress.  The result is a view of a bz3_bound(x.numel())-byte allocation (.clone() it to drop the slack).  Synchronises
    x's device first; raises Bz3Error with the return code on failure."""
    import torch

    x = _device_u8(x, "x")
    L = lib or load()
    n = x.numel()
    out = torch.empty(L.bz3_bound(n), dtype=torch.uint8, device=x.device)
    size = C.c_size_t(out.numel())
    torch.cuda.synchronize(x.device)
    rc = L.bz3_hip_compress_device(block_size, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), n, C.byref(size))
    if rc != BZ3_OK:
        raise Bz3Error(rc, "bz3_hip_compress_device")
    return out[: size.value]


def decompress_tensor(frame, out=None, lib=None):
    """The bytes of a .bz3 frame held in a contiguous torch.uint8 GPU tensor, decoded on its GPU.  `out`: a contiguous uint8 tensor
    on the same device to decode into (its size is the capacity); by default one of the frame's decoded size
    (bz3_hip_frame_decoded_size_device).  Returns the view of `out` holding the decoded bytes; raises Bz3Error with the return code
    of bz3_hip_decompress_device, whose `.out` holds the bytes of the chunks decoded before the error."""
    import torch

    frame = _device_u8(frame, "frame")
    L = lib or load()
    torch.cuda.synchronize(frame.device)
    if out is None:
        need = C.c_size_t(0)
        # a frame with a bad header still decodes (and fails) like bz3_decompress: size `out` for the well-formed chunks before it
        L.bz3_hip_frame_decoded_size_device(C.c_void_p(frame.data_ptr()), frame.numel(), C.byref(need))
        out = torch.empty(need.value, dtype=torch.uint8, device=frame.device)
    else:
        out = _device_u8(out, "out")
    size = C.c_size_t(out.numel())
    rc = L.bz3_hip_decompress_device(C.c_void_p(frame.data_ptr()), C.c_void_p(out.data_ptr()), frame.numel(), C.byref(size))
    if rc != BZ3_OK:
        raise Bz3Error(rc, "bz3_hip_decompress_device", out[: size.value])
    return out[: size.value]


def _same_device(ts, what):
    dev = ts[0].device
    for t in ts:
        if t.device != dev:
            raise ValueError(f"{what}: all tensors must be on one GPU ({dev} and {t.device})")
    return dev


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _carve(total, sizes, device):
    """Views of one uint8 allocation on `device`, of the given sizes, each starting at a multiple of 16 bytes."""
    import torch

    offs, o = [], 0
    for n in sizes:
        offs.append(o)
        o += (n + 15) & ~15
    buf = torch.empty(max(o, 1), dtype=torch.uint8, device=device)
    return [buf[a : a + n] for a, n in zip(offs, sizes)]


def compress_tensors(xs, block_size=16 << 20, lib=None):
    """compress_tensor for many tensors in ONE call (bz3_hip_compress_device_many): frame i is exactly compress_tensor(xs[i],
    block_size).  Blocks of all tensors share windows of up to 256 blocks, so many small tensors (a state_dict) code in a few CM
    launches instead of one per tensor.  All tensors must be contiguous torch.uint8 tensors on one GPU; one device synchronisation
    per call.  The frames are views of one allocation of bz3_bound bytes per tensor (.clone() one to drop the rest).  Raises
    Bz3Error (with .index / .codes / .outs) if any frame fails.  [] returns []."""
    import torch

    xs = [_device_u8(x, f"xs[{i}]") for i, x in enumerate(xs)]
    if not xs:
        return []
    dev = _same_device(xs, "compress_tensors")
    L = lib or load()
    n = len(xs)
    caps = [L.bz3_bound(x.numel()) for x in xs]
    outs = _carve(sum(caps), caps, dev)
    in_sizes = (C.c_size_t * n)(*[x.numel() for x in xs])
    out_sizes = (C.c_size_t * n)(*caps)
    rcs = (C.c_int * n)()
    torch.cuda.synchronize(dev)
    rc = L.bz3_hip_compress_device_many(block_size, n, _ptrs(xs), in_sizes, _ptrs(outs), out_sizes, rcs)
    frames = [o[: out_sizes[i]] for i, o in enumerate(outs)]
    if rc != BZ3_OK:
        codes = list(rcs)
        idx = next(i for i, c in enumerate(codes) if c != BZ3_OK)
        raise Bz3Error(rc, "bz3_hip_compress_device_many", index=idx, codes=codes, outs=frames)
    return frames


def decompress_tensors(frames, outs=None, lib=None):
    """decompress_tensor for many frames in ONE call (bz3_hip_decompress_device_many): result i is exactly
    decompress_tensor(frames[i], outs[i]).  `outs`: contiguous uint8 tensors on the frames' GPU, one per frame (their sizes are the
    capacities); by default views of one allocation sized with bz3_hip_frame_decoded_sizes_device.  One device synchronisation per
    call.  Raises Bz3Error (with .index / .codes / .outs, the bytes committed per frame) if any frame fails.  [] returns []."""
    import torch

    frames = [_device_u8(f, f"frames[{i}]") for i, f in enumerate(frames)]
    if not frames:
        return []
    dev = _same_device(frames, "decompress_tensors")
    L = lib or load()
    n = len(frames)
    in_ptrs = _ptrs(frames)
    in_sizes = (C.c_size_t * n)(*[f.numel() for f in frames])
    torch.cuda.synchronize(dev)
    if outs is None:
        need = (C.c_size_t * n)()
        rcs = (C.c_int * n)()
        # a frame with a bad header still decodes (and fails) like bz3_decompress: size its output for the well-formed chunks before it
        L.bz3_hip_frame_decoded_sizes_device(n, in_ptrs, in_sizes, need, rcs)
        outs = _carve(sum(need), list(need), dev)
    else:
        outs = [_device_u8(o, f"outs[{i}]") for i, o in enumerate(outs)]
        if len(outs) != n:
            raise ValueError(f"decompress_tensors: {n} frames and {len(outs)} outputs")
        _same_device(frames + outs, "decompress_tensors")
    out_sizes = (C.c_size_t * n)(*[o.numel() for o in outs])
    rcs = (C.c_int * n)()
    rc = L.bz3_hip_decompress_device_many(n, in_ptrs, in_sizes, _ptrs(outs), out_sizes, rcs)
    res = [o[: out_sizes[i]] for i, o in enumerate(outs)]
    if rc != BZ3_OK:
        codes = list(rcs)
        idx = next(i for i, c in enumerate(codes) if c != BZ3_OK)
        raise Bz3Error(rc, "bz3_hip_decompress_device_many", index=idx, codes=codes, outs=res)
    return res


def shard_blocks(n_blocks, world_size, rank):
    """Block -> GPU partition of SURVEY.md section 8e: block k belongs to rank k mod world_size."""
    return [k for k in range(n_blocks) if k % world_size == rank]
