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
        "bz3_hip_debug_set_unbwt_log_stride": (None, [C.c_int]),
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
        "bz3_hip_compress_device_planes": (C.c_int, [u32, u32, vp, vp, sz, C.POINTER(sz)]),
        "bz3_hip_decompress_device_planes": (C.c_int, [u32, vp, vp, sz, C.POINTER(sz)]),
        "bz3_hip_compress_device_planes_many": (C.c_int, [u32, i32, C.POINTER(u32), C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_decompress_device_planes_many": (C.c_int, [i32, C.POINTER(u32), C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_debug_planes": (i32, [vp, vp, C.POINTER(C.c_uint64), i32]),
        "bz3_hip_compress_device_delta": (C.c_int, [u32, u32, vp, vp, vp, sz, C.POINTER(sz)]),
        "bz3_hip_decompress_device_delta": (C.c_int, [u32, vp, vp, sz, vp, sz, C.POINTER(sz)]),
        "bz3_hip_compress_device_delta_many": (C.c_int, [u32, i32, C.POINTER(u32), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_decompress_device_delta_many": (C.c_int, [i32, C.POINTER(u32), C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_crc32c_device": (C.c_int, [vp, sz, u32, C.POINTER(u32)]),
        "bz3_hip_crc32c_device_many": (C.c_int, [i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(u32), C.POINTER(u32)]),
        "bz3_hip_debug_crc_launches": (C.c_uint, [C.c_int]),
        "bz3_hip_debug_delta": (i32, [vp, vp, vp, C.POINTER(C.c_uint64), i32]),
        "bz3_hip_decompress_device_range": (C.c_int, [u32, vp, sz, C.c_uint64, vp, sz, vp, C.POINTER(sz)]),
        "bz3_hip_decompress_device_range_many": (C.c_int, [i32, C.POINTER(u32), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_uint64), C.POINTER(vp), C.POINTER(sz),
                                                           C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_debug_range": (i32, [vp, vp, vp, C.POINTER(C.c_uint64), i32]),
        "bz3_hip_decompress_device_strided": (C.c_int, [u32, vp, sz, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, vp, sz, vp, C.POINTER(sz)]),
        "bz3_hip_decompress_device_strided_many": (C.c_int, [i32, C.POINTER(u32), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_uint64), C.POINTER(vp), C.POINTER(sz),
                                                             C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_debug_strided": (i32, [vp, vp, vp, C.POINTER(C.c_uint64), i32]),
        "bz3_hip_decompress_device_select": (C.c_int, [u32, vp, sz, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), vp, sz, vp, C.POINTER(sz)]),
        "bz3_hip_decompress_device_select_many": (C.c_int, [i32, C.POINTER(u32), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_uint64), C.POINTER(C.POINTER(C.c_uint64)),
                                                            C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_debug_select": (i32, [vp, vp, vp, C.POINTER(C.c_uint64), i32, C.POINTER(C.c_uint64), C.c_uint64]),
        "bz3_hip_update_device_range": (C.c_int, [u32, vp, sz, C.c_uint64, vp, sz, vp, vp, C.POINTER(sz)]),
        "bz3_hip_update_device_range_many": (C.c_int, [i32, C.POINTER(u32), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_uint64), C.POINTER(vp), C.POINTER(sz), C.POINTER(vp),
                                                       C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_debug_patch": (i32, [vp, vp, vp, C.POINTER(C.c_uint64), i32]),
        "bz3_hip_update_device_select": (C.c_int, [u32, vp, sz, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), vp, sz, vp, vp, C.POINTER(sz)]),
        "bz3_hip_update_device_select_many": (C.c_int, [i32, C.POINTER(u32), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_uint64), C.POINTER(C.POINTER(C.c_uint64)),
                                                        C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_debug_patch_select": (i32, [vp, vp, vp, C.POINTER(C.c_uint64), i32, C.POINTER(C.c_uint64), C.c_uint64]),
        "bz3_hip_resize_device": (C.c_int, [u32, u32, vp, sz, C.c_uint64, vp, sz, vp, vp, C.POINTER(sz)]),
        "bz3_hip_resize_device_many": (C.c_int, [i32, C.POINTER(u32), C.POINTER(u32), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_uint64), C.POINTER(vp), C.POINTER(sz),
                                                 C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]),
        "bz3_hip_debug_replane": (i32, [vp, vp, C.POINTER(C.c_uint64), i32]),
        "bz3_hip_sync_device": (C.c_int, [u32, vp, sz, vp, vp, sz, vp, vp, C.POINTER(sz), C.POINTER(u32)]),
        "bz3_hip_sync_device_many": (C.c_int, [i32, C.POINTER(u32), C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.POINTER(vp),
                                               C.POINTER(vp), C.POINTER(sz), C.POINTER(u32), C.POINTER(C.c_int)]),
        "bz3_hip_debug_diff": (i32, [vp, vp, C.POINTER(C.c_uint64), i32, C.POINTER(u32)]),
        "bz3_hip_last_timings": (None, [vp, C.POINTER(C.c_float)]),
        "bz3_hip_last_bwt_stats": (None, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_uint64)]),
        "bz3_hip_stage_crc32c": (u32, [vp, sz, u32]),
        "bz3_hip_stage_mrle_encode": (i32, [vp, i32, vp]),
        "bz3_hip_stage_mrle_decode": (C.c_int, [vp, vp, i32, i32]),
        "bz3_hip_stage_lzp_encode": (i32, [vp, i32, vp]),
        "bz3_hip_stage_lzp_decode": (i32, [vp, i32, vp, i32]),
        "bz3_hip_debug_lzp_encode": (i32, [vp, i32, vp, vp]),
        "bz3_hip_stage_bwt": (i32, [vp, vp, i32]),
        "bz3_hip_stage_unbwt": (i32, [vp, vp, i32, i32]),
        "bz3_hip_debug_unbwt_many": (i32, [vp, vp, vp, vp, i32]),
        "bz3_hip_debug_bwt_many": (i32, [vp, vp, vp, vp, i32]),
        "bz3_hip_debug_bwt_record": (i32, [vp, i32, vp, C.POINTER(i32), vp, u32]),
        "bz3_hip_debug_bwt_record_many": (i32, [vp, vp, vp, vp, i32, vp, u32]),
        "bz3_hip_debug_set_bwt_batch": (None, [C.c_int]),
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

    def lzp_encode_stats(self, data):
        """lzp_encode plus the driver's record (bz3_hip_debug_lzp_encode): (n, bytes, dict)."""
        out = (C.c_uint8 * (len(data) + 64))()
        st = (C.c_uint32 * 6)()
        n = self.lib.bz3_hip_debug_lzp_encode(_cbuf(data, len(data)), len(data), out, st)
        keys = ("end_pos", "n_matches", "iterations", "evaluated", "event_cap", "window_positions")
        return n, (C.string_at(out, n) if n > 0 else b""), dict(zip(keys, (int(x) for x in st)))

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

    def bwt_many(self, blocks):
        """blocks: bytes objects, through the batched forward BWT in runs of at most eight in the order given.  (rc, [(index, bytes), ...])."""
        k = len(blocks)
        ins = [_cbuf(d, len(d)) for d in blocks]
        outs = [(C.c_uint8 * max(1, len(d)))() for d in blocks]
        inp = (C.c_void_p * max(1, k))(*[C.cast(b, C.c_void_p) for b in ins])
        outp = (C.c_void_p * max(1, k))(*[C.cast(b, C.c_void_p) for b in outs])
        n = (C.c_int32 * max(1, k))(*[len(d) for d in blocks])
        idx = (C.c_int32 * max(1, k))()
        rc = self.lib.bz3_hip_debug_bwt_many(inp, outp, n, idx, k)
        return rc, [(int(i), C.string_at(o, len(d))) for i, o, d in zip(idx, outs, blocks)]

    BWT_RECORD_CAP = 1024  # words offered per record (the library says how many it writes)

    @staticmethod
    def _bwt_record(w):
        """The flat record of bwt.hip's bwt_record_flatten as a dict."""
        geo = ("WR_A", "WR_G", "TL_GROUP", "TL_COUNT", "TL_CAP", "WR_CAP", "VLC_WINDOW", "VLC_MAXLEN", "SP_GROUP", "big_cap", "WW_KEY", "TL_KEY", "BW_KEY", "BG_TILE", "RT_WAVES")
        r = {"n": w[1], "deep": w[2], "h": w[3], "stats": {"rounds": w[6], "radix_passes": w[7], "sorted_elements": w[8] | (w[9] << 32)}, "big_rounds": w[10]}
        r["geo"] = dict(zip(geo, w[12:12 + len(geo)]))
        max_passes, max_rounds = w[27], w[28]
        r["vlc"] = tuple(w[32:288])
        at = 288
        keys = ("g", "big", "given_up", "overflow", "tail", "tail_valid", "mid")
        r["passes"] = tuple(dict(zip(keys, w[at + 8 * k: at + 8 * k + 7])) for k in range(w[4]))
        at += 8 * max_passes
        r["rounds"] = tuple((w[at + 2 * k], w[at + 2 * k + 1]) for k in range(w[5]))
        assert w[0] == at + 2 * max_rounds, "the record's layout is not the one this reader knows"
        return r

    def bwt_record(self, data):
        """The forward BWT of one block alone and what the sorter did with it: (index, bytes, record)."""
        out = (C.c_uint8 * max(1, len(data)))()
        idx = C.c_int32()
        rec = (C.c_uint32 * self.BWT_RECORD_CAP)()
        rc = self.lib.bz3_hip_debug_bwt_record(_cbuf(data, len(data)), len(data), out, C.byref(idx), rec, self.BWT_RECORD_CAP)
        assert rc == 0, rc
        return idx.value, C.string_at(out, len(data)), self._bwt_record([int(x) for x in rec])

    def bwt_record_many(self, blocks):
        """bwt_many with a record per block: (rc, [(index, bytes, record), ...])."""
        k = len(blocks)
        ins = [_cbuf(d, len(d)) for d in blocks]
        outs = [(C.c_uint8 * max(1, len(d)))() for d in blocks]
        inp = (C.c_void_p * max(1, k))(*[C.cast(b, C.c_void_p) for b in ins])
        outp = (C.c_void_p * max(1, k))(*[C.cast(b, C.c_void_p) for b in outs])
        n = (C.c_int32 * max(1, k))(*[len(d) for d in blocks])
        idx = (C.c_int32 * max(1, k))()
        cap = self.BWT_RECORD_CAP
        rec = (C.c_uint32 * (cap * max(1, k)))()
        rc = self.lib.bz3_hip_debug_bwt_record_many(inp, outp, n, idx, k, rec, cap)
        flat = [int(x) for x in rec]
        return rc, [(int(i), C.string_at(o, len(d)), self._bwt_record(flat[cap * q: cap * (q + 1)])) for q, (i, o, d) in enumerate(zip(idx, outs, blocks))]

    def unbwt_many(self, jobs):
        """jobs: (bytes, index) pairs, through the batched inverse BWT in runs of at most four in the order given.  (rc, [bytes, ...])."""
        k = len(jobs)
        ins = [_cbuf(d, len(d)) for d, _ in jobs]
        outs = [(C.c_uint8 * max(1, len(d)))() for d, _ in jobs]
        inp = (C.c_void_p * max(1, k))(*[C.cast(b, C.c_void_p) for b in ins])
        outp = (C.c_void_p * max(1, k))(*[C.cast(b, C.c_void_p) for b in outs])
        n = (C.c_int32 * max(1, k))(*[len(d) for d, _ in jobs])
        idx = (C.c_int32 * max(1, k))(*[i for _, i in jobs])
        rc = self.lib.bz3_hip_debug_unbwt_many(inp, outp, n, idx, k)
        return rc, [C.string_at(o, len(d)) for o, (d, _) in zip(outs, jobs)]

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


def _planes_arg(planes, n):
    """`planes` of the batched calls: an int for every tensor, or one int per tensor."""
    ks = [int(planes)] * n if isinstance(planes, int) else [int(k) for k in planes]
    if len(ks) != n:
        raise ValueError(f"planes: {len(ks)} element sizes for {n} tensors")
    for k in ks:
        if k not in (1, 2, 4, 8):
            raise ValueError(f"planes must be 1, 2, 4 or 8, not {k}")
    return ks


def _base_u8(base, x, what, same_size=True):
    """A base for the uint8 tensor `x`: None, or a contiguous uint8 tensor on x's GPU (of x's size)."""
    if base is None:
        return None
    base = _device_u8(base, what)
    if base.device != x.device:
        raise ValueError(f"{what} is on {base.device}, the tensor on {x.device}")
    if same_size and base.numel() != x.numel():
        raise ValueError(f"{what} holds {base.numel()} bytes, the tensor {x.numel()}")
    return base


def _bases_arg(bases, n):
    bases = [None] * n if bases is None else list(bases)
    if len(bases) != n:
        raise ValueError(f"bases: {len(bases)} entries for {n} tensors")
    return bases


def _ptrs_or_null(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def compress_tensor(x, block_size=16 << 20, lib=None, planes=1, base=None):
    """The .bz3 frame of the bytes of `x` (a contiguous torch.uint8 GPU tensor; view a tensor of another dtype with
    .view(torch.uint8).flatten(), or use pack_tensor), computed on x's GPU: a uint8 tensor on the same device holding exactly the
    frame bytes of bz3_compress.  The result is a view of a bz3_bound(x.numel())-byte allocation (.clone() it to drop the slack).
    Synchronises x's device first; raises Bz3Error with the return code on failure.  `planes` = 2, 4 or 8: every block is split into
    the byte planes of its `planes`-byte elements first (bz3_hip_compress_device_planes); pass the same value to decompress_tensor.
    As bz3_compress does (src/libbz3.c:914), an input whose size is a non-zero multiple of the block size loses its last block without
    an error: pack_tensor chooses a block size at which nothing is lost.  `base`: a contiguous uint8 tensor of x's size on x's GPU, an
    earlier version of the same bytes: the frame is then that of the byte-wise difference (x - base) mod 256
    (bz3_hip_compress_device_delta), far smaller where the two are close, and decodes only with the same `base`."""
    import torch

    x = _device_u8(x, "x")
    (k,) = _planes_arg(planes, 1)
    base = _base_u8(base, x, "base")
    L = lib or load()
    n = x.numel()
    out = torch.empty(L.bz3_bound(n), dtype=torch.uint8, device=x.device)
    size = C.c_size_t(out.numel())
    torch.cuda.synchronize(x.device)
    rc = L.bz3_hip_compress_device_delta(block_size, k, C.c_void_p(x.data_ptr()), None if base is None else C.c_void_p(base.data_ptr()),
                                         C.c_void_p(out.data_ptr()), n, C.byref(size))
    if rc != BZ3_OK:
        raise Bz3Error(rc, "bz3_hip_compress_device_delta")
    return out[: size.value]


def decompress_tensor(frame, out=None, lib=None, planes=1, base=None):
    """The bytes of a .bz3 frame held in a contiguous torch.uint8 GPU tensor, decoded on its GPU.  `out`: a contiguous uint8 tensor
    on the same device to decode into (its size is the capacity); by default one of the frame's decoded size
    (bz3_hip_frame_decoded_size_device).  Returns the view of `out` holding the decoded bytes; raises Bz3Error with the return code
    of bz3_hip_decompress_device_planes, whose `.out` holds the bytes of the chunks decoded before the error.  `planes`: the value the
    frame was compressed with (it is not stored in the frame).  `base`: the tensor the frame was compressed against (neither is it
    stored; another base gives other bytes and no error).  `out` may be `base` itself, which is then updated in place; otherwise the
    two must not overlap.  With a base the capacity is the smaller of the two sizes."""
    import torch

    frame = _device_u8(frame, "frame")
    (k,) = _planes_arg(planes, 1)
    base = _base_u8(base, frame, "base", same_size=False)
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
    rc = L.bz3_hip_decompress_device_delta(k, C.c_void_p(frame.data_ptr()), None if base is None else C.c_void_p(base.data_ptr()),
                                           0 if base is None else base.numel(), C.c_void_p(out.data_ptr()), frame.numel(), C.byref(size))
    if rc != BZ3_OK:
        raise Bz3Error(rc, "bz3_hip_decompress_device_delta", out[: size.value])
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


def _compress_many(L, xs, block_sizes, ks, dev, slack=False, bases=None):
    """One bz3_hip_compress_device_delta_many call per distinct block size (one, unless pack_state_dict had to move some): frames
    in the order of xs.  `slack`: room for the frame and chunk headers on top of bz3_bound, which covers the coded blocks alone (a
    small incompressible tensor's frame is a few bytes longer than bz3_bound of its size)."""
    import torch

    n = len(xs)
    bases = _bases_arg(bases, n)
    caps = [L.bz3_bound(x.numel()) + ((13 + 8 * (x.numel() // _KiB65 + 2) + 15) & ~15 if slack else 0) for x in xs]
    outs = _carve(sum(caps), caps, dev)
    frames, codes = [None] * n, [BZ3_OK] * n
    torch.cuda.synchronize(dev)
    for bs in sorted(set(block_sizes)):
        idx = [i for i in range(n) if block_sizes[i] == bs]
        g = len(idx)
        out_sizes = (C.c_size_t * g)(*[caps[i] for i in idx])
        rcs = (C.c_int * g)()
        L.bz3_hip_compress_device_delta_many(bs, g, (C.c_uint32 * g)(*[ks[i] for i in idx]), _ptrs([xs[i] for i in idx]), _ptrs_or_null([bases[i] for i in idx]),
                                             (C.c_size_t * g)(*[xs[i].numel() for i in idx]), _ptrs([outs[i] for i in idx]), out_sizes, rcs)
        for j, i in enumerate(idx):
            frames[i], codes[i] = outs[i][: out_sizes[j]], rcs[j]
    if any(c != BZ3_OK for c in codes):
        idx = next(i for i, c in enumerate(codes) if c != BZ3_OK)
        raise Bz3Error(codes[idx], "bz3_hip_compress_device_delta_many", index=idx, codes=codes, outs=frames)
    return frames


def compress_tensors(xs, block_size=16 << 20, lib=None, planes=1, bases=None):
    """compress_tensor for many tensors in ONE call (bz3_hip_compress_device_planes_many): frame i is exactly compress_tensor(xs[i],
    block_size, planes=planes[i]).  Blocks of all tensors share windows of up to 256 blocks, so many small tensors (a state_dict) code
    in a few CM launches instead of one per tensor.  All tensors must be contiguous torch.uint8 tensors on one GPU; one device
    synchronisation per call.  The frames are views of one allocation of bz3_bound bytes per tensor (.clone() one to drop the rest).
    `planes`: an int, or one int per tensor.  Raises Bz3Error (with .index / .codes / .outs) if any frame fails.  [] returns [].  As
    bz3_compress does (src/libbz3.c:914), a tensor whose size is a non-zero multiple of the block size loses its last block without an
    error: pack_state_dict chooses block sizes at which nothing is lost.  `bases`: one entry per tensor, None or the tensor's base as
    in compress_tensor; tensors with and without a base share the call."""
    xs = [_device_u8(x, f"xs[{i}]") for i, x in enumerate(xs)]
    if not xs:
        return []
    ks = _planes_arg(planes, len(xs))
    bases = [_base_u8(b, x, f"bases[{i}]") for i, (b, x) in enumerate(zip(_bases_arg(bases, len(xs)), xs))]
    dev = _same_device(xs, "compress_tensors")
    return _compress_many(lib or load(), xs, [block_size] * len(xs), ks, dev, bases=bases)


def decompress_tensors(frames, outs=None, lib=None, planes=1, bases=None):
    """decompress_tensor for many frames in ONE call (bz3_hip_decompress_device_planes_many): result i is exactly
    decompress_tensor(frames[i], outs[i], planes=planes[i]).  `outs`: contiguous uint8 tensors on the frames' GPU, one per frame (their
    sizes are the capacities); by default views of one allocation sized with bz3_hip_frame_decoded_sizes_device.  `planes`: an int, or
    one int per frame.  One device synchronisation per call.  Raises Bz3Error (with .index / .codes / .outs, the bytes committed per
    frame) if any frame fails.  [] returns [].  `bases`: one entry per frame, None or the frame's base as in decompress_tensor;
    outs[i] may be bases[i]."""
    import torch

    frames = [_device_u8(f, f"frames[{i}]") for i, f in enumerate(frames)]
    if not frames:
        return []
    ks = _planes_arg(planes, len(frames))
    bases = [_base_u8(b, f, f"bases[{i}]", same_size=False) for i, (b, f) in enumerate(zip(_bases_arg(bases, len(frames)), frames))]
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
    rc = L.bz3_hip_decompress_device_delta_many(n, (C.c_uint32 * n)(*ks), in_ptrs, in_sizes, _ptrs_or_null(bases),
                                                (C.c_size_t * n)(*[0 if b is None else b.numel() for b in bases]), _ptrs(outs), out_sizes, rcs)
    res = [o[: out_sizes[i]] for i, o in enumerate(outs)]
    if rc != BZ3_OK:
        codes = list(rcs)
        idx = next(i for i, c in enumerate(codes) if c != BZ3_OK)
        raise Bz3Error(rc, "bz3_hip_decompress_device_delta_many", index=idx, codes=codes, outs=res)
    return res


def _decompress_partial(name, frames, request, outs, planes, bases, lib):
    """The body of decompress_tensors_range, _strided and _select.  request(n) validates the caller's request for the n frames and returns
    (the bytes asked of every frame, the C entry point's name, its parameter arrays between in_sizes and bases)."""
    import torch

    frames = [_device_u8(f, f"frames[{i}]") for i, f in enumerate(frames)]
    n = len(frames)
    nbytes, entry, params = request(n)
    if not frames:
        return []
    ks = _planes_arg(planes, n)
    bases = [_base_u8(b, f, f"bases[{i}]", same_size=False) for i, (b, f) in enumerate(zip(_bases_arg(bases, n), frames))]
    dev = _same_device(frames, name)
    L = lib or load()
    if outs is None:
        outs = _carve(sum(nbytes), nbytes, dev)
    else:
        outs = [_device_u8(o, f"outs[{i}]") for i, o in enumerate(outs)]
        if len(outs) != n:
            raise ValueError(f"{name}: {n} frames and {len(outs)} outputs")
        _same_device(frames + outs, name)
    for i, (o, b, w) in enumerate(zip(outs, bases, nbytes)):
        if o.numel() < w or (b is not None and b.numel() < w):
            raise ValueError(f"{name}: outs[{i}] / bases[{i}] hold fewer than the {w} bytes asked for")
    torch.cuda.synchronize(dev)
    out_sizes = (C.c_size_t * n)(*nbytes)
    rcs = (C.c_int * n)()
    rc = getattr(L, entry)(n, (C.c_uint32 * n)(*ks), _ptrs(frames), (C.c_size_t * n)(*[f.numel() for f in frames]), *params, _ptrs_or_null(bases),
                           (C.c_size_t * n)(*[0 if b is None else w for b, w in zip(bases, nbytes)]), _ptrs(outs), out_sizes, rcs)
    res = [o[: out_sizes[i]] for i, o in enumerate(outs)]
    if rc != BZ3_OK:
        codes = list(rcs)
        idx = next(i for i, c in enumerate(codes) if c != BZ3_OK)
        raise Bz3Error(rc, entry, index=idx, codes=codes, outs=res)
    return res


def decompress_tensors_range(frames, offsets, nbytes, outs=None, planes=1, bases=None, lib=None):
    """Bytes [offsets[i], offsets[i] + nbytes[i]) of what frames[i] decodes to, for many frames in ONE call
    (bz3_hip_decompress_device_range_many): only the chunks that hold bytes of a range are decoded (plus a walk over the chunk headers
    before the range); that saves GPU work, while one call still takes at least one block's decode time ("Range decode").  Returns uint8 tensors, shorter than nbytes[i]
    where the range runs past the end of the frame (pread's rule; never an error).  `outs`: contiguous uint8 tensors of at least
    nbytes[i] bytes to read into; by default views of one allocation.  `planes` as in decompress_tensors.  `bases[i]`: None, or the
    base's bytes OF THE RANGE (at least nbytes[i] of them: bases[i][j] pairs with byte offsets[i] + j); outs[i] may be bases[i].  The
    same frame may appear more than once.  Raises Bz3Error with .index / .codes / .outs (per frame the range bytes committed before its
    error) as decompress_tensors does.  [] returns []."""
    def request(n):
        offs, sizes = [int(o) for o in offsets], [int(w) for w in nbytes]
        if len(offs) != n or len(sizes) != n:
            raise ValueError(f"decompress_tensors_range: {n} frames, {len(offs)} offsets and {len(sizes)} sizes")
        if any(o < 0 for o in offs) or any(w < 0 for w in sizes):
            raise ValueError("decompress_tensors_range: offsets and sizes must not be negative")
        return sizes, "bz3_hip_decompress_device_range_many", [(C.c_uint64 * n)(*offs)]

    return _decompress_partial("decompress_tensors_range", frames, request, outs, planes, bases, lib)


def decompress_tensor_range(frame, offset, nbytes, out=None, planes=1, base=None, lib=None):
    """Bytes [offset, offset + nbytes) of what `frame` decodes to (bz3_hip_decompress_device_range): the uint8 tensor of the bytes
    read, shorter than nbytes past the end of the frame.  decompress_tensors_range for one frame; Bz3Error's `.out` holds the range
    bytes committed before the error."""
    try:
        return decompress_tensors_range([frame], [offset], [nbytes], None if out is None else [out], planes=planes, bases=None if base is None else [base], lib=lib)[0]
    except Bz3Error as e:
        raise Bz3Error(e.code, "bz3_hip_decompress_device_range", e.outs[0]) from None


def _index_set_arg(name, n, offsets, strides, counts, pieces, datas=None):
    """The index sets of the n frames of decompress_tensors_select and update_tensors_select, validated: (the bytes every set names, the
    (offset, stride, count) of every frame, its pieces, the C call's `params` and `pieces` arrays).  datas: an update's data tensors, each of which
    must hold all the bytes of its set."""
    cols = [[int(v) for v in col] for col in (offsets, strides, counts)]
    lists = [[(int(a), int(l)) for a, l in pl] for pl in pieces]
    if any(len(col) != n for col in cols) or len(lists) != n or (datas is not None and len(datas) != n):
        raise ValueError(f"{name}: {n} frames and {[len(col) for col in cols]} offsets, strides and counts, {len(lists)} piece lists" +
                         ("" if datas is None else f", {len(datas)} data tensors"))
    params = list(zip(*cols))
    nbytes = []
    for i, ((o, s, c), pl) in enumerate(zip(params, lists)):
        if min(o, s, c) < 0 or any(a < 0 or l < 0 for a, l in pl):
            raise ValueError(f"{name}: offsets, strides, counts and pieces must not be negative")
        if any(a + l >= 1 << 64 for a, l in pl) or any(a + l > b for (a, l), (b, _) in zip(pl, pl[1:])):
            raise ValueError(f"{name}: the pieces of frame {i} do not ascend")
        L, end = sum(l for _, l in pl), pl[-1][0] + pl[-1][1] if pl else 0
        if L and c and ((c > 1 and s < end) or c * L >= 1 << 64 or o + (c - 1) * s + end >= 1 << 64):
            raise ValueError(f"{name}: ({o}, {s}, {c}) and the pieces of frame {i} are no index set")
        if datas is not None and datas[i].numel() != c * L:
            raise ValueError(f"{name}: datas[{i}] holds {datas[i].numel()} bytes, the index set of frame {i} {c * L}")
        nbytes.append(c * L)
    arrs = [(C.c_uint64 * max(1, 2 * len(pl)))(*[v for p in pl for v in p]) for pl in lists]
    ptrs = (C.POINTER(C.c_uint64) * n)(*[C.cast(a, C.POINTER(C.c_uint64)) for a in arrs])
    ptrs.arrays = arrs  # alive as long as their pointers
    return nbytes, params, lists, [(C.c_uint64 * (4 * n))(*[v for p, pl in zip(params, lists) for v in (*p, len(pl))]), ptrs]


def _update_partial(name, frames, datas, request, planes, bases, lib, block_sizes):
    """The body of update_tensors_range and _select.  request(n, datas) validates the caller's request for the n frames and returns (the C entry
    point's name, its parameter arrays between in_sizes and datas, whether the 13 header bytes of the frames must be read whatever block_sizes is,
    recoded(i, block size, chunks): a bound on the chunks of frame i that are coded again; chunks: every frame's count of them, or None where the
    headers were not read)."""
    import torch

    frames = [_device_u8(f, f"frames[{i}]") for i, f in enumerate(frames)]
    n = len(frames)
    datas = [_device_u8(d, f"datas[{i}]") for i, d in enumerate(datas)]
    entry, params, heads_needed, recoded = request(n, datas)
    if not frames:
        return []
    ks = _planes_arg(planes, n)
    bases = [_base_u8(b, d, f"bases[{i}]") for i, (b, d) in enumerate(zip(_bases_arg(bases, n), datas))]
    dev = _same_device(frames + datas, name)
    L = lib or load()
    chunks = None
    if heads_needed:
        heads = torch.stack([torch.nn.functional.pad(f[:13], (0, 13 - min(13, f.numel()))) for f in frames]).cpu().numpy()
        chunks = [int.from_bytes(bytes(h[9:13]), "little") for h in heads]
        if block_sizes is None:
            block_sizes = [int.from_bytes(bytes(h[5:9]), "little") for h in heads]
    bss = [min(max(int(b), _KiB65), _MiB511) for b in block_sizes]  # (a header that lies: the call refuses it, or finds the output too small)
    if len(bss) != n:
        raise ValueError(f"{name}: {n} frames and {len(bss)} block sizes")
    caps = [f.numel() + recoded(i, bs, chunks) * L.bz3_bound(bs) for i, (f, bs) in enumerate(zip(frames, bss))]
    outs = _carve(sum(caps), caps, dev)
    out_sizes = (C.c_size_t * n)(*caps)
    rcs = (C.c_int * n)()
    torch.cuda.synchronize(dev)
    rc = getattr(L, entry)(n, (C.c_uint32 * n)(*ks), _ptrs(frames), (C.c_size_t * n)(*[f.numel() for f in frames]), *params, _ptrs(datas),
                           (C.c_size_t * n)(*[d.numel() for d in datas]), _ptrs_or_null(bases), _ptrs(outs), out_sizes, rcs)
    res = [o[: out_sizes[i]] for i, o in enumerate(outs)]
    if rc != BZ3_OK:
        codes = list(rcs)
        idx = next(i for i, c in enumerate(codes) if c != BZ3_OK)
        raise Bz3Error(codes[idx], entry, index=idx, codes=codes, outs=res)
    return res


def update_tensors_range(frames, offsets, datas, planes=1, bases=None, lib=None, block_sizes=None):
    """New frames in which the bytes [offsets[i], offsets[i] + datas[i].numel()) of what frames[i] decodes to are replaced by datas[i], for many
    frames in ONE call (bz3_hip_update_device_range_many) and one synchronisation: only the chunks that hold bytes of a range are coded again, of
    those only the (at most two per frame) that the range cuts are decoded first, and every other chunk is copied as it is, undecoded (DESIGN.md,
    "Range update").  Result i is byte for byte the frame compress_tensor gives for the updated bytes.  frames and datas: contiguous uint8
    tensors on one GPU; a range must lie inside what its frame decodes to (an update never grows a tensor; Bz3Error with BZ3_ERR_DATA_TOO_BIG),
    and an empty datas[i] gives a copy of the frame.  `planes` as in decompress_tensors.  `bases[i]`: None, or for a frame made against a base the
    base's bytes OF THE RANGE, as many as datas[i].  `block_sizes`: the block sizes of the frames where the caller knows them
    (PackedTensor.block_size); without them the 13 header bytes of all frames are read from the device once, which is a second synchronisation.
    They only size the outputs, which are views of one allocation of frames[i].numel() + (datas[i].numel() // block size + 2) *
    bz3_bound(block size) bytes each (.clone() one to drop the rest).  The inputs are never written.  Raises Bz3Error with .index / .codes / .outs
    as compress_tensors does; a frame that fails has no output.  [] returns []."""
    def request(n, datas):
        offs = [int(o) for o in offsets]
        if len(offs) != n or len(datas) != n:
            raise ValueError(f"update_tensors_range: {n} frames, {len(offs)} offsets and {len(datas)} data tensors")
        if any(o < 0 for o in offs):
            raise ValueError("update_tensors_range: offsets must not be negative")
        return "bz3_hip_update_device_range_many", [(C.c_uint64 * n)(*offs)], block_sizes is None, lambda i, bs, chunks: datas[i].numel() // bs + 2

    return _update_partial("update_tensors_range", frames, datas, request, planes, bases, lib, block_sizes)


def update_tensor_range(frame, offset, data, planes=1, base=None, lib=None, block_size=None):
    """The frame in which the bytes [offset, offset + data.numel()) of what `frame` decodes to are replaced by `data`
    (bz3_hip_update_device_range): update_tensors_range for one frame."""
    try:
        return update_tensors_range([frame], [offset], [data], planes=planes, bases=None if base is None else [base], lib=lib,
                                    block_sizes=None if block_size is None else [block_size])[0]
    except Bz3Error as e:
        raise Bz3Error(e.code, "bz3_hip_update_device_range") from None


def _joined_pieces(pl):
    """The number of pieces of a list once the empty ones are dropped and neighbours that touch are joined."""
    n, end = 0, None
    for a, l in pl:
        if l:
            n += a != end
            end = a + l
    return n


def update_tensors_select(frames, offsets, strides, counts, pieces, datas, planes=1, bases=None, lib=None, block_sizes=None):
    """New frames in which an index set of what frames[i] decodes to is replaced by datas[i], for many frames in ONE call
    (bz3_hip_update_device_select_many): the index set is that of decompress_tensors_select -- counts[i] periods strides[i] bytes apart from
    offsets[i] on, of every period the pieces pieces[i] as (start, len) -- and datas[i] holds its new bytes in output order, all
    counts[i] * sum(len) of them (ValueError otherwise: an update names all its bytes).  Only the chunks that hold a byte of a piece are coded
    again; of those the ones the set does not cover whole are decoded first, each once however many pieces it holds, and every other chunk is
    copied as it is, undecoded ("Index update").  Result i is byte for byte the frame compress_tensor gives for the updated bytes.
    Pieces shorter than 16 elements of planes[i] bytes are scattered byte by byte: correct and slow.  The set must lie inside what its frame
    decodes to (Bz3Error with BZ3_ERR_DATA_TOO_BIG); an empty one gives a copy of the frame.  `bases[i]`: None, or for a frame made against a
    base the base's bytes OF THE INDEX SET in output order, as many as datas[i].  ValueError for what decompress_tensors_select refuses.  The 13
    header bytes of all frames are read from the device once; with the block size bs (block_sizes[i] where given) and the number of chunks they
    size the outputs, views of one allocation of frames[i].numel() + min(chunks, W // bs + 2 * pieces * counts[i]) * bz3_bound(bs) bytes each
    (pieces: after joining neighbours that touch; .clone() a result to drop the rest).  The inputs are never written.  Raises Bz3Error with
    .index / .codes / .outs as update_tensors_range does; a frame that fails has no output.  [] returns []."""
    def request(n, datas):
        _, params, lists, args = _index_set_arg("update_tensors_select", n, offsets, strides, counts, pieces, datas)
        joined = [_joined_pieces(pl) for pl in lists]
        return "bz3_hip_update_device_select_many", args, True, lambda i, bs, chunks: min(chunks[i], datas[i].numel() // bs + 2 * joined[i] * params[i][2])

    return _update_partial("update_tensors_select", frames, datas, request, planes, bases, lib, block_sizes)


def update_tensor_select(frame, offset, stride, count, pieces, data, planes=1, base=None, lib=None, block_size=None):
    """The frame in which `count` periods' pieces (start, len), `stride` bytes apart from `offset` on, of what `frame` decodes to are replaced by
    `data` (bz3_hip_update_device_select): update_tensors_select for one frame."""
    try:
        return update_tensors_select([frame], [offset], [stride], [count], [pieces], [data], planes=planes, bases=None if base is None else [base], lib=lib,
                                     block_sizes=None if block_size is None else [block_size])[0]
    except Bz3Error as e:
        raise Bz3Error(e.code, "bz3_hip_update_device_select") from None


def decompress_tensors_strided(frames, offsets, runs, strides, counts, outs=None, planes=1, bases=None, lib=None):
    """A strided byte set of what every frame decodes to, for many frames in ONE call (bz3_hip_decompress_device_strided_many): of frame i
    the counts[i] runs of runs[i] bytes whose starts lie strides[i] bytes apart from offsets[i] on, one after the other -- a slice along
    any dimension of a row-major tensor.  Only the chunks that hold a byte of a run are decoded: chunks that lie wholly in a gap between
    two runs are skipped like those before the first run.  Returns uint8 tensors, shorter than counts[i] * runs[i] where the set runs
    past the end of the frame (pread's rule; never an error).  `outs`: contiguous uint8 tensors of at least counts[i] * runs[i] bytes to
    read into; by default views of one allocation.  `planes` as in
    decompress_tensors.  `bases[i]`: None, or the base's bytes OF THE SLICE in output order (bases[i][t] pairs with output byte t; at
    least as many as are asked for); outs[i] may be bases[i].  ValueError for a negative number, for strides[i] < runs[i] where
    counts[i] > 1 and runs[i] > 0, and for a set that does not fit 64 bits.  The same frame may appear more than once.  Raises Bz3Error
    with .index / .codes / .outs (per frame the bytes committed before its error) as decompress_tensors does.  [] returns []."""
    def request(n):
        cols = [[int(v) for v in col] for col in (offsets, runs, strides, counts)]
        if any(len(col) != n for col in cols):
            raise ValueError(f"decompress_tensors_strided: {n} frames and {[len(col) for col in cols]} offsets, runs, strides and counts")
        params = list(zip(*cols))
        for i, (o, r, s, c) in enumerate(params):
            if min(o, r, s, c) < 0:
                raise ValueError("decompress_tensors_strided: offsets, runs, strides and counts must not be negative")
            if r and c and ((c > 1 and s < r) or c * r >= 1 << 64 or o + (c - 1) * s + r >= 1 << 64):
                raise ValueError(f"decompress_tensors_strided: ({o}, {r}, {s}, {c}) of frame {i} is no strided range")
        return [r * c for _, r, _, c in params], "bz3_hip_decompress_device_strided_many", [(C.c_uint64 * (4 * n))(*[v for p in params for v in p])]

    return _decompress_partial("decompress_tensors_strided", frames, request, outs, planes, bases, lib)


def decompress_tensor_strided(frame, offset, run, stride, count, out=None, planes=1, base=None, lib=None):
    """`count` runs of `run` bytes, `stride` bytes apart from `offset` on, of what `frame` decodes to (bz3_hip_decompress_device_strided):
    decompress_tensors_strided for one frame; Bz3Error's `.out` holds the bytes committed before the error."""
    try:
        return decompress_tensors_strided([frame], [offset], [run], [stride], [count], None if out is None else [out], planes=planes, bases=None if base is None else [base],
                                          lib=lib)[0]
    except Bz3Error as e:
        raise Bz3Error(e.code, "bz3_hip_decompress_device_strided", e.outs[0]) from None


def decompress_tensors_select(frames, offsets, strides, counts, pieces, outs=None, planes=1, bases=None, lib=None):
    """An index set of what every frame decodes to, for many frames in ONE call (bz3_hip_decompress_device_select_many): of frame i
    counts[i] periods whose starts lie strides[i] bytes apart from offsets[i] on, and of every period the pieces pieces[i], a sequence of
    (start, len) relative to the period's start, ascending and disjoint -- an index_select along any dimension of a row-major tensor
    with a strictly increasing index.  Only the chunks that hold a byte of a piece are decoded, each of them once however many pieces it
    holds; chunks that lie wholly in a gap between two pieces are skipped like those before the first.  Returns uint8 tensors, shorter
    than counts[i] * sum(len) where the set runs past the end of the frame (pread's rule; never an error).  `outs`: contiguous uint8
    tensors of at least counts[i] * sum(len) bytes to read into; by default views of one allocation.  `planes` as in decompress_tensors.
    `bases[i]`: None, or the base's bytes OF THE INDEX SET in output order (at least as many as are asked for); outs[i] may be bases[i].
    ValueError for a negative number, for pieces that overlap or descend, for a last piece that ends behind strides[i] where
    counts[i] > 1, and for a set that does not fit 64 bits.  The same frame may appear more than once.  Raises Bz3Error with .index /
    .codes / .outs (per frame the bytes committed before its error) as decompress_tensors does.  [] returns []."""
    def request(n):
        nbytes, _, _, args = _index_set_arg("decompress_tensors_select", n, offsets, strides, counts, pieces)
        return nbytes, "bz3_hip_decompress_device_select_many", args

    return _decompress_partial("decompress_tensors_select", frames, request, outs, planes, bases, lib)


def decompress_tensor_select(frame, offset, stride, count, pieces, out=None, planes=1, base=None, lib=None):
    """Of `count` periods, `stride` bytes apart from `offset` on, the pieces (start, len) of what `frame` decodes to
    (bz3_hip_decompress_device_select): decompress_tensors_select for one frame; Bz3Error's `.out` holds the bytes committed before the
    error."""
    try:
        return decompress_tensors_select([frame], [offset], [stride], [count], [pieces], None if out is None else [out], planes=planes, bases=None if base is None else [base],
                                         lib=lib)[0]
    except Bz3Error as e:
        raise Bz3Error(e.code, "bz3_hip_decompress_device_select", e.outs[0]) from None


# ---- typed tensors ------------------------------------------------------------------------------------------------------------
# The byte-plane element size pack_tensor uses when `planes` is None, by dtype name: the component size where the measurements of
# DESIGN.md ("Typed tensors") show the planes frame smaller than the interleaved one, 1 where they show it larger or no different
# (16-bit floats, int32) and for every dtype nobody measured.
DEFAULT_PLANES = {
    "float32": 4,
    "float64": 8,
    "int64": 8,
    "complex64": 4,
    "complex128": 8,
    "bfloat16": 1,
    "float16": 1,
    "int32": 1,
    "int16": 1,
    "int8": 1,
    "uint8": 1,
    "bool": 1,
}
# The same for a tensor packed against a base (pack_tensor's `base`): 1 for every dtype but those listed.  After the byte-wise difference
# the planes frame is between 2.6 % larger and 2 % smaller than the interleaved one for float32, bfloat16 and float16, which is no reason
# to take the planes kernel; float64 is 5.5 - 6.8 % smaller with planes at every step size measured ("Delta frames";
# tools/delta_table.py).
DELTA_PLANES = {"float64": 8}
_KiB65, _MiB511 = 65 * 1024, 511 << 20


def default_planes(dtype):
    """DEFAULT_PLANES[dtype] (1 for a dtype that is not in the table)."""
    return DEFAULT_PLANES.get(str(dtype).replace("torch.", ""), 1)


def delta_default_planes(dtype):
    """DELTA_PLANES[dtype] (1 for a dtype that is not in the table): the default `planes` of a tensor packed against a base."""
    return DELTA_PLANES.get(str(dtype).replace("torch.", ""), 1)


def _lossless_block_size(nbytes, block_size, planes):
    """The block size the typed calls hand to the library for a tensor of `nbytes` bytes: the multiple of `planes` closest to
    `block_size` at which bz3_compress drops nothing.  bz3_compress gives its last block nbytes % bs bytes (src/libbz3.c:914), so a
    size that is a non-zero multiple of bs loses a block, unless bs > nbytes, where :877 replaces bs by bz3_bound(nbytes) and the
    input is one block.  The result bs satisfies: bs % planes == 0; 65 KiB <= bs; the block size in effect after :877-878 is at most
    511 MiB; and nbytes == 0, or bs > nbytes, or nbytes % bs != 0.  It is searched downwards from block_size (clamped to
    [65 KiB, 511 MiB] and rounded down to a multiple of planes) in steps of planes, and upwards from there once the 65 KiB floor is
    reached.  Pure arithmetic: no GPU, no library call."""
    if planes not in (1, 2, 4, 8):
        raise ValueError(f"planes must be 1, 2, 4 or 8, not {planes}")

    def ok(bs):
        eff = max(_KiB65, bs if bs <= nbytes else nbytes + nbytes // 50 + 32)  # :877-878 (bz3_bound)
        return eff <= _MiB511 and (nbytes == 0 or bs > nbytes or nbytes % bs != 0)

    start = min(max(int(block_size), _KiB65), _MiB511)
    start -= start % planes
    bs = start
    if bs > nbytes > 0 and not ok(bs):  # one block of bz3_bound(nbytes) > 511 MiB: no size above nbytes will do either
        bs = nbytes - nbytes % planes
    while bs >= _KiB65:
        if ok(bs):
            return bs
        bs -= planes
    bs = start + planes
    while not ok(bs):
        bs += planes
    return bs


class PackedTensor:
    """A tensor as pack_tensor leaves it: `frame` (a uint8 GPU tensor holding a .bz3 frame of the tensor's bytes, split into byte planes
    of `planes` bytes per block), and what unpack_tensor needs to restore it: `dtype`, `shape`, `planes`, `block_size` (the one really
    used, see _lossless_block_size) and `nbytes`.  `delta`: the frame holds the byte-wise difference from a base tensor, which
    unpack_tensor must be given again; `base_crc` is then the checksum of that base's bytes (bz3_hip_crc32c_device, init 1), else None.
    `crc`: the same checksum of the tensor's own bytes (those the frame decodes to once a base is added and the planes are merged), or
    None where it was not recorded: what `verify=True` checks after a decode and what the next delta's `base_crc` must equal (check_chain)."""

    __slots__ = ("frame", "dtype", "shape", "planes", "block_size", "nbytes", "delta", "base_crc", "crc")

    def __init__(self, frame, dtype, shape, planes, block_size, nbytes, delta=False, base_crc=None, crc=None):
        self.frame, self.dtype, self.shape, self.planes, self.block_size, self.nbytes = frame, dtype, shape, planes, block_size, nbytes
        self.delta, self.base_crc, self.crc = delta, base_crc, crc

    def __repr__(self):
        d = f", delta against a base of crc {self.base_crc:#010x}" if self.delta and self.base_crc is not None else (", delta" if self.delta else "")
        return f"PackedTensor({self.dtype}, {tuple(self.shape)}, planes={self.planes}, block_size={self.block_size}{d}, {self.frame.numel()} of {self.nbytes} bytes)"


def _as_bytes(x, what):
    import torch

    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise TypeError(f"{what} must be a torch tensor on a GPU")
    x = x.detach().contiguous()
    if x.is_complex():
        x = torch.view_as_real(x)
    return x.reshape(-1).view(torch.uint8)


def _from_bytes(raw, dtype, shape):
    import torch

    if dtype.is_complex:
        return torch.view_as_complex(raw.view(torch.empty(0, dtype=dtype).real.dtype).reshape(tuple(shape) + (2,)))
    return raw.view(dtype).reshape(shape)


def _base_bytes(base, nbytes, device, what):
    """The bytes of a typed base for a tensor of `nbytes` bytes on `device`: TypeError unless a GPU tensor, ValueError for another GPU or
    size.  A non-contiguous base is read through a contiguous copy, as a non-contiguous tensor is (only a contiguous one can be
    updated in place, which the check of `out` sees to)."""
    if base is None:
        return None
    b = _as_bytes(base, what)
    if b.device != device:
        raise ValueError(f"{what} is on {b.device}, the tensor on {device}")
    if b.numel() != nbytes:
        raise ValueError(f"{what} holds {b.numel()} bytes, the tensor {nbytes}")
    return b


def base_crc(raw, lib=None):
    """bz3_hip_crc32c_device over a contiguous uint8 GPU tensor, as PackedTensor.base_crc records it (init 1, the codec's)."""
    import torch

    raw = _device_u8(raw, "raw")
    torch.cuda.synchronize(raw.device)
    crc = C.c_uint32(0)
    rc = (lib or load()).bz3_hip_crc32c_device(C.c_void_p(raw.data_ptr()), raw.numel(), 1, C.byref(crc))
    if rc != BZ3_OK:
        raise Bz3Error(rc, "bz3_hip_crc32c_device")
    return crc.value


def crc32c_tensors(ts, inits=None, lib=None):
    """base_crc for many tensors in ONE call (bz3_hip_crc32c_device_many: at most two kernel launches whatever their number): the list
    of the checksums of contiguous torch.uint8 tensors on one GPU, result i exactly base_crc(ts[i]) when inits is None.  `inits`: one
    start state per tensor (default 1, the codec's).  Tensors of size 0 are allowed and yield their start state; tensors may repeat and
    overlap.  One device synchronisation per call.  [] returns []."""
    import torch

    ts = [_device_u8(t, f"ts[{i}]") for i, t in enumerate(ts)]
    if not ts:
        return []
    n = len(ts)
    if inits is not None:
        inits = [int(v) for v in inits]
        if len(inits) != n:
            raise ValueError(f"crc32c_tensors: {len(inits)} start states for {n} tensors")
    dev = _same_device(ts, "crc32c_tensors")
    torch.cuda.synchronize(dev)
    crcs = (C.c_uint32 * n)()
    rc = (lib or load()).bz3_hip_crc32c_device_many(n, (C.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in ts]), (C.c_size_t * n)(*[t.numel() for t in ts]),
                                                    None if inits is None else (C.c_uint32 * n)(*inits), crcs)
    if rc != BZ3_OK:
        raise Bz3Error(rc, "bz3_hip_crc32c_device_many")
    return list(crcs)


def _crcs_where(ts, lib):
    """crc32c_tensors of the entries of `ts` that are not None, in one call; None for the others."""
    idx = [i for i, t in enumerate(ts) if t is not None]
    out = [None] * len(ts)
    for i, c in zip(idx, crc32c_tensors([ts[i] for i in idx], lib=lib)):
        out[i] = c
    return out


def _pack_many(xs, block_size, planes, lib, bases=None, checksum=True):
    raws = [_as_bytes(x, f"tensor {i}") for i, x in enumerate(xs)]
    braws = [_base_bytes(b, r.numel(), r.device, f"base {i}") for i, (b, r) in enumerate(zip(_bases_arg(bases, len(xs)), raws))]
    ks = [default_planes(x.dtype) if b is None else delta_default_planes(x.dtype) for x, b in zip(xs, braws)] if planes is None else _planes_arg(planes, len(xs))
    bss = [_lossless_block_size(r.numel(), block_size, k) for r, k in zip(raws, ks)]
    if any(bs % k for bs, k in zip(bss, ks)):  # every chunk starts an element: what keeps typed slices on the 16-byte path of the strided merge
        raise AssertionError("a lossless block size must be a multiple of the element size")
    dev = _same_device(raws, "pack")
    L = lib or load()
    frames = _compress_many(L, raws, bss, ks, dev, slack=True, bases=braws)
    crcs = _crcs_where(braws + (raws if checksum else []), L)  # every base and every content checksum of the call in one batched call
    own = crcs[len(xs) :] if checksum else [None] * len(xs)
    return [PackedTensor(f, x.dtype, x.shape, k, bs, r.numel(), b is not None, c, o) for f, x, k, bs, r, b, c, o in zip(frames, xs, ks, bss, raws, braws, crcs, own)]


def _check_bases(ps, braws, labels, lib):
    """ValueError for the first base whose checksum is not its tensor's base_crc: one batched call over all of them."""
    got = _crcs_where([b if b is not None and p.base_crc is not None else None for p, b in zip(ps, braws)], lib)
    for p, g, label in zip(ps, got, labels):
        if g is not None and g != p.base_crc:
            raise ValueError(f"unpack: base {label} is not the tensor this frame was packed against (its checksum differs)")


def _unpack_many(ps, outs, lib, bases=None, check_base=True, verify=False, names=None):
    import torch

    for p in ps:
        if not isinstance(p, PackedTensor):
            raise TypeError("unpack: a PackedTensor is expected")
    bases = _bases_arg(bases, len(ps))
    braws = []
    for i, (p, b) in enumerate(zip(ps, bases)):
        if p.delta and b is None:
            raise ValueError(f"unpack: tensor {i} was packed against a base, which is needed to restore it")
        if not p.delta:
            b = None  # (a base beside a tensor that was packed without one is not used)
        braws.append(_base_bytes(b, p.nbytes, p.frame.device, f"base {i}"))
    L = lib or load()
    if check_base:  # before anything is decoded or written: the codec cannot tell a wrong base, it would return noise
        _check_bases(ps, braws, range(len(ps)), L)
    if outs is None:
        dev = _same_device([p.frame for p in ps], "unpack")
        # every output at a multiple of 16 bytes, so that any dtype can view it
        raws = _carve(0, [p.nbytes for p in ps], dev)
        res = None
    else:
        res = outs
        raws = []
        for p, o in zip(ps, outs):
            if not isinstance(o, torch.Tensor) or o.dtype != p.dtype or o.shape != p.shape or not o.is_contiguous():
                raise TypeError("unpack: `out` must be a contiguous tensor of the packed dtype and shape")
            raws.append(_as_bytes(o, "out"))
    got = decompress_tensors([p.frame for p in ps], raws, lib=lib, planes=[p.planes for p in ps], bases=braws)
    for p, g in zip(ps, got):
        if g.numel() != p.nbytes:
            raise ValueError(f"unpack: the frame decodes to {g.numel()} bytes, the tensor has {p.nbytes}")
    if verify:  # one batched call over the outputs
        got = _crcs_where([r if p.crc is not None else None for p, r in zip(ps, raws)], L)
        for i, (p, g) in enumerate(zip(ps, got)):
            if g is not None and g != p.crc:
                raise ValueError(f"unpack: the decoded bytes of tensor {i if names is None else repr(names[i])} do not have the checksum recorded when it was packed")
    return res if res is not None else [_from_bytes(r, p.dtype, p.shape) for r, p in zip(raws, ps)]


def pack_tensor(x, block_size=16 << 20, planes=None, lib=None, base=None, checksum=True):
    """Losslessly compresses a GPU tensor of any dtype and shape on its GPU: a PackedTensor whose `.frame` is an ordinary .bz3 frame.
    Non-contiguous input is made contiguous; zero-element and 0-d tensors round-trip; a CPU tensor is a TypeError.  `planes`: the
    byte-plane element size (1, 2, 4 or 8: bz3_hip_compress_device_planes), by default DEFAULT_PLANES for x's dtype.  The block size
    handed to the library is _lossless_block_size(nbytes, block_size, planes), never one at which bz3_compress would drop the last
    block (src/libbz3.c:914); it is recorded in the result.  The frame decodes anywhere: bz3_decompress gives S(x), the tensor's bytes
    with every chunk split into planes; merge_k per chunk restores them.  Cost of the planes: the split and the merge
    ride on the launches that move blocks into and out of their slots, so they add no pass.  The low mantissa planes of floats are
    incompressible and such blocks can take the slower CM route, so time is the user's trade against size; measured on an MI355X on 256
    fp32 tensors of 16 MiB of N(0, 0.02) (tools/planes_probe.py, profiles/planes_probe.json): pack_state_dict + unpack_state_dict at
    planes=4 took 16.28 s + 30.75 s for frames of 0.8366 of the input, compress_tensors + decompress_tensors at planes=1 and the same
    block size 16.48 s + 31.08 s for 0.8610.  The tensors unpack_tensor / unpack_state_dict return are views of one allocation per call.
    `base`: an earlier version of x (a GPU tensor of x's size in bytes on x's GPU; another size or GPU: ValueError, the CPU or no tensor:
    TypeError).  The frame then codes the byte-wise difference from it (bz3_hip_compress_device_delta) and the result records
    delta=True and the base's checksum; `planes` then defaults to DELTA_PLANES (1 for every dtype but float64).  unpack_tensor needs the same base again.
    `checksum`: record the checksum of x's own bytes in the result's `.crc` (one more read of x, in the same batched call as the base's
    checksum); the frame does not depend on it."""
    return _pack_many([x], block_size, None if planes is None else [planes], lib, [base], checksum)[0]


def unpack_tensor(p, out=None, lib=None, base=None, check_base=True, verify=False):
    """The tensor a PackedTensor holds, on the frame's GPU, in `out` if given (a contiguous tensor of p.dtype and p.shape).  Raises
    Bz3Error if the frame does not decode and ValueError if it decodes to another number of bytes than p.nbytes.  A tensor packed
    against a base needs `base` (a GPU tensor, the one it was packed against): ValueError without it, for a base of another size, and, unless
    check_base=False, for one whose checksum is not p.base_crc -- all raised before anything is decoded or written, because decoding
    against another base returns other bytes and no error.  The check reads the base once.  `out` may be `base`: it is updated in place.
    `verify`: after decoding, ValueError unless the decoded bytes have the checksum p.crc (skipped where p.crc is None).  That is after
    the write: with `out` being `base`, the base has been overwritten by then."""
    return _unpack_many([p], None if out is None else [out], lib, [base], check_base, verify)[0]


def _row_bytes(p, what):
    if not isinstance(p, PackedTensor):
        raise TypeError("unpack: a PackedTensor is expected")
    if len(p.shape) == 0:
        raise ValueError(f"{what}: a 0-d tensor has no rows")
    return p.nbytes // p.shape[0] if p.shape[0] else 0


def _unpack_rows_many(ps, rows, outs, lib, bases):
    """Rows rows[i] = (start, stop) of dimension 0 of every PackedTensor (None: the whole tensor), in ONE
    bz3_hip_decompress_device_range_many call.  bases[i]: the same rows of the base.  (A tensor that comes back whole is read as the range
    of its bytes: a frame that decodes to more is not noticed here.)"""
    shapes, spans = [], []
    for i, (p, r) in enumerate(zip(ps, rows)):
        if not isinstance(p, PackedTensor):
            raise TypeError("unpack: a PackedTensor is expected")
        if r is None:
            shapes.append(tuple(p.shape))
            spans.append((0, p.nbytes))
            continue
        rb = _row_bytes(p, f"tensor {i}")
        start, stop = int(r[0]), int(r[1])
        if not 0 <= start <= stop <= p.shape[0]:
            raise ValueError(f"rows ({start}, {stop}) of a tensor of {p.shape[0]} rows")
        shapes.append((stop - start, *p.shape[1:]))
        spans.append((start * rb, (stop - start) * rb))
    frames, planes, sizes = [p.frame for p in ps], [p.planes for p in ps], [w for _, w in spans]
    return _unpack_parts_many(ps, shapes, sizes, [], outs, lib, bases, "rows",
                              lambda raws, braws: decompress_tensors_range(frames, [o for o, _ in spans], sizes, raws, planes=planes, bases=braws, lib=lib))



def unpack_tensor_rows(p, start, stop, out=None, base=None, lib=None):
    """Rows [start, stop) of dimension 0 of the tensor a PackedTensor holds, in its dtype, of shape (stop - start, *p.shape[1:]), on the
    frame's GPU: only the chunks of the frame that hold bytes of those rows are decoded (bz3_hip_decompress_device_range), so a
    tensor-parallel rank that loads 1/N of the rows decodes about 1/N of the chunks.  ValueError for a 0-d tensor and unless
    0 <= start <= stop <= p.shape[0]; Bz3Error if the frame fails or returns fewer bytes than the rows hold.  `out`: a contiguous
    tensor of that dtype and shape.  A tensor packed against a base needs `base`: THE SAME ROWS of the base (a GPU tensor of the
    dtype and of the rows' shape; `out` may be it).  PackedTensor.base_crc covers the whole base and cannot be checked against a slice
    of it: the caller vouches that these are rows of the right base (another base gives other bytes and no error)."""
    return _unpack_rows_many([p], [(start, stop)], None if out is None else [out], lib, [base])[0]


def _update_rows_many(ps, rows, bases, lib):
    """rows[i] = (start, values): the PackedTensors with rows [start, start + len(values)) of dimension 0 replaced, through ONE
    bz3_hip_update_device_range_many call.  bases[i]: the same rows of the base.  Every argument is checked before any GPU work."""
    import torch

    offs = []
    for i, (p, (start, values)) in enumerate(zip(ps, rows)):
        rb = _row_bytes(p, f"tensor {i}")
        start = int(start)
        if not isinstance(values, torch.Tensor) or values.device.type != "cuda":
            raise TypeError(f"update: the rows of tensor {i} must be a torch tensor on a GPU")
        if values.dtype != p.dtype or values.dim() != len(p.shape) or tuple(values.shape[1:]) != tuple(p.shape[1:]):
            raise TypeError(f"update: the rows of tensor {i} must be {p.dtype} of shape (rows, {', '.join(map(str, p.shape[1:]))})")
        if not 0 <= start <= start + values.shape[0] <= p.shape[0]:
            raise ValueError(f"update: rows ({start}, {start + values.shape[0]}) of a tensor of {p.shape[0]} rows")
        offs.append(start * rb)
    return _update_parts_many(ps, [tuple(v.shape) for _, v in rows], [v for _, v in rows], bases, lib, "rows",
                              lambda i: (f"tensor {i}", f"the rows of tensor {i}", f"base {i}"),
                              lambda frames, raws, braws, **kw: update_tensors_range(frames, offs, raws, bases=braws, **kw))


def update_tensor_rows(p, start, values, base=None, lib=None):
    """A new PackedTensor that holds p's tensor with rows [start, start + len(values)) of dimension 0 replaced by `values`, on the frame's GPU,
    without the tensor ever being materialised: only the chunks of the frame that hold bytes of those rows are coded again
    (bz3_hip_update_device_range), the others are copied.  Its frame is byte for byte the one pack_tensor gives for the updated tensor at
    p.block_size and p.planes.  `values`: a GPU tensor of p's dtype and trailing shape (TypeError otherwise); the rows must lie inside
    p.shape[0] (ValueError; a 0-d tensor has no rows): an update never grows a tensor.  All of that is checked before any GPU work.  A tensor
    packed against a base needs `base`: THE SAME ROWS of the base, of values' shape (ValueError without them); as with unpack_tensor_rows,
    base_crc covers the whole base and cannot vouch for a slice of it.  planes, block_size, dtype, shape, nbytes, delta and base_crc are
    carried over; `crc` of the result is None, because the checksum of the whole tensor cannot be had without the bytes of the chunks that were
    only copied (verify=True skips such a tensor; pack it anew, or unpack and checksum it, where a checksum is wanted).  `p` is unchanged."""
    return _update_rows_many([p], [(start, values)], [base], lib)[0]


def _effective_block_size(block_size, nbytes):
    """The block size bz3_compress codes `nbytes` bytes with under `block_size` (src/libbz3.c:877-878)."""
    return max(_KiB65, block_size if block_size <= nbytes else nbytes + nbytes // 50 + 32)


def resize_tensors(frames, keeps, datas, planes=1, bases=None, block_sizes=None, lib=None):
    """New frames that decode to the first keeps[i] bytes of what frames[i] decodes to followed by datas[i], for many frames in ONE call
    (bz3_hip_resize_device_many) and one synchronisation: the chunks that lie wholly inside the kept bytes are copied as they are, undecoded; of
    the others at most one per frame is decoded first, the one the kept bytes end in ("Resize").  Result i is byte for byte the frame
    compress_tensor gives for the new bytes at block_sizes[i].  frames and datas: contiguous uint8 tensors on one GPU (an empty datas[i]
    truncates).  `block_sizes` is required: the block sizes the frames were made with (PackedTensor.block_size), which the header of a frame of
    one block does not tell.  `planes` as in decompress_tensors.  `bases[i]`: None, or for a frame made against a base the base's bytes OF THE
    APPENDED RANGE, as many as datas[i].  A new size that is a non-zero multiple of its block size would lose a block and is refused
    (BZ3_ERR_INIT), as is a frame that bz3_compress would not have written.  The outputs are views of one allocation (.clone() one to drop the
    rest).  The inputs are never written.  Raises Bz3Error with .index / .codes / .outs as compress_tensors does.  [] returns []."""
    import torch

    frames = [_device_u8(f, f"frames[{i}]") for i, f in enumerate(frames)]
    n = len(frames)
    datas = [_device_u8(d, f"datas[{i}]") for i, d in enumerate(datas)]
    keeps = [int(k) for k in keeps]
    if block_sizes is None:
        raise ValueError("resize_tensors: block_sizes is required")
    bss = [int(b) for b in block_sizes]
    if len(keeps) != n or len(datas) != n or len(bss) != n:
        raise ValueError(f"resize_tensors: {n} frames, {len(keeps)} sizes to keep, {len(datas)} data tensors and {len(bss)} block sizes")
    if any(k < 0 for k in keeps) or any(not 0 < b < 1 << 32 for b in bss):
        raise ValueError("resize_tensors: sizes to keep must not be negative, block sizes must be positive")
    if not frames:
        return []
    ks = _planes_arg(planes, n)
    bases = [_base_u8(b, d, f"bases[{i}]") for i, (b, d) in enumerate(zip(_bases_arg(bases, n), datas))]
    dev = _same_device(frames + datas, "resize_tensors")
    L = lib or load()
    caps = []
    for f, keep, d, bs in zip(frames, keeps, datas, bss):
        total = keep + d.numel()
        eff = _effective_block_size(bs, total)
        rebuilt = -(-total // eff) - keep // eff  # the chunks from the one the kept bytes end in on
        caps.append(13 + f.numel() + rebuilt * (8 + L.bz3_bound(min(eff, total))))
    outs = _carve(sum(caps), caps, dev)
    out_sizes = (C.c_size_t * n)(*caps)
    rcs = (C.c_int * n)()
    torch.cuda.synchronize(dev)
    rc = L.bz3_hip_resize_device_many(n, (C.c_uint32 * n)(*bss), (C.c_uint32 * n)(*ks), _ptrs(frames), (C.c_size_t * n)(*[f.numel() for f in frames]),
                                      (C.c_uint64 * n)(*keeps), (C.c_void_p * n)(*[d.data_ptr() if d.numel() else None for d in datas]),
                                      (C.c_size_t * n)(*[d.numel() for d in datas]), _ptrs_or_null(bases), _ptrs(outs), out_sizes, rcs)
    res = [o[: out_sizes[i]] for i, o in enumerate(outs)]
    if rc != BZ3_OK:
        codes = list(rcs)
        idx = next(i for i, c in enumerate(codes) if c != BZ3_OK)
        raise Bz3Error(codes[idx], "bz3_hip_resize_device_many", index=idx, codes=codes, outs=res)
    return res


def _resize_rows_many(ps, specs, bases, lib):
    """specs[i] = (keep_rows, values or None): the PackedTensors that hold the first keep_rows rows of dimension 0 followed by the rows of
    `values`.  bases[i]: the rows of the base that pair with `values`.  Every argument is checked before any GPU work; then one
    bz3_hip_resize_device_many call per distinct block size, the tensors whose new size is not lossless at their block size apart (repacked),
    and one batched checksum call."""
    import math

    import torch

    L = lib or load()
    plan = []
    for i, (p, (keep_rows, values), b) in enumerate(zip(ps, specs, _bases_arg(bases, len(ps)))):
        _row_bytes(p, f"tensor {i}")
        keep_rows = int(keep_rows)
        if not 0 <= keep_rows <= p.shape[0]:
            raise ValueError(f"resize: {keep_rows} rows to keep of a tensor of {p.shape[0]} rows")
        if values is not None:
            if not isinstance(values, torch.Tensor) or values.device.type != "cuda":
                raise TypeError(f"resize: the rows of tensor {i} must be a torch tensor on a GPU")
            if values.dtype != p.dtype or values.dim() != len(p.shape) or tuple(values.shape[1:]) != tuple(p.shape[1:]):
                raise TypeError(f"resize: the rows of tensor {i} must be {p.dtype} of shape (rows, {', '.join(map(str, p.shape[1:]))})")
            if values.device != p.frame.device:
                raise ValueError(f"resize: the rows of tensor {i} are on {values.device}, the frame on {p.frame.device}")
        added = 0 if values is None else values.shape[0]
        if not (p.delta and added):
            b = None  # (a base beside a tensor that was packed without one, or beside no new rows, is not used)
        elif b is None:
            raise ValueError(f"resize: tensor {i} was packed against a base, whose rows are needed to code the new ones")
        elif not isinstance(b, torch.Tensor) or b.dtype != p.dtype or tuple(b.shape) != tuple(values.shape):
            raise ValueError(f"resize: base {i} must hold the same rows of the base: {p.dtype} {tuple(values.shape)}")
        rb = math.prod(p.shape[1:]) * torch.empty(0, dtype=p.dtype).element_size()
        raw = _as_bytes(values, f"the rows of tensor {i}") if added else torch.empty(0, dtype=torch.uint8, device=p.frame.device)
        braw = _base_bytes(b, raw.numel(), p.frame.device, f"base {i}")
        shape = (keep_rows + added, *p.shape[1:])
        plan.append((keep_rows * rb, raw, braw, shape, (keep_rows + added) * rb, keep_rows == p.shape[0]))
    frames, sizes = [None] * len(ps), [p.block_size for p in ps]
    groups = {}
    for i, (p, (keep, raw, braw, shape, nbytes, _)) in enumerate(zip(ps, plan)):
        if _lossless_block_size(nbytes, p.block_size, p.planes) == p.block_size:
            groups.setdefault(p.block_size, []).append(i)
            continue
        # the new size would lose a block at p.block_size: the bytes the frame codes (the difference from the base for a delta tensor) are
        # decoded, cut, joined with the new ones and coded again at the nearest lossless block size
        old = decompress_tensors([p.frame], planes=[p.planes], lib=L)[0]
        new = torch.cat([old[:keep], raw if braw is None else raw - braw])
        sizes[i] = _lossless_block_size(nbytes, p.block_size, p.planes)
        frames[i] = _compress_many(L, [new], [sizes[i]], [p.planes], new.device, slack=True)[0]
    for bs, idx in groups.items():
        got = resize_tensors([ps[i].frame for i in idx], [plan[i][0] for i in idx], [plan[i][1] for i in idx], planes=[ps[i].planes for i in idx],
                             bases=[plan[i][2] for i in idx], block_sizes=[bs] * len(idx), lib=L)
        for i, f in zip(idx, got):
            frames[i] = f
    # the codec's checksum has no final xor, so it chains: the checksum of an appended tensor is that of the new rows started from the old one
    chain = [(i, which) for i, (p, pl) in enumerate(zip(ps, plan)) if pl[5]
             for which in ("crc", "base_crc") if getattr(p, which) is not None and (which == "crc" or pl[2] is not None)]
    sums = crc32c_tensors([plan[i][1] if which == "crc" else plan[i][2] for i, which in chain], inits=[getattr(ps[i], which) for i, which in chain], lib=L) if chain else []
    out = []
    for i, (p, pl) in enumerate(zip(ps, plan)):
        out.append([p, pl, {"crc": p.crc if pl[5] else None, "base_crc": p.base_crc if pl[5] else None}])
    for (i, which), c in zip(chain, sums):
        out[i][2][which] = c
    return [PackedTensor(frames[i], p.dtype, torch.Size(pl[3]), p.planes, sizes[i], pl[4], p.delta, crcs["base_crc"], crcs["crc"]) for i, (p, pl, crcs) in enumerate(out)]


def resize_tensor_rows(p, keep_rows, values=None, base=None, lib=None):
    """A new PackedTensor that holds the first keep_rows rows of dimension 0 of p's tensor followed by the rows of `values` (None: none), on the
    frame's GPU, without the tensor ever being materialised (bz3_hip_resize_device): the chunks of the frame that lie wholly inside the kept rows
    are copied undecoded, at most one chunk is decoded, and only the chunks from there on are coded.  Its frame is byte for byte the one
    pack_tensor gives for the new tensor at p.block_size and p.planes.  `values`: a GPU tensor of p's dtype and trailing shape (TypeError
    otherwise); 0 <= keep_rows <= p.shape[0] (ValueError; a 0-d tensor has no rows).  A tensor packed against a base needs `base` for the new
    rows: the rows of the grown base that pair with `values`, of values' shape (ValueError without them).  All of that is checked before any GPU
    work.  FALLBACK: where the new size is not lossless at p.block_size (a non-zero multiple of it: _lossless_block_size(new nbytes,
    p.block_size, p.planes) != p.block_size), the tensor's bytes are decoded, joined and packed again as pack_tensor(block_size=p.block_size)
    packs them, and the result's `block_size` DIFFERS from p's.  shape and nbytes are the new tensor's; planes, dtype and delta are carried over.
    After a pure append (keep_rows == p.shape[0]) `crc` is the checksum of the grown tensor where p.crc is known, chained from it over the new
    rows alone (crc32c_tensors with inits), and `base_crc` likewise that of the grown base; after a truncation both are None, as after an update
    (check_chain reports such links as unchecked).  `p` is unchanged."""
    return _resize_rows_many([p], [(keep_rows, values)], [base], lib)[0]


def append_tensor_rows(p, values, base=None, lib=None):
    """resize_tensor_rows(p, p.shape[0], values): p's tensor with the rows of `values` appended along dimension 0 -- a KV cache or a token buffer
    that grows, an embedding table that gains vocabulary rows -- at the cost of the last chunk's decode and the new chunks' encode."""
    _row_bytes(p, "append")
    return _resize_rows_many([p], [(p.shape[0], values)], [base], lib)[0]


def truncate_tensor_rows(p, rows, lib=None):
    """resize_tensor_rows(p, rows): the first `rows` rows of dimension 0 of p's tensor."""
    return _resize_rows_many([p], [(rows, None)], [None], lib)[0]


def append_state_dict_rows(packed, rows, base=None, lib=None):
    """append_tensor_rows for several tensors of a packed state dict: `rows` is {name: values}, and the result a new dict in which those names have
    the grown PackedTensors and every other name the PackedTensor of `packed` itself.  One batched bz3_hip_resize_device_many call per distinct
    block size among the named tensors, as pack_state_dict makes one compress call per block size.  `base`: {name: the rows of that tensor's
    grown base that pair with its new rows}, needed for the named tensors that were packed against one.  A name that is not in `packed`:
    ValueError.  Everything is checked before any GPU work; `packed` is unchanged."""
    unknown = [k for k in rows if k not in packed]
    if unknown:
        raise ValueError(f"append_state_dict_rows: rows for {unknown[0]!r}, which is not in the dict")
    names = list(rows)
    out = dict(packed)
    if names:
        for k in names:
            _row_bytes(packed[k], f"tensor {k!r}")
        out.update(zip(names, _resize_rows_many([packed[k] for k in names], [(packed[k].shape[0], rows[k]) for k in names],
                                                [None if base is None else base.get(k) for k in names], lib)))
    return out


def sync_tensors(frames, datas, olds, planes=1, bases=None, block_sizes=None, lib=None, counts=False):
    """New frames of datas[i] made from frames[i], which decode to olds[i], for many frames in ONE call (bz3_hip_sync_device_many) and one
    synchronisation, when nobody knows where the tensors changed: datas[i] is compared with olds[i] on the device, chunk by chunk and byte for
    byte, only the chunks that differ are coded again, from datas[i] alone, and every other chunk is copied as it is.  Nothing is decoded
    ("Sync").  Result i is byte for byte the frame compress_tensor gives for datas[i], provided olds[i] is what frames[i] decodes to:
    the caller vouches for that.  frames, datas and olds: contiguous uint8 tensors on one GPU, datas[i] and olds[i] of one size, which must be the
    size frames[i] decodes to (Bz3Error with BZ3_ERR_DATA_TOO_BIG otherwise; resize_tensors changes a size).  `planes` as in decompress_tensors.
    `bases[i]`: None, or for a frame made against a base THE WHOLE base, of datas[i]'s size.  `block_sizes`: the block sizes the frames were made
    with where the caller knows them (PackedTensor.block_size); without them the 13 header bytes of all frames are read from the device once,
    which is a second synchronisation.  They only size the outputs, which are views of one allocation with room for every chunk coded again,
    13 + chunks * (8 + bz3_bound(block size)) bytes each (.clone() one to drop the rest).  The inputs are never written.  Returns the list of
    frames, and with counts=True also the list of the numbers of chunks that were coded again.  Raises Bz3Error with .index / .codes / .outs as
    compress_tensors does; a frame that fails has no output.  [] returns []."""
    import torch

    frames = [_device_u8(f, f"frames[{i}]") for i, f in enumerate(frames)]
    n = len(frames)
    datas = [_device_u8(d, f"datas[{i}]") for i, d in enumerate(datas)]
    olds = [_device_u8(o, f"olds[{i}]") for i, o in enumerate(olds)]
    if len(datas) != n or len(olds) != n:
        raise ValueError(f"sync_tensors: {n} frames, {len(datas)} data tensors and {len(olds)} old tensors")
    for i, (d, o) in enumerate(zip(datas, olds)):
        if d.numel() != o.numel():
            raise ValueError(f"sync_tensors: datas[{i}] holds {d.numel()} bytes, olds[{i}] {o.numel()}")
    if not frames:
        return ([], []) if counts else []
    ks = _planes_arg(planes, n)
    bases = [_base_u8(b, d, f"bases[{i}]") for i, (b, d) in enumerate(zip(_bases_arg(bases, n), datas))]
    dev = _same_device(frames + datas + olds, "sync_tensors")
    L = lib or load()
    if block_sizes is None:
        heads = torch.stack([torch.nn.functional.pad(f[:13], (0, 13 - min(13, f.numel()))) for f in frames]).cpu().numpy()
        bss = [int.from_bytes(bytes(h[5:9]), "little") for h in heads]
        # (a header that lies: a chunk takes 8 bytes of its frame at least, and the call refuses the frame or finds the output too small)
        chunks = [min(int.from_bytes(bytes(h[9:13]), "little"), max(f.numel() - 13, 0) // 8) for h, f in zip(heads, frames)]
    else:
        if len(block_sizes) != n:
            raise ValueError(f"sync_tensors: {n} frames and {len(block_sizes)} block sizes")
        bss = [_effective_block_size(int(b), d.numel()) for b, d in zip(block_sizes, datas)]
        chunks = [-(-d.numel() // bs) for d, bs in zip(datas, bss)]
    bss = [min(max(b, _KiB65), _MiB511) for b in bss]
    caps = [13 + c * (8 + L.bz3_bound(bs)) for c, bs in zip(chunks, bss)]
    outs = _carve(sum(caps), caps, dev)
    out_sizes = (C.c_size_t * n)(*caps)
    recoded = (C.c_uint32 * n)()
    rcs = (C.c_int * n)()
    torch.cuda.synchronize(dev)
    rc = L.bz3_hip_sync_device_many(n, (C.c_uint32 * n)(*ks), _ptrs(frames), (C.c_size_t * n)(*[f.numel() for f in frames]),
                                    (C.c_void_p * n)(*[d.data_ptr() if d.numel() else None for d in datas]),
                                    (C.c_void_p * n)(*[o.data_ptr() if o.numel() else None for o in olds]), (C.c_size_t * n)(*[d.numel() for d in datas]),
                                    _ptrs_or_null(bases), _ptrs(outs), out_sizes, recoded, rcs)
    res = [o[: out_sizes[i]] for i, o in enumerate(outs)]
    if rc != BZ3_OK:
        codes = list(rcs)
        idx = next(i for i, c in enumerate(codes) if c != BZ3_OK)
        raise Bz3Error(codes[idx], "bz3_hip_sync_device_many", index=idx, codes=codes, outs=res)
    return (res, list(recoded)) if counts else res


def sync_tensor_bytes(frame, data, old, planes=1, base=None, block_size=None, lib=None, counts=False):
    """The frame of `data` made from `frame`, which decodes to `old` (bz3_hip_sync_device): sync_tensors for one frame.  With counts=True the
    pair (frame, chunks coded again)."""
    try:
        got = sync_tensors([frame], [data], [old], planes=planes, bases=None if base is None else [base], lib=lib,
                           block_sizes=None if block_size is None else [block_size], counts=counts)
    except Bz3Error as e:
        raise Bz3Error(e.code, "bz3_hip_sync_device") from None
    return (got[0][0], got[1][0]) if counts else got[0]


def _sync_many(ps, xs, prevs, bases, check_prev, lib, labels):
    """The PackedTensors of xs[i] made from ps[i], which hold prevs[i]: every argument is checked before any GPU work, then ONE batched checksum
    call over every prev that is checked, every base whose checksum is known and every new tensor, then one bz3_hip_sync_device_many call per
    distinct block size.  Returns (the PackedTensors, per tensor (chunks coded again, chunks))."""
    import torch

    raws, praws, braws = [], [], []
    for p, x, prev, b, label in zip(ps, xs, prevs, bases, labels):
        if not isinstance(p, PackedTensor):
            raise TypeError("sync: a PackedTensor is expected")
        for t, what in ((x, "the new tensor"), (prev, "the previous tensor")):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != p.dtype or tuple(t.shape) != tuple(p.shape):
                raise TypeError(f"sync: {what} of {label} must be a {p.dtype} GPU tensor of shape {tuple(p.shape)}")
            if t.device != p.frame.device:
                raise ValueError(f"sync: {what} of {label} is on {t.device}, the frame on {p.frame.device}")
        if p.delta and b is None:
            raise ValueError(f"sync: {label} was packed against a base, which is needed to code its changed chunks")
        if not p.delta:
            b = None  # (a base beside a tensor that was packed without one is not used)
        raws.append(_as_bytes(x, f"the new tensor of {label}"))
        praws.append(_as_bytes(prev, f"the previous tensor of {label}"))
        braws.append(_base_bytes(b, p.nbytes, p.frame.device, f"the base of {label}"))
    n = len(ps)
    if not n:
        return [], []
    L = lib or load()
    # one batched call: the previous tensors that are checked, the bases whose checksum is known, and the new tensors
    sums = _crcs_where([r if check_prev and p.crc is not None else None for p, r in zip(ps, praws)] +
                       [b if b is not None and p.base_crc is not None else None for p, b in zip(ps, braws)] + raws, L)
    for p, got, gotb, label in zip(ps, sums[:n], sums[n : 2 * n], labels):
        if got is not None and got != p.crc:
            raise ValueError(f"sync: the previous tensor of {label} is not the tensor this frame was packed from (its checksum differs)")
        if gotb is not None and gotb != p.base_crc:
            raise ValueError(f"sync: the base of {label} is not the tensor this frame was packed against (its checksum differs)")
    frames, recoded = [None] * n, [0] * n
    for bs in sorted({p.block_size for p in ps}):
        idx = [i for i in range(n) if ps[i].block_size == bs]
        got, cnt = sync_tensors([ps[i].frame for i in idx], [raws[i] for i in idx], [praws[i] for i in idx], planes=[ps[i].planes for i in idx],
                                bases=[braws[i] for i in idx], block_sizes=[bs] * len(idx), lib=L, counts=True)
        for i, f, c in zip(idx, got, cnt):
            frames[i], recoded[i] = f, c
    chunks = [-(-p.nbytes // _effective_block_size(p.block_size, p.nbytes)) for p in ps]
    out = [PackedTensor(f, p.dtype, p.shape, p.planes, p.block_size, p.nbytes, p.delta, p.base_crc, c) for f, p, c in zip(frames, ps, sums[2 * n :])]
    return out, list(zip(recoded, chunks))


def sync_tensor(p, x, prev, base=None, check_prev=True, lib=None):
    """A new PackedTensor of `x` made from p, which holds `prev`, when nobody knows where the tensor changed -- a fine-tune with frozen layers, an
    MoE step that reached a few experts, a sparse embedding step --: x is compared with prev on the GPU, chunk by chunk and byte for byte, only
    the chunks that differ are coded again and every other chunk of p.frame is copied undecoded (bz3_hip_sync_device; nothing is decoded).  Its
    frame is byte for byte the one pack_tensor gives for x at p.block_size and p.planes.  `x` and `prev`: GPU tensors of p's dtype and shape on
    the frame's GPU (TypeError otherwise).  `base`: as in pack_tensor, the WHOLE base, needed where p was packed against one (ValueError without
    it, or where its checksum is not p.base_crc).  `check_prev`: where p.crc is known, the checksum of prev's bytes must equal it (ValueError),
    which is checked before any coding work and in the same batched call (crc32c_tensors) as the checksum of x, the result's `crc`; with
    check_prev=False, or p.crc None, the caller vouches that prev is what p holds (another prev gives a frame that mixes old and new chunks, and
    no error).  planes, block_size, dtype, shape, nbytes, delta and base_crc are carried over.  `p` is unchanged."""
    return _sync_many([p], [x], [prev], [base], check_prev, lib, ["the tensor"])[0][0]


def sync_state_dict(packed, sd, prev, base=None, check_prev=True, lib=None, stats=None):
    """sync_tensor for the tensors of a dict: `sd` is {name: new tensor}, `prev` {name: the tensor packed[name] holds} (it may hold more names),
    and the result a new dict in which the names of sd have new PackedTensors and every other name the PackedTensor of `packed` itself.  One
    bz3_hip_sync_device_many call per distinct block size over the names of sd, whose changed chunks share its windows of up to 256 blocks: a
    checkpoint of which 1 % changed codes 1 % of its chunks, in one window where pack_state_dict takes chunks / 256.  `base`: {name: base} for
    the tensors that were packed against one.  A name of sd that is not in `packed`, or that `prev` lacks: ValueError.  `stats`: a dict that
    gets {name: (chunks coded again, chunks)}.  Everything is checked before any GPU work; `packed` is unchanged."""
    for k in sd:
        if k not in packed:
            raise ValueError(f"sync_state_dict: {k!r} is not in the packed dict")
        if k not in prev:
            raise ValueError(f"sync_state_dict: the previous tensor of {k!r} is missing")
    names = list(sd)
    out = dict(packed)
    if names:
        got, counts = _sync_many([packed[k] for k in names], [sd[k] for k in names], [prev[k] for k in names],
                                 [None if base is None else base.get(k) for k in names], check_prev, lib, [repr(k) for k in names])
        out.update(zip(names, got))
        if isinstance(stats, dict):
            stats.update(zip(names, counts))
    return out


def _slice_of(p, sl, what):
    """(shape, (offset, run, stride, count)) of the slice sl = (dim, start, stop) of a PackedTensor; None is the whole tensor."""
    if not isinstance(p, PackedTensor):
        raise TypeError("unpack: a PackedTensor is expected")
    shape = tuple(p.shape)
    if sl is None:
        return shape, (0, p.nbytes, p.nbytes, 1)
    dim, start, stop = (int(v) for v in sl)
    if not shape:
        raise ValueError(f"{what}: a 0-d tensor has no dimension to slice")
    if not -len(shape) <= dim < len(shape):
        raise ValueError(f"{what}: dimension {dim} of a tensor of {len(shape)} dimensions")
    dim %= len(shape)
    if not 0 <= start <= stop <= shape[dim]:
        raise ValueError(f"{what}: ({start}, {stop}) of a dimension of {shape[dim]}")
    numel, inner, count = 1, 1, 1
    for d, v in enumerate(shape):
        numel *= v
        if d > dim:
            inner *= v
        if d < dim:
            count *= v
    inner *= p.nbytes // numel if numel else 0  # the element's bytes (a complex element whole)
    return shape[:dim] + (stop - start,) + shape[dim + 1 :], (start * inner, (stop - start) * inner, shape[dim] * inner, count)


def _unpack_parts_many(ps, shapes, sizes, whole, outs, lib, bases, what, decode):
    """What the partial unpack calls share.  Tensor i comes back with shapes[i] from the sizes[i] bytes that decode(raws, braws) reads
    into the uint8 views raws (a list of the tensors it got, shorter where a frame ran out); bases[i]: the same part of the base, `what`
    its name in messages; whole: the tensors that come back whole."""
    import torch

    bases = _bases_arg(bases, len(ps))
    braws = []
    for i, (p, b, w, shape) in enumerate(zip(ps, bases, sizes, shapes)):
        if p.delta and b is None:
            raise ValueError(f"unpack: tensor {i} was packed against a base, which is needed to restore it")
        if not p.delta:
            b = None
        elif not isinstance(b, torch.Tensor) or b.dtype != p.dtype or tuple(b.shape) != shape:
            raise ValueError(f"unpack: base {i} must hold the same {what} of the base: {p.dtype} {shape}")
        braws.append(_base_bytes(b, w, p.frame.device, f"base {i}"))
    dev = _same_device([p.frame for p in ps], "unpack")
    if outs is None:
        raws = _carve(0, sizes, dev)  # every output at a multiple of 16 bytes, so that any dtype can view it
    else:
        raws = []
        for p, o, shape in zip(ps, outs, shapes):
            if not isinstance(o, torch.Tensor) or o.dtype != p.dtype or tuple(o.shape) != shape or not o.is_contiguous():
                raise TypeError(f"unpack: `out` must be a contiguous tensor of the packed dtype and of the {what}'{'' if what.endswith('s') else 's'} shape")
            raws.append(_as_bytes(o, "out"))
    got = decode(raws, braws)
    for i, (g, w) in enumerate(zip(got, sizes)):
        if g.numel() != w:
            raise Bz3Error(BZ3_ERR_TRUNCATED_DATA, f"unpack: the frame of tensor {i} holds {g.numel()} of the {w} bytes of its {what};", g)
    if whole:  # a tensor that comes back whole must be all its frame decodes to (unpack_tensor fails with BZ3_ERR_DATA_TOO_BIG on a longer frame): one walk over those frames' chunk headers
        n = len(whole)
        need, rcs = (C.c_size_t * n)(), (C.c_int * n)()
        (lib or load()).bz3_hip_frame_decoded_sizes_device(n, _ptrs([ps[i].frame for i in whole]), (C.c_size_t * n)(*[ps[i].frame.numel() for i in whole]), need, rcs)
        for i, d in zip(whole, need):
            if d != ps[i].nbytes:
                raise Bz3Error(BZ3_ERR_DATA_TOO_BIG if d > ps[i].nbytes else BZ3_ERR_TRUNCATED_DATA, f"unpack: the frame of tensor {i} decodes to {d} bytes, the tensor has {ps[i].nbytes};")
    return list(outs) if outs is not None else [_from_bytes(r, p.dtype, shape) for r, p, shape in zip(raws, ps, shapes)]


def _unpack_slices_many(ps, slices, outs, lib, bases):
    """The slices slices[i] = (dim, start, stop) of every PackedTensor (None: the whole tensor), in ONE
    bz3_hip_decompress_device_strided_many call.  bases[i]: the same slice of the base."""
    shapes, params = [], []
    for i, (p, sl) in enumerate(zip(ps, slices)):
        shape, q = _slice_of(p, sl, f"tensor {i}")
        shapes.append(shape)
        params.append(q)
    frames, planes = [p.frame for p in ps], [p.planes for p in ps]
    return _unpack_parts_many(ps, shapes, [q[1] * q[3] for q in params], [i for i, sl in enumerate(slices) if sl is None], outs, lib, bases, "slice",
                              lambda raws, braws: decompress_tensors_strided(frames, *zip(*params), raws, planes=planes, bases=braws, lib=lib))


def unpack_tensor_slice(p, dim, start, stop, out=None, base=None, lib=None):
    """x.narrow(dim, start, stop - start) of the tensor x a PackedTensor holds, contiguous, in p.dtype, on the frame's GPU, without the
    whole tensor ever existing there (bz3_hip_decompress_device_strided).  With e the element's bytes and inner = e * prod(shape[dim + 1:])
    the slice is prod(shape[:dim]) runs of (stop - start) * inner bytes, shape[dim] * inner bytes apart, from byte start * inner on.  Only
    the chunks of the frame that hold a byte of a run are decoded: a slice of dimension 0 decodes about its share of the chunks
    (unpack_tensor_rows, whose result this is for dim = 0); a slice of an inner dimension decodes every chunk unless
    shape[dim] * inner exceeds the block size, so that whole chunks fall between two runs -- what it always saves is the full-size
    buffer and the second copy.  Runs shorter than 16 elements of p.planes bytes are gathered byte by byte: correct and
    slow.  A negative `dim` counts from the end.  ValueError for a 0-d tensor, a bad `dim`, and unless
    0 <= start <= stop <= p.shape[dim]; Bz3Error if the frame fails or returns fewer bytes than the slice holds.  `out`: a contiguous
    tensor of p.dtype and of the slice's shape.  A tensor packed against a base needs `base`: THE SAME SLICE of the base, of the dtype and
    of the slice's shape; it may have any strides (base.narrow(dim, start, stop - start) will do) and is then read through a contiguous
    copy; `out` may be it when it is contiguous.  PackedTensor.base_crc covers the whole base and cannot be checked against a slice of it:
    the caller vouches that this is a slice of the right base."""
    return _unpack_slices_many([p], [(dim, start, stop)], None if out is None else [out], lib, [base])[0]


def _index_list(index, what):
    """`index` (a list, a numpy array or a 1-D integer tensor; a device tensor is copied to the host) as a list of ints."""
    if hasattr(index, "detach") and hasattr(index, "cpu"):  # a torch tensor
        if index.dim() != 1 or index.is_floating_point() or index.is_complex() or str(index.dtype) == "torch.bool":
            raise ValueError(f"{what}: the index must be a 1-D integer tensor")
        return [int(v) for v in index.detach().cpu().tolist()]
    if hasattr(index, "ndim") and hasattr(index, "tolist"):  # a numpy array
        if index.ndim != 1 or index.dtype.kind not in "iu":
            raise ValueError(f"{what}: the index must be a 1-D integer array")
        return [int(v) for v in index.tolist()]
    out = []
    for v in index:
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{what}: the index must hold integers")
        out.append(int(v))
    return out


def _index_of(p, sel, what):
    """(shape, (offset, stride, count, pieces), index) of sel = (dim, index), an index_select of a PackedTensor along `dim` with a strictly
    increasing index: runs of consecutive indices are one piece each.  (shape, strided request, None) for sel = None, the whole
    tensor, and for a slice (dim, start, stop), as one piece."""
    if sel is None or len(sel) == 3:
        shape, (o, r, s, c) = _slice_of(p, sel, what)
        return shape, (o, s, c, [(0, r)]), None
    shape, (_, _, stride, count) = _slice_of(p, (sel[0], 0, 0), what)  # (validates p and dim)
    dim = int(sel[0]) % len(p.shape)
    size = p.shape[dim]
    inner = stride // size if size else 0
    idx = _index_list(sel[1], what)
    if any(not 0 <= i < size for i in idx):
        raise ValueError(f"{what}: index out of range for a dimension of {size}")
    if any(a >= b for a, b in zip(idx, idx[1:])):
        raise ValueError(f"{what}: the index must be strictly increasing here")
    pieces = []
    for i in idx:
        if pieces and pieces[-1][0] + pieces[-1][1] == i * inner:
            pieces[-1] = (pieces[-1][0], pieces[-1][1] + inner)
        else:
            pieces.append((i * inner, inner))
    return tuple(p.shape[:dim]) + (len(idx),) + tuple(p.shape[dim + 1 :]), (0, stride, count if idx else 0, pieces), idx


def _unpack_index_many(ps, sels, outs, lib, bases):
    """For every PackedTensor sels[i] = (dim, index) (strictly increasing), a slice (dim, start, stop) or None (the whole tensor), in ONE
    bz3_hip_decompress_device_select_many call.  bases[i]: the same index_select of the base."""
    shapes, reqs = [], []
    for i, (p, sel) in enumerate(zip(ps, sels)):
        shape, q, _ = _index_of(p, sel, f"tensor {i}")
        shapes.append(shape)
        reqs.append(q)
    frames, planes = [p.frame for p in ps], [p.planes for p in ps]
    return _unpack_parts_many(ps, shapes, [q[2] * sum(l for _, l in q[3]) for q in reqs], [i for i, sel in enumerate(sels) if sel is None], outs, lib, bases, "part",
                              lambda raws, braws: decompress_tensors_select(frames, *zip(*reqs), raws, planes=planes, bases=braws, lib=lib))


def _sorted_unique(index, what):
    """(the index as a list, its sorted unique values, for every entry its place among those; None where the index is strictly increasing)."""
    idx = _index_list(index, what)
    if all(a < b for a, b in zip(idx, idx[1:])):
        return idx, idx, None
    uniq = sorted(set(idx))
    where = {v: j for j, v in enumerate(uniq)}
    return idx, uniq, [where[v] for v in idx]


def unpack_tensor_index(p, dim, index, out=None, base=None, lib=None):
    """x.index_select(dim, index) of the tensor x a PackedTensor holds, contiguous, in p.dtype, on the frame's GPU, without the whole tensor
    ever existing there (bz3_hip_decompress_device_select): chosen experts of an [E, ...] tensor, rows of an embedding table, columns.
    `index`: a list, a numpy array or a 1-D integer tensor (a device tensor is copied to the host; the call is synchronous anyway) with
    values in [0, p.shape[dim]), else ValueError.  With e the element's bytes and inner = e * prod(shape[dim + 1:]), every run of
    consecutive indices i .. i + n - 1 is one piece (i * inner, n * inner) of prod(shape[:dim]) periods shape[dim] * inner bytes apart.
    Only the chunks of the frame that hold a byte of a piece are decoded, each once however many pieces it holds.  Pieces shorter than 16
    elements of p.planes bytes are gathered byte by byte: correct and slow.  An index that is not strictly increasing (a permutation,
    duplicates) decodes its sorted unique values and finishes with one torch.index_select on that result, which then exists beside the
    output.  A negative `dim` counts from the end.  `out`: a contiguous tensor of p.dtype and of the result's shape.  A tensor packed
    against a base needs `base`: THE SAME index_select of the base, of the dtype and the result's shape (any strides; `out` may be it
    when it is contiguous); there the index must be strictly increasing, else ValueError.  PackedTensor.base_crc covers the whole base
    and cannot be checked against a part of it: the caller vouches that this is the right base.  An empty index returns an empty tensor
    of the result's shape.  Bz3Error if the frame fails or returns fewer bytes than asked of it."""
    import torch

    idx, uniq, where = _sorted_unique(index, "unpack_tensor_index")
    if where is None:
        return _unpack_index_many([p], [(dim, idx)], None if out is None else [out], lib, [base])[0]
    if isinstance(p, PackedTensor) and p.delta:
        raise ValueError("unpack_tensor_index: a tensor packed against a base takes a strictly increasing index (its base is given in the index's order)")
    part = _unpack_index_many([p], [(dim, uniq)], None, lib, [None])[0]
    d = int(dim) % len(p.shape)
    shape = tuple(p.shape[:d]) + (len(idx),) + tuple(p.shape[d + 1 :])
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != p.dtype or tuple(out.shape) != shape or not out.is_contiguous()):
        raise TypeError("unpack: `out` must be a contiguous tensor of the packed dtype and of the result's shape")
    order = torch.tensor(where, dtype=torch.int64, device=part.device)
    if out is None:
        return torch.index_select(part, d, order)
    torch.index_select(part, d, order, out=out)
    return out


def _update_parts_many(ps, shapes, values, bases, lib, what, words, update):
    """What the partial update calls share: the PackedTensors with a part of shapes[i] replaced by values[i], a tensor of that shape, through the
    ONE call update(frames, the values' bytes, the bases' bytes, planes=, lib=, block_sizes=), which returns the new frames.  bases[i]: the same part
    of the base, `what` its name in messages ("rows", "part"); words(i): tensor i's name, that of its values and that of its base.  Every argument
    is checked before any GPU work."""
    import torch

    raws, braws = [], []
    for i, (p, shape, v, b) in enumerate(zip(ps, shapes, values, _bases_arg(bases, len(ps)))):
        name, vname, bname = words(i)
        if not isinstance(v, torch.Tensor) or v.device.type != "cuda":
            raise TypeError(f"update: {vname} must be a torch tensor on a GPU")
        if v.dtype != p.dtype or tuple(v.shape) != tuple(shape):
            raise TypeError(f"update: {vname} must be {p.dtype} of shape {tuple(shape)}")
        if p.delta and b is None:
            raise ValueError(f"update: {name} was packed against a base, whose {'rows are needed to code the new ones' if what == 'rows' else what + ' is needed to code the new one'}")
        if not p.delta:
            b = None
        elif not isinstance(b, torch.Tensor) or b.dtype != p.dtype or tuple(b.shape) != tuple(shape):
            raise ValueError(f"update: {bname} must hold the same {what} of the base: {p.dtype} {tuple(shape)}")
        raw = _as_bytes(v, vname)
        raws.append(raw)
        braws.append(_base_bytes(b, raw.numel(), p.frame.device, bname))
    frames = update([p.frame for p in ps], raws, braws, planes=[p.planes for p in ps], lib=lib, block_sizes=[p.block_size for p in ps])
    return [PackedTensor(f, p.dtype, p.shape, p.planes, p.block_size, p.nbytes, p.delta, p.base_crc, None) for f, p in zip(frames, ps)]


def _update_index_many(ps, sels, values, bases, lib, names=None):
    """For every PackedTensor sels[i] = (dim, index) (strictly increasing) or a slice (dim, start, stop): the PackedTensors with that part replaced
    by values[i], through ONE bz3_hip_update_device_select_many call.  bases[i]: the same part of the base."""
    whats = [f"tensor {i}" if names is None else repr(names[i]) for i in range(len(ps))]
    shapes, reqs = [], []
    for p, sel, what in zip(ps, sels, whats):
        shape, q, _ = _index_of(p, sel, f"update: {what}")
        shapes.append(shape)
        reqs.append(q)
    return _update_parts_many(ps, shapes, values, bases, lib, "part", lambda i: (whats[i], f"the values of {whats[i]}", f"the base of {whats[i]}"),
                              lambda frames, raws, braws, **kw: update_tensors_select(frames, *zip(*reqs), raws, bases=braws, **kw))


def update_tensor_slice(p, dim, start, stop, values, base=None, lib=None):
    """The write mirror of unpack_tensor_slice: a new PackedTensor that holds p's tensor x with x.narrow(dim, start, stop - start) replaced by
    `values`, on the frame's GPU, without the tensor ever being materialised (bz3_hip_update_device_select with one piece per period: a
    column block of a weight matrix).  Its frame is byte for byte the one pack_tensor gives for the updated tensor at p.block_size and p.planes.
    Only the chunks that hold a byte of the slice are coded again; a slice of an inner dimension usually touches every chunk, and each is then
    decoded once and coded once -- what the call saves is the full-size tensor and the chunks between two runs where there are any.  Runs
    shorter than 16 elements of p.planes bytes are scattered byte by byte: correct and slow.  `values`: a GPU tensor of p's dtype and of the
    slice's shape (TypeError otherwise; any strides); ValueError for a 0-d tensor, a bad `dim` and unless 0 <= start <= stop <= p.shape[dim].  All
    of that is checked before any GPU work.  A tensor packed against a base needs `base`: THE SAME SLICE of the base.  Everything but `crc`,
    which is None as after update_tensor_rows, is carried over; `p` is unchanged."""
    return _update_index_many([p], [(dim, start, stop)], [values], [base], lib)[0]


def _update_index_arg(p, dim, index, values, has_base, what):
    """((dim, the sorted index), values in that order) for an index_copy: duplicates are a ValueError, and an index that is not increasing is
    sorted on the host and `values` permuted once on the device."""
    import torch

    idx = _index_list(index, what)
    if len(set(idx)) != len(idx):
        raise ValueError(f"{what}: the index holds duplicates, for which index_copy has no defined result")
    if all(a < b for a, b in zip(idx, idx[1:])):
        return (dim, idx), values
    if has_base:
        raise ValueError(f"{what}: a tensor packed against a base takes a strictly increasing index (its base is given in the index's order)")
    order = sorted(range(len(idx)), key=idx.__getitem__)
    sel = (dim, [idx[j] for j in order])
    shape, _, _ = _index_of(p, sel, what)  # (validates p, dim and the index's range before anything is moved)
    if not isinstance(values, torch.Tensor) or values.device.type != "cuda":
        raise TypeError(f"{what}: the values must be a torch tensor on a GPU")
    if values.dtype != p.dtype or tuple(values.shape) != tuple(shape):
        raise TypeError(f"{what}: the values must be {p.dtype} of shape {tuple(shape)}")
    return sel, torch.index_select(values, int(dim) % len(p.shape), torch.tensor(order, dtype=torch.int64, device=values.device))


def update_tensor_index(p, dim, index, values, base=None, lib=None):
    """A new PackedTensor that holds x.index_copy(dim, index, values) of the tensor x a PackedTensor holds, on the frame's GPU, without the tensor
    ever being materialised (bz3_hip_update_device_select): the embedding rows a sparse optimiser step touched, a handful of experts of an
    [E, ...] tensor, scattered columns.  Its frame is byte for byte the one pack_tensor gives for the updated tensor at p.block_size and
    p.planes.  `index` is what unpack_tensor_index accepts, with values in [0, p.shape[dim]), but duplicates are a ValueError: index_copy with
    duplicates has no defined result.  Every run of consecutive indices is one piece, as there.  Only the chunks of the frame that hold a byte of
    a piece are coded again; of those the ones the pieces do not cover whole are decoded first, each once however many pieces it holds, and
    every other chunk is copied undecoded.  Pieces shorter than 16 elements of p.planes bytes are scattered byte by byte: correct and slow.  An
    index that is not increasing is sorted on the host and `values` permuted once on the device with torch.index_select; with a base such an
    index is a ValueError, as on the read side.  `values`: a GPU tensor of p's dtype and of the shape of x.index_select(dim, index) (TypeError
    otherwise).  All of that is checked before any GPU work.  A tensor packed against a base needs `base`: THE SAME index_select of the base.
    planes, block_size, dtype, shape, nbytes, delta and base_crc are carried over; `crc` of the result is None (update_tensor_rows says why).  An
    empty index gives a copy of the frame.  `p` is unchanged."""
    if not isinstance(p, PackedTensor):
        raise TypeError("update: a PackedTensor is expected")
    sel, values = _update_index_arg(p, dim, index, values, p.delta, "update_tensor_index")
    return _update_index_many([p], [sel], [values], [base], lib)[0]


def update_state_dict(packed, rows=None, slices=None, index=None, base=None, lib=None):
    """The write mirror of unpack_state_dict's three keywords: `rows` is {name: (start, values)} (update_tensor_rows), `slices`
    {name: (dim, start, stop, values)} (update_tensor_slice) and `index` {name: (dim, index, values)} (update_tensor_index).  Every named tensor goes
    through ONE bz3_hip_update_device_select_many call, and the result is a new dict in which those names have new PackedTensors (crc None) and
    every other name the PackedTensor of `packed` itself.  `base`: {name: the same part of that tensor's base}, needed for the named tensors that
    were packed against one.  A name in more than one keyword, or one that is not in `packed`: ValueError.  Everything is checked before any GPU
    work; `packed` is unchanged."""
    import torch

    want = {}
    for arg, d in (("rows", rows), ("slices", slices), ("index", index)):
        for k, v in (d or {}).items():
            if k in want:
                raise ValueError(f"update_state_dict: {k!r} is named by more than one of rows, slices and index")
            if k not in packed:
                raise ValueError(f"update_state_dict: {arg} for {k!r}, which is not in the dict")
            want[k] = (arg, tuple(v))
    names = list(want)
    out = dict(packed)
    if not names:
        return out
    sels, values = [], []
    for k in names:
        arg, v = want[k]
        p = packed[k]
        if not isinstance(p, PackedTensor):
            raise TypeError("update: a PackedTensor is expected")
        if arg == "rows":
            start, vals = v
            _row_bytes(p, repr(k))
            if not isinstance(vals, torch.Tensor):
                raise TypeError(f"update: the rows of {k!r} must be a torch tensor on a GPU")
            sels.append((0, int(start), int(start) + (vals.shape[0] if vals.dim() else 0)))
        elif arg == "slices":
            dim, start, stop, vals = v
            sels.append((dim, start, stop))
        else:
            dim, idx, vals = v
            sel, vals = _update_index_arg(p, dim, idx, vals, p.delta, f"update_state_dict: {k!r}")
            sels.append(sel)
        values.append(vals)
    out.update(zip(names, _update_index_many([packed[k] for k in names], sels, values, [None if base is None else base.get(k) for k in names], lib, names)))
    return out


def pack_state_dict(sd, block_size=16 << 20, planes=None, lib=None, base=None, checksum=True):
    """pack_tensor for every tensor of a dict, batched: {name: PackedTensor}, each equal to pack_tensor(sd[name], block_size, planes).
    One bz3_hip_compress_device_delta_many call per distinct lossless block size (the C call takes one block size): the tensors whose
    size is no multiple of `block_size` share one call and its windows of up to 256 blocks; those whose block size had to move
    (_lossless_block_size) go in one more call per moved size, typically one or two.  All tensors on one GPU.  `planes`: None
    (DEFAULT_PLANES per dtype; DELTA_PLANES for a tensor packed against a base), an int, or {name: int}.  `base`: a dict of earlier versions (the
    previous checkpoint, the model a fine-tune started from): a tensor whose name is in it with the same dtype and shape is packed
    against it (pack_tensor's `base`), every other one without a base, all in the same calls.  `checksum`: record every tensor's own
    checksum in its `.crc`; these and the bases' checksums are computed by ONE bz3_hip_crc32c_device_many call per pack call."""
    names = list(sd)
    if isinstance(planes, dict):
        planes = [planes[k] for k in names]
    if not names:
        return {}
    bases = None
    if base is not None:
        bases = [base.get(k) for k in names]
        bases = [b if b is not None and getattr(b, "dtype", None) == sd[k].dtype and getattr(b, "shape", None) == sd[k].shape else None for k, b in zip(names, bases)]
    return dict(zip(names, _pack_many([sd[k] for k in names], block_size, planes, lib, bases, checksum)))


def unpack_state_dict(packed, lib=None, base=None, inplace=False, check_base=True, rows=None, verify=False, slices=None, index=None):
    """The tensors of pack_state_dict's result, decoded in ONE batched call (bz3_hip_decompress_device_delta_many).  `base`: the dict
    pack_state_dict was given; every tensor packed against a base needs its entry (unpack_tensor's rules and check_base).  With
    inplace=True those base tensors themselves are updated and returned (no second copy of the model in memory); tensors packed
    without a base are returned in new memory as usual.  `rows`: {name: (start, stop)}: those tensors come back as their rows
    [start, stop) of dimension 0 alone (unpack_tensor_rows), the names not in it whole, all of them through ONE
    bz3_hip_decompress_device_range_many call that decodes only the chunks it needs.  `base` is then the whole base dict as ever: check_base checks
    every base tensor whole against its base_crc (one read of it, for the tensors read by rows too), then their rows are taken here.
    With inplace=True, ValueError.  All bases are checked by one batched checksum call, before anything is decoded.  `verify`: after
    decoding, one more batched call over the outputs and a ValueError that names the first tensor whose bytes do not have its `.crc`
    (tensors without one are skipped); with inplace=True the bases have been overwritten by then.  With `rows`, ValueError: a checksum
    of the whole cannot vouch for a slice.  `slices`: {name: (dim, start, stop)}: those tensors come back as
    x.narrow(dim, start, stop - start) (unpack_tensor_slice), the names in `rows` as their rows and the others whole, all of them through
    ONE bz3_hip_decompress_device_strided_many call.  `base`, check_base, verify and inplace are as with `rows`: the whole base dict,
    every base checked whole, its slice taken here; ValueError with verify=True or inplace=True.  A name in both `rows` and `slices`:
    ValueError.  slices=None runs what the function ran before it had the argument.  `index`: {name: (dim, index)}: those tensors come back
    as x.index_select(dim, index) (unpack_tensor_index; an index that is not strictly increasing is sorted and made unique for the decode
    and restored by one torch.index_select, which a tensor packed against a base does not allow), the names in `rows` and `slices` as
    there and the others whole, all of them through ONE bz3_hip_decompress_device_select_many call.  `base`, check_base, verify and
    inplace are as with `slices`.  A name in more than one of `rows`, `slices` and `index`: ValueError.  index=None runs what the function
    ran before it had the argument."""
    names = list(packed)
    if index is not None or slices is not None or rows is not None:
        # one partial path: the narrowest call that the arguments given call for reads every tensor, whole ones included
        arg, part = ("index", "a part of") if index is not None else ("slices", "a slice of") if slices is not None else ("rows", "rows for")
        if verify:
            raise ValueError(f"unpack_state_dict: verify=True and {arg} do not go together (the checksum covers the whole tensor)")
        if inplace:
            raise ValueError(f"unpack_state_dict: {arg} and inplace=True do not go together")
        want = {k: (0, int(r[0]), int(r[1])) for k, r in (rows or {}).items()}  # rows are slices of dimension 0
        for k, sl in (slices or {}).items():
            if k in want:
                raise ValueError(f"unpack_state_dict: {k!r} is in both rows and slices")
            want[k] = tuple(sl)
        order = {}
        for k, (dim, idx) in (index or {}).items():
            if k in want:
                raise ValueError(f"unpack_state_dict: {k!r} is in index and in rows or slices")
            if k in packed:
                _, uniq, order[k] = _sorted_unique(idx, repr(k))
                want[k] = (dim, uniq)
            else:
                want[k] = (dim, idx)
        unknown = [k for k in want if k not in packed]
        if unknown:
            raise ValueError(f"unpack_state_dict: {part} {unknown[0]!r}, which is not in the dict")
        if not names:
            return {}
        import torch

        ps = [packed[k] for k in names]
        sels = [want.get(k) for k in names]
        for k, p, sel in zip(names, ps, sels):  # every request is validated before anything is read (rows alone: by _unpack_rows_many, in its own words)
            if arg != "rows":
                _index_of(p, sel, repr(k))
            if order.get(k) is not None and p.delta:
                raise ValueError(f"unpack_state_dict: {k!r} was packed against a base and takes a strictly increasing index")
        bases, whole = [], []
        L = lib or load()
        for k, p, sel in zip(names, ps, sels):
            b = base.get(k) if base is not None and p.delta else None
            fits = isinstance(b, torch.Tensor) and b.dtype == p.dtype and tuple(b.shape) == tuple(p.shape)
            # the whole base is at hand here, for the tensors read in part too: check it as unpack_tensor does, before anything is decoded
            whole.append(_base_bytes(b, p.nbytes, p.frame.device, f"base {k!r}") if check_base and fits and p.base_crc is not None else None)
            if fits and sel is not None and len(sel) == 3:
                if arg != "rows" or (len(p.shape) and 0 <= sel[1] <= sel[2] <= p.shape[0]):
                    b = b.narrow(int(sel[0]) % len(p.shape), int(sel[1]), int(sel[2]) - int(sel[1]))
            elif fits and sel is not None:
                b = b.index_select(int(sel[0]) % len(p.shape), torch.tensor(sel[1], dtype=torch.int64, device=b.device))
            bases.append(b)
        _check_bases(ps, whole, [repr(k) for k in names], L)
        if arg == "index":
            parts = _unpack_index_many(ps, sels, None, lib, bases)
        elif arg == "slices":
            parts = _unpack_slices_many(ps, sels, None, lib, bases)
        else:
            parts = _unpack_rows_many(ps, [None if sel is None else sel[1:] for sel in sels], None, lib, bases)
        got = dict(zip(names, parts))
        for k, where in order.items():
            if where is not None:
                got[k] = torch.index_select(got[k], int(index[k][0]) % len(packed[k].shape), torch.tensor(where, dtype=torch.int64, device=got[k].device))
        return got
    if not names:
        return {}
    ps = [packed[k] for k in names]
    bases = [base.get(k) if base is not None and p.delta else None for k, p in zip(names, ps)]
    if not inplace or not any(p.delta for p in ps):
        return dict(zip(names, _unpack_many(ps, None, lib, bases, check_base, verify, names)))
    # in place: the delta tensors decode into their bases, the others into new memory; one call
    import torch

    fresh = _carve(0, [0 if p.delta else p.nbytes for p in ps], _same_device([p.frame for p in ps], "unpack"))
    outs = []
    for k, p, b, f in zip(names, ps, bases, fresh):
        if not p.delta:
            outs.append(_from_bytes(f, p.dtype, p.shape))
        elif not isinstance(b, torch.Tensor) or b.dtype != p.dtype or b.shape != p.shape:
            raise ValueError(f"unpack: {k} was packed against a base of {p.dtype} {tuple(p.shape)}, which is needed to restore it")
        else:
            outs.append(b)
    return dict(zip(names, _unpack_many(ps, outs, lib, bases, check_base, verify, names)))


def update_state_dict_rows(packed, rows, base=None, lib=None):
    """update_tensor_rows for several tensors of a packed state dict in ONE bz3_hip_update_device_range_many call: `rows` is
    {name: (start, values)}, and the result a new dict in which those names have new PackedTensors (crc None) and every other name the
    PackedTensor of `packed` itself.  `base`: {name: the same rows of that tensor's base}, needed for the named tensors that were packed
    against one.  A name that is not in `packed`: ValueError.  Everything is checked before any GPU work; `packed` is unchanged."""
    unknown = [k for k in rows if k not in packed]
    if unknown:
        raise ValueError(f"update_state_dict_rows: rows for {unknown[0]!r}, which is not in the dict")
    names = list(rows)
    out = dict(packed)
    if names:
        out.update(zip(names, _update_rows_many([packed[k] for k in names], [rows[k] for k in names], [None if base is None else base.get(k) for k in names], lib)))
    return out


# ---- chains of checkpoints ----------------------------------------------------------------------------------------------------
def check_chain(steps):
    """Validates a chain of packed dicts (pack_state_dict's results, oldest first) from their metadata alone: no GPU, no frame is read.
    Step 0 must hold no delta tensor; for every delta tensor of step t + 1, step t must hold that name with the same dtype, shape and
    nbytes, and its `base_crc` must equal steps[t][name].crc.  ValueError names the first violation (the step and the tensor).  Returns
    the links that could not be checked because one of the two checksums is None: a list of (t, name), the link from step t to t + 1."""
    unchecked = []
    for t, step in enumerate(steps):
        for name, p in step.items():
            if not isinstance(p, PackedTensor):
                raise TypeError(f"check_chain: step {t}: {name!r} is not a PackedTensor")
            if not p.delta:
                continue
            if t == 0:
                raise ValueError(f"check_chain: step 0: {name!r} is a delta tensor, and there is no step before it")
            q = steps[t - 1].get(name)
            if q is None:
                raise ValueError(f"check_chain: step {t}: {name!r} is a delta tensor, and step {t - 1} does not hold that name")
            if q.dtype != p.dtype or tuple(q.shape) != tuple(p.shape) or q.nbytes != p.nbytes:
                raise ValueError(f"check_chain: step {t}: {name!r} is {p.dtype} {tuple(p.shape)} of {p.nbytes} bytes, in step {t - 1} it is {q.dtype} {tuple(q.shape)} of {q.nbytes}")
            if p.base_crc is None or q.crc is None:
                unchecked.append((t - 1, name))
            elif p.base_crc != q.crc:
                raise ValueError(f"check_chain: step {t}: {name!r} was packed against a base of checksum {p.base_crc:#010x}, in step {t - 1} it has {q.crc:#010x}")
    return unchecked


def unpack_chain(steps, verify=True, lib=None):
    """The tensors of the last of a chain of packed dicts (a full checkpoint, then deltas, oldest first).  check_chain runs first, so a
    broken chain fails before anything is decoded.  Step 0 is unpacked whole; every later step is unpacked in place against the result so
    far with check_base=False: the metadata links and the chunk CRCs of the frames stand in for reading every base again.  Tensors of a
    step that are not deltas come back in new memory and names a step does not hold are dropped.  `verify` goes to the last step's
    unpack_state_dict: its outputs are checked against their `.crc`.  An empty chain is a ValueError."""
    steps = list(steps)
    if not steps:
        raise ValueError("unpack_chain: no steps")
    check_chain(steps)
    last = len(steps) - 1
    current = unpack_state_dict(steps[0], lib=lib, verify=verify and last == 0)
    for t in range(1, len(steps)):
        current = unpack_state_dict(steps[t], lib=lib, base=current, inplace=True, check_base=False, verify=verify and t == last)
    return current


# ---- checkpoint files ---------------------------------------------------------------------------------------------------------
# b"BZ3TNSR1" | u64 little-endian H | H bytes of UTF-8 JSON, right-padded with spaces so that 16 + H is a multiple of 64 | the data
# section: the frames in dict order, each at a multiple of 16 bytes from the section's start, zero padding between (DESIGN.md,
# "Checkpoint files and batched checksums").  Every frame is an ordinary .bz3 frame.
PACKED_MAGIC = b"BZ3TNSR1"
_ENTRY_KEYS = ("dtype", "shape", "planes", "block_size", "nbytes", "delta", "base_crc", "crc", "offset", "size")


def _opt_int(v):
    return None if v is None else int(v)


def save_packed(path, packed, metadata=None):
    """Writes a {name: PackedTensor} dict (pack_state_dict's result) and `metadata` (anything json can serialise; default {}) to one file
    that load_packed reads back.  The frames may be on any device, the CPU included: those of a GPU are gathered into one buffer there
    and come to the host in ONE copy.  The file is written as path + ".tmp" and then renamed over `path` (os.replace), so a failed save
    leaves an existing file as it was."""
    import json

    import torch

    names = list(packed)
    entries, offs, o = {}, [], 0
    for k in names:
        p = packed[k]
        if not isinstance(k, str) or not isinstance(p, PackedTensor):
            raise TypeError("save_packed: a dict of str -> PackedTensor is expected")
        if not isinstance(p.frame, torch.Tensor) or p.frame.dtype != torch.uint8 or p.frame.dim() != 1:
            raise TypeError(f"save_packed: the frame of {k!r} must be a one-dimensional torch.uint8 tensor")
        size = p.frame.numel()
        entries[k] = {"dtype": str(p.dtype).replace("torch.", ""), "shape": [int(d) for d in p.shape], "planes": int(p.planes), "block_size": int(p.block_size),
                      "nbytes": int(p.nbytes), "delta": bool(p.delta), "base_crc": _opt_int(p.base_crc), "crc": _opt_int(p.crc), "offset": o, "size": size}
        offs.append(o)
        o += (size + 15) & ~15
    head = json.dumps({"version": 1, "metadata": {} if metadata is None else metadata, "tensors": entries}, ensure_ascii=False).encode("utf-8")
    head += b" " * ((0 - (16 + len(head))) % 64)
    host = {}
    for dev in {packed[k].frame.device for k in names}:
        mine = [k for k in names if packed[k].frame.device == dev]
        if dev.type == "cpu":
            host.update({k: packed[k].frame.contiguous() for k in mine})
        else:  # one gather on the device, one copy to the host
            parts = torch.cat([packed[k].frame for k in mine]).cpu().split([packed[k].frame.numel() for k in mine])
            host.update(dict(zip(mine, parts)))
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(PACKED_MAGIC + len(head).to_bytes(8, "little") + head)
            at = 0
            for k, off in zip(names, offs):
                f.write(b"\0" * (off - at))
                f.write(memoryview(host[k].numpy()))
                at = off + host[k].numel()
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def _read_packed_header(f, path):
    """(entries, metadata, offset of the data section, file size) of an open checkpoint file; ValueError for a malformed header."""
    import json
    import math

    import torch

    size = os.fstat(f.fileno()).st_size
    fixed = f.read(16)
    if len(fixed) < 16 or fixed[:8] != PACKED_MAGIC:
        raise ValueError(f"{path}: not a packed tensor file (it does not start with {PACKED_MAGIC!r})")
    hlen = int.from_bytes(fixed[8:], "little")
    if 16 + hlen > size:
        raise ValueError(f"{path}: the header of {hlen} bytes runs past the end of the file")
    try:
        head = json.loads(f.read(hlen).decode("utf-8"))
    except ValueError as e:  # UnicodeDecodeError and json.JSONDecodeError are both ValueErrors
        raise ValueError(f"{path}: the header is not JSON: {e}") from None
    if not isinstance(head, dict) or head.get("version") != 1:
        raise ValueError(f"{path}: version {head.get('version') if isinstance(head, dict) else None!r} of the format, this code reads version 1")
    entries, metadata = head.get("tensors"), head.get("metadata", {})
    if not isinstance(entries, dict):
        raise ValueError(f"{path}: the header holds no tensors")
    for k, e in entries.items():
        if not isinstance(e, dict) or any(key not in e for key in _ENTRY_KEYS):
            raise ValueError(f"{path}: the entry of {k!r} is incomplete")
        dtype = getattr(torch, e["dtype"], None) if isinstance(e["dtype"], str) else None
        if not isinstance(dtype, torch.dtype):
            raise ValueError(f"{path}: {k!r} has the unknown dtype {e['dtype']!r}")
        if e["planes"] not in (1, 2, 4, 8):
            raise ValueError(f"{path}: {k!r} has planes = {e['planes']!r}, which must be 1, 2, 4 or 8")
        if not isinstance(e["shape"], list) or any(not isinstance(d, int) or d < 0 for d in e["shape"]):
            raise ValueError(f"{path}: {k!r} has the shape {e['shape']!r}")
        if e["nbytes"] != math.prod(e["shape"]) * torch.empty(0, dtype=dtype).element_size():
            raise ValueError(f"{path}: {k!r} has nbytes = {e['nbytes']!r}, which is not what {e['dtype']} {e['shape']} holds")
        if any(not isinstance(e[key], int) or isinstance(e[key], bool) or e[key] < 0 for key in ("offset", "size", "block_size")):
            raise ValueError(f"{path}: {k!r} has a bad offset, size or block size")
    return entries, metadata, 16 + hlen, size


def packed_index(path):
    """(entries, metadata) of a file save_packed wrote, from its header alone (no frame is read): entries is {name: {"dtype", "shape",
    "planes", "block_size", "nbytes", "delta", "base_crc", "crc", "offset", "size"}} as the format holds them.  ValueError for a
    malformed header."""
    with open(path, "rb") as f:
        entries, metadata, _, _ = _read_packed_header(f, path)
    return entries, metadata


def load_packed(path, device, names=None):
    """The {name: PackedTensor} dict a file of save_packed holds, with the frames on `device` (a GPU or "cpu"), ready for
    unpack_state_dict / unpack_chain.  `names`: load these tensors alone, in this order (a name the file does not hold: KeyError); only
    their byte ranges are read, into one host buffer that goes to the device in ONE copy; the frames are views of that copy, each at a
    multiple of 16 bytes.  ValueError for a malformed header and for a selected frame that runs past the end of the file; a corrupt frame
    body is found by the decoder (Bz3Error from unpack_*), not here."""
    import torch

    with open(path, "rb") as f:
        entries, _, data_at, size = _read_packed_header(f, path)
        names = list(entries) if names is None else list(names)
        for k in names:
            if k not in entries:
                raise KeyError(k)
            if data_at + entries[k]["offset"] + entries[k]["size"] > size:
                raise ValueError(f"{path}: the frame of {k!r} runs past the end of the file")
        offs, o = [], 0
        for k in names:
            offs.append(o)
            o += (entries[k]["size"] + 15) & ~15
        host = torch.zeros(max(o, 1), dtype=torch.uint8)
        view = memoryview(host.numpy())
        for k, a in zip(names, offs):
            f.seek(data_at + entries[k]["offset"])
            if f.readinto(view[a : a + entries[k]["size"]]) != entries[k]["size"]:
                raise ValueError(f"{path}: the frame of {k!r} could not be read whole")
    buf = host.to(device)
    out = {}
    for k, a in zip(names, offs):
        e = entries[k]
        out[k] = PackedTensor(buf[a : a + e["size"]], getattr(torch, e["dtype"]), torch.Size(e["shape"]), e["planes"], e["block_size"], e["nbytes"], bool(e["delta"]),
                              e["base_crc"], e["crc"])
    return out


def shard_blocks(n_blocks, world_size, rank):
    """Block -> GPU partition of SURVEY.md section 8e: block k belongs to rank k mod world_size."""
    return [k for k in range(n_blocks) if k % world_size == rank]
