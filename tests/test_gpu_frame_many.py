"""-m gpu: the batched frame calls on device memory (include/bz3_hip.h bz3_hip_compress_device_many /
bz3_hip_decompress_device_many / bz3_hip_frame_decoded_sizes_device; bzip3_amd.compress_tensors / decompress_tensors) on torch
tensors: every frame of a batch equals its single-frame call and the real reference, and a batch shares CM launches."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
from oracle_lib import require_ref

pytestmark = pytest.mark.gpu


def _dev(data, room=None):
    import torch

    t = torch.zeros(max(1, room if room is not None else len(data)), dtype=torch.uint8, device="cuda:0")
    if len(data):
        t[: len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    return t[: room if room is not None else len(data)]


def _host(t):
    return bytes(t.cpu().numpy()) if t.numel() else b""


def _ref_frame(bs, data):
    ref = require_ref()
    out = (C.c_uint8 * (ref.lib.bz3_bound(len(data)) + 64))()
    osz = C.c_size_t(len(out))
    assert ref.lib.bz3_compress(bs, data, out, len(data), C.byref(osz)) == 0
    return bytes(out[: osz.value])


def _pieces(text, sizes, seed):
    rng = np.random.default_rng(seed)
    big = text * (max(sizes) // len(text) + 2)
    out = []
    for n in sizes:
        o = int(rng.integers(0, len(big) - n))
        out.append(big[o : o + n])
    return out


def test_batch_parity_over_several_windows(gpu_lib, text):
    """About 300 text tensors of 65-400 KiB and three multi-block ones: more than one window of 256 blocks.  Every frame equals the
    reference's (and, on a sample, compress_tensor's); the batch decodes back."""
    import torch

    rng = np.random.default_rng(21)
    sizes = [int(v) for v in rng.integers(65 * 1024, 400 * 1024, size=300)]
    sizes[17] = 65 * 1024  # exactly the smallest block size
    sizes += [3 * (1 << 20) + 333, 2 * (1 << 20), (1 << 20) + 1]
    datas = _pieces(text, sizes, 22)
    xs = [_dev(d) for d in datas]
    frames = bzip3_amd.compress_tensors(xs, 1 << 20)
    assert len(frames) == len(xs)
    for i, d in enumerate(datas):
        assert _host(frames[i]) == _ref_frame(1 << 20, d), ("reference", i, len(d))
    for i in list(range(0, len(xs), 29)) + [len(xs) - 3, len(xs) - 1]:
        assert torch.equal(frames[i], bzip3_amd.compress_tensor(xs[i], 1 << 20)), ("compress_tensor", i)
    backs = bzip3_amd.decompress_tensors(frames)
    for i, d in enumerate(datas):
        want = len(d) if len(d) % (1 << 20) else len(d) - (1 << 20)  # (sic) src/libbz3.c:914: an exact multiple drops its last block
        assert backs[i].numel() == want and torch.equal(backs[i], xs[i][:want]), ("round trip", i)
    sizes_out = (C.c_size_t * len(frames))()
    rcs = (C.c_int * len(frames))()
    ptrs = (C.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
    lens = (C.c_size_t * len(frames))(*[f.numel() for f in frames])
    assert gpu_lib.bz3_hip_frame_decoded_sizes_device(len(frames), ptrs, lens, sizes_out, rcs) == 0
    assert list(sizes_out) == [b.numel() for b in backs]
    assert bzip3_amd.compress_tensors([]) == [] and bzip3_amd.decompress_tensors([]) == []


def test_batching_shares_cm_launches(gpu_lib, text):
    """300 single-block frames in one call take no more CM launches than one 300-block frame of the same blocks, and far fewer than
    one launch per frame."""
    bs = 80 * 1024
    data = (text * 4)[: 300 * bs]
    x = _dev(data)
    xs = [x[i * bs : (i + 1) * bs] for i in range(300)]
    gpu_lib.bz3_hip_debug_cm_launches(1)
    frames = bzip3_amd.compress_tensors(xs, 1 << 20)  # one full block each (block size bz3_bound(80 KiB); at 80 KiB the one chunk would be the empty one of :914)
    batched = gpu_lib.bz3_hip_debug_cm_launches(1)
    out = _dev(b"", gpu_lib.bz3_bound(len(data)))
    osz = C.c_size_t(out.numel())
    assert gpu_lib.bz3_hip_compress_device(bs, x.data_ptr(), out.data_ptr(), len(data), C.byref(osz)) == 0
    one_frame = gpu_lib.bz3_hip_debug_cm_launches(1)
    assert 0 < batched <= one_frame and batched < 300 / 8, (batched, one_frame)
    backs = bzip3_amd.decompress_tensors(frames)
    assert b"".join(_host(b) for b in backs) == data


def test_a_corrupt_frame_fails_alone(gpu_lib, text):
    bs = 1 << 20
    datas = _pieces(text, [int(v) for v in np.random.default_rng(5).integers(100_000, 3 << 20, size=20)], 6)
    frames = [_ref_frame(bs, d) for d in datas]
    bad = bytearray(frames[10])
    bad[13 + 8 + 300] ^= 0x08  # inside chunk 0's coded bytes
    frames[10] = bytes(bad)
    ref = require_ref()
    rb = (C.c_uint8 * (len(datas[10]) + 16))()
    rsz = C.c_size_t(len(rb))
    rc_ref = ref.lib.bz3_decompress(frames[10], rb, len(frames[10]), C.byref(rsz))
    assert rc_ref != 0
    outs = [_dev(b"", len(d) + 16) for d in datas]
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.decompress_tensors([_dev(f) for f in frames], outs=outs)
    err = e.value
    assert err.index == 10 and err.code == rc_ref
    assert err.codes == [0] * 10 + [rc_ref] + [0] * 9
    assert _host(err.outs[10]) == bytes(rb[: rsz.value])
    for i, d in enumerate(datas):
        if i != 10:
            assert _host(err.outs[i]) == d, i


def test_a_host_pointer_fails_the_whole_call(gpu_lib, text):
    import torch

    datas = _pieces(text, [200_000, 300_000, 150_000], 8)
    xs = [_dev(d) for d in datas]
    cpu = torch.frombuffer(bytearray(datas[1]), dtype=torch.uint8)
    outs = [torch.full((gpu_lib.bz3_bound(len(d)),), 7, dtype=torch.uint8, device="cuda:0") for d in datas]
    torch.cuda.synchronize()
    n = 3
    ins = (C.c_void_p * n)(xs[0].data_ptr(), cpu.data_ptr(), xs[2].data_ptr())
    in_sizes = (C.c_size_t * n)(*map(len, datas))
    out_sizes = (C.c_size_t * n)(*[o.numel() for o in outs])
    rcs = (C.c_int * n)()
    optr = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    INIT = bzip3_amd.BZ3_ERR_INIT
    assert gpu_lib.bz3_hip_compress_device_many(1 << 20, n, ins, in_sizes, optr, out_sizes, rcs) == INIT
    assert list(rcs) == [INIT] * n and list(out_sizes) == [0] * n
    assert all(bool((o == 7).all()) for o in outs), "a rejected call wrote output"
    frames = bzip3_amd.compress_tensors(xs, 1 << 20)
    host_out = (C.c_uint8 * 400_000)()
    optr = (C.c_void_p * n)(outs[0].data_ptr(), C.addressof(host_out), outs[2].data_ptr())
    fptr = (C.c_void_p * n)(*[f.data_ptr() for f in frames])
    flen = (C.c_size_t * n)(*[f.numel() for f in frames])
    out_sizes = (C.c_size_t * n)(*[400_000] * n)
    assert gpu_lib.bz3_hip_decompress_device_many(n, fptr, flen, optr, out_sizes, rcs) == INIT
    assert list(rcs) == [INIT] * n and list(out_sizes) == [0] * n
    assert all(bool((o == 7).all()) for o in outs), "a rejected call wrote output"
    with pytest.raises(TypeError):
        bzip3_amd.compress_tensors([xs[0], cpu])


def test_headroom_rule_holds_after_a_batch(gpu_lib, text):
    import torch

    datas = _pieces(text, [4 << 20] * 5 + [300_000] * 40, 9)
    frames = bzip3_amd.compress_tensors([_dev(d) for d in datas], 4 << 20)
    bzip3_amd.decompress_tensors(frames)
    torch.cuda.synchronize()
    free_b, _ = torch.cuda.mem_get_info(0)
    assert free_b >= gpu_lib.bz3_hip_workspace_headroom() or gpu_lib.bz3_hip_debug_cached_bytes(0) == 0
