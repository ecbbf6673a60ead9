"""-m gpu: the frame API on device memory (include/bz3_hip.h bz3_hip_compress_device / bz3_hip_decompress_device /
bz3_hip_frame_decoded_size_device; bzip3_amd.compress_tensor / decompress_tensor) with torch tensors as device buffers,
compared with the product's host frame API and the real reference."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
import datagen
import frame_cases
from oracle_lib import require_ref

pytestmark = pytest.mark.gpu


def _dev(data, room=None):
    import torch

    t = torch.zeros(max(1, room if room is not None else len(data)), dtype=torch.uint8, device="cuda:0")
    if len(data):
        t[: len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _host(t, n):
    return bytes(t[:n].cpu().numpy()) if n else b""


class TorchFrames:
    """libbz3.h's frame API as frame_cases.check calls it, backed by the device entry points on torch tensors."""

    def __init__(self, lib):
        self.lib = lib
        self.bz3_bound = lib.bz3_bound

    def bz3_compress(self, bs, data, out, n, osz):
        src, dst = _dev(bytes(data[:n])), _dev(b"", osz._obj.value)
        rc = self.lib.bz3_hip_compress_device(bs, src.data_ptr(), dst.data_ptr(), n, osz)
        C.memmove(out, _host(dst, osz._obj.value), osz._obj.value)
        return rc

    def bz3_decompress(self, frame, out, n, osz):
        src, dst = _dev(bytes(frame[:n])), _dev(b"", osz._obj.value)
        rc = self.lib.bz3_hip_decompress_device(src.data_ptr(), dst.data_ptr(), n, osz)
        C.memmove(out, _host(dst, osz._obj.value), osz._obj.value)
        return rc


def _ref_frame(bs, data):
    ref = require_ref()
    out = (C.c_uint8 * (ref.lib.bz3_bound(len(data)) + 64))()
    osz = C.c_size_t(len(out))
    assert ref.lib.bz3_compress(bs, data, out, len(data), C.byref(osz)) == 0
    return bytes(out[: osz.value])


def _host_frame(lib, bs, data):
    out = (C.c_uint8 * (lib.bz3_bound(len(data)) + 64))()
    osz = C.c_size_t(len(out))
    assert lib.bz3_compress(bs, data, out, len(data), C.byref(osz)) == 0
    return bytes(out[: osz.value])


def test_device_frames_match_the_reference(gpu_lib, text):
    """Good frames, the 15 malformed frames and the short output of frame_cases at 65 KiB and 1 MiB, plus 65 KiB + 7 (unaligned scatter)."""
    frame_cases.check(TorchFrames(gpu_lib), text[: 4 * 65 * 1024 + 1234], 65 * 1024)
    frame_cases.check(TorchFrames(gpu_lib), (text * 3)[: 4 * (1 << 20) + 777], 1 << 20)
    bs = 65 * 1024 + 7
    frame_cases.check(TorchFrames(gpu_lib), text[: 4 * bs + 999], bs)


@pytest.mark.parametrize("kind", ["text_odd_tail", "text_exact_multiple", "random_odd_block"])
def test_compress_tensor_round_trip(gpu_lib, text, kind):
    import torch

    if kind == "text_odd_tail":
        bs, data = 2 << 20, (text * 30)[: 64 * (2 << 20) + 12345]
    elif kind == "text_exact_multiple":
        bs, data = 2 << 20, (text * 10)[: 16 * (2 << 20)]
    else:
        bs, data = (1 << 20) + 13, datagen.random_bytes(6 * ((1 << 20) + 13) + 1001, seed=7)
    x = _dev(data)
    keep = x.clone()
    frame = bzip3_amd.compress_tensor(x, bs)
    assert frame.device == x.device and frame.dtype == torch.uint8
    got = _host(frame, frame.numel())
    assert got == _host_frame(gpu_lib, bs, data), "device frame differs from the product's host bz3_compress"
    assert got == _ref_frame(bs, data), "device frame differs from the reference"
    assert torch.equal(x, keep), "compress_tensor wrote to its input"
    if kind == "random_odd_block":
        # a full incompressible block codes to more than block_size bytes, which the reference's own decoder rejects as a malformed
        # chunk header (src/libbz3.c:969): the device decoder must fail the same way, with the same bytes committed
        ref = require_ref()
        rb = (C.c_uint8 * (len(data) + 16))()
        rsz = C.c_size_t(len(rb))
        rc_ref = ref.lib.bz3_decompress(got, rb, len(got), C.byref(rsz))
        assert rc_ref == bzip3_amd.BZ3_ERR_MALFORMED_HEADER
        with pytest.raises(bzip3_amd.Bz3Error) as e:
            bzip3_amd.decompress_tensor(frame, out=_dev(b"", len(data) + 16))
        assert e.value.code == rc_ref and _host(e.value.out, e.value.out.numel()) == bytes(rb[: rsz.value])
        return
    # an exact multiple of the block size: the reference's last chunk is empty (src/libbz3.c:914, sic), its block is not in the frame
    n = len(data) if len(data) % bs else len(data) - bs
    back = bzip3_amd.decompress_tensor(frame)
    assert back.numel() == n and torch.equal(back, keep[:n])
    out = torch.full((len(data) + 100,), 7, dtype=torch.uint8, device="cuda:0")
    back2 = bzip3_amd.decompress_tensor(frame, out=out)
    assert back2.data_ptr() == out.data_ptr() and torch.equal(back2, keep[:n]) and bool((out[n:] == 7).all())
    size = C.c_size_t(0)
    assert gpu_lib.bz3_hip_frame_decoded_size_device(frame.data_ptr(), frame.numel(), C.byref(size)) == 0 and size.value == n


def test_short_output_capacity(gpu_lib, text):
    data = (text * 3)[: 5 * (1 << 20) + 5]
    x = _dev(data)
    out = _dev(b"", gpu_lib.bz3_bound(len(data)) - 1)
    osz = C.c_size_t(out.numel())
    assert gpu_lib.bz3_hip_compress_device(1 << 20, x.data_ptr(), out.data_ptr(), len(data), C.byref(osz)) == bzip3_amd.BZ3_ERR_DATA_TOO_BIG
    assert osz.value == 0
    frame = bzip3_amd.compress_tensor(x, 1 << 20)
    # decode into 3.5 blocks of room: the host path and the reference commit three blocks and report DATA_TOO_BIG
    room = 3 * (1 << 20) + (1 << 19)
    host_back = (C.c_uint8 * room)()
    hsz = C.c_size_t(room)
    fb = _host(frame, frame.numel())
    rc_host = gpu_lib.bz3_decompress(fb, host_back, len(fb), C.byref(hsz))
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.decompress_tensor(frame, out=_dev(b"", room))
    assert e.value.code == rc_host == bzip3_amd.BZ3_ERR_DATA_TOO_BIG
    assert _host(e.value.out, e.value.out.numel()) == bytes(host_back[: hsz.value]) == data[: 3 << 20]


def test_corrupted_chunk_in_a_multi_window_frame(gpu_lib, text, monkeypatch):
    """A CRC failure in chunk 7 of 12 with windows of 3 blocks: the chunks of the first two windows are committed, then the
    chunk before the bad one in its own window; same code and bytes as the reference."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    bs = 1 << 20
    data = (text * 5)[: 11 * bs + 4321]
    frame = bytearray(_ref_frame(bs, data))
    off = 13
    for _ in range(7):
        off += 8 + int.from_bytes(frame[off : off + 4], "little")
    frame[off + 8 + 500] ^= 0x10  # inside chunk 7's coded bytes
    ref = require_ref()
    rb = (C.c_uint8 * (len(data) + 16))()
    rsz = C.c_size_t(len(rb))
    rc_ref = ref.lib.bz3_decompress(bytes(frame), rb, len(frame), C.byref(rsz))
    assert rc_ref != 0
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.decompress_tensor(_dev(bytes(frame)), out=_dev(b"", len(data) + 16))
    assert e.value.code == rc_ref
    assert _host(e.value.out, e.value.out.numel()) == bytes(rb[: rsz.value]) == data[: 7 * bs]
    # a bad chunk HEADER in window 3: the chunks before it decode and are committed, then MALFORMED_HEADER
    frame2 = bytearray(_ref_frame(bs, data))
    off = 13
    for _ in range(8):
        off += 8 + int.from_bytes(frame2[off : off + 4], "little")
    frame2[off + 4 : off + 8] = (0xFFFFFFFF).to_bytes(4, "little")
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.decompress_tensor(_dev(bytes(frame2)))
    assert e.value.code == bzip3_amd.BZ3_ERR_MALFORMED_HEADER and _host(e.value.out, e.value.out.numel()) == data[: 8 * bs]


def test_pointers_must_be_device_memory_of_one_gpu(gpu_lib, text):
    import torch

    data = text[: 300000]
    x = _dev(data)
    out = _dev(b"", gpu_lib.bz3_bound(len(data)))
    host = (C.c_uint8 * out.numel())()
    osz = C.c_size_t(out.numel())
    assert gpu_lib.bz3_hip_compress_device(1 << 20, x.data_ptr(), host, len(data), C.byref(osz)) == bzip3_amd.BZ3_ERR_INIT
    osz = C.c_size_t(out.numel())
    assert gpu_lib.bz3_hip_compress_device(1 << 20, data, out.data_ptr(), len(data), C.byref(osz)) == bzip3_amd.BZ3_ERR_INIT
    frame = bzip3_amd.compress_tensor(x, 1 << 20)
    fb = _host(frame, frame.numel())
    osz = C.c_size_t(len(data))
    assert gpu_lib.bz3_hip_decompress_device(fb, out.data_ptr(), len(fb), C.byref(osz)) == bzip3_amd.BZ3_ERR_INIT
    size = C.c_size_t(0)
    assert gpu_lib.bz3_hip_frame_decoded_size_device(fb, len(fb), C.byref(size)) == bzip3_amd.BZ3_ERR_INIT
    with pytest.raises(TypeError):
        bzip3_amd.compress_tensor(x.cpu())
    if torch.cuda.device_count() > 1:
        y = x.to("cuda:1")
        torch.cuda.synchronize("cuda:1")
        osz = C.c_size_t(out.numel())
        assert gpu_lib.bz3_hip_compress_device(1 << 20, y.data_ptr(), out.data_ptr(), len(data), C.byref(osz)) == bzip3_amd.BZ3_ERR_INIT
        # the states follow the buffers, not bz3_hip_bind_device
        gpu_lib.bz3_hip_bind_device(0)
        try:
            f1 = bzip3_amd.compress_tensor(y, 1 << 20)
        finally:
            gpu_lib.bz3_hip_bind_device(-1)
        assert f1.device == y.device and _host(f1, f1.numel()) == fb


def test_headroom_rule_holds_after_a_call(gpu_lib, text):
    import torch

    x = _dev((text * 4)[: 20 << 20])
    frame = bzip3_amd.compress_tensor(x, 4 << 20)
    bzip3_amd.decompress_tensor(frame)
    torch.cuda.synchronize()
    free_b, _ = torch.cuda.mem_get_info(0)
    assert free_b >= gpu_lib.bz3_hip_workspace_headroom() or gpu_lib.bz3_hip_debug_cached_bytes(0) == 0


def test_copy_segments_on_the_gpu(gpu_lib):
    """The emulator suite's alignment / length sweep of k_copy_segments, on torch tensors."""
    import torch

    rng = np.random.default_rng(12)

    def case(spec):
        room = sum(n for _, _, n in spec) + 80 * len(spec) + 64
        src = torch.from_numpy(rng.integers(0, 256, size=room, dtype=np.uint8)).to("cuda:0")
        dst = torch.full((room,), 0xA5, dtype=torch.uint8, device="cuda:0")
        src_np, want = src.cpu().numpy(), dst.cpu().numpy().copy()
        sa, da = src.data_ptr(), dst.data_ptr()
        table, s_off, d_off = [], 0, 0
        for a_s, a_d, n in spec:
            s_off += (a_s - (sa + s_off)) % 16
            d_off += (a_d - (da + d_off)) % 16
            table += [s_off, d_off, n]
            want[d_off : d_off + n] = src_np[s_off : s_off + n]
            s_off += n + int(rng.integers(0, 40))
            d_off += n + int(rng.integers(1, 40))
        assert max(s_off, d_off) <= room
        torch.cuda.synchronize()
        t = (C.c_uint64 * len(table))(*table)
        assert gpu_lib.bz3_hip_debug_copy_segments(sa, da, t, len(table) // 3) == 0
        assert np.array_equal(dst.cpu().numpy(), want)

    for n in (0, 1, 15, 16, 17, 31, 4095, 4097):
        case([(a, b, n) for a in range(16) for b in range(16)])
    case([(int(rng.integers(0, 16)), int(rng.integers(0, 16)), int(rng.integers(0, 200_000))) for _ in range(64)])
    case([(int(rng.integers(0, 16)), int(rng.integers(0, 16)), int(rng.integers(1 << 20, 9 << 20))) for _ in range(6)])
