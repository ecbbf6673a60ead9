"""-m gpu: the resize on a real device (include/bz3_hip.h bz3_hip_resize_device[_many], the replane segment of bzip3_amd/csrc/planes.hpp;
bzip3_amd's resize_tensors, append_tensor_rows, truncate_tensor_rows, resize_tensor_rows and append_state_dict_rows).  The cases and the oracle are
those of test_frame_resize_emu -- the reference's frame of the new bytes, numpy for S, D and pos, never the library under test --, on device
memory; the oracle of the typed calls is torch.cat and torch's own slicing, packed afresh."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
from test_frame_delta_emu import _r16
from test_frame_planes_emu import BS
from test_frame_resize_emu import (appends_share_launches, block_size_changes, copied_chunks_are_not_decoded, delta_frames_match_reference, frames_match_reference,
                                   many_equal_single_calls, mixed_spec_replane, replane_case, resize_cap, resize_errors, sweep_specs_replane)
from test_frame_update_emu import FILL, INIT, pattern
from test_gpu_frame_delta import _gpu_alloc
from test_gpu_frame_planes import _host
from test_gpu_frame_update import _bits, _dev, _tensor

pytestmark = pytest.mark.gpu
MiB = 1 << 20


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_replane_kernel_sweep_on_the_gpu(gpu_lib, k):
    """The emulator suite's sweep on device memory: every kept size at every count and tail length 0..k-1, new lengths below, equal to and above
    the old one, the three alignments."""
    rng = np.random.default_rng(93 + 10 * k)
    for spec in sweep_specs_replane(rng, k):
        replane_case(gpu_lib.bz3_hip_debug_replane, rng, spec, _gpu_alloc)


def test_replane_kernel_large_and_mixed_on_the_gpu(gpu_lib):
    """Four segments of 1 - 9 MiB per k that keep a random number of bytes in a chunk that grows or shrinks, and the mixed launch."""
    rng = np.random.default_rng(94)
    for k in (1, 2, 4, 8):
        big = []
        for i in range(4):
            len_old = int(rng.integers(MiB, 9 * MiB))
            a = int(rng.integers(1, len_old + 1))
            len_new = int(rng.integers(a, len_old + 1)) if i % 2 else len_old + int(rng.integers(1, MiB))
            big.append((_r16(rng), _r16(rng), len_old, len_new, k, a))
        replane_case(gpu_lib.bz3_hip_debug_replane, rng, big, _gpu_alloc)
    replane_case(gpu_lib.bz3_hip_debug_replane, rng, mixed_spec_replane(rng), _gpu_alloc)


# ---- frames -------------------------------------------------------------------------------------------------------------------
def gpu_resize_call(lib, bs, k, frame, keep, data, base=None, cap=None):
    """test_frame_resize_emu.resize_call on device memory: (rc, *out_size, out[0, cap) after the call)."""
    import torch

    cap = resize_cap(lib, bs, frame, keep, len(data)) if cap is None else cap
    f, d, out = _dev(frame), _dev(data), _dev(bytes([FILL]) * cap)
    b = None if base is None else _dev(base)
    osz = C.c_size_t(cap)
    torch.cuda.synchronize()
    rc = lib.bz3_hip_resize_device(bs, k, f.data_ptr(), len(frame), keep, d.data_ptr(), len(data), None if b is None else b.data_ptr(), out.data_ptr(), C.byref(osz))
    assert _host(f)[: len(frame)] == bytes(frame) and _host(d)[: len(data)] == bytes(data) and (b is None or _host(b)[: len(base)] == bytes(base)), "an input was written"
    return rc, osz.value, _host(out)[:cap]


def gpu_many_call(lib, bss, ks, frames, keeps, datas, bases, caps=None):
    import torch

    n = len(frames)
    caps = [resize_cap(lib, bs, f, keep, len(d)) for bs, f, keep, d in zip(bss, frames, keeps, datas)] if caps is None else caps
    ins, dbufs, outs = [_dev(f) for f in frames], [_dev(d) for d in datas], [_dev(bytes([FILL]) * c) for c in caps]
    bbufs = [None if b is None else _dev(b) for b in bases]
    ptrs = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    out_sizes, rcs = (C.c_size_t * n)(*caps), (C.c_int * n)(*([77] * n))
    torch.cuda.synchronize()
    rc = lib.bz3_hip_resize_device_many(n, (C.c_uint32 * n)(*bss), (C.c_uint32 * n)(*ks), ptrs(ins), (C.c_size_t * n)(*map(len, frames)), (C.c_uint64 * n)(*keeps), ptrs(dbufs),
                                        (C.c_size_t * n)(*map(len, datas)), ptrs(bbufs), ptrs(outs), out_sizes, rcs)
    return rc, [(rcs[i], out_sizes[i], _host(outs[i])[: caps[i]]) for i in range(n)]


@pytest.mark.parametrize("chunks", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_resizes_of_a_frame_match_the_reference(gpu_lib, k, chunks, monkeypatch):
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    frames_match_reference(gpu_lib, k, chunks, gpu_resize_call)


@pytest.mark.parametrize("k", [1, 2, 8])
def test_effective_block_size_changes(gpu_lib, k):
    block_size_changes(gpu_lib, k, gpu_resize_call)


@pytest.mark.parametrize("k", [1, 4])
def test_resizes_of_a_delta_frame(gpu_lib, k):
    delta_frames_match_reference(gpu_lib, k, gpu_resize_call)


def test_copied_chunks_are_not_decoded(gpu_lib):
    copied_chunks_are_not_decoded(gpu_lib, gpu_resize_call)


def test_resize_errors_leave_out_untouched(gpu_lib):
    import torch

    case, data = resize_errors(gpu_lib, gpu_resize_call)
    frame, T = case.frame, case.T
    cap = len(frame) + 3 * gpu_lib.bz3_bound(BS)
    arena = _dev(bytes([FILL]) * (cap + 2 * len(frame) + 2000))
    arena[: len(frame)] = _dev(frame)
    arena[cap - 1 : cap - 1 + len(data)] = _dev(data)
    d, f = _dev(data), _dev(frame)
    before = _host(arena)
    torch.cuda.synchronize()
    at = lambda off: arena.data_ptr() + off  # noqa: E731
    for args in ((at(0), d.data_ptr(), None, at(len(frame) - 1)),  # out overlaps in
                 (f.data_ptr(), at(cap - 1), None, at(0)),  # out overlaps data
                 (f.data_ptr(), d.data_ptr(), at(cap - 1), at(0))):  # out overlaps base
        osz = C.c_size_t(cap)
        assert gpu_lib.bz3_hip_resize_device(BS, 2, args[0], len(frame), T, args[1], len(data), args[2], args[3], C.byref(osz)) == INIT
        assert osz.value == 0 and _host(arena) == before
    osz = C.c_size_t(cap)  # adjacent: fine
    assert gpu_lib.bz3_hip_resize_device(BS, 2, f.data_ptr(), len(frame), T, at(cap), len(data), None, at(0), C.byref(osz)) == 0


def test_many_resizes_equal_their_single_calls(gpu_lib, monkeypatch):
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    many_equal_single_calls(gpu_lib, gpu_many_call, gpu_resize_call)


def test_many_appends_share_their_cm_launches(gpu_lib):
    appends_share_launches(gpu_lib, gpu_many_call)
    assert gpu_lib.bz3_hip_resize_device_many(0, None, None, None, None, None, None, None, None, None, None, None) == 0
    assert gpu_lib.bz3_hip_resize_device_many(2, None, None, None, None, None, None, None, None, None, None, None) == INIT


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
TYPED = [("float32", None, (300, 256)), ("float64", None, (150, 256)), ("bfloat16", None, (700, 200)), ("float16", 2, (700, 200)), ("uint8", None, (1000, 333)),
         ("int64", None, (150, 256)), ("complex64", None, (200, 128))]  # a few hundred KiB: several chunks of 65 KiB; planes 4, 8, 1, 2, 1, 8, 4


@pytest.mark.parametrize("dtype,planes,shape", TYPED, ids=[t for t, _, _ in TYPED])
def test_append_and_truncate_equal_a_fresh_pack(gpu_lib, dtype, planes, shape):
    """Rows appended and cut off in the packed form: the frame is the one pack_tensor gives for torch.cat / the slice, unpacking gives that tensor
    bit for bit, the checksum after an append is that of the grown tensor, and p is unchanged."""
    import torch

    x = _tensor(dtype, shape, 5)
    p = bzip3_amd.pack_tensor(x, 65 << 10, planes=planes, lib=gpu_lib)
    assert planes is None or p.planes == planes
    frame0 = p.frame.clone()
    for rows in (1, 3, shape[0] // 2, 2 * shape[0]):
        values = _tensor(dtype, (rows,) + shape[1:], 6 + rows)
        want = torch.cat([x, values])
        fresh = bzip3_amd.pack_tensor(want, 65 << 10, planes=p.planes, lib=gpu_lib)
        if fresh.block_size != p.block_size:
            continue  # (the fallback has a test of its own)
        q = bzip3_amd.append_tensor_rows(p, values, lib=gpu_lib)
        assert torch.equal(q.frame, fresh.frame), rows
        assert (q.dtype, tuple(q.shape), q.planes, q.block_size, q.nbytes, q.delta, q.base_crc) == (p.dtype, tuple(want.shape), p.planes, p.block_size, fresh.nbytes, False, None)
        assert q.crc == fresh.crc == bzip3_amd.crc32c_tensors([bzip3_amd._as_bytes(want, "want")], lib=gpu_lib)[0], rows
        got = bzip3_amd.unpack_tensor(q, verify=True, lib=gpu_lib)
        assert got.dtype == x.dtype and got.shape == want.shape and torch.equal(_bits(got), _bits(want)), rows
    for rows in (shape[0] - 1, shape[0] // 2, 1, 0):
        want = x[:rows]
        fresh = bzip3_amd.pack_tensor(want, 65 << 10, planes=p.planes, lib=gpu_lib)
        if fresh.block_size != p.block_size:
            continue
        q = bzip3_amd.truncate_tensor_rows(p, rows, lib=gpu_lib)
        assert torch.equal(q.frame, fresh.frame), rows
        assert q.crc is None and q.base_crc is None and tuple(q.shape) == tuple(want.shape) and q.nbytes == fresh.nbytes
        assert torch.equal(_bits(bzip3_amd.unpack_tensor(q, lib=gpu_lib)), _bits(want)), rows
    values = _tensor(dtype, (7,) + shape[1:], 77)
    want = torch.cat([x[:100], values])
    q = bzip3_amd.resize_tensor_rows(p, 100, values, lib=gpu_lib)
    assert torch.equal(q.frame, bzip3_amd.pack_tensor(want, 65 << 10, planes=p.planes, lib=gpu_lib).frame) and q.crc is None
    assert torch.equal(bzip3_amd.resize_tensor_rows(p, shape[0], lib=gpu_lib).frame, p.frame)
    assert torch.equal(p.frame, frame0) and tuple(p.shape) == shape, "p was changed"


def test_append_to_a_delta_tensor(gpu_lib):
    import torch

    base = _tensor("float32", (300, 256), 11)
    x = base + _tensor("float32", (300, 256), 12) * 0.01
    p = bzip3_amd.pack_tensor(x, 65 << 10, base=base, lib=gpu_lib)
    assert p.delta
    more_base = _tensor("float32", (70, 256), 14)
    values = more_base + _tensor("float32", (70, 256), 13) * 0.01
    want, grown = torch.cat([x, values]), torch.cat([base, more_base])
    fresh = bzip3_amd.pack_tensor(want, 65 << 10, planes=p.planes, base=grown, lib=gpu_lib)
    assert fresh.block_size == p.block_size
    q = bzip3_amd.append_tensor_rows(p, values, base=more_base, lib=gpu_lib)
    assert torch.equal(q.frame, fresh.frame) and q.delta and (q.base_crc, q.crc) == (fresh.base_crc, fresh.crc)
    assert torch.equal(_bits(bzip3_amd.unpack_tensor(q, base=grown, verify=True, lib=gpu_lib)), _bits(want))
    t = bzip3_amd.truncate_tensor_rows(p, 120, lib=gpu_lib)
    assert t.delta and t.base_crc is None and t.crc is None
    assert torch.equal(t.frame, bzip3_amd.pack_tensor(x[:120], 65 << 10, planes=p.planes, base=base[:120], lib=gpu_lib).frame)
    with pytest.raises(ValueError):
        bzip3_amd.append_tensor_rows(p, values, lib=gpu_lib)  # the base's rows are required
    with pytest.raises(ValueError):
        bzip3_amd.append_tensor_rows(p, values, base=more_base[:69], lib=gpu_lib)


def test_a_size_that_would_lose_a_block_is_repacked(gpu_lib):
    """260 rows of 256 float32 are exactly four blocks of 65 KiB: the append falls back to a fresh pack at another block size."""
    import torch

    x = _tensor("float32", (200, 256), 31)
    p = bzip3_amd.pack_tensor(x, 65 << 10, lib=gpu_lib)
    assert p.block_size == 65 << 10
    values = _tensor("float32", (60, 256), 32)
    want = torch.cat([x, values])
    q = bzip3_amd.append_tensor_rows(p, values, lib=gpu_lib)
    fresh = bzip3_amd.pack_tensor(want, 65 << 10, lib=gpu_lib)
    assert q.block_size == fresh.block_size != p.block_size and torch.equal(q.frame, fresh.frame) and q.crc == fresh.crc
    assert torch.equal(_bits(bzip3_amd.unpack_tensor(q, verify=True, lib=gpu_lib)), _bits(want))
    t = bzip3_amd.truncate_tensor_rows(p, 130, lib=gpu_lib)  # two blocks exactly
    assert t.block_size != p.block_size and torch.equal(_bits(bzip3_amd.unpack_tensor(t, lib=gpu_lib)), _bits(x[:130]))
    base = _tensor("float32", (200, 256), 33)
    pd = bzip3_amd.pack_tensor(x, 65 << 10, base=base, planes=4, lib=gpu_lib)
    more_base = _tensor("float32", (60, 256), 34)
    qd = bzip3_amd.append_tensor_rows(pd, values, base=more_base, lib=gpu_lib)
    assert qd.delta and qd.block_size != pd.block_size
    assert torch.equal(_bits(bzip3_amd.unpack_tensor(qd, base=torch.cat([base, more_base]), verify=True, lib=gpu_lib)), _bits(want))


def test_resize_tensors_on_raw_frames(gpu_lib):
    import torch

    raw = _dev(pattern(3 * BS + 999, 31))
    frame = bzip3_amd.compress_tensor(raw, 65 << 10, lib=gpu_lib, planes=2)
    data = _dev(pattern(BS + 50, 32))
    got = bzip3_amd.resize_tensors([frame, frame], [raw.numel(), BS + 10], [data, data[:0]], planes=2, block_sizes=[65 << 10] * 2, lib=gpu_lib)
    assert torch.equal(got[0], bzip3_amd.compress_tensor(torch.cat([raw, data]), 65 << 10, lib=gpu_lib, planes=2))
    assert torch.equal(got[1], bzip3_amd.compress_tensor(raw[: BS + 10].clone(), 65 << 10, lib=gpu_lib, planes=2))
    assert bzip3_amd.resize_tensors([], [], [], block_sizes=[], lib=gpu_lib) == []
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.resize_tensors([frame, frame], [0, raw.numel() + 1], [data, data], planes=2, block_sizes=[65 << 10] * 2, lib=gpu_lib)
    assert e.value.code == bzip3_amd.BZ3_ERR_DATA_TOO_BIG and e.value.index == 1 and e.value.codes == [0, bzip3_amd.BZ3_ERR_DATA_TOO_BIG]
    assert torch.equal(e.value.outs[0], bzip3_amd.compress_tensor(data, 65 << 10, lib=gpu_lib, planes=2)) and e.value.outs[1].numel() == 0


def test_append_state_dict_rows_is_one_call_per_block_size(gpu_lib, monkeypatch):
    import torch

    # "c" holds exactly 5 blocks of 65 KiB, and 6 once it has grown, so its block size has to move both times: two distinct block sizes in the dict
    sd = {"a": _tensor("float32", (300, 256), 21), "b": _tensor("bfloat16", (700, 200), 22), "c": _tensor("uint8", (320, 1040), 23), "step": _tensor("float32", (), 24)}
    assert sd["c"].numel() == 5 * 65 * 1024
    base = {"a": _tensor("float32", (300, 256), 25)}
    packed = bzip3_amd.pack_state_dict(sd, 65 << 10, base=base, lib=gpu_lib)
    assert packed["a"].delta and len({packed[k].block_size for k in "abc"}) == 2
    calls = []
    entry = "bz3_hip_resize_device_many"
    monkeypatch.setattr(gpu_lib, entry, (lambda real: lambda *a: calls.append(a[0]) or real(*a))(getattr(gpu_lib, entry)))
    rows = {"a": _tensor("float32", (5, 256), 26), "b": _tensor("bfloat16", (10, 200), 27), "c": _tensor("uint8", (64, 1040), 28)}
    more_base = {"a": _tensor("float32", (5, 256), 29)}
    got = bzip3_amd.append_state_dict_rows(packed, rows, base=more_base, lib=gpu_lib)
    assert sorted(calls) == [1, 2]
    assert list(got) == list(packed) and got["step"] is packed["step"] and got["a"] is not packed["a"]
    grown = {k: torch.cat([sd[k], rows[k]]) if k in rows else sd[k] for k in sd}
    fresh = bzip3_amd.pack_state_dict(grown, 65 << 10, base={"a": torch.cat([base["a"], more_base["a"]])}, lib=gpu_lib)
    for k in sd:
        assert torch.equal(got[k].frame, fresh[k].frame) and (got[k].block_size, got[k].crc, got[k].base_crc, tuple(got[k].shape)) == (
            fresh[k].block_size, fresh[k].crc, fresh[k].base_crc, tuple(fresh[k].shape)), k
    assert bzip3_amd.append_state_dict_rows(packed, {}, lib=gpu_lib) == packed
    with pytest.raises(ValueError):
        bzip3_amd.append_state_dict_rows(packed, {"nope": rows["b"]}, lib=gpu_lib)


def test_argument_errors_raise_before_any_gpu_call(gpu_lib, monkeypatch):
    import torch

    x = _tensor("float32", (300, 256), 41)
    p = bzip3_amd.pack_tensor(x, 65 << 10, lib=gpu_lib)
    monkeypatch.setattr(gpu_lib, "bz3_hip_resize_device_many", lambda *a: pytest.fail("the library was called"))
    v = _tensor("float32", (4, 256), 42)
    for values, err in ((v.to(torch.float16), TypeError), (v[:, :255], TypeError), (v.reshape(-1), TypeError), (v.cpu(), TypeError), ([1.0, 2.0], TypeError)):
        with pytest.raises(err):
            bzip3_amd.append_tensor_rows(p, values, lib=gpu_lib)
    for rows in (-1, 301):
        with pytest.raises(ValueError):
            bzip3_amd.truncate_tensor_rows(p, rows, lib=gpu_lib)
    with pytest.raises(TypeError):
        bzip3_amd.append_tensor_rows(p.frame, v, lib=gpu_lib)
    with pytest.raises(ValueError):
        bzip3_amd.append_tensor_rows(bzip3_amd.pack_tensor(_tensor("float32", (), 43), lib=gpu_lib), v, lib=gpu_lib)
    with pytest.raises(ValueError):
        bzip3_amd.resize_tensors([p.frame], [0, 1], [p.frame], block_sizes=[p.block_size], lib=gpu_lib)
    with pytest.raises(ValueError):
        bzip3_amd.resize_tensors([p.frame], [-1], [p.frame], block_sizes=[p.block_size], lib=gpu_lib)
    with pytest.raises(ValueError):
        bzip3_amd.resize_tensors([p.frame], [0], [p.frame], lib=gpu_lib)
    with pytest.raises(TypeError):
        bzip3_amd.resize_tensors([p.frame], [0], [x], block_sizes=[p.block_size], lib=gpu_lib)
