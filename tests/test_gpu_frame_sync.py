"""-m gpu: the sync on a real device (include/bz3_hip.h bz3_hip_sync_device[_many], k_diff_segments of bzip3_amd/csrc/planes.hpp through
bz3_hip_debug_diff; bzip3_amd's sync_tensors, sync_tensor_bytes, sync_tensor and sync_state_dict).  The cases and the oracle are those of
test_frame_sync_emu -- the reference's frame of the new bytes, numpy for S, D and the comparison, never the library under test --, on device
memory; the typed calls are held against pack_tensor of the new tensor, the path they replace."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
from test_frame_planes_emu import BS
from test_frame_sync_emu import (ALIGNS, LENGTHS, diff_case, dirty_chunks_share_launches, frames_match_reference, many_equal_single_calls, mixed_groups, nothing_is_decoded,
                                 sweep_groups, sync_cap, sync_errors)
from test_frame_update_emu import FILL, INIT
from test_gpu_frame_planes import _host, _make
from test_gpu_frame_update import _bits, _dev

pytestmark = pytest.mark.gpu
MiB = 1 << 20


def _gpu_aligned(a):
    """(address, reader) of a device copy of the array; torch's allocations are 16-byte aligned."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a) if len(a) else np.zeros(1, dtype=np.uint8)).to("cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t.data_ptr(), lambda: t.cpu().numpy()[: len(a)]


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("al_b", ALIGNS)
@pytest.mark.parametrize("al_a", ALIGNS)
@pytest.mark.parametrize("n", LENGTHS)
def test_diff_kernel_every_seam_at_every_alignment_pair(gpu_lib, n, al_a, al_b):
    """The emulator suite's sweep on device memory: equal runs, and one flipped byte at the run's two ends, on either side of every 16-byte seam
    of either side's granules, and in the guard bytes just outside the run."""
    rng = np.random.default_rng(950 + 256 * n + 16 * al_a + al_b)
    for groups in sweep_groups(n, al_a, al_b):
        diff_case(gpu_lib.bz3_hip_debug_diff, rng, groups, _gpu_aligned)


def test_diff_kernel_mixed_and_large_on_the_gpu(gpu_lib):
    """The mixed launch in which every third run differs, every run in an allocation of its own; four pairs of 1 - 9 MiB that differ in one byte at
    a random place beside the same pairs equal."""
    rng = np.random.default_rng(96)
    diff_case(gpu_lib.bz3_hip_debug_diff, rng, mixed_groups(rng), _gpu_aligned, exact=True)
    diff_case(gpu_lib.bz3_hip_debug_diff, rng, mixed_groups(rng), _gpu_aligned)
    big = []
    for i in range(4):
        n = int(rng.integers(MiB, 9 * MiB))
        big.append((ALIGNS[i % 3], ALIGNS[(i + i // 3) % 3], n, [None, int(rng.integers(0, n))]))
    diff_case(gpu_lib.bz3_hip_debug_diff, rng, big, _gpu_aligned)
    diff_case(gpu_lib.bz3_hip_debug_diff, rng, [], _gpu_aligned)


# ---- frames -------------------------------------------------------------------------------------------------------------------
def gpu_sync_call(lib, k, frame, data, old, base=None, cap=None):
    """test_frame_sync_emu.sync_call on device memory: (rc, *out_size, out[0, cap) after the call, *recoded)."""
    import torch

    cap = sync_cap(lib, frame) if cap is None else cap
    f, d, out = _dev(frame), _dev(data), _dev(bytes([FILL]) * cap)
    o = d if old is data else None if old is None else _dev(old)
    b = None if base is None else _dev(base)
    osz, rec = C.c_size_t(cap), C.c_uint32(77)
    torch.cuda.synchronize()
    rc = lib.bz3_hip_sync_device(k, f.data_ptr(), len(frame), d.data_ptr(), None if o is None else o.data_ptr(), len(data), None if b is None else b.data_ptr(), out.data_ptr(),
                                 C.byref(osz), C.byref(rec))
    assert _host(f)[: len(frame)] == bytes(frame) and _host(d)[: len(data)] == bytes(data) and (o is None or _host(o)[: len(old)] == bytes(old)), "an input was written"
    assert b is None or _host(b)[: len(base)] == bytes(base), "the base was written"
    return rc, osz.value, _host(out)[:cap], rec.value


def gpu_many_call(lib, ks, frames, datas, olds, bases, caps=None):
    import torch

    n = len(frames)
    caps = [sync_cap(lib, f) for f in frames] if caps is None else caps
    ins, dbufs, obufs, outs = [_dev(f) for f in frames], [_dev(d) for d in datas], [_dev(o) for o in olds], [_dev(bytes([FILL]) * c) for c in caps]
    bbufs = [None if b is None else _dev(b) for b in bases]
    ptrs = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    out_sizes, rcs, rec = (C.c_size_t * n)(*caps), (C.c_int * n)(*([77] * n)), (C.c_uint32 * n)(*([77] * n))
    torch.cuda.synchronize()
    rc = lib.bz3_hip_sync_device_many(n, (C.c_uint32 * n)(*ks), ptrs(ins), (C.c_size_t * n)(*map(len, frames)), ptrs(dbufs), ptrs(obufs), (C.c_size_t * n)(*map(len, datas)),
                                      ptrs(bbufs), ptrs(outs), out_sizes, rec, rcs)
    return rc, [(rcs[i], out_sizes[i], _host(outs[i])[: caps[i]], rec[i]) for i in range(n)]


@pytest.mark.parametrize("with_base", [False, True], ids=["plain", "base"])
@pytest.mark.parametrize("chunks", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_syncs_of_a_frame_match_the_reference(gpu_lib, k, chunks, with_base):
    frames_match_reference(gpu_lib, k, chunks, with_base, gpu_sync_call)


def test_no_chunk_is_decoded(gpu_lib):
    nothing_is_decoded(gpu_lib, gpu_sync_call)


def test_sync_errors_leave_out_untouched(gpu_lib):
    import torch

    case, new, need = sync_errors(gpu_lib, gpu_sync_call)
    frame, T = case.frame, case.T
    cap = sync_cap(gpu_lib, frame)
    given = [frame, new, case.x, bytes(T)]
    for which in range(4):  # out overlapping each of in, data, old and base: the last byte of out[0, cap) is the input's first
        arena = _dev(bytes([FILL]) * (cap + len(frame) + T + 64))
        arena[cap - 1 : cap - 1 + len(given[which])] = _dev(given[which])
        bufs = [_dev(g) for g in given]
        args = [t.data_ptr() for t in bufs]
        args[which] = arena.data_ptr() + cap - 1
        before = _host(arena)
        osz, rec = C.c_size_t(cap), C.c_uint32(77)
        torch.cuda.synchronize()
        assert gpu_lib.bz3_hip_sync_device(2, args[0], len(frame), args[1], args[2], T, args[3], arena.data_ptr(), C.byref(osz), C.byref(rec)) == INIT, which
        assert (osz.value, rec.value) == (0, 0) and _host(arena) == before, which
    arena = _dev(bytes([FILL]) * (cap + T))
    arena[cap:] = _dev(new)
    osz = C.c_size_t(cap)  # adjacent: fine; data and old may be one buffer; recoded may be NULL
    f = _dev(frame)
    torch.cuda.synchronize()
    assert gpu_lib.bz3_hip_sync_device(2, f.data_ptr(), len(frame), arena.data_ptr() + cap, arena.data_ptr() + cap, T, None, arena.data_ptr(), C.byref(osz), None) == 0
    assert _host(arena)[: osz.value] == frame


def test_many_syncs_equal_their_single_calls(gpu_lib, monkeypatch):
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    many_equal_single_calls(gpu_lib, gpu_many_call, gpu_sync_call)


def test_many_dirty_chunks_share_their_cm_launch(gpu_lib):
    dirty_chunks_share_launches(gpu_lib, gpu_many_call)
    assert gpu_lib.bz3_hip_sync_device_many(0, None, None, None, None, None, None, None, None, None, None, None) == 0
    assert gpu_lib.bz3_hip_sync_device_many(2, None, None, None, None, None, None, None, None, None, None, None) == INIT


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
SHAPES = {"float32": (300, 256), "float64": (150, 256), "int64": (150, 256), "complex64": (200, 128), "complex128": (100, 128), "bfloat16": (700, 200), "float16": (700, 200),
          "int32": (300, 256), "int16": (700, 200), "int8": (1000, 333), "uint8": (1000, 333), "bool": (1000, 333)}  # a few hundred KiB: several chunks of 65 KiB


def _changed(x, rows):
    """x with the given rows replaced by other values of its dtype."""
    import torch

    y = x.clone()
    for r in rows:
        y[r] = ~x[r] if x.dtype == torch.bool else x[r] + 1
    return y


@pytest.mark.parametrize("dtype", list(bzip3_amd.DEFAULT_PLANES))
def test_sync_tensor_equals_a_fresh_pack(gpu_lib, dtype):
    """A few rows of a tensor change and nobody says which: the synced frame is the one pack_tensor gives for the new tensor, with its checksum;
    unpacking verifies and gives the new tensor bit for bit; everything else is carried over and p is unchanged."""
    import torch

    assert set(SHAPES) == set(bzip3_amd.DEFAULT_PLANES)
    shape = SHAPES[dtype]
    prev = _make(dtype, int(np.prod(shape)), 5, shape)
    p = bzip3_amd.pack_tensor(prev, 65 << 10, lib=gpu_lib)
    frame0 = p.frame.clone()
    for rows in ([], [0], [shape[0] - 1], [3, shape[0] // 2], range(shape[0])):
        x = _changed(prev, rows)
        fresh = bzip3_amd.pack_tensor(x, 65 << 10, lib=gpu_lib)
        q = bzip3_amd.sync_tensor(p, x, prev, lib=gpu_lib)
        assert torch.equal(q.frame, fresh.frame), list(rows)[:4]
        assert (q.dtype, q.shape, q.planes, q.block_size, q.nbytes, q.delta, q.base_crc) == (p.dtype, p.shape, p.planes, p.block_size, p.nbytes, False, None)
        assert q.crc == fresh.crc is not None
        got = bzip3_amd.unpack_tensor(q, verify=True, lib=gpu_lib)
        assert got.dtype == x.dtype and got.shape == x.shape and torch.equal(_bits(got), _bits(x))
    assert torch.equal(p.frame, frame0), "p was changed"


def test_check_prev(gpu_lib, monkeypatch):
    import torch

    prev = _make("float32", 300 * 256, 11, (300, 256))
    x = _changed(prev, [7])
    p = bzip3_amd.pack_tensor(prev, 65 << 10, lib=gpu_lib)
    wrong = _changed(prev, [200])
    real = gpu_lib.bz3_hip_sync_device_many
    monkeypatch.setattr(gpu_lib, "bz3_hip_sync_device_many", lambda *a: pytest.fail("the library was called"))
    with pytest.raises(ValueError):
        bzip3_amd.sync_tensor(p, x, wrong, lib=gpu_lib)  # before any coding work
    for bad, err in ((x.to(torch.float16), TypeError), (x[:299], TypeError), (x.cpu(), TypeError), ([1.0], TypeError)):
        with pytest.raises(err):
            bzip3_amd.sync_tensor(p, bad, prev, lib=gpu_lib)
        with pytest.raises(err):
            bzip3_amd.sync_tensor(p, x, bad, lib=gpu_lib)
    with pytest.raises(TypeError):
        bzip3_amd.sync_tensor(p.frame, x, prev, lib=gpu_lib)
    monkeypatch.setattr(gpu_lib, "bz3_hip_sync_device_many", real)
    fresh = bzip3_amd.pack_tensor(x, 65 << 10, lib=gpu_lib)
    assert torch.equal(bzip3_amd.sync_tensor(p, x, prev, lib=gpu_lib).frame, fresh.frame)
    # the caller vouches: a wrong prev raises nothing where it is not checked, and chunk 0 (row 7) is then still coded again
    q = bzip3_amd.sync_tensor(p, x, wrong, check_prev=False, lib=gpu_lib)
    nocrc = bzip3_amd.pack_tensor(prev, 65 << 10, checksum=False, lib=gpu_lib)
    assert nocrc.crc is None
    q2 = bzip3_amd.sync_tensor(nocrc, x, wrong, lib=gpu_lib)
    assert torch.equal(q.frame, q2.frame) and q.crc == q2.crc == fresh.crc
    assert torch.equal(bzip3_amd.sync_tensor(nocrc, x, prev, lib=gpu_lib).frame, fresh.frame)


def test_sync_tensors_on_raw_frames(gpu_lib):
    import torch

    from test_frame_update_emu import pattern

    old = _dev(pattern(3 * BS + 999, 31))
    frame = bzip3_amd.compress_tensor(old, 65 << 10, lib=gpu_lib, planes=2)
    new = old.clone()
    new[BS + 5] ^= 1
    new[3 * BS + 998] ^= 1
    want = bzip3_amd.compress_tensor(new, 65 << 10, lib=gpu_lib, planes=2)
    for block_sizes in (None, [65 << 10] * 2):
        got, counts = bzip3_amd.sync_tensors([frame, frame], [new, old], [old, old], planes=2, block_sizes=block_sizes, counts=True, lib=gpu_lib)
        assert torch.equal(got[0], want) and torch.equal(got[1], frame) and counts == [2, 0]
    assert torch.equal(bzip3_amd.sync_tensors([frame], [new], [old], planes=2, lib=gpu_lib)[0], want)
    assert torch.equal(bzip3_amd.sync_tensor_bytes(frame, new, old, planes=2, block_size=65 << 10, lib=gpu_lib), want)
    f, c = bzip3_amd.sync_tensor_bytes(frame, new, old, planes=2, counts=True, lib=gpu_lib)
    assert torch.equal(f, want) and c == 2
    assert bzip3_amd.sync_tensors([], [], [], lib=gpu_lib) == [] and bzip3_amd.sync_tensors([], [], [], counts=True, lib=gpu_lib) == ([], [])
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.sync_tensors([frame, frame], [new, new[:-1]], [old, old[:-1]], planes=2, lib=gpu_lib)
    assert e.value.code == bzip3_amd.BZ3_ERR_DATA_TOO_BIG and e.value.index == 1 and e.value.codes == [0, bzip3_amd.BZ3_ERR_DATA_TOO_BIG]
    assert torch.equal(e.value.outs[0], want) and e.value.outs[1].numel() == 0
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.sync_tensor_bytes(frame, new[:-1], old[:-1], planes=2, lib=gpu_lib)
    assert e.value.code == bzip3_amd.BZ3_ERR_DATA_TOO_BIG
    with pytest.raises(ValueError):
        bzip3_amd.sync_tensors([frame], [new], [old[:-1]], lib=gpu_lib)
    with pytest.raises(ValueError):
        bzip3_amd.sync_tensors([frame], [new, new], [old], lib=gpu_lib)
    with pytest.raises(TypeError):
        bzip3_amd.sync_tensors([frame], [new.view(torch.int8)], [old], lib=gpu_lib)


def test_sync_state_dict(gpu_lib, monkeypatch):
    import torch

    prev = {"a": _make("float32", 300 * 256, 21, (300, 256)), "b": _make("bfloat16", 700 * 200, 22, (700, 200)), "c": _make("uint8", 320 * 1040, 23, (320, 1040)),
            "step": _make("float32", 1, 24, ()), "frozen": _make("float16", 700 * 200, 25, (700, 200))}
    assert prev["c"].numel() == 5 * 65 * 1024  # its block size has to move: two distinct block sizes in the dict
    base = {"a": _make("float32", 300 * 256, 26, (300, 256))}
    packed = bzip3_amd.pack_state_dict(prev, 65 << 10, base=base, lib=gpu_lib)
    assert packed["a"].delta and len({packed[k].block_size for k in "abc"}) == 2
    sd = {"a": _changed(prev["a"], [0, 299]), "b": prev["b"].clone(), "c": _changed(prev["c"], [100]), "step": prev["step"] + 1}
    calls = []
    entry = "bz3_hip_sync_device_many"
    monkeypatch.setattr(gpu_lib, entry, (lambda real: lambda *a: calls.append(a[0]) or real(*a))(getattr(gpu_lib, entry)))
    stats = {}
    got = bzip3_amd.sync_state_dict(packed, sd, prev, base=base, stats=stats, lib=gpu_lib)
    assert sorted(calls) == [1, 3]  # one call per distinct block size
    assert list(got) == list(packed) and got["frozen"] is packed["frozen"] and got["a"] is not packed["a"]
    fresh = bzip3_amd.pack_state_dict(sd, 65 << 10, base=base, lib=gpu_lib)
    for k in sd:
        assert torch.equal(got[k].frame, fresh[k].frame) and (got[k].block_size, got[k].planes, got[k].crc, got[k].base_crc, got[k].delta, tuple(got[k].shape)) == (
            fresh[k].block_size, fresh[k].planes, fresh[k].crc, fresh[k].base_crc, fresh[k].delta, tuple(fresh[k].shape)), k
    chunks = {k: -(-packed[k].nbytes // max(65 << 10, min(packed[k].block_size, packed[k].nbytes + packed[k].nbytes // 50 + 32))) for k in sd}
    assert stats == {"a": (2, chunks["a"]), "b": (0, chunks["b"]), "c": (1, chunks["c"]), "step": (1, 1)} and chunks["a"] == 5
    # a delta-packed dict synced against the same base decodes with that base
    back = bzip3_amd.unpack_state_dict(got, base=base, verify=True, lib=gpu_lib)
    assert all(torch.equal(_bits(back[k]), _bits(sd[k] if k in sd else prev[k])) for k in prev)
    assert bzip3_amd.sync_state_dict(packed, {}, prev, lib=gpu_lib) == packed
    # an unknown or a missing name, a missing base: before any GPU work
    monkeypatch.setattr(gpu_lib, entry, lambda *a: pytest.fail("the library was called"))
    monkeypatch.setattr(gpu_lib, "bz3_hip_crc32c_device_many", lambda *a: pytest.fail("the library was called"))
    with pytest.raises(ValueError):
        bzip3_amd.sync_state_dict(packed, {"nope": sd["b"]}, prev, lib=gpu_lib)
    with pytest.raises(ValueError):
        bzip3_amd.sync_state_dict(packed, sd, {k: v for k, v in prev.items() if k != "b"}, base=base, lib=gpu_lib)
    with pytest.raises(ValueError):
        bzip3_amd.sync_state_dict(packed, sd, prev, lib=gpu_lib)  # "a" was packed against a base
    assert got["frozen"] is packed["frozen"] and list(packed) == list(prev)
