"""-m gpu: the index update on a real device (include/bz3_hip.h bz3_hip_update_device_select[_many], the select split of
bzip3_amd/csrc/planes.hpp; bzip3_amd's update_tensor[s]_select, update_tensor_slice, update_tensor_index and update_state_dict).  The cases and
the oracles are those of test_frame_update_select_emu -- the reference's frame of the updated bytes, numpy for S, D, phi and the select split's
formula, never the library under test --, on device memory; the oracle of the typed calls is torch's own index_copy / slice assignment followed by
the reference's frame of S(D(the result's bytes))."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
from oracle_lib import require_ref
from test_frame_delta_emu import D
from test_frame_planes_emu import BS, S, _ref_compress
from test_frame_select_emu import _pieces_arg, _seg, phi, piece_list, total
from test_frame_update_emu import FILL, INIT, LAST
from test_frame_update_select_emu import (covered_and_corrupt_chunks, debug_patch_select_rejects, decode_once, default_cap, delta_frames_match_reference, every_request_form, frames_match_reference,
                                          many_equal_single_calls, mixed_spec_patch_select, normal_forms_are_the_range_update, patch_select_case, periods_spec_patch_select,
                                          sweep_specs_patch_select, update_refusals)
from test_gpu_frame_delta import _gpu_alloc
from test_gpu_frame_planes import _host, _make, _raw
from test_gpu_frame_update import _dev, gpu_update_call

pytestmark = pytest.mark.gpu
MiB = 1 << 20


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_select_split_sweep_on_the_gpu(gpu_lib, k, has_base):
    """The emulator suite's sweep on device memory: every piece count, piece length and end at every source count, the three alignments."""
    rng = np.random.default_rng(121 + 10 * k + has_base)
    for spec in sweep_specs_patch_select(rng, k, has_base):
        patch_select_case(gpu_lib.bz3_hip_debug_patch_select, rng, spec, _gpu_alloc)


def test_select_split_large_periods_and_mixed_on_the_gpu(gpu_lib):
    """Four slots of 1 - 9 MiB per k with random piece tables (the tile index and the 32-bit chunk arithmetic at large values), the periods and
    first bytes, the mixed launch and the hook's refusals, on device memory."""
    rng = np.random.default_rng(121)
    for k in (1, 2, 4, 8):
        big = []
        for i in range(4):
            pieces = piece_list(rng, int(rng.integers(2, 200)), k, 16 * k * int(rng.integers(2, 400)))
            big.append(_seg(rng, pieces, k, i % 2, int(rng.integers(MiB, 8 * MiB)) // k * k + int(rng.integers(0, k)), i % 3))
            assert big[-1][3] < 2 ** 31
        patch_select_case(gpu_lib.bz3_hip_debug_patch_select, rng, big, _gpu_alloc)
    patch_select_case(gpu_lib.bz3_hip_debug_patch_select, rng, periods_spec_patch_select(rng), _gpu_alloc)
    patch_select_case(gpu_lib.bz3_hip_debug_patch_select, rng, mixed_spec_patch_select(rng), _gpu_alloc)
    patch_select_case(gpu_lib.bz3_hip_debug_patch_select, rng, [], _gpu_alloc)


def test_debug_patch_select_rejects_bad_arguments_on_the_gpu(gpu_lib):
    import torch

    buf = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    debug_patch_select_rejects(lambda s, b, d, *a: gpu_lib.bz3_hip_debug_patch_select(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), *a))
    assert _host(buf) == bytes(256)


# ---- frames -------------------------------------------------------------------------------------------------------------------
def gpu_select_update_call(lib, k, frame, offset, stride, count, pieces, data, base=None, cap=None, w=None):
    """test_frame_update_select_emu.select_update_call on device memory: (rc, *out_size, out[0, cap) after the call)."""
    import torch

    cap = default_cap(lib, frame) if cap is None else cap
    f, d, out = _dev(frame), _dev(data), _dev(bytes([FILL]) * cap)
    b = None if base is None else _dev(base)
    osz = C.c_size_t(cap)
    torch.cuda.synchronize()
    rc = lib.bz3_hip_update_device_select(k, f.data_ptr(), len(frame), offset, stride, count, len(pieces), _pieces_arg(pieces), d.data_ptr(), len(data) if w is None else w,
                                          None if b is None else b.data_ptr(), out.data_ptr(), C.byref(osz))
    assert _host(f)[: len(frame)] == bytes(frame) and _host(d)[: len(data)] == bytes(data) and (b is None or _host(b)[: len(base)] == bytes(base)), "an input was written"
    return rc, osz.value, _host(out)[:cap]


def gpu_many_call(lib, ks, frames, params, lists, datas, bases, caps=None):
    import torch

    n = len(frames)
    caps = [default_cap(lib, f) for f in frames] if caps is None else caps
    ins, dbufs, outs = [_dev(f) for f in frames], [_dev(d) for d in datas], [_dev(bytes([FILL]) * c) for c in caps]
    bbufs = [None if b is None else _dev(b) for b in bases]
    ptrs = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    out_sizes, rcs = (C.c_size_t * n)(*caps), (C.c_int * n)(*([77] * n))
    arrs = [_pieces_arg(l) for l in lists]
    pp = (C.POINTER(C.c_uint64) * n)(*[C.cast(a, C.POINTER(C.c_uint64)) if l else None for a, l in zip(arrs, lists)])
    torch.cuda.synchronize()
    rc = lib.bz3_hip_update_device_select_many(n, (C.c_uint32 * n)(*ks), ptrs(ins), (C.c_size_t * n)(*map(len, frames)),
                                               (C.c_uint64 * (4 * n))(*[v for p, l in zip(params, lists) for v in (*p, len(l))]), pp, ptrs(dbufs), (C.c_size_t * n)(*map(len, datas)),
                                               ptrs(bbufs), ptrs(outs), out_sizes, rcs)
    return rc, [(rcs[i], out_sizes[i], _host(outs[i])[: caps[i]]) for i in range(n)]


@pytest.mark.parametrize("chunks", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_index_updates_of_a_frame_match_the_reference(gpu_lib, k, chunks, monkeypatch):
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    frames_match_reference(gpu_lib, k, chunks, gpu_select_update_call)


@pytest.mark.parametrize("k", [1, 4])
def test_index_updates_of_a_delta_frame(gpu_lib, k):
    delta_frames_match_reference(gpu_lib, k, gpu_select_update_call)


def test_covered_chunks_are_not_decoded_and_corrupt_cut_chunks_fail(gpu_lib):
    covered_and_corrupt_chunks(gpu_lib, gpu_select_update_call)


def test_requests_in_range_form_are_the_range_update(gpu_lib):
    normal_forms_are_the_range_update(gpu_lib, gpu_select_update_call, gpu_update_call)


def test_a_chunk_with_many_pieces_is_decoded_once(gpu_lib):
    decode_once(gpu_lib, gpu_select_update_call)


def test_refusals_leave_out_untouched(gpu_lib):
    import torch

    case, req, data = update_refusals(gpu_lib, gpu_select_update_call)
    frame, pieces = case.frame, _pieces_arg(req[3])
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
        assert gpu_lib.bz3_hip_update_device_select(2, args[0], len(frame), *req[:3], 2, pieces, args[1], len(data), args[2], args[3], C.byref(osz)) == INIT
        assert osz.value == 0 and _host(arena) == before
    osz = C.c_size_t(cap)  # adjacent: fine
    assert gpu_lib.bz3_hip_update_device_select(2, f.data_ptr(), len(frame), *req[:3], 2, pieces, at(cap), len(data), None, at(0), C.byref(osz)) == 0


def test_many_updates_equal_their_single_calls_across_windows(gpu_lib, monkeypatch):
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    many_equal_single_calls(gpu_lib, gpu_many_call, gpu_select_update_call)
    many = gpu_lib.bz3_hip_update_device_select_many
    assert many(0, None, None, None, None, None, None, None, None, None, None, None) == 0
    assert many(2, None, None, None, None, None, None, None, None, None, None, None) == INIT


class _PackedBytes:
    """A uint8 tensor of five chunks of 65 KiB and a short one, packed with element size 4 (with_base: against a base).  Tensor and base are bytes
    of few values, so that every chunk codes to less than the block size: the format has no chunk that does not."""

    def __init__(self, lib, with_base, seed):
        import torch

        self.sizes = [BS] * 5 + [LAST]
        self.starts, self.T = [j * BS for j in range(6)], 5 * BS + LAST
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randint(0, 7, (self.T,), generator=g, dtype=torch.uint8).to("cuda:0")
        self.base = torch.randint(0, 5, (self.T,), generator=g, dtype=torch.uint8).to("cuda:0") if with_base else None
        self.p = bzip3_amd.pack_tensor(self.x, BS, planes=4, base=self.base, lib=lib)
        assert self.p.block_size == BS and self.p.delta == with_base


@pytest.mark.parametrize("window", [2, 16])
def test_one_call_holds_every_request_form(gpu_lib, window, monkeypatch):
    """The device twin of test_frame_update_select_emu's test of this name, through update_tensors_select: the five request forms in ONE call, in
    windows of two chunks and in one window, whose patch launch then holds whole, clipped and select splits.  Every frame is the one pack_tensor
    gives for the updated tensor."""
    import torch

    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", str(window))
    cases, params, lists = every_request_form(lambda wb, seed: _PackedBytes(gpu_lib, wb, seed))
    datas, bases, wants = [], [], []
    for i, (c, (offset, stride, count), pieces) in enumerate(zip(cases, params, lists)):
        idx = torch.from_numpy(phi(offset, stride, pieces, count * total(pieces))).to("cuda:0")
        datas.append(torch.randint(0, 9, (idx.numel(),), generator=torch.Generator().manual_seed(70 + i), dtype=torch.uint8).to("cuda:0"))
        bases.append(None if c.base is None else c.base[idx])
        wants.append(c.x.index_copy(0, idx, datas[-1]))
    got = bzip3_amd.update_tensors_select([c.p.frame for c in cases], *zip(*params), lists, datas, planes=4, bases=bases, lib=gpu_lib, block_sizes=[BS] * 5)
    for i, (c, f, want) in enumerate(zip(cases, got, wants)):
        assert torch.equal(f, bzip3_amd.pack_tensor(want, BS, planes=4, base=c.base, lib=gpu_lib).frame), ("frames differ", i)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def _bits(x):
    import torch

    return torch.view_as_real(x) if x.is_complex() else x.contiguous().reshape(-1).view(torch.uint8)


def _tensor(dtype, shape, seed):
    import torch

    n = int(np.prod(shape))
    if dtype == "int8":
        return torch.randint(-3, 4, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int8).reshape(shape).to("cuda:0")
    return _make(dtype, n, seed, shape).to("cuda:0")


def ref_frame(p, want, base=None):
    """The reference's frame of S(D(want's bytes, the base's bytes)) at p's block size and element size."""
    ref = require_ref().lib
    d = _raw(want) if base is None else bytes(D(_raw(want), _raw(base)))
    rc, f = _ref_compress(ref, p.block_size, S(d, p.block_size, p.planes, ref.bz3_bound))
    assert rc == 0
    return f


def check_packed(q, p, want, base=None):
    assert _host(q.frame) == ref_frame(p, want, base), "the frame is not the reference's frame of the updated tensor"
    assert q.crc is None and (q.dtype, q.shape, q.planes, q.block_size, q.nbytes, q.delta, q.base_crc) == (p.dtype, p.shape, p.planes, p.block_size, p.nbytes, p.delta, p.base_crc)


TYPED = [("bfloat16", (24, 64, 750), 2), ("float32", (20, 30, 1000), 4), ("int8", (30, 50, 1500), 1), ("complex64", (9, 40, 1000), 4)]  # 3 chunks of 1 MiB
OPS = [("dim0", 0, 5, False), ("last", -1, 40, False), ("middle_permuted", 1, 7, True), ("slice", 1, 0, False)]


@pytest.mark.parametrize("op,dim,n_idx,permute", OPS, ids=[o for o, *_ in OPS])
@pytest.mark.parametrize("dtype,shape,planes", TYPED, ids=[t for t, _, _ in TYPED])
def test_update_tensor_index_and_slice_equal_the_reference_frame(gpu_lib, dtype, shape, planes, op, dim, n_idx, permute):
    """index_copy along dim 0 and the last dim with an increasing index, along a middle dim with a permutation, and a slice along an inner dim: the
    frame is the reference's frame of the tensor torch's own index_copy or slice assignment gives; p is unchanged."""
    import torch

    x = _tensor(dtype, shape, 5)
    p = bzip3_amd.pack_tensor(x, MiB, planes=planes, lib=gpu_lib)
    assert 3 <= -(-p.nbytes // p.block_size) <= 6
    frame0 = p.frame.clone()
    if op == "slice":
        values = _tensor(dtype, (shape[0], 9, shape[2]), 9)
        want = x.clone()
        want[:, 11:20] = values
        q = bzip3_amd.update_tensor_slice(p, 1, 11, 20, values, lib=gpu_lib)
        assert torch.equal(_bits(bzip3_amd.unpack_tensor(q, lib=gpu_lib)), _bits(want))
        empty = bzip3_amd.update_tensor_index(p, 0, [], values[:0].reshape(0, *shape[1:]), lib=gpu_lib)
        assert torch.equal(empty.frame, frame0)  # an empty index: the frame itself
    else:
        rng = np.random.default_rng(7 + n_idx)
        idx = sorted(int(v) for v in rng.choice(shape[dim], size=n_idx, replace=False))
        idx[1] = idx[0] + 1  # (two neighbours: one piece)
        if permute:
            idx = [idx[j] for j in rng.permutation(len(idx))]
        vshape = list(shape)
        vshape[dim] = len(idx)
        values = _tensor(dtype, tuple(vshape), 6 + dim)
        want = x.index_copy(dim % 3, torch.tensor(idx, device=x.device), values)
        q = bzip3_amd.update_tensor_index(p, dim, idx if dim else torch.tensor(idx, device=x.device), values, lib=gpu_lib)
    check_packed(q, p, want)
    assert torch.equal(p.frame, frame0) and p.crc is not None, "p was changed"


def test_update_tensor_index_of_a_delta_tensor(gpu_lib):
    import torch

    shape = (20, 30, 1000)
    base = _tensor("float32", shape, 11)
    x = base + _tensor("float32", shape, 12) * 0.01
    p = bzip3_amd.pack_tensor(x, MiB, base=base, lib=gpu_lib)
    assert p.delta
    idx = [3, 4, 17, 29]
    index = torch.tensor(idx, device=x.device)
    values = _tensor("float32", (20, 4, 1000), 13)
    want = x.index_copy(1, index, values)
    part = base.index_select(1, index)
    q = bzip3_amd.update_tensor_index(p, 1, idx, values, base=part, lib=gpu_lib)
    check_packed(q, p, want, base)
    assert torch.equal(_bits(bzip3_amd.unpack_tensor(q, base=base, lib=gpu_lib)), _bits(want))
    with pytest.raises(ValueError):
        bzip3_amd.update_tensor_index(p, 1, idx, values, lib=gpu_lib)  # the base's part is required
    with pytest.raises(ValueError):
        bzip3_amd.update_tensor_index(p, 1, idx, values, base=part[:, :3], lib=gpu_lib)
    with pytest.raises(ValueError):
        bzip3_amd.update_tensor_index(p, 1, [4, 3, 17, 40], values, base=part, lib=gpu_lib)  # with a base the index must increase


def test_update_state_dict_is_one_call(gpu_lib, monkeypatch):
    import torch

    sd = {"a": _tensor("float32", (300, 256), 21), "b": _tensor("bfloat16", (700, 200), 22), "c": _tensor("int8", (1000, 333), 23), "d": _tensor("float32", (64, 40, 30), 24),
          "step": _tensor("float32", (), 25)}
    base = {"a": _tensor("float32", (300, 256), 26)}
    packed = bzip3_amd.pack_state_dict(sd, 65 << 10, base=base, lib=gpu_lib)
    assert packed["a"].delta and not packed["b"].delta
    calls = []
    entry = "bz3_hip_update_device_select_many"
    monkeypatch.setattr(gpu_lib, entry, (lambda real: lambda *a: calls.append(entry) or real(*a))(getattr(gpu_lib, entry)))
    rows = {"a": (10, _tensor("float32", (5, 256), 27))}
    slices = {"b": (1, 50, 70, _tensor("bfloat16", (700, 20), 28))}
    index = {"c": (0, [900, 3, 4, 500], _tensor("int8", (4, 333), 29)), "d": (1, torch.tensor([1, 2, 39]), _tensor("float32", (64, 3, 30), 30))}
    got = bzip3_amd.update_state_dict(packed, rows=rows, slices=slices, index=index, base={"a": base["a"][10:15]}, lib=gpu_lib)
    assert calls == [entry]
    assert list(got) == list(packed) and got["step"] is packed["step"] and all(got[k] is not packed[k] for k in "abcd")
    want = {k: v.clone() for k, v in sd.items()}
    want["a"][10:15] = rows["a"][1]
    want["b"][:, 50:70] = slices["b"][3]
    want["c"] = want["c"].index_copy(0, torch.tensor(index["c"][1], device="cuda:0"), index["c"][2])
    want["d"] = want["d"].index_copy(1, index["d"][1].to("cuda:0"), index["d"][2])
    for k in "abcd":
        check_packed(got[k], packed[k], want[k], base.get(k))
    assert bzip3_amd.update_state_dict(packed, lib=gpu_lib) == packed
    for kw in ({"rows": {"nope": rows["a"]}}, {"rows": rows, "index": {"a": (0, [1], rows["a"][1][:1])}}, {"slices": {"b": slices["b"]}, "rows": {"b": (0, slices["b"][3])}}):
        with pytest.raises(ValueError):
            bzip3_amd.update_state_dict(packed, lib=gpu_lib, **kw)


def test_update_tensors_select_on_raw_frames(gpu_lib):
    """The uint8 layer: an index set of a compress_tensor frame replaced, with the block size read from the frame header and given."""
    import torch

    from test_frame_select_emu import phi
    from test_frame_update_emu import pattern

    raw = _dev(pattern(3 * BS + 999, 31))
    frame = bzip3_amd.compress_tensor(raw, 65 << 10, lib=gpu_lib, planes=2)
    req = (BS - 500, 3000, 40, [(0, 64), (100, 31)])
    data = _dev(pattern(40 * 95, 32))
    want = np.frombuffer(_host(raw), dtype=np.uint8).copy()
    want[phi(req[0], req[1], req[3], 40 * 95)] = np.frombuffer(_host(data), dtype=np.uint8)
    ref = require_ref().lib
    fresh = _ref_compress(ref, 65 << 10, S(bytes(want), 65 << 10, 2, ref.bz3_bound))[1]
    for bs in (None, 65 << 10):
        assert _host(bzip3_amd.update_tensor_select(frame, *req, data, planes=2, lib=gpu_lib, block_size=bs)) == fresh
    assert bzip3_amd.update_tensors_select([], [], [], [], [], [], lib=gpu_lib) == []
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.update_tensors_select([frame, frame], [req[0], raw.numel() - 3000], [3000] * 2, [40] * 2, [req[3]] * 2, [data, data], planes=2, lib=gpu_lib)
    assert e.value.code == bzip3_amd.BZ3_ERR_DATA_TOO_BIG and e.value.index == 1 and e.value.codes == [0, bzip3_amd.BZ3_ERR_DATA_TOO_BIG]
    assert _host(e.value.outs[0]) == fresh and e.value.outs[1].numel() == 0


def test_argument_errors_raise_before_any_gpu_call(gpu_lib, monkeypatch):
    import torch

    x = _tensor("float32", (30, 40, 50), 41)
    p = bzip3_amd.pack_tensor(x, 65 << 10, lib=gpu_lib)
    monkeypatch.setattr(gpu_lib, "bz3_hip_update_device_select_many", lambda *a: pytest.fail("the library was called"))
    v = _tensor("float32", (30, 3, 50), 42)
    for dim, index, values, err in ((1, [1, 2, 40], v, ValueError), (1, [-1, 2, 3], v, ValueError), (1, [1, 2, 2], v, ValueError), (3, [1, 2, 3], v, ValueError),
                                    (1, [1.5, 2, 3], v, ValueError), (1, [1, 2, 3], v.to(torch.float16), TypeError), (1, [1, 2, 3], v[:, :2], TypeError),
                                    (1, [3, 2, 1], v[:, :2], TypeError), (1, [1, 2, 3], v.cpu(), TypeError), (1, [1, 2, 3], [1.0], TypeError), (0, [1, 2, 3], v, TypeError)):
        with pytest.raises(err):
            bzip3_amd.update_tensor_index(p, dim, index, values, lib=gpu_lib)
    with pytest.raises(TypeError):
        bzip3_amd.update_tensor_index(p.frame, 1, [1, 2, 3], v, lib=gpu_lib)
    for dim, start, stop, values, err in ((1, 38, 41, v, ValueError), (1, 5, 4, v, ValueError), (-4, 0, 3, v, ValueError), (1, 0, 3, v.to(torch.float16), TypeError),
                                          (1, 0, 4, v, TypeError), (1, 0, 3, v.cpu(), TypeError)):
        with pytest.raises(err):
            bzip3_amd.update_tensor_slice(p, dim, start, stop, values, lib=gpu_lib)
    with pytest.raises(ValueError):
        bzip3_amd.update_tensor_slice(bzip3_amd.pack_tensor(_tensor("float32", (), 43), lib=gpu_lib), 0, 0, 1, v, lib=gpu_lib)
    f, d = p.frame, p.frame[:10]
    for args in (([f], [0, 1], [9], [1], [[(0, 10)]], [d]), ([f], [-1], [9], [1], [[(0, 10)]], [d]), ([f], [0], [9], [1], [[(5, 5), (0, 5)]], [d]), ([f], [0], [9], [2], [[(0, 10)]], [d]),
                 ([f], [0], [20], [1], [[(0, 9)]], [d]), ([f], [0], [20], [1], [[(0, 11)]], [d])):
        with pytest.raises(ValueError):
            bzip3_amd.update_tensors_select(*args, lib=gpu_lib)
    with pytest.raises(TypeError):
        bzip3_amd.update_tensors_select([f], [0], [20], [1], [[(0, 10)]], [x], lib=gpu_lib)
