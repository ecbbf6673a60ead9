"""-m gpu: the index decode calls on a real device (include/bz3_hip.h bz3_hip_decompress_device_select[_many], the select merge of
bzip3_amd/csrc/planes.hpp, the walk with a piece table of frame.hpp; bzip3_amd's decompress_tensor[s]_select, unpack_tensor_index and
unpack_state_dict(index=...)).  The oracle of a request is full[phi(t)], `full` from the real reference, numpy merge_k per chunk and
numpy D_inv (test_frame_range_emu.Case), never from the library under test; the oracle of a typed index_select is torch's on the tensor
that was packed."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
from oracle_lib import require_ref
from test_frame_range_emu import GUARD, INIT, MALFORMED, Case, _flip, _with_header, stream_for
from test_frame_select_emu import (DST_COUNTS, _pieces_arg, _seg, committed_below, frame_requests, in_place_spec_select, index_base, mixed_spec_select, piece_list, select_case,
                                   sweep_specs_select, total, want_select)
from test_gpu_frame_delta import _gpu_alloc
from test_gpu_frame_planes import _host, _make, _raw
from test_gpu_frame_range import _dev
from test_gpu_frame_strided import gpu_strided_call

pytestmark = pytest.mark.gpu
KiB65 = 65 << 10


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_select_kernel_sweep_on_the_gpu(gpu_lib, k, has_base):
    """The emulator suite's sweep on device memory: every piece count and end at the tile-edge destination counts, then the three
    alignments."""
    rng = np.random.default_rng(95 + 10 * k + has_base)
    for spec in sweep_specs_select(rng, k, has_base, counts=DST_COUNTS):
        select_case(gpu_lib.bz3_hip_debug_select, rng, spec, _gpu_alloc)


def test_select_kernel_mixed_in_place_and_many_tiles_on_the_gpu(gpu_lib):
    """The mixed launch, the in-place launch, and per k one segment of about a hundred tiles over a list of 1000 pieces, on device memory."""
    rng = np.random.default_rng(96)
    call = gpu_lib.bz3_hip_debug_select
    select_case(call, rng, mixed_spec_select(rng), _gpu_alloc)
    select_case(call, rng, in_place_spec_select(rng), _gpu_alloc, in_place=True)
    select_case(call, rng, [_seg(rng, piece_list(rng, 1000, k, 16 * k * 40), k, k % 4 == 0, 400_000 * k + 3, k % 3) for k in (1, 2, 4, 8)], _gpu_alloc)


# ---- frames -------------------------------------------------------------------------------------------------------------------
def gpu_select_call(lib, k, frame, offset, stride, count, pieces, cap, base=None, in_place=False, room=None):
    """(rc, *out_size, out[0, w + GUARD) after the call, before it).  frame: host bytes or a device tensor; base: the base's bytes of the
    index set (host bytes)."""
    import torch

    frame_t = frame if isinstance(frame, torch.Tensor) else _dev(frame)
    room = (min(cap, count * total(pieces)) if room is None else room) + GUARD
    before = (bytes(base) + b"\xa5" * room)[:room] if in_place else b"\xa5" * room
    out = _dev(before)
    b = out if in_place else None if base is None else _dev(base)
    osz = C.c_size_t(cap)
    torch.cuda.synchronize()
    rc = lib.bz3_hip_decompress_device_select(k, frame_t.data_ptr(), frame_t.numel(), offset, stride, count, len(pieces), _pieces_arg(pieces), None if b is None else b.data_ptr(),
                                              0 if base is None else room - GUARD if in_place else len(base), out.data_ptr(), C.byref(osz))
    return rc, osz.value, _host(out)[:room], before


def gpu_check_select(lib, case, frame_t, offset, stride, count, pieces, cap=None, in_place=False):
    cap = count * total(pieces) if cap is None else cap
    base = index_base(case, offset, stride, count, pieces, cap)
    rc, r, got, before = gpu_select_call(lib, case.k, frame_t, offset, stride, count, pieces, cap, base, in_place and base is not None)
    want = want_select(case, offset, stride, count, pieces, cap)
    assert (rc, r) == (0, len(want)), (offset, stride, count, pieces[:4], cap, rc, r, len(want))
    assert got[:r] == want, ("bytes differ", offset, stride, count, pieces[:4], cap)
    assert got[r:] == before[r:], ("wrote beyond the index set", offset, stride, count, pieces[:4], cap)


CASES = [(k, wb, bs) for bs in (KiB65, KiB65 + 3) for k in (1, 2, 4, 8) for wb in (0, 1)]


@pytest.mark.parametrize("k,with_base,bs", CASES, ids=[f"k{k}-{'base' if wb else 'plain'}-{bs}" for k, wb, bs in CASES])
def test_select_requests_of_a_frame_match_the_reference(gpu_lib, k, with_base, bs, monkeypatch):
    """Four full blocks of 65 KiB (65 KiB + 3) and a short one, windows of two chunks: the emulator suite's requests, and on the full chunks
    long pieces in every chunk and a period shorter than a chunk that runs through all of them, in place where there is a base."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    case = Case(require_ref().lib, bs, k, with_base, stream_for(bs, blocks=4))
    assert len(case.sizes) == 5 and case.sizes[:4] == [bs] * 4
    frame_t = _dev(case.frame)
    for offset, stride, count, pieces, cap in frame_requests(case):
        gpu_check_select(gpu_lib, case, frame_t, offset, stride, count, pieces, cap)
    gpu_check_select(gpu_lib, case, frame_t, 10, 0, 1, [(j * bs + 100 * j, bs // 2 + 7 * j) for j in range(5)], in_place=True)
    gpu_check_select(gpu_lib, case, frame_t, bs - 30, 20000, 13, [(0, 4096), (5000, 33), (5040, 8000), (19000, 1000)], in_place=True)


def test_equivalence_refusals_and_skipping(gpu_lib, monkeypatch):
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    ref = require_ref().lib
    bs = KiB65 + 3
    case = Case(ref, bs, 4, 1, stream_for(bs, blocks=4))
    s = case.starts
    # one piece after normalisation is the strided call: bytes, rc, *out_size
    for frame in (case.frame, _flip(case.frame, 2)):
        frame_t = _dev(frame)
        for (offset, stride, count, pieces, cap), strided in (((s[1] - 50, 2 * bs, 2, [(7, bs + 100)], 10 ** 9), (s[1] - 43, bs + 100, 2 * bs, 2)),
                                                              ((s[1] - 48, 3000, 40, [(0, 300), (300, 0), (300, 500), (800, 200)], 30_001), (s[1] - 48, 1000, 3000, 40)),
                                                              ((s[2] - 20, 500, 3, [(0, 100), (200, 50)], 64), (s[2] - 20, 100, 500, 3))):
            w = min(cap, count * total(pieces))
            base = index_base(case, offset, stride, count, pieces, cap)
            assert gpu_select_call(gpu_lib, 4, frame_t, offset, stride, count, pieces, cap, base, room=w) == gpu_strided_call(gpu_lib, 4, frame_t, *strided, w, base)
    # invalid lists, before any write
    frame_t = _dev(case.frame)
    for offset, stride, count, pieces in ((0, 100, 2, [(0, 10), (5, 10)]), (0, 100, 2, [(20, 10), (0, 10)]), (0, 25, 2, [(0, 10), (20, 6)]), (0, 100, 2, [(0, 10), (200, 0)]), (0, 2 ** 34, 2 ** 31, [(0, 2 ** 32), (2 ** 33, 2 ** 32)]),
                                          (2 ** 64 - 51, 20, 4, [(0, 5), (10, 5)]), (0, 2 ** 40, 2, [(5, 2 ** 64 - 4), (2 ** 64 - 1, 0)])):
        rc, r, got, before = gpu_select_call(gpu_lib, 4, frame_t, offset, stride, count, pieces, 64, room=64)
        assert (rc, r) == (INIT, 0) and got == before, (offset, stride, count, pieces)
    out, osz = _dev(b"\xa5" * 64), C.c_size_t(64)
    assert gpu_lib.bz3_hip_decompress_device_select(4, frame_t.data_ptr(), frame_t.numel(), 0, 100, 2, 2, None, None, 0, out.data_ptr(), C.byref(osz)) == INIT  # NULL pieces, m > 0
    assert osz.value == 0 and _host(out) == b"\xa5" * 64
    pieces = [(0, 60), (100, 40)]
    arena = _dev(index_base(case, 0, 300, 10, pieces, 1000) + b"\xa5" * 3000)  # a partial overlap of out and base
    before = _host(arena)
    osz = C.c_size_t(4000)
    assert gpu_lib.bz3_hip_decompress_device_select(4, frame_t.data_ptr(), frame_t.numel(), 0, 300, 10, 2, _pieces_arg(pieces), arena.data_ptr(), 4000, arena.data_ptr() + 16, C.byref(osz)) == INIT
    assert _host(arena) == before and osz.value == 0
    for pieces in ([], [(7, 0)]):  # m == 0 and L == 0: the header alone
        assert gpu_select_call(gpu_lib, 4, frame_t, 5, 9, 4, pieces, 64, room=64)[:2] == (0, 0)
        assert gpu_select_call(gpu_lib, 4, _dev(case.frame[:12]), 5, 9, 4, pieces, 64, room=64)[:2] == (MALFORMED, 0)
    # chunks 0, 2 and 4 are needed: chunk 1 lies in a gap inside a period, chunk 3 between two periods
    offset, stride, count, pieces = 100, 4 * bs, 2, [(0, bs // 2), (2 * bs + 10, 3000)]
    w = count * total(pieces)
    base = index_base(case, offset, stride, count, pieces, w)
    good = want_select(case, offset, stride, count, pieces, w)
    for j in range(5):
        rc, r, got, before = gpu_select_call(gpu_lib, 4, _flip(case.frame, j), offset, stride, count, pieces, w, base)
        if j % 2:
            assert (rc, r) == (0, len(good)) and got[:r] == good, ("a corrupt payload in a gap was noticed", j)
        else:
            assert rc != 0 and r == committed_below(offset, stride, pieces, w, s[j]) == (0, 0, bs // 2, 0, bs // 2 + 3000)[j] and got[:r] == good[:r], (j, rc, r)
        assert got[r:] == before[r:], j
        rc, r, got, before = gpu_select_call(gpu_lib, 4, _with_header(case.frame, j, orig=-5), offset, stride, count, pieces, w, base)
        assert rc == MALFORMED and r == committed_below(offset, stride, pieces, w, s[j]) and got[:r] == good[:r] and got[r:] == before[r:], (j, rc, r)


def test_select_calls_decode_a_chunk_once_however_many_pieces_it_holds(gpu_lib, monkeypatch):
    """Five chunks.  Pieces in chunks 0, 2 and 4 with windows of two chunks: 2 CM launches, the full decode takes 3.  Windows of one chunk:
    three pieces in chunk 1 and one in chunk 3 take exactly 2 launches; the same four pieces as four range entries of one _many call take 4."""
    import torch

    bs = KiB65
    case = Case(require_ref().lib, bs, 1, 0, stream_for(bs, blocks=4))
    frame_t = _dev(case.frame)
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    gpu_lib.bz3_hip_debug_cm_launches(1)
    gpu_check_select(gpu_lib, case, frame_t, 10, 0, 1, [(0, 100), (2 * bs + 5, 100), (4 * bs, 100)])
    assert gpu_lib.bz3_hip_debug_cm_launches(1) == 2
    gpu_check_select(gpu_lib, case, frame_t, 0, 0, 1, [(0, 100), (200, case.T - 200)])
    assert gpu_lib.bz3_hip_debug_cm_launches(1) == 3
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "1")
    pieces = [(bs + 10, 100), (bs + 500, 64), (2 * bs - 300, 200), (3 * bs + 7, 100)]
    gpu_check_select(gpu_lib, case, frame_t, 0, 0, 1, pieces)
    assert gpu_lib.bz3_hip_debug_cm_launches(1) == 2
    n = len(pieces)
    outs = [_dev(b"\xa5" * l) for _, l in pieces]
    out_sizes, rcs = (C.c_size_t * n)(*[l for _, l in pieces]), (C.c_int * n)()
    torch.cuda.synchronize()
    assert gpu_lib.bz3_hip_decompress_device_range_many(n, None, (C.c_void_p * n)(*[frame_t.data_ptr()] * n), (C.c_size_t * n)(*[frame_t.numel()] * n),
                                                        (C.c_uint64 * n)(*[a for a, _ in pieces]), None, None, (C.c_void_p * n)(*[o.data_ptr() for o in outs]), out_sizes, rcs) == 0
    assert b"".join(_host(o) for o in outs) == want_select(case, 0, 0, 1, pieces, 10 ** 9)
    assert gpu_lib.bz3_hip_debug_cm_launches(1) == 4


def test_many_select_requests_equal_their_single_calls(gpu_lib, monkeypatch):
    import torch

    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    ref = require_ref().lib
    bs = KiB65 + 3
    cases = [Case(ref, bs, k, wb, stream_for(bs, blocks=nb, last=last), seed=290 + i) for i, (k, wb, nb, last) in enumerate(((2, 1, 2, 777), (1, 0, 1, 50), (8, 1, 4, 1234), (4, 0, 0, 100)))]
    # (case, (offset, stride, count), pieces, *out_size): piece lists, a strided, a contiguous and an empty request, the same frame three times
    plan = [(0, (bs - 30, 500, 9), [(0, 40), (41, 19), (100, 7)], 10 ** 6), (1, (0, 10, 10 ** 4), [(0, 4), (4, 6)], 10 ** 6), (2, (10, 2 * bs, 3), [(0, 3000), (4000, 2000), (bs, 64)], 10 ** 6),
            (2, (bs + 7, 1024, 200), [(0, 16), (20, 30), (64, 18)], 64 * 200 - 9), (3, (7, 11, 9), [(0, 2), (3, 1), (5, 2)], 10 ** 6), (0, (5, 9, 9), [], 50),
            (2, (3 * bs - 8, 40, 4000), [(0, 16), (17, 16)], 10 ** 6), (3, (3, 20, 4), [(1, 8)], 10 ** 6)]
    n = len(plan)
    frame_ts = [_dev(cases[c].frame) for c, *_ in plan]
    ks = [cases[c].k for c, *_ in plan]
    ws = [min(cap, p[2] * total(l)) for _, p, l, cap in plan]
    bases = [index_base(cases[c], *p, l, cap) for c, p, l, cap in plan]
    outs = [_dev(b"\xa5" * (w + GUARD)) for w in ws]
    base_ts = [None if b is None else _dev(b) for b in bases]
    out_sizes, rcs = (C.c_size_t * n)(*[cap for *_, cap in plan]), (C.c_int * n)(*([77] * n))
    vp = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    arrs = [_pieces_arg(l) for _, _, l, _ in plan]
    torch.cuda.synchronize()
    rc = gpu_lib.bz3_hip_decompress_device_select_many(n, (C.c_uint32 * n)(*ks), vp(frame_ts), (C.c_size_t * n)(*[f.numel() for f in frame_ts]),
                                                       (C.c_uint64 * (4 * n))(*[v for _, p, l, _ in plan for v in (*p, len(l))]),
                                                       (C.POINTER(C.c_uint64) * n)(*[C.cast(a, C.POINTER(C.c_uint64)) for a in arrs]), vp(base_ts),
                                                       (C.c_size_t * n)(*[0 if b is None else len(b) for b in bases]), vp(outs), out_sizes, rcs)
    assert rc == 0
    for i, (c, p, l, cap) in enumerate(plan):
        want = want_select(cases[c], *p, l, cap)
        assert (rcs[i], out_sizes[i]) == (0, len(want)) and _host(outs[i]) == want + b"\xa5" * (ws[i] + GUARD - len(want)), i
        assert gpu_select_call(gpu_lib, ks[i], frame_ts[i], *p, l, cap, bases[i])[:3] == (0, len(want), _host(outs[i])), ("single call", i)


# ---- python ---------------------------------------------------------------------------------------------------------------------
SHAPE = (6, 25, 501)  # about 300 KB of float32: five blocks at the 65 KiB floor, so that index sets cross chunks
INDEX_DTYPES = ["float32", "bfloat16", "int8", "complex64"]


def _indices(size, rng):
    """Sorted, a permutation, duplicates, empty, arange."""
    some = sorted({int(v) for v in rng.integers(0, size, size=max(2, size // 3))})
    return [("sorted", some), ("permutation", [int(v) for v in rng.permutation(size)]), ("duplicates", [size - 1, 0, 0, size // 2, size - 1]), ("empty", []), ("arange", list(range(size)))]


@pytest.mark.parametrize("dtype", INDEX_DTYPES)
def test_unpack_tensor_index(gpu_lib, dtype):
    import torch

    rng = np.random.default_rng(5)
    numel = SHAPE[0] * SHAPE[1] * SHAPE[2]
    x = _make(dtype, numel, 31, SHAPE)
    base = _make(dtype, numel, 32, SHAPE)
    dev = x.device
    sel = lambda t, dim, idx: t.index_select(dim, torch.tensor(idx, dtype=torch.int64, device=dev))  # noqa: E731
    for b in (None, base):
        p = bzip3_amd.pack_tensor(x, 65 << 10, base=b)
        assert p.delta == (b is not None)
        for dim in (0, 1, 2, -2):
            for name, idx in _indices(SHAPE[dim % 3], rng):
                increasing = all(a < z for a, z in zip(idx, idx[1:]))
                if b is not None and not increasing:
                    with pytest.raises(ValueError):
                        bzip3_amd.unpack_tensor_index(p, dim, idx, base=sel(b, dim, idx))
                    continue
                want = sel(x, dim, idx)
                y = bzip3_amd.unpack_tensor_index(p, dim, idx, base=None if b is None else sel(b, dim, idx))
                assert y.dtype == x.dtype and y.shape == want.shape and y.is_contiguous() and _raw(y) == _raw(want), (dtype, dim, name)
                if name == "arange":
                    z = bzip3_amd.unpack_tensor_slice(p, dim, 0, len(idx), base=None if b is None else b)
                    assert _raw(y) == _raw(z)
        for dim, idx in ((1, [3, 4, 5, 11, 24]), (2, [500, 7, 7, 100]) if b is None else (2, [7, 100, 101, 500])):
            want = sel(x, dim, idx)
            out = torch.empty_like(want, memory_format=torch.contiguous_format)
            assert bzip3_amd.unpack_tensor_index(p, dim, idx, out=out, base=None if b is None else sel(b, dim, idx)) is out and _raw(out) == _raw(want)
            if b is not None:
                over = sel(b, dim, idx).contiguous()
                assert bzip3_amd.unpack_tensor_index(p, dim, idx, out=over, base=over) is over and _raw(over) == _raw(want)
        # the index as a numpy array and as a device tensor
        idx = [1, 2, 4]
        for form in (np.array(idx), torch.tensor(idx, device=dev), torch.tensor(idx, dtype=torch.int32)):
            assert _raw(bzip3_amd.unpack_tensor_index(p, 0, form, base=None if b is None else sel(b, 0, idx))) == _raw(sel(x, 0, idx))
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor_index(p, 1, [3, 11])  # a delta tensor without its base
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor_index(p, 1, [3, 11], base=base)  # the whole base is not the index_select of the base
    plain = bzip3_amd.pack_tensor(x, 65 << 10)
    for dim, idx in ((3, [0]), (-4, [0]), (1, [-1]), (1, [25]), (2, [0, 501]), (0, [1.5]), (0, torch.tensor([[1]])), (0, torch.tensor([1.0]))):
        with pytest.raises(ValueError):
            bzip3_amd.unpack_tensor_index(plain, dim, idx)
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor_index(bzip3_amd.pack_tensor(x[0, 0, 0], 65 << 10), 0, [0])  # 0-d
    with pytest.raises(TypeError):
        bzip3_amd.unpack_tensor_index(plain, 1, [3, 11], out=torch.empty_like(x))
    short = bzip3_amd.PackedTensor(plain.frame[: plain.frame.numel() // 2], plain.dtype, plain.shape, plain.planes, plain.block_size, plain.nbytes)
    with pytest.raises(bzip3_amd.Bz3Error):
        bzip3_amd.unpack_tensor_index(short, 1, [20, 24])


def test_chosen_experts_decode_their_chunks_once(gpu_lib, monkeypatch):
    """(16, 40, 256) float32 at 65 KiB blocks: an expert is 40 KiB, so chunks hold parts of up to three experts.  With windows of one chunk
    the CM launches count the chunks decoded: experts 1, 2 and 9 take the chunks that hold them, once each, fewer than the full unpack's."""
    import torch

    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "1")
    x = _make("float32", 16 * 40 * 256, 41, (16, 40, 256))
    p = bzip3_amd.pack_tensor(x, 65 << 10, planes=4)
    e, chunks = 40 * 1024, -(-p.nbytes // p.block_size)
    needed = len({c for i in (1, 2, 9) for c in range(i * e // p.block_size, ((i + 1) * e - 1) // p.block_size + 1)})
    assert needed < chunks
    gpu_lib.bz3_hip_debug_cm_launches(1)
    y = bzip3_amd.unpack_tensor_index(p, 0, [1, 2, 9])
    assert gpu_lib.bz3_hip_debug_cm_launches(1) == needed
    assert torch.equal(y, x[[1, 2, 9]])


def test_decompress_tensors_select(gpu_lib):
    import torch

    x = _make("float32", 300_001, 21).view(torch.uint8).flatten()
    frame = bzip3_amd.compress_tensor(x, 65 << 10, planes=4)

    def want(offset, stride, count, pieces):
        per = torch.cat([torch.arange(a, a + l) for a, l in pieces]) if pieces else torch.zeros(0, dtype=torch.int64)
        idx = (torch.arange(count).unsqueeze(1) * stride + per.unsqueeze(0) + offset).flatten()
        return x[idx[idx < x.numel()].to(x.device)]

    for q in ((0, 70_000, 10, [(0, 4000), (4100, 64), (66_000, 3000)]), (70_001, 50, 999, [(0, 3), (4, 1), (30, 17)]), (x.numel() - 500, 300, 5, [(0, 100), (150, 8)]),
              (123_456, 1, 1, [(0, 100_000), (100_001, 50_000)]), (5, 9, 3, [])):
        assert torch.equal(bzip3_amd.decompress_tensor_select(frame, *q, planes=4), want(*q)), q
    a, b = (5, 100, 7, [(0, 10), (20, 5)]), (66_560, 1000, 300, [(0, 64), (128, 64), (900, 100)])
    gots = bzip3_amd.decompress_tensors_select([frame, frame], *zip(a, b), planes=4)
    assert torch.equal(gots[0], want(*a)) and torch.equal(gots[1], want(*b))
    out = torch.zeros(105, dtype=torch.uint8, device=x.device)
    got = bzip3_amd.decompress_tensor_select(frame, *a, out=out, planes=4)
    assert torch.equal(got, want(*a)) and got.data_ptr() == out.data_ptr()
    with pytest.raises(ValueError):
        bzip3_amd.decompress_tensor_select(frame, *a, out=out[:45], planes=4)  # an `out` smaller than the set, as in decompress_tensors_range
    bad = frame.clone()
    bad[13 + 8 + 40] ^= 0x40
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.decompress_tensors_select([frame, bad], [0, 10], [100, 100], [9, 9], [[(0, 4), (8, 4)], [(0, 4), (8, 4)]], planes=4)
    assert e.value.index == 1 and e.value.codes[0] == 0 and torch.equal(e.value.outs[0], want(0, 100, 9, [(0, 4), (8, 4)])) and e.value.outs[1].numel() == 0
    assert bzip3_amd.decompress_tensors_select([], [], [], [], []) == []
    for q in ((0, 100, 2, [(0, 10), (5, 10)]), (0, 14, 2, [(0, 10), (12, 3)]), (-1, 100, 2, [(0, 1)]), (0, 100, 2, [(0, -1)]), (2 ** 64 - 5, 20, 1, [(0, 2), (4, 2)])):
        with pytest.raises(ValueError):
            bzip3_amd.decompress_tensor_select(frame, *q)
    with pytest.raises(ValueError):
        bzip3_amd.decompress_tensors_select([frame], [0], [10], [1], [])


def test_unpack_state_dict_index(gpu_lib, monkeypatch):
    import torch

    sd = {"w": _make("float32", 64 * 1000, 1, (64, 1000)), "b": _make("bfloat16", 777, 2, (777,)), "ids": _make("int64", 40_000, 3, (200, 200)), "step": _make("int32", 1, 4, ()),
          "e": _make("float32", 0, 5, (0, 3)), "x": _make("float16", 8 * 30 * 100, 6, (8, 30, 100)), "r": _make("float32", 50 * 40, 7, (50, 40)), "s": _make("int8", 90 * 70, 8, (90, 70))}
    base = {"w": _make("float32", 64 * 1000, 8, (64, 1000)), "ids": _make("int64", 40_000, 9, (200, 200)), "x": _make("float16", 8 * 30 * 100, 10, (8, 30, 100))}
    packed = bzip3_amd.pack_state_dict(sd, 65 << 10, base=base)
    whole = bzip3_amd.unpack_state_dict(packed, base=base, verify=True)
    index = {"w": (0, [0, 3, 4, 5, 63]), "ids": (-1, np.array([1, 2, 199])), "b": (0, torch.tensor([776, 0, 0, 5], device=sd["b"].device)), "e": (0, [])}
    slices = {"x": (1, 10, 20)}
    rows = {"r": (10, 20)}
    calls = []
    real = gpu_lib.bz3_hip_decompress_device_select_many

    def counting(*a):
        calls.append(a[0])
        return real(*a)

    monkeypatch.setattr(gpu_lib, "bz3_hip_decompress_device_select_many", counting)
    got = bzip3_amd.unpack_state_dict(packed, base=base, index=index, slices=slices, rows=rows, lib=gpu_lib)
    assert calls == [len(sd)], "all tensors go through one _select_many call"
    assert list(got) == list(sd)
    for name, y in got.items():
        want = whole[name]
        assert torch.equal(want, sd[name])
        if name in index:
            d, idx = index[name]
            want = want.index_select(d, torch.as_tensor(idx, dtype=torch.int64).to(want.device))
        elif name in slices:
            d, a, z = slices[name]
            want = want.narrow(d, a, z - a)
        elif name in rows:
            want = want[slice(*rows[name])]
        assert y.dtype == want.dtype and y.shape == want.shape and y.is_contiguous() and torch.equal(y, want), name
    for kw in ({"inplace": True}, {"verify": True}, {"rows": {"w": (0, 1)}}, {"slices": {"ids": (0, 0, 1)}}):  # a name given twice raises
        with pytest.raises(ValueError):
            bzip3_amd.unpack_state_dict(packed, base=base, index=index, **kw)
    for bad in ({"w": (2, [0])}, {"w": (1, [1000])}, {"w": (0, [3, 1])}, {"step": (0, [0])}, {"nope": (0, [0])}):  # ("w" has a base: its index must increase)
        with pytest.raises(ValueError):
            bzip3_amd.unpack_state_dict(packed, base=base, index=bad)
    with pytest.raises(ValueError):
        bzip3_amd.unpack_state_dict(packed, index=index)  # delta tensors without their bases
    wrong = dict(base)
    wrong["x"] = base["x"] + 1  # another base: caught by its checksum, whole, though the tensor is read in part
    with pytest.raises(ValueError):
        bzip3_amd.unpack_state_dict(packed, base=wrong, index=index)
    bzip3_amd.unpack_state_dict(packed, base=wrong, index=index, check_base=False)  # (other bytes, no error: the caller vouches)


# ---- every request form in one call ---------------------------------------------------------------------------------------------
def test_one_call_holds_every_request_form_on_the_gpu(gpu_lib, monkeypatch):
    """test_frame_select_emu.test_one_call_holds_every_request_form on the device: five frames of element size 4 (a block of 65 KiB and a short
    one), two of them with a base, in one bz3_hip_decompress_device_select_many call: a one-run range, the whole tensor, a two-run strided request, a
    two-piece select request and a select request cut to w <= l_0, at windows of two chunks and of eight (all six chunks in one launch).
    The oracle is unpack_tensor's result indexed with torch."""
    import torch

    bs, numel = 65 << 10, (65 << 10) // 4 + 1500
    x, y, base = (_make("float32", numel, seed) for seed in (51, 52, 53))
    px, py = bzip3_amd.pack_tensor(x, bs, planes=4), bzip3_amd.pack_tensor(y, bs, planes=4, base=base)
    assert px.block_size == py.block_size == bs and py.delta
    full = [bzip3_amd.unpack_tensor(px).view(torch.uint8).flatten(), bzip3_amd.unpack_tensor(py, base=base).view(torch.uint8).flatten()]
    assert _raw(full[0]) == _raw(x) and _raw(full[1]) == _raw(y)
    base_raw = base.view(torch.uint8).flatten()
    T = 4 * numel
    # (tensor, (offset, stride, count), pieces, the bytes asked for)
    plan = [(1, (bs + 10, 0, 1), [(0, 777)], 777), (0, (0, 0, 1), [(0, T)], T), (0, (bs + 5, 1000, 2), [(3, 401)], 802), (1, (bs + 100, 2000, 2), [(0, 300), (650, 130)], 860),
            (0, (bs + 9, 900, 3), [(4, 500), (600, 100)], 333)]

    def phi(offset, stride, count, pieces, w):
        per = torch.cat([torch.arange(a, a + l) for a, l in pieces])
        return (torch.arange(count).unsqueeze(1) * stride + per.unsqueeze(0) + offset).flatten()[:w].to(x.device)

    idx = [phi(*p, l, w) for _, p, l, w in plan]
    n = len(plan)
    frames = [(px, py)[t].frame for t, *_ in plan]
    base_ts = [base_raw[i] if t else None for (t, *_), i in zip(plan, idx)]
    vp = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    arrs = [_pieces_arg(l) for _, _, l, _ in plan]
    for window in ("2", "8"):
        monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", window)
        outs = [torch.full((w + 8,), 0xA5, dtype=torch.uint8, device=x.device) for *_, w in plan]
        out_sizes, rcs = (C.c_size_t * n)(*[w for *_, w in plan]), (C.c_int * n)(*([77] * n))  # (the last frame's *out_size cuts its request to w <= l_0)
        torch.cuda.synchronize()
        rc = gpu_lib.bz3_hip_decompress_device_select_many(n, (C.c_uint32 * n)(*([4] * n)), vp(frames), (C.c_size_t * n)(*[f.numel() for f in frames]),
                                                           (C.c_uint64 * (4 * n))(*[v for _, p, l, _ in plan for v in (*p, len(l))]),
                                                           (C.POINTER(C.c_uint64) * n)(*[C.cast(a, C.POINTER(C.c_uint64)) for a in arrs]), vp(base_ts),
                                                           (C.c_size_t * n)(*[0 if b is None else b.numel() for b in base_ts]), vp(outs), out_sizes, rcs)
        assert rc == 0 and list(rcs) == [0] * n
        for i, ((t, p, l, w), o) in enumerate(zip(plan, outs)):
            assert out_sizes[i] == w and torch.equal(o[:w], full[t][idx[i]]), (window, i)
            assert bool((o[w:] == 0xA5).all()), ("wrote beyond the request", window, i)


def test_unpack_state_dict_takes_the_narrowest_call(gpu_lib, monkeypatch):
    """rows= alone goes through bz3_hip_decompress_device_range_many, slices= + rows= through _strided_many, index= + slices= + rows= through
    _select_many, one call each, on a dict of an (8, 1024) tensor packed against a base, a (4, 64, 256) tensor and a 0-d one; the error of a
    truncated frame read by rows names the range call."""
    import torch

    sd = {"a": _make("float32", 8 * 1024, 61, (8, 1024)), "b": _make("float32", 4 * 64 * 256, 62, (4, 64, 256)), "step": _make("int32", 1, 63, ())}
    base = {"a": _make("float32", 8 * 1024, 64, (8, 1024))}
    packed = bzip3_amd.pack_state_dict(sd, 65 << 10, base=base)
    assert packed["a"].delta and not packed["b"].delta
    calls = []
    for name in ("range", "strided", "select"):
        entry = f"bz3_hip_decompress_device_{name}_many"
        monkeypatch.setattr(gpu_lib, entry, (lambda real, name: lambda *a: calls.append(name) or real(*a))(getattr(gpu_lib, entry), name))
    sel = lambda t, dim, idx: t.index_select(dim, torch.tensor(idx, dtype=torch.int64, device=t.device))  # noqa: E731
    for kw, via, want in (({"rows": {"a": (2, 5)}}, "range", {"a": sd["a"][2:5], "b": sd["b"], "step": sd["step"]}),
                          ({"slices": {"b": (1, 10, 20)}, "rows": {"a": (2, 5)}}, "strided", {"a": sd["a"][2:5], "b": sd["b"][:, 10:20], "step": sd["step"]}),
                          ({"index": {"b": (2, [1, 5, 6, 200])}, "slices": {}, "rows": {"a": (0, 8)}}, "select", {"a": sd["a"], "b": sel(sd["b"], 2, [1, 5, 6, 200]), "step": sd["step"]}),
                          ({"index": {"a": (1, [0, 7, 1023])}, "slices": {"b": (0, 1, 3)}, "rows": {}}, "select", {"a": sel(sd["a"], 1, [0, 7, 1023]), "b": sd["b"][1:3], "step": sd["step"]})):
        del calls[:]
        got = bzip3_amd.unpack_state_dict(packed, base=base, lib=gpu_lib, **kw)
        assert calls == [via], (kw, calls)
        assert list(got) == list(sd)
        for k, w in want.items():
            assert got[k].dtype == w.dtype and got[k].shape == w.shape and got[k].is_contiguous() and torch.equal(got[k], w), (via, k)
    p = packed["b"]
    short = dict(packed, b=bzip3_amd.PackedTensor(p.frame[: p.frame.numel() // 2], p.dtype, p.shape, p.planes, p.block_size, p.nbytes))
    with pytest.raises(bzip3_amd.Bz3Error, match="bz3_hip_decompress_device_range_many"):
        bzip3_amd.unpack_state_dict(short, base=base, rows={"b": (2, 4)}, lib=gpu_lib)
