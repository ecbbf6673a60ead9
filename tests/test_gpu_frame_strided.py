"""-m gpu: the strided range calls on a real device (include/bz3_hip.h bz3_hip_decompress_device_strided[_many], the strided merge of
bzip3_amd/csrc/planes.hpp, the walk with a period of frame.hpp; bzip3_amd's decompress_tensor[s]_strided, unpack_tensor_slice and
unpack_state_dict(slices=...)).  The oracle of a request is full[phi(t)], `full` from the real reference, numpy merge_k per chunk and
numpy D_inv (test_frame_range_emu.Case), never from the library under test; the oracle of a typed slice is torch's narrow of the
tensor that was packed."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
from oracle_lib import require_ref
from test_frame_delta_emu import _r16
from test_frame_range_emu import GUARD, INIT, MALFORMED, Case, _flip, _with_header, stream_for
from test_frame_strided_emu import (committed_below, fit, frame_requests, in_place_strided_case, mixed_spec_strided, slice_base, strided_case, sweep_specs_strided, want_strided)
from test_gpu_frame_delta import _gpu_alloc
from test_gpu_frame_planes import DTYPES, _host, _make, _raw
from test_gpu_frame_range import _dev, gpu_range_call

pytestmark = pytest.mark.gpu
MiB = 1 << 20
KiB65 = 65 << 10
SWEEP_COUNTS = (0, 1, 17, 4079, 4080, 4081, 8160, 8161)  # the emulator suite's sweep at the tile edges and the smallest counts


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_strided_kernel_sweep_on_the_gpu(gpu_lib, k, has_base):
    """The emulator suite's sweep on device memory: every run, stride, first and end at the tile-edge counts and every tail length
    0..k-1, then the three alignments."""
    rng = np.random.default_rng(81 + 10 * k + has_base)
    for spec in sweep_specs_strided(rng, k, has_base, counts=SWEEP_COUNTS):
        strided_case(gpu_lib.bz3_hip_debug_strided, rng, spec, _gpu_alloc)


def test_strided_kernel_large_mixed_and_in_place_on_the_gpu(gpu_lib):
    """Four chunks of 1 - 9 MiB per k with runs of kilobytes, the mixed launch and the in-place launch, on device memory."""
    rng = np.random.default_rng(82)
    call = gpu_lib.bz3_hip_debug_strided
    for k in (1, 2, 4, 8):
        big = []
        for i in range(4):
            elems, tail = int(rng.integers(MiB, 9 * MiB)) // k, int(rng.integers(0, k))
            run = k * int(rng.integers(16, 4096)) + (i == 3)
            stride, first = run + k * int(rng.integers(1, 9000)) + (i == 2), int(rng.integers(1, run + 1))
            c0, nbytes = fit(k * int(rng.integers(0, 5000)), first, run, stride, elems * k + tail - 1 - int(rng.integers(0, 3)))
            big.append((_r16(rng), _r16(rng), _r16(rng), elems, tail, k, i % 2, c0, first, run, stride, nbytes))
        strided_case(call, rng, big, _gpu_alloc)
    strided_case(call, rng, mixed_spec_strided(rng), _gpu_alloc)
    in_place_strided_case(call, rng, _gpu_alloc)
    in_place_strided_case(call, rng, _gpu_alloc, sizes=(3 * MiB + 5, 1_000_003))


# ---- frames -------------------------------------------------------------------------------------------------------------------
def gpu_strided_call(lib, k, frame_t, offset, run, stride, count, cap, base=None, in_place=False):
    """(rc, *out_size, out[0, w + GUARD) after the call, before it).  base: the base's bytes of the slice (host bytes)."""
    import torch

    room = min(cap, count * run) + GUARD
    before = (bytes(base) + b"\xa5" * room)[:room] if in_place else b"\xa5" * room
    out = _dev(before)
    b = out if in_place else None if base is None else _dev(base)
    osz = C.c_size_t(cap)
    torch.cuda.synchronize()
    rc = lib.bz3_hip_decompress_device_strided(k, frame_t.data_ptr(), frame_t.numel(), offset, run, stride, count, None if b is None else b.data_ptr(),
                                               0 if base is None else room - GUARD if in_place else len(base), out.data_ptr(), C.byref(osz))
    return rc, osz.value, _host(out)[:room], before


def gpu_check_strided(lib, case, frame_t, offset, run, stride, count, cap=None, in_place=False):
    cap = count * run if cap is None else cap
    base = slice_base(case, offset, run, stride, count, cap)
    rc, r, got, before = gpu_strided_call(lib, case.k, frame_t, offset, run, stride, count, cap, base, in_place and base is not None)
    want = want_strided(case, offset, run, stride, count, cap)
    assert (rc, r) == (0, len(want)), (offset, run, stride, count, cap, rc, r, len(want))
    assert got[:r] == want, ("bytes differ", offset, run, stride, count, cap)
    assert got[r:] == before[r:], ("wrote beyond the slice", offset, run, stride, count, cap)


CASES = [(k, wb, bs) for bs in (KiB65, KiB65 + 3) for k in (1, 2, 4, 8) for wb in (0, 1)]


@pytest.mark.parametrize("k,with_base,bs", CASES, ids=[f"k{k}-{'base' if wb else 'plain'}-{bs}" for k, wb, bs in CASES])
def test_strided_requests_of_a_frame_match_the_reference(gpu_lib, k, with_base, bs, monkeypatch):
    """Four full blocks of 65 KiB (65 KiB + 3) and a short one, windows of two chunks: the emulator suite's requests, and on the full chunks
    runs in every chunk with one and with no chunk in the gaps, in place where there is a base."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    case = Case(require_ref().lib, bs, k, with_base, stream_for(bs, blocks=4))
    assert len(case.sizes) == 5 and case.sizes[:4] == [bs] * 4
    frame_t = _dev(case.frame)
    for offset, run, stride, count, cap in frame_requests(case):
        gpu_check_strided(gpu_lib, case, frame_t, offset, run, stride, count, cap)
    gpu_check_strided(gpu_lib, case, frame_t, 10, 100, 2 * bs, 3, in_place=True)
    gpu_check_strided(gpu_lib, case, frame_t, bs - 30, 4096, 20000, 13, in_place=True)


def test_equivalence_refusals_and_skipping(gpu_lib, monkeypatch):
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    ref = require_ref().lib
    bs = KiB65 + 3
    case = Case(ref, bs, 4, 1, stream_for(bs, blocks=4))
    s = case.starts
    # count == 1 and stride == run are the range call: bytes, rc, *out_size
    for frame in (case.frame, _flip(case.frame, 2)):
        frame_t = _dev(frame)
        for offset, run, stride, count, cap in ((s[1] - 50, 2 * bs + 100, 7, 1, 10 ** 9), (s[1] - 48, 1000, 1000, 140, 100_001), (case.T - 10, 8, 8, 4, 64)):
            w = min(cap, count * run)
            base = (case.base[offset : offset + w] + bytes(w))[:w]
            assert gpu_strided_call(gpu_lib, 4, frame_t, offset, run, stride, count, w, base) == gpu_range_call(gpu_lib, 4, frame_t, offset, w, base)
    # invalid periods, before any write
    frame_t = _dev(case.frame)
    for offset, run, stride, count in ((0, 10, 9, 2), (0, 2 ** 33, 2 ** 33, 2 ** 31), (2 ** 64 - 51, 10, 20, 4)):
        out = _dev(b"\xa5" * 64)
        osz = C.c_size_t(64)
        assert gpu_lib.bz3_hip_decompress_device_strided(4, frame_t.data_ptr(), frame_t.numel(), offset, run, stride, count, None, 0, out.data_ptr(), C.byref(osz)) == INIT
        assert osz.value == 0 and _host(out) == b"\xa5" * 64
    arena = _dev(slice_base(case, 0, 100, 300, 10, 1000) + b"\xa5" * 3000)  # a partial overlap of out and base
    before = _host(arena)
    osz = C.c_size_t(4000)
    assert gpu_lib.bz3_hip_decompress_device_strided(4, frame_t.data_ptr(), frame_t.numel(), 0, 100, 300, 10, arena.data_ptr(), 4000, arena.data_ptr() + 16, C.byref(osz)) == INIT
    assert _host(arena) == before
    # chunks 0, 2 and 4 are needed, chunks 1 and 3 lie in the gaps
    offset, run, stride, count = 100, bs // 2, 2 * bs, 3
    w = count * run
    base = slice_base(case, offset, run, stride, count, w)
    good = want_strided(case, offset, run, stride, count, w)
    for j in range(5):
        rc, r, got, before = gpu_strided_call(gpu_lib, 4, _dev(_flip(case.frame, j)), offset, run, stride, count, w, base)
        if j % 2:
            assert (rc, r) == (0, len(good)) and got[:r] == good, ("a corrupt payload in a gap was noticed", j)
        else:
            assert rc != 0 and r == committed_below(offset, run, stride, w, s[j]) == (j // 2) * run and got[:r] == good[:r], (j, rc, r)
        assert got[r:] == before[r:], j
        rc, r, got, before = gpu_strided_call(gpu_lib, 4, _dev(_with_header(case.frame, j, orig=-5)), offset, run, stride, count, w, base)
        assert rc == MALFORMED and r == ((j + 1) // 2) * run and got[:r] == good[:r] and got[r:] == before[r:], (j, rc, r)


def test_strided_calls_launch_the_cm_stage_for_the_needed_chunks_only(gpu_lib, monkeypatch):
    """Five chunks, windows of two: runs in chunks 0, 2 and 4 take ceil(3 / 2) = 2 CM launches, the full decode ceil(5 / 2) = 3."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    case = Case(require_ref().lib, KiB65, 1, 0, stream_for(KiB65, blocks=4))
    frame_t = _dev(case.frame)
    gpu_lib.bz3_hip_debug_cm_launches(1)
    gpu_check_strided(gpu_lib, case, frame_t, 10, 100, 2 * KiB65, 3)
    assert gpu_lib.bz3_hip_debug_cm_launches(1) == 2
    gpu_check_strided(gpu_lib, case, frame_t, 0, case.T, case.T, 1)
    assert gpu_lib.bz3_hip_debug_cm_launches(1) == 3


def test_many_strided_requests_equal_their_single_calls(gpu_lib, monkeypatch):
    import torch

    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    ref = require_ref().lib
    bs = KiB65 + 3
    cases = [Case(ref, bs, k, wb, stream_for(bs, blocks=nb, last=last), seed=190 + i) for i, (k, wb, nb, last) in enumerate(((2, 1, 2, 777), (1, 0, 1, 50), (8, 1, 4, 1234), (4, 0, 0, 100)))]
    plan = [(0, (bs - 30, 60, 500, 9), 10 ** 6), (1, (0, 10, 10, 10 ** 5), 10 ** 6), (2, (10, 5000, 2 * bs, 3), 10 ** 6), (2, (bs + 7, 64, 1024, 200), 64 * 200 - 9),
            (3, (7, 5, 11, 30), 10 ** 6), (0, (5, 0, 9, 9), 50), (2, (3 * bs - 8, 16, 17, 4000), 10 ** 6)]
    n = len(plan)
    frame_ts = [_dev(cases[c].frame) for c, *_ in plan]
    ks = [cases[c].k for c, *_ in plan]
    ws = [min(cap, p[1] * p[3]) for _, p, cap in plan]
    bases = [slice_base(cases[c], *p, cap) for c, p, cap in plan]
    outs = [_dev(b"\xa5" * (w + GUARD)) for w in ws]
    base_ts = [None if b is None else _dev(b) for b in bases]
    out_sizes, rcs = (C.c_size_t * n)(*[cap for *_, cap in plan]), (C.c_int * n)(*([77] * n))
    vp = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    torch.cuda.synchronize()
    rc = gpu_lib.bz3_hip_decompress_device_strided_many(n, (C.c_uint32 * n)(*ks), vp(frame_ts), (C.c_size_t * n)(*[f.numel() for f in frame_ts]),
                                                        (C.c_uint64 * (4 * n))(*[v for _, p, _ in plan for v in p]), vp(base_ts),
                                                        (C.c_size_t * n)(*[0 if b is None else len(b) for b in bases]), vp(outs), out_sizes, rcs)
    assert rc == 0
    for i, (c, p, cap) in enumerate(plan):
        want = want_strided(cases[c], *p, cap)
        assert (rcs[i], out_sizes[i]) == (0, len(want)) and _host(outs[i]) == want + b"\xa5" * (ws[i] + GUARD - len(want)), i
        assert gpu_strided_call(gpu_lib, ks[i], frame_ts[i], *p, cap, bases[i])[:3] == (0, len(want), _host(outs[i])), ("single call", i)


# ---- python ---------------------------------------------------------------------------------------------------------------------
SHAPE = (6, 25, 501)  # about 300 KB of float32: five blocks at the 65 KiB floor, so that slices cross chunks
SLICES = ((0, 2), (2, 5), (4, 6), (3, 3))  # the two ends, interior, empty (scaled to the dimension below)


def _scaled(dim, start, stop):
    f = SHAPE[dim] // 6
    return start * f, (stop * f if stop < 6 else SHAPE[dim])


@pytest.mark.parametrize("dtype", DTYPES)
def test_unpack_tensor_slice(gpu_lib, dtype):
    import torch

    numel = SHAPE[0] * SHAPE[1] * SHAPE[2]
    x = _make(dtype, numel, 31, SHAPE)
    base = _make(dtype, numel, 32, SHAPE)
    for b in (None, base):
        p = bzip3_amd.pack_tensor(x, 65 << 10, base=b)
        assert p.delta == (b is not None)
        for dim in (0, 1, 2, -2):
            for a, z in SLICES:
                start, stop = _scaled(dim % 3, a, z)
                want = x.narrow(dim, start, stop - start)
                y = bzip3_amd.unpack_tensor_slice(p, dim, start, stop, base=None if b is None else b.narrow(dim, start, stop - start))
                assert y.dtype == x.dtype and y.shape == want.shape and y.is_contiguous() and torch.equal(y, want) and _raw(y) == _raw(want), (dtype, dim, start, stop)
        for dim, start, stop in ((1, 3, 11), (2, 100, 164)):
            want = x.narrow(dim, start, stop - start)
            out = torch.empty_like(want, memory_format=torch.contiguous_format)
            assert bzip3_amd.unpack_tensor_slice(p, dim, start, stop, out=out, base=None if b is None else b.narrow(dim, start, stop - start)) is out and torch.equal(out, want)
            if b is not None:
                over = b.narrow(dim, start, stop - start).contiguous()
                assert bzip3_amd.unpack_tensor_slice(p, dim, start, stop, out=over, base=over) is over and torch.equal(over, want)
        assert torch.equal(bzip3_amd.unpack_tensor_slice(p, 0, 1, 4, base=None if b is None else b[1:4]), bzip3_amd.unpack_tensor_rows(p, 1, 4, base=None if b is None else b[1:4]))
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor_slice(p, 1, 3, 11)  # a delta tensor without its base
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor_slice(p, 1, 3, 11, base=base)  # the whole base is not the slice of the base
    plain = bzip3_amd.pack_tensor(x, 65 << 10)
    for dim, start, stop in ((3, 0, 1), (-4, 0, 1), (1, -1, 3), (1, 3, 2), (1, 0, 26), (2, 0, 502)):
        with pytest.raises(ValueError):
            bzip3_amd.unpack_tensor_slice(plain, dim, start, stop)
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor_slice(bzip3_amd.pack_tensor(x[0, 0, 0], 65 << 10), 0, 0, 0)  # 0-d
    with pytest.raises(TypeError):
        bzip3_amd.unpack_tensor_slice(plain, 1, 3, 11, out=torch.empty_like(x))
    short = bzip3_amd.PackedTensor(plain.frame[: plain.frame.numel() // 2], plain.dtype, plain.shape, plain.planes, plain.block_size, plain.nbytes)
    with pytest.raises(bzip3_amd.Bz3Error):
        bzip3_amd.unpack_tensor_slice(short, 1, 20, 25)


def test_a_middle_slice_with_a_wide_stride_decodes_fewer_chunks(gpu_lib, monkeypatch):
    """(4, 40, 1024) float32 at 65 KiB blocks: dimension 1 has a stride of 160 KiB, more than two blocks; rows [0, 4) of it are four runs of
    16 KiB.  With windows of one chunk the CM launches count the chunks decoded: fewer than the full unpack's."""
    import torch

    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "1")
    x = _make("float32", 4 * 40 * 1024, 41, (4, 40, 1024))
    p = bzip3_amd.pack_tensor(x, 65 << 10, planes=4)
    chunks = -(-p.nbytes // p.block_size)
    runs = [(i * 40 * 4096, i * 40 * 4096 + 4 * 4096) for i in range(4)]
    needed = len({c for a, z in runs for c in range(a // p.block_size, (z - 1) // p.block_size + 1)})
    assert needed < chunks
    gpu_lib.bz3_hip_debug_cm_launches(1)
    y = bzip3_amd.unpack_tensor_slice(p, 1, 0, 4)
    assert gpu_lib.bz3_hip_debug_cm_launches(1) == needed
    assert torch.equal(y, x[:, 0:4])
    assert torch.equal(bzip3_amd.unpack_tensor(p), x)
    assert gpu_lib.bz3_hip_debug_cm_launches(1) == chunks


def test_decompress_tensors_strided(gpu_lib):
    import torch

    x = _make("float32", 300_001, 21).view(torch.uint8).flatten()
    frame = bzip3_amd.compress_tensor(x, 65 << 10, planes=4)

    def want(offset, run, stride, count):
        idx = (torch.arange(count).unsqueeze(1) * stride + torch.arange(run).unsqueeze(0) + offset).flatten()
        return x[idx[idx < x.numel()].to(x.device)]

    for q in ((0, 4000, 70_000, 10), (70_001, 3, 5, 999), (x.numel() - 500, 100, 300, 5), (123_456, 200_000, 1, 1)):
        assert torch.equal(bzip3_amd.decompress_tensor_strided(frame, *q, planes=4), want(*q)), q
    gots = bzip3_amd.decompress_tensors_strided([frame, frame], [5, 66_560], [10, 64], [100, 1000], [7, 300], planes=4)
    assert torch.equal(gots[0], want(5, 10, 100, 7)) and torch.equal(gots[1], want(66_560, 64, 1000, 300))
    out = torch.zeros(70, dtype=torch.uint8, device=x.device)
    assert torch.equal(bzip3_amd.decompress_tensor_strided(frame, 5, 10, 100, 7, out=out, planes=4), want(5, 10, 100, 7)) and out.data_ptr() == bzip3_amd.decompress_tensor_strided(frame, 5, 10, 100, 7, out=out, planes=4).data_ptr()
    with pytest.raises(ValueError):
        bzip3_amd.decompress_tensor_strided(frame, 5, 10, 100, 7, out=out[:45], planes=4)  # an `out` smaller than the set, as in decompress_tensors_range
    bad = frame.clone()
    bad[13 + 8 + 40] ^= 0x40
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.decompress_tensors_strided([frame, bad], [0, 10], [10, 10], [100, 100], [9, 9], planes=4)
    assert e.value.index == 1 and e.value.codes[0] == 0 and torch.equal(e.value.outs[0], want(0, 10, 100, 9)) and e.value.outs[1].numel() == 0
    assert bzip3_amd.decompress_tensors_strided([], [], [], [], []) == []
    for q in ((0, 10, 9, 2), (-1, 10, 20, 2), (2 ** 64 - 5, 10, 20, 1)):
        with pytest.raises(ValueError):
            bzip3_amd.decompress_tensor_strided(frame, *q)


def test_unpack_state_dict_slices(gpu_lib, monkeypatch):
    import torch

    sd = {"w": _make("float32", 64 * 1000, 1, (64, 1000)), "b": _make("bfloat16", 777, 2, (777,)), "ids": _make("int64", 40_000, 3, (200, 200)), "step": _make("int32", 1, 4, ()),
          "e": _make("float32", 0, 5, (0, 3)), "x": _make("float16", 8 * 30 * 100, 6, (8, 30, 100)), "r": _make("float32", 50 * 40, 7, (50, 40))}
    base = {"w": _make("float32", 64 * 1000, 8, (64, 1000)), "ids": _make("int64", 40_000, 9, (200, 200)), "x": _make("float16", 8 * 30 * 100, 10, (8, 30, 100))}
    packed = bzip3_amd.pack_state_dict(sd, 65 << 10, base=base)
    whole = bzip3_amd.unpack_state_dict(packed, base=base)
    slices = {"w": (1, 250, 500), "ids": (-1, 199, 200), "b": (0, 0, 0), "x": (1, 10, 20), "e": (1, 1, 3)}
    rows = {"r": (10, 20)}
    calls = []
    real = gpu_lib.bz3_hip_decompress_device_strided_many

    def counting(*a):
        calls.append(a[0])
        return real(*a)

    monkeypatch.setattr(gpu_lib, "bz3_hip_decompress_device_strided_many", counting)
    got = bzip3_amd.unpack_state_dict(packed, base=base, slices=slices, rows=rows, lib=gpu_lib)
    assert calls == [len(sd)], "all tensors go through one _strided_many call"
    assert list(got) == list(sd)
    for name, y in got.items():
        want = whole[name]
        if name in slices:
            d, a, z = slices[name]
            want = want.narrow(d, a, z - a)
        elif name in rows:
            want = want[slice(*rows[name])]
        assert torch.equal(whole[name], sd[name])
        assert y.dtype == want.dtype and y.shape == want.shape and y.is_contiguous() and torch.equal(y, want), name
    for kw in ({"inplace": True}, {"verify": True}, {"rows": {"w": (0, 1)}}):
        with pytest.raises(ValueError):
            bzip3_amd.unpack_state_dict(packed, base=base, slices=slices, **kw)
    for bad in ({"w": (2, 0, 1)}, {"w": (1, 3, 1001)}, {"step": (0, 0, 1)}, {"nope": (0, 0, 1)}):
        with pytest.raises(ValueError):
            bzip3_amd.unpack_state_dict(packed, base=base, slices=bad)
    with pytest.raises(ValueError):
        bzip3_amd.unpack_state_dict(packed, slices=slices)  # delta tensors without their bases
    r = packed["r"]  # a tensor that comes back whole must be all its frame decodes to, as in unpack_tensor
    longer = dict(packed, r=bzip3_amd.PackedTensor(r.frame, r.dtype, (49, 40), r.planes, r.block_size, r.nbytes - 160, crc=None))
    for call in (lambda: bzip3_amd.unpack_tensor(longer["r"]), lambda: bzip3_amd.unpack_state_dict(longer, base=base, slices=slices)):
        with pytest.raises(bzip3_amd.Bz3Error) as e:
            call()
        assert e.value.code == bzip3_amd.BZ3_ERR_DATA_TOO_BIG
    wrong = dict(base)
    wrong["x"] = base["x"] + 1  # another base: caught by its checksum, whole, though the tensor is read by a slice
    with pytest.raises(ValueError):
        bzip3_amd.unpack_state_dict(packed, base=wrong, slices=slices)
    bzip3_amd.unpack_state_dict(packed, base=wrong, slices=slices, check_base=False)  # (other bytes, no error: the caller vouches)
