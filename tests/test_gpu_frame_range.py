"""-m gpu: the range calls on a real device (include/bz3_hip.h bz3_hip_decompress_device_range[_many], the clipped merge of
bzip3_amd/csrc/planes.hpp, the skipping walk of frame.hpp; bzip3_amd's decompress_tensor[s]_range, unpack_tensor_rows and
unpack_state_dict(rows=...)).  The oracle of a range is full[offset : offset + w], `full` from the real reference, numpy merge_k per
chunk and numpy D_inv (test_frame_range_emu.Case), never from the library under test."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
import mutants
from oracle_lib import require_ref
from test_frame_delta_emu import _chunks, _r16, _with_chunk
from test_frame_range_emu import (GUARD, INIT, MALFORMED, TRUNCATED, U64, Case, _flip, _with_header, frame_ranges, in_place_range_case, mixed_spec_range, range_case, range_model,
                                  stream_for, sweep_specs_range, synthetic_frame)
from test_gpu_frame_delta import _gpu_alloc
from test_gpu_frame_planes import DTYPES, _host, _make, _raw

pytestmark = pytest.mark.gpu
MiB = 1 << 20
KiB65 = 65 << 10


def _dev(b):
    import torch

    t = torch.from_numpy(np.frombuffer(bytes(b) if len(b) else b"\0", dtype=np.uint8).copy()).to("cuda:0")
    return t


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_range_kernel_sweep_on_the_gpu(gpu_lib, k, has_base):
    """The emulator suite's sweep on device memory: every clip pair at every count and every tail length 0..k-1, the three alignments."""
    rng = np.random.default_rng(61 + 10 * k + has_base)
    for spec in sweep_specs_range(rng, k, has_base):
        range_case(gpu_lib.bz3_hip_debug_range, rng, spec, _gpu_alloc)


def test_range_kernel_large_mixed_and_in_place_on_the_gpu(gpu_lib):
    """Four segments of 1 - 9 MiB per k clipped at random interior bytes, the mixed launch and the in-place launch, on device memory."""
    rng = np.random.default_rng(61)
    call = gpu_lib.bz3_hip_debug_range
    for k in (1, 2, 4, 8):
        big = []
        for i in range(4):
            elems, tail = int(rng.integers(MiB, 9 * MiB)) // k, int(rng.integers(0, k))
            a, b = sorted(int(v) for v in rng.integers(1, elems * k + tail, size=2))
            big.append((_r16(rng), _r16(rng), _r16(rng), elems, tail, k, i % 2, a, b))
        range_case(call, rng, big, _gpu_alloc)
    range_case(call, rng, mixed_spec_range(rng), _gpu_alloc)
    in_place_range_case(call, rng, _gpu_alloc)
    in_place_range_case(call, rng, _gpu_alloc, sizes=(3 * MiB + 5, 1_000_003))


# ---- frames -------------------------------------------------------------------------------------------------------------------
def gpu_range_call(lib, k, frame_t, offset, w, base=None, in_place=False, cap=None):
    """(rc, *out_size, out[0, w + GUARD) after the call, before it).  base: the base's bytes of the range (host bytes)."""
    import torch

    room = w + GUARD
    before = (bytes(base) + b"\xa5" * room)[:room] if in_place else b"\xa5" * room
    out = _dev(before)
    b = out if in_place else None if base is None else _dev(base)
    osz = C.c_size_t(w if cap is None else cap)
    torch.cuda.synchronize()
    rc = lib.bz3_hip_decompress_device_range(k, frame_t.data_ptr(), frame_t.numel(), offset, None if b is None else b.data_ptr(),
                                             0 if base is None else cap if cap is not None else w if in_place else len(base), out.data_ptr(), C.byref(osz))
    return rc, osz.value, _host(out)[:room], before


def gpu_check_range(lib, case, frame_t, offset, w, in_place=False):
    base = None if case.base is None else (case.base[offset : offset + w] + bytes(w))[:w]
    rc, r, got, before = gpu_range_call(lib, case.k, frame_t, offset, w, base, in_place)
    want = case.want(offset, w)
    assert (rc, r) == (0, len(want)), (offset, w, rc, r)
    assert got[:r] == want, ("bytes differ", offset, w)
    assert got[r:] == before[r:], ("wrote beyond the range", offset, w)


CASES = [(k, wb, KiB65 + 7) for k in (1, 2, 4, 8) for wb in (0, 1)] + [(4, 1, MiB + 7)]


@pytest.mark.parametrize("k,with_base,bs", CASES, ids=[f"k{k}-{'base' if wb else 'plain'}-{bs}" for k, wb, bs in CASES])
def test_ranges_of_a_frame_match_the_reference(gpu_lib, k, with_base, bs, monkeypatch):
    """Five full blocks of 65 KiB + 7 (1 MiB + 7) and a short one, windows of two chunks: every block starts inside an element and has a
    tail.  The whole frame, w = 0, every chunk boundary, one byte, the end of the frame, a short read, an overflowing end."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    case = Case(require_ref().lib, bs, k, with_base, stream_for(bs))
    assert len(case.sizes) == 6 and case.sizes[:5] == [bs] * 5
    frame_t = _dev(case.frame)
    for offset, w in frame_ranges(case):
        if w == U64:  # (no buffer of that size: the capacity is a number to the call, which writes r bytes)
            # (with a base, in place: two separate buffers of 2^64 bytes each would overlap whatever their addresses)
            rc, r, got, before = gpu_range_call(gpu_lib, k, frame_t, offset, 40, case.base[offset:] if with_base else None, in_place=bool(with_base), cap=U64)
            assert (rc, r) == (0, case.T - offset) and got[:r] == case.full[offset:] and got[r:] == before[r:]
        else:
            gpu_check_range(gpu_lib, case, frame_t, offset, w)
    gpu_check_range(gpu_lib, case, frame_t, bs - 100, 2 * bs + 300, in_place=bool(with_base))


def test_partial_overlap_of_out_and_base_is_refused(gpu_lib):
    import torch

    case = Case(require_ref().lib, KiB65 + 7, 4, 1, stream_for(KiB65 + 7, blocks=1))
    frame_t = _dev(case.frame)
    arena = _dev(case.base[:1000] + b"\xa5" * 3000)
    before = _host(arena)
    for off in (1, 16, 999):
        osz = C.c_size_t(1000)
        assert gpu_lib.bz3_hip_decompress_device_range(4, frame_t.data_ptr(), frame_t.numel(), 0, arena.data_ptr(), 1000, arena.data_ptr() + off, C.byref(osz)) == INIT
        assert _host(arena) == before
    osz = C.c_size_t(1000)
    assert gpu_lib.bz3_hip_decompress_device_range(4, frame_t.data_ptr(), frame_t.numel(), 0, arena.data_ptr(), 1000, arena.data_ptr() + 1000, C.byref(osz)) == 0
    assert osz.value == 1000 and _host(arena)[1000:2000] == case.full[:1000] and _host(arena)[:1000] == case.base[:1000]


# ---- skipping is real -----------------------------------------------------------------------------------------------------------
def _gpu_full(lib, k, frame, base, room):
    import torch

    f, out = _dev(frame), _dev(b"\xa5" * room)
    b = None if base is None else _dev(base)
    osz = C.c_size_t(room)
    torch.cuda.synchronize()
    rc = lib.bz3_hip_decompress_device_delta(k, f.data_ptr(), None if b is None else b.data_ptr(), 0 if base is None else len(base), out.data_ptr(), f.numel(), C.byref(osz))
    return rc, osz.value


def test_corrupt_chunks_outside_and_inside_the_range(gpu_lib):
    ref = require_ref().lib
    bs = KiB65 + 7
    case = Case(ref, bs, 4, 1, stream_for(bs, blocks=3))
    s = case.starts
    offset, w = s[1] + 10, bs - 20  # inside chunk 1
    for j in (0, 2, 3):  # wholly before the range, wholly after it: the full call fails, the range call does not notice
        bad = _flip(case.frame, j)
        assert _gpu_full(gpu_lib, case.k, bad, case.base, case.T)[0] != 0
        rc, r, got, before = gpu_range_call(gpu_lib, case.k, _dev(bad), offset, w, case.base[offset : offset + w])
        assert (rc, r) == (0, w) and got[:w] == case.want(offset, w) and got[w:] == before[w:], j
    offset, w = s[1] - 50, 50 + bs + 70  # chunks 0 (clipped), 1 (whole), 2 (clipped)
    for j in (0, 1, 2):
        bad = _flip(case.frame, j)
        full_rc = _gpu_full(gpu_lib, case.k, bad, case.base, case.T)[0]
        rc, r, got, before = gpu_range_call(gpu_lib, case.k, _dev(bad), offset, w, case.base[offset : offset + w])
        want_r = max(0, min(s[j], offset + w) - offset)
        assert rc == full_rc != 0 and r == want_r, (j, rc, full_rc, r, want_r)
        assert got[:r] == case.want(offset, r) and got[r:] == before[r:], j


def test_header_mutants_before_inside_and_beyond_the_range(gpu_lib):
    ref = require_ref().lib
    bs = KiB65 + 7
    case = Case(ref, bs, 2, 0, stream_for(bs, blocks=3))
    s, frame = case.starts, case.frame
    offset, w = s[1] + 5, bs + 20  # chunks 1 and 2; chunk 0 lies before the range, chunk 3 beyond its end

    def check(bad, label):
        rc, r, got, before = gpu_range_call(gpu_lib, 2, _dev(bad), offset, w)
        want = range_model(ref, bad, 2, offset, w)
        assert (rc, got[:r]) == want, (label, rc, want[0], r, len(want[1]))
        assert got[r:] == before[r:], ("wrote beyond the committed bytes", label)
        return rc, r

    cut = len(frame) - 10
    for j in range(4):
        for label, bad in (("size<0", _with_header(frame, j, size=-1)), ("size>bs", _with_header(frame, j, size=bs + 1)), ("orig<0", _with_header(frame, j, orig=-5)),
                           ("truncated", _with_header(frame[:cut], j, size=bs))):
            rc, r = check(bad, (label, j))
            if j == 0:
                assert rc != 0 and r == 0, (label, j)
            elif j == 3:
                assert (rc, r) == (0, w), (label, j)
            else:
                assert rc in (MALFORMED, TRUNCATED) and r == max(0, s[j] - offset), (label, j, rc, r)
    blocks = _chunks(frame)
    for (blk, orig), it in zip(mutants.mutants([b for b, _ in blocks], [o for _, o in blocks], 20, seed=11), range(20)):
        j = it % 4
        if orig != blocks[j][1]:
            continue
        rc, r = check(_with_chunk(frame, j, blk, orig), ("mutant", it, j))
        if j in (0, 3):
            assert (rc, r) == (0, w), ("a chunk outside the range was noticed", it, j)


def _many(lib, ks, frame_ts, offsets, ws, base_ts=None):
    import torch

    n = len(frame_ts)
    outs = [_dev(b"\xa5" * (w + GUARD)) for w in ws]
    out_sizes, rcs = (C.c_size_t * n)(*ws), (C.c_int * n)(*([77] * n))
    vp = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    torch.cuda.synchronize()
    rc = lib.bz3_hip_decompress_device_range_many(n, None if ks is None else (C.c_uint32 * n)(*ks), vp(frame_ts), (C.c_size_t * n)(*[f.numel() for f in frame_ts]),
                                                  (C.c_uint64 * n)(*offsets), None if base_ts is None else vp(base_ts),
                                                  None if base_ts is None else (C.c_size_t * n)(*[0 if b is None else b.numel() for b in base_ts]), vp(outs), out_sizes, rcs)
    return rc, list(rcs), list(out_sizes), [_host(o) for o in outs]


def test_range_calls_launch_the_cm_stage_for_their_chunks_only(gpu_lib, monkeypatch):
    """Six frames of four chunks, windows of three, each range inside one chunk: two CM launches; the full decode takes eight."""
    import torch

    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    case = Case(require_ref().lib, KiB65, 1, 0, stream_for(KiB65, blocks=3))
    n = 6
    frame_ts = [_dev(case.frame) for _ in range(n)]
    offs = [case.starts[i % 4] + 100 + i for i in range(n)]
    ws = [500] * n
    gpu_lib.bz3_hip_debug_cm_launches(1)
    rc, rcs, sizes, outs = _many(gpu_lib, None, frame_ts, offs, ws)
    assert gpu_lib.bz3_hip_debug_cm_launches(1) == 2
    assert rc == 0 and rcs == [0] * n and sizes == ws
    assert all(outs[i] == case.want(offs[i], 500) + b"\xa5" * GUARD for i in range(n))
    backs = bzip3_amd.decompress_tensors(frame_ts)
    assert gpu_lib.bz3_hip_debug_cm_launches(1) == 8
    assert all(_host(b) == case.full for b in backs)


def test_five_thousand_empty_chunks_before_the_data(gpu_lib):
    """More skipped chunks than the walk has records, none of them decoded."""
    payload = stream_for(KiB65, blocks=0, last=3000)
    frame_t = _dev(synthetic_frame(require_ref().lib, 5000, payload))
    gpu_lib.bz3_hip_debug_cm_launches(1)
    rc, r, got, before = gpu_range_call(gpu_lib, 1, frame_t, 0, 3000)
    assert (rc, r) == (0, 3000) and got[:r] == payload and got[r:] == before[r:]
    assert gpu_lib.bz3_hip_debug_cm_launches(1) == 1


# ---- many -----------------------------------------------------------------------------------------------------------------------
def test_many_ranges_equal_their_single_calls(gpu_lib, monkeypatch):
    """Frames with different k, offsets, bases (none, separate, in place) and lengths, an empty frame and a w = 0 frame, windows of three
    chunks; then with one frame corrupt: no other frame's result changes.  Whole-call errors: a bad element size, a host pointer, n < 0."""
    import torch

    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    ref = require_ref().lib
    bs = KiB65 + 7
    cases = [Case(ref, bs, k, wb, stream_for(bs, blocks=nb, last=last), seed=90 + i)
             for i, (k, wb, nb, last) in enumerate(((2, 1, 2, 777), (1, 0, 1, 50), (8, 1, 3, 1234), (4, 0, 0, 100), (4, 1, 2, 9)))]
    plan = [(0, bs - 30, 100, 0), (1, 0, 10 ** 6, 0), (2, 2 * bs - 1, bs + 2, 1), (3, 7, 50, 0), (4, bs + 1, bs + 100, 1), (0, 5, 0, 0), (2, 10, 70_000, 0), (1, bs + 49, 9, 0)]
    empty = bzip3_amd.compress_tensor(torch.empty(0, dtype=torch.uint8, device="cuda:0"), bs).clone()

    def run(frames):
        n = len(plan) + 1
        frame_ts = [_dev(f) for f in frames] + [empty]
        ks = [cases[c].k for c, *_ in plan] + [2]
        offsets = [o for _, o, _, _ in plan] + [0]
        ws = [w for _, _, w, _ in plan] + [40]
        bases = [None if cases[c].base is None else (cases[c].base[o : o + w] + bytes(w))[:w] for c, o, w, _ in plan]  # (zeros past the frame's end, as the single calls get)
        befores = [(bases[i] + b"\xa5" * GUARD) if ip else b"\xa5" * (w + GUARD) for i, (c, o, w, ip) in enumerate(plan)] + [b"\xa5" * (40 + GUARD)]
        outs = [_dev(b) for b in befores]
        base_ts = [outs[i] if ip else None if bases[i] is None else _dev(bases[i]) for i, (c, o, w, ip) in enumerate(plan)] + [None]
        out_sizes, rcs = (C.c_size_t * n)(*ws), (C.c_int * n)(*([77] * n))
        vp = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
        torch.cuda.synchronize()
        rc = gpu_lib.bz3_hip_decompress_device_range_many(n, (C.c_uint32 * n)(*ks), vp(frame_ts), (C.c_size_t * n)(*[f.numel() for f in frame_ts]), (C.c_uint64 * n)(*offsets),
                                                          vp(base_ts), (C.c_size_t * n)(*[0 if b is None else ws[i] for i, b in enumerate(base_ts)]), vp(outs), out_sizes, rcs)
        got = [(rcs[i], out_sizes[i], _host(outs[i])) for i in range(n)]
        singles = []
        for i, (c, o, w, ip) in enumerate(plan):
            b = None if cases[c].base is None else (cases[c].base[o : o + w] + bytes(w))[:w]
            singles.append(gpu_range_call(gpu_lib, ks[i], frame_ts[i], o, w, b, bool(ip))[:3])
        return rc, got, befores, singles

    frames = [cases[c].frame for c, *_ in plan]
    rc, got, befores, singles = run(frames)
    assert rc == 0
    for i, (c, o, w, ip) in enumerate(plan):
        want = cases[c].want(o, w)
        assert got[i][:2] == (0, len(want)) and got[i][2][: len(want)] == want and got[i][2][len(want) :] == befores[i][len(want) :], i
        assert got[i] == singles[i], ("single call", i)
    assert got[-1] == (0, 0, b"\xa5" * (40 + GUARD))
    frames2 = list(frames)
    frames2[2] = _flip(frames[2], 2)
    rc2, got2, _, singles2 = run(frames2)
    assert rc2 == got2[2][0] != 0 and got2[2][1] == 1 and got2[2] == singles2[2]
    assert [g for i, g in enumerate(got2) if i != 2] == [g for i, g in enumerate(got) if i != 2]
    # whole-call errors, before any write
    f = _dev(cases[1].frame)
    host = (C.c_uint8 * 64)()
    for ks, outs, n in (([3], [_dev(b"\xa5" * 64)], 1), ([1], [None], 1), ([1], [_dev(b"\xa5" * 64)], -1)):
        out_sizes, rcs = (C.c_size_t * 1)(64), (C.c_int * 1)(77)
        op = (C.c_void_p * 1)(C.addressof(host) if outs[0] is None else outs[0].data_ptr())
        rc = gpu_lib.bz3_hip_decompress_device_range_many(n, (C.c_uint32 * 1)(*ks), (C.c_void_p * 1)(f.data_ptr()), (C.c_size_t * 1)(f.numel()), None, None, None, op, out_sizes, rcs)
        assert rc == INIT and (n < 0 or (rcs[0], out_sizes[0]) == (INIT, 0))
        assert bytes(host) == bytes(64) and (outs[0] is None or _host(outs[0]) == b"\xa5" * 64)


# ---- python ---------------------------------------------------------------------------------------------------------------------
ROWS = ((0, 0), (0, 37), (5, 6), (36, 37))


@pytest.mark.parametrize("dtype", DTYPES)
def test_unpack_tensor_rows(gpu_lib, dtype):
    """(37, 1001) of every dtype at 65 KiB blocks (several blocks for all but the one-byte dtypes): rows equal x[start:stop], with and
    without a base."""
    import torch

    x = _make(dtype, 37 * 1001, 11, (37, 1001))
    base = _make(dtype, 37 * 1001, 12, (37, 1001))
    for b in (None, base):
        p = bzip3_amd.pack_tensor(x, 65 << 10, base=b)
        assert p.delta == (b is not None)
        for start, stop in ROWS:
            y = bzip3_amd.unpack_tensor_rows(p, start, stop, base=None if b is None else b[start:stop])
            assert y.dtype == x.dtype and tuple(y.shape) == (stop - start, 1001) and torch.equal(y, x[start:stop]) and _raw(y) == _raw(x[start:stop]), (dtype, start, stop)
        out = torch.empty_like(x[5:9])
        assert bzip3_amd.unpack_tensor_rows(p, 5, 9, out=out, base=None if b is None else b[5:9]) is out and torch.equal(out, x[5:9])
    if b is not None:
        over = base[5:9].clone()
        assert bzip3_amd.unpack_tensor_rows(p, 5, 9, out=over, base=over) is over and torch.equal(over, x[5:9])
        with pytest.raises(ValueError):
            bzip3_amd.unpack_tensor_rows(p, 5, 9)  # a delta tensor without its base
    plain = bzip3_amd.pack_tensor(x, 65 << 10)
    for start, stop in ((-1, 3), (3, 2), (0, 38)):
        with pytest.raises(ValueError):
            bzip3_amd.unpack_tensor_rows(plain, start, stop)
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor_rows(bzip3_amd.pack_tensor(x[0, 0], 65 << 10), 0, 0)  # 0-d
    short = bzip3_amd.PackedTensor(plain.frame[: plain.frame.numel() // 2], plain.dtype, plain.shape, plain.planes, plain.block_size, plain.nbytes)
    with pytest.raises(bzip3_amd.Bz3Error):
        bzip3_amd.unpack_tensor_rows(short, 30, 37)


def test_decompress_tensor_range_is_the_slice(gpu_lib):
    import torch

    x = _make("float32", 300_001, 21).view(torch.uint8).flatten()
    frame = bzip3_amd.compress_tensor(x, 65 << 10, planes=4)
    for offset, w in ((0, x.numel()), (70_000, 3), (x.numel() - 5, 100), (x.numel() + 9, 4), (123_456, 200_000)):
        got = bzip3_amd.decompress_tensor_range(frame, offset, w, planes=4)
        assert torch.equal(got, x[offset : offset + w]), (offset, w)
    gots = bzip3_amd.decompress_tensors_range([frame, frame], [5, 66_560], [10, 66_560], planes=4)
    assert torch.equal(gots[0], x[5:15]) and torch.equal(gots[1], x[66_560 : 2 * 66_560])
    bad = frame.clone()
    bad[13 + 8 + 40] ^= 0x40
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.decompress_tensors_range([frame, bad], [0, 10], [100, 100], planes=4)
    assert e.value.index == 1 and e.value.codes[0] == 0 and torch.equal(e.value.outs[0], x[:100]) and e.value.outs[1].numel() == 0
    assert bzip3_amd.decompress_tensors_range([], [], []) == []


def test_unpack_state_dict_rows(gpu_lib, monkeypatch):
    import torch

    sd = {"w": _make("float32", 64 * 1000, 1, (64, 1000)), "b": _make("bfloat16", 777, 2, (777,)), "ids": _make("int64", 40_000, 3, (200, 200)), "step": _make("int32", 1, 4, ()),
          "e": _make("float32", 0, 5, (0, 3))}
    base = {"w": _make("float32", 64 * 1000, 6, (64, 1000)), "ids": _make("int64", 40_000, 7, (200, 200))}
    packed = bzip3_amd.pack_state_dict(sd, 65 << 10, base=base)
    whole = bzip3_amd.unpack_state_dict(packed, base=base)
    rows = {"w": (16, 32), "ids": (199, 200), "b": (0, 0)}
    calls = []
    real = gpu_lib.bz3_hip_decompress_device_range_many

    def counting(*a):
        calls.append(a[0])
        return real(*a)

    monkeypatch.setattr(gpu_lib, "bz3_hip_decompress_device_range_many", counting)
    got = bzip3_amd.unpack_state_dict(packed, base=base, rows=rows, lib=gpu_lib)
    assert calls == [len(sd)], "all tensors go through one _range_many call"
    assert list(got) == list(sd)
    for name, y in got.items():
        want = whole[name][slice(*rows[name])] if name in rows else whole[name]
        assert y.dtype == want.dtype and y.shape == want.shape and torch.equal(y, want), name
        assert torch.equal(want, sd[name][slice(*rows[name])] if name in rows else sd[name])
    with pytest.raises(ValueError):
        bzip3_amd.unpack_state_dict(packed, base=base, rows=rows, inplace=True)
    with pytest.raises(ValueError):
        bzip3_amd.unpack_state_dict(packed, base=base, rows={"w": (3, 99)})
    with pytest.raises(ValueError):
        bzip3_amd.unpack_state_dict(packed, base=base, rows={"step": (0, 1)})  # 0-d
    with pytest.raises(ValueError):
        bzip3_amd.unpack_state_dict(packed, base=base, rows={"nope": (0, 1)})
    with pytest.raises(ValueError):
        bzip3_amd.unpack_state_dict(packed, rows=rows)  # delta tensors without their bases
    for name in ("w", "ids"):  # another base: caught by its checksum, for a tensor read by rows and for one read whole
        wrong = dict(base)
        wrong[name] = base[name] + 1
        with pytest.raises(ValueError):
            bzip3_amd.unpack_state_dict(packed, base=wrong, rows={"w": (16, 32)})
        bzip3_amd.unpack_state_dict(packed, base=wrong, rows={"w": (16, 32)}, check_base=False)  # (other bytes, no error: the caller vouches)
