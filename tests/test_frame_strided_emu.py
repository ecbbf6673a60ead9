"""CPU tests of the strided range calls (include/bz3_hip.h bz3_hip_decompress_device_strided[_many], the strided merge of
bzip3_amd/csrc/planes.hpp through bz3_hip_debug_strided, the walk with a period of frame.hpp) under the fiber emulation of the HIP
execution model (tests/emu).

The oracle of a request is always full[phi(t)], phi(t) = offset + (t // run) * stride + t % run: `full` is the reference's
bz3_decompress (oracle/_ref/libbz3ref.so), numpy merge_k per chunk and numpy D_inv (test_frame_range_emu.Case), never the library under
test.  The kernel's oracle is numpy indexing of merge_k(src) with c(u) written out from its definition.

BZ3_EMU_LIB=<path> runs the module on another build of the emulator library, as test_frame_range_emu does; every buffer handed to the
library comes from test_frame_delta_emu._buf and lies inside a larger allocation."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bzip3_amd
from oracle_lib import require_ref
from test_frame_delta_emu import NO_BASE, D_inv, _buf, _host_alloc, _r16
from test_frame_planes_emu import BS, _ref_compress, _vp, merge_k
from test_frame_range_emu import ALL_COUNTS, GUARD, INIT, MALFORMED, TILE, U64, Case, _flip, _with_header, range_call, stream_for

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu():
    if os.environ.get("BZ3_EMU_LIB"):
        return bzip3_amd._declare(C.CDLL(os.environ["BZ3_EMU_LIB"]))
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def chunk_bytes(c0, first, run, stride, nbytes):
    """c(u) for u < nbytes, from the definition in planes.hpp."""
    u = np.arange(nbytes, dtype=np.int64)
    v = u - first
    return np.where(u < first, c0 + u, c0 + first + (stride - run) + (v // run) * stride + v % run)


def fit(c0, first, run, stride, last):
    """(c0', nbytes) of a segment whose last chunk byte is `last`: c0 is moved up where `last` would fall into a gap."""
    if last < c0 + first:
        return c0, last - c0 + 1
    d = last - (c0 + first + stride - run)
    if d < 0:  # in the gap behind the first piece
        return last - first + 1, first
    i, r = divmod(d, stride)
    if r < run:
        return c0, first + i * run + r + 1
    return c0 + r - (run - 1), first + (i + 1) * run


def runs_for(k):
    return sorted({r for r in (1, k - 1, k, k + 1, 15, 16, 17, 16 * k - 1, 16 * k, 16 * k + 1, TILE * k + 1) if r > 0})


def strides_for(run, k):
    return (run, run + 1, run + k, run + 16, 3 * run + 5)


def periods_for(rng, elems, tail, k):
    """(c0, first, run, stride, nbytes) of the sweep for a chunk of elems * k + tail bytes: every run and stride, first = 1, run and an
    interior value, the last piece ending exactly at len, one byte before it and inside the tail (the three ends rotate through the
    other choices, so that every (first, end) pair occurs)."""
    n, it = elems * k + tail, 0
    ends = (n - 1, n - 2, elems * k + tail // 2 if tail else n - 1 - k)
    for run in runs_for(k):
        for stride in strides_for(run, k):
            for first in dict.fromkeys((1, run, (run + 1) // 2)):
                last = ends[it % 3]
                it += 1
                if last < 0:
                    continue
                c0, nbytes = fit(min(int(rng.integers(0, 40)), last), first, run, stride, last)
                assert nbytes >= 1 and chunk_bytes(c0, first, run, stride, nbytes)[-1] == last < n
                yield c0, first, run, stride, nbytes


def lay_out_strided(rng, spec, addrs, src_np, base_np):
    """spec: (slot, base, dst alignment mod 16, elements, tail bytes, k, has base, c0, first, run, stride, nbytes) per segment, one after
    the other with gaps.  Returns the hook's table and the expected writes."""
    table, writes, offs = [], [], [0, 0, 0]
    for a_s, a_b, a_d, elems, tail, k, has_base, c0, first, run, stride, nbytes in spec:
        n = elems * k + tail
        for j, al in enumerate((a_s, a_b, a_d)):
            offs[j] += (al - (addrs[j] + offs[j])) % 16
        s, bo, d = offs
        table += [s, bo if has_base else NO_BASE, d, n, k | 0x100, c0, first, run, stride, nbytes]
        x = merge_k(src_np[s : s + n], k)[chunk_bytes(c0, first, run, stride, nbytes)] if nbytes else np.zeros(0, dtype=np.uint8)
        writes.append((d, D_inv(x, base_np[bo : bo + nbytes]) if has_base else x))
        offs[0] += n + int(rng.integers(0, 40))
        offs[1] += nbytes + int(rng.integers(1, 40))
        offs[2] += nbytes + int(rng.integers(1, 40))  # at least one untouched byte between destination segments
    return table, writes, offs


def strided_case(call, rng, spec, alloc):
    """alloc(array) -> (object for the hook, address, numpy reader); call(src, base, dst, table, n) -> rc.  The whole destination is
    compared against a 0xA5 fill with the expected writes, the inputs against themselves."""
    room_s = sum(s[3] * s[5] + s[4] for s in spec) + 56 * len(spec) + 64
    room_d = sum(s[-1] for s in spec) + 56 * len(spec) + 64
    src_np = rng.integers(0, 256, size=room_s, dtype=np.uint8)
    base_np = rng.integers(0, 256, size=room_d, dtype=np.uint8)
    src, base, dst = alloc(src_np), alloc(base_np), alloc(np.full(room_d, 0xA5, dtype=np.uint8))
    want = np.full(room_d, 0xA5, dtype=np.uint8)
    table, writes, ends = lay_out_strided(rng, spec, (src[1], base[1], dst[1]), src_np, base_np)
    assert ends[0] <= room_s - 16 and max(ends[1:]) <= room_d - 16
    for off, b in writes:
        want[off : off + len(b)] = b
    t = (C.c_uint64 * max(1, len(table)))(*table)
    assert call(src[0], base[0], dst[0], t, len(table) // 10) == 0
    bad = np.nonzero(dst[2]() != want)[0]
    assert bad.size == 0, ("bytes differ at", bad[:8], [table[10 * i : 10 * i + 10] for i in range(len(spec)) if any(table[10 * i + 2] <= b < table[10 * i + 2] + table[10 * i + 9] for b in bad[:8])][:2])
    assert np.array_equal(src[2](), src_np) and np.array_equal(base[2](), base_np), "an input was written"


def sweep_specs_strided(rng, k, has_base, counts=ALL_COUNTS, alignments=True):
    """One launch per element count and tail length 0..k-1: every period of periods_for, all at random alignments; then (`alignments`)
    each of the three alignments through all 16 values with the other two random, on a chunk of two tiles and a little with a random
    period that ends at the chunk's last byte."""
    for elems in counts:
        for tail in range(k):
            spec = [(_r16(rng), _r16(rng), _r16(rng), elems, tail, k, has_base, *p) for p in periods_for(rng, elems, tail, k)]
            if spec:
                yield spec
    if not alignments:
        return
    spec = []
    for which in range(3):
        for al16 in range(16):
            al = [_r16(rng), _r16(rng), _r16(rng)]
            al[which] = al16
            elems, tail = 2 * TILE + int(rng.integers(1, 300)), int(rng.integers(0, k))
            run = int(rng.integers(16 * k, 40 * k))
            stride, first = run + int(rng.integers(1, 3 * k)) * (1 if al16 % 2 else k), int(rng.integers(1, run + 1))
            c0, nbytes = fit(int(rng.integers(0, 40)) * k, first, run, stride, elems * k + tail - 1)
            spec.append((*al, elems, tail, k, has_base, c0, first, run, stride, nbytes))
    yield spec


def mixed_spec_strided(rng):
    """One launch that holds strided, clipped (one piece inside the chunk), whole (one piece that is the chunk) and plain (k = 1, one
    piece) segments of every k, with and without a base."""
    spec = []
    for _ in range(2):
        for k in (1, 2, 4, 8):
            for has in (0, 1):
                elems, tail = int(rng.integers(600, 9000)), int(rng.integers(0, k))
                n = elems * k + tail
                run = int(rng.integers(1, 50 * k))
                stride, first = run + int(rng.integers(0, 100)), int(rng.integers(1, run + 1))
                c0, nbytes = fit(int(rng.integers(0, 300)), first, run, stride, n - 1 - int(rng.integers(0, 9)))
                spec.append((_r16(rng), _r16(rng), _r16(rng), elems, tail, k, has, c0, first, run, stride, nbytes))  # strided
                a, b = sorted(int(v) for v in rng.integers(0, n + 1, size=2))
                spec.append((_r16(rng), _r16(rng), _r16(rng), elems, tail, k, has, a, max(b - a, 1), max(b - a, 1) + 3, n + 7, b - a))  # one piece: clipped (k = 1: plain)
                spec.append((_r16(rng), _r16(rng), _r16(rng), elems, tail, k, has, 0, n, n, n, n))  # one piece, the whole chunk
    return spec


def in_place_strided_case(call, rng, alloc, sizes=(17, 4079, 4081, 9000, 70_001)):
    """dst == base: (merge_k(src)[c(u)] + dst) written over dst, every k, several tiles."""
    spec = []
    for k in (1, 2, 4, 8):
        for e in sizes:
            tail = int(rng.integers(0, k))
            run = int(rng.integers(1, 64 * k)) if e < 9000 else k * int(rng.integers(16, 600))
            stride, first = run + k * int(rng.integers(1, 40)), int(rng.integers(1, run + 1))
            c0, nbytes = fit(k * int(rng.integers(0, 9)), first, run, stride, e * k + tail - 1)
            spec.append((_r16(rng), _r16(rng), e, tail, k, c0, first, run, stride, nbytes))
    room_s = sum(e * k + t for _, _, e, t, k, *_ in spec) + 56 * len(spec) + 64
    src_np = rng.integers(0, 256, size=room_s, dtype=np.uint8)
    old = rng.integers(0, 256, size=room_s, dtype=np.uint8)
    src, dst = alloc(src_np), alloc(old)
    want, table, offs = old.copy(), [], [0, 0]
    for a_s, a_d, elems, tail, k, c0, first, run, stride, nbytes in spec:
        n = elems * k + tail
        offs[0] += (a_s - (src[1] + offs[0])) % 16
        offs[1] += (a_d - (dst[1] + offs[1])) % 16
        s, d = offs
        table += [s, d, d, n, k | 0x100, c0, first, run, stride, nbytes]
        want[d : d + nbytes] = D_inv(merge_k(src_np[s : s + n], k)[chunk_bytes(c0, first, run, stride, nbytes)], old[d : d + nbytes])
        offs[0] += n + int(rng.integers(1, 40))
        offs[1] += nbytes + int(rng.integers(1, 40))
    assert max(offs) <= room_s - 16
    t = (C.c_uint64 * len(table))(*table)
    assert call(src[0], dst[0], dst[0], t, len(table) // 10) == 0
    bad = np.nonzero(dst[2]() != want)[0]
    assert bad.size == 0, ("bytes differ at", bad[:8])
    assert np.array_equal(src[2](), src_np)


@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("elems", ALL_COUNTS)
def test_strided_kernel_every_period_at_every_tail(emu, elems, k, has_base):
    rng = np.random.default_rng(700 + 100 * elems + 10 * k + has_base)
    for spec in sweep_specs_strided(rng, k, has_base, counts=(elems,), alignments=False):
        strided_case(emu.bz3_hip_debug_strided, rng, spec, _host_alloc)


@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_strided_kernel_every_alignment(emu, k, has_base):
    rng = np.random.default_rng(700 + 10 * k + has_base)
    for spec in sweep_specs_strided(rng, k, has_base, counts=()):
        strided_case(emu.bz3_hip_debug_strided, rng, spec, _host_alloc)


def test_strided_kernel_mixed_segments_in_one_launch(emu):
    rng = np.random.default_rng(72)
    strided_case(emu.bz3_hip_debug_strided, rng, mixed_spec_strided(rng), _host_alloc)
    strided_case(emu.bz3_hip_debug_strided, rng, [], _host_alloc)


def test_strided_kernel_in_place(emu):
    in_place_strided_case(emu.bz3_hip_debug_strided, np.random.default_rng(73), _host_alloc)


def test_debug_strided_rejects_bad_arguments(emu):
    buf = _buf(b"", 256)
    call = emu.bz3_hip_debug_strided
    assert call(buf, buf, buf, None, -1) == INIT
    assert call(buf, buf, buf, None, 0) == 0
    ok = (0, 0, 128, 100, 2 | 0x100, 3, 2, 4, 10, 30)  # pieces [3, 5), [11, 15), ... : the last byte is c(29) = 3 + 29 + 7 * 6 = 74
    assert int(chunk_bytes(*ok[5:])[-1]) == 74
    for mode in (0, 2, 3 | 0x100, 16 | 0x100, 2 | 0x300, 2 | 0x500):  # the split direction, bad element sizes, stray bits
        assert call(buf, buf, buf, (C.c_uint64 * 10)(*ok[:4], mode, *ok[5:]), 1) == INIT
    for length in (74, 10, 0):  # the last chunk byte is not below len
        assert call(buf, buf, buf, (C.c_uint64 * 10)(*ok[:3], length, *ok[4:]), 1) == INIT
    for c0, first, run, stride, nbytes in ((3, 0, 4, 10, 30), (3, 5, 4, 10, 30), (3, 2, 0, 10, 30), (3, 2, 4, 3, 30), (U64 - 5, 2, 4, 10, 30), (3, 2, 4, U64, 30), (80, 1, 1, 1, 21)):
        assert call(buf, buf, buf, (C.c_uint64 * 10)(*ok[:5], c0, first, run, stride, nbytes), 1) == INIT, (c0, first, run, stride, nbytes)
    assert call(buf, buf, buf, (C.c_uint64 * 10)(*ok[:3], 2 ** 31, *ok[4:]), 1) == INIT
    assert bytes(buf) == bytes(256)
    assert call(buf, None, buf, (C.c_uint64 * 10)(0, NO_BASE, 128, 75, *ok[4:]), 1) == 0  # (the last byte is the chunk's last)


# ---- frames -------------------------------------------------------------------------------------------------------------------
def phi(offset, run, stride, w):
    t = np.arange(w, dtype=np.int64)
    return offset + (t // run) * stride + t % run


def want_strided(case, offset, run, stride, count, cap, base=None):
    """The bytes the contract asks for: full[phi(t)] for t < w with phi(t) < T."""
    w = min(cap, count * run)
    if w == 0:
        return b""
    idx = phi(offset, run, stride, w)
    idx = idx[idx < case.T]
    return bytes(np.frombuffer(case.full, dtype=np.uint8)[idx])


def strided_call(lib, k, frame, offset, run, stride, count, cap, base=None, in_place=False, room=None):
    """(rc, *out_size, the bytes of out[0, room + GUARD) after the call, what they were before).  base: the base's bytes of the slice."""
    room = (min(cap, count * run) if room is None else room) + GUARD
    before = (bytes(base) + b"\xa5" * room)[:room] if in_place else b"\xa5" * room
    out = _buf(before)
    b = out if in_place else None if base is None else _buf(base)
    osz = C.c_size_t(cap)
    rc = lib.bz3_hip_decompress_device_strided(k, _buf(frame), len(frame), offset, run, stride, count, b, 0 if base is None else room - GUARD if in_place else len(base), out,
                                               C.byref(osz))
    return rc, osz.value, bytes(out)[:room], before


def slice_base(case, offset, run, stride, count, cap):
    """The base's bytes of the slice, in output order (zeros where phi(t) runs past T)."""
    if case.base is None:
        return None
    w = min(cap, count * run)
    idx = phi(offset, run, stride, w)
    padded = np.concatenate([np.frombuffer(case.base, dtype=np.uint8), np.zeros(int(idx.max()) + 1 if w else 1, dtype=np.uint8)])
    return bytes(padded[idx]) if w else b"\0"


def check_strided(lib, case, offset, run, stride, count, cap=None, in_place=False):
    cap = count * run if cap is None else cap
    base = slice_base(case, offset, run, stride, count, cap)
    rc, r, got, before = strided_call(lib, case.k, case.frame, offset, run, stride, count, cap, base, in_place and base is not None)
    want = want_strided(case, offset, run, stride, count, cap)
    assert (rc, r) == (0, len(want)), (offset, run, stride, count, cap, rc, r, len(want))
    assert got[:r] == want, ("bytes differ", offset, run, stride, count, cap)
    assert got[r:] == before[r:], ("wrote beyond the slice", offset, run, stride, count, cap)


def frame_requests(case):
    """(offset, run, stride, count, *out_size or None).  Chunk 4 is the short one: what needs no full chunk is asked of it, because a full
    chunk costs the emulator about a second.  (count == 1, stride == run and an *out_size of one run are the equivalence test's.)"""
    s, bs, T = case.starts, case.bs, case.T
    yield s[4] + 50, 20, 100, 10, None  # runs inside one chunk
    yield s[4] + 3, 1, 7, 150, None  # the byte path
    yield s[4] - 30, 60, 500, 3, None  # a run across a chunk boundary, and more behind it
    yield s[1], bs, 2 * bs, 2, None  # runs equal to chunks 1 and 3; chunk 2 lies wholly in the gap
    yield s[1] + 10, 100, 3 * bs, 2, None  # chunks 2 and 3 lie wholly in the gap
    yield s[4] + 7, 50, 300, 4, 4 * 50 - 23  # *out_size smaller than W: the last run is cut
    yield T - 700, 300, 500, 3, None  # runs past T: short
    yield T + 5, 30, 50, 4, None  # wholly past T
    yield 5, 0, 9, 4, None  # W = 0
    yield 5, 9, 9, 0, None


@pytest.mark.parametrize("with_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("bs", [BS, BS + 3])
def test_strided_requests_of_a_frame_match_the_reference(emu, bs, k, with_base, monkeypatch):
    """Four full blocks of 65 KiB (65 KiB + 3: every block starts inside an element and has a tail) and a short one; windows of two chunks."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    case = Case(require_ref().lib, bs, k, with_base, stream_for(bs, blocks=4))
    assert len(case.sizes) == 5 and case.sizes[:4] == [bs] * 4
    for offset, run, stride, count, cap in frame_requests(case):
        check_strided(emu, case, offset, run, stride, count, cap)
    if with_base:
        check_strided(emu, case, case.starts[4] + 5, 60, 200, 5, in_place=True)


def test_count_one_and_stride_equal_run_are_the_range_call(emu, monkeypatch):
    """Bytes, rc and *out_size of the range call with *out_size = min(*out_size, W), for a good frame and for one with a corrupt chunk."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    bs = BS + 3
    case = Case(require_ref().lib, bs, 4, 1, stream_for(bs, blocks=2))
    s = case.starts
    for frame in (case.frame, _flip(case.frame, 1)):
        for offset, run, stride, count, cap in ((s[2] - 50, 300, 7, 1, 10 ** 9), (s[2] - 48, 100, 100, 7, 10 ** 9), (s[2] - 48, 10, 10, 14, 101), (case.T - 10, 8, 8, 4, 64),
                                                (0, 16, 16, 0, 64)):
            w = min(cap, count * run)
            base = (case.base[offset : offset + w] + bytes(w))[:w] if w else b"\0"
            got = strided_call(emu, 4, frame, offset, run, stride, count, cap, base, room=w)
            ref = range_call(emu, 4, frame, offset, w, base)
            assert got == ref, (offset, run, stride, count, cap, got[:2], ref[:2])


# ---- skipping is real -----------------------------------------------------------------------------------------------------------
def committed_below(offset, run, stride, w, p):
    """The number of t < w with phi(t) < p."""
    return int((phi(offset, run, stride, w) < p).sum())


def test_corrupt_chunks_in_the_gaps_are_skipped_and_needed_ones_commit_a_prefix(emu, monkeypatch):
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    ref = require_ref().lib
    bs = BS + 3
    case = Case(ref, bs, 2, 1, stream_for(bs, blocks=2))
    s = case.starts
    offset, run, stride, count = 100, 1200, 2 * bs, 2  # chunks 0 and 2 (the short one cuts the second run); chunk 1 lies in the gap
    w = count * run
    base = slice_base(case, offset, run, stride, count, w)
    good = want_strided(case, offset, run, stride, count, w)
    assert len(good) == run + (case.T - (offset + stride)) and run < len(good) < w
    bad = _flip(case.frame, 1)  # a corrupt payload in a gap is not noticed
    assert range_call(emu, 2, bad, 0, 50)[:2] == (0, 50) and range_call(emu, 2, bad, s[1], 50, base[:50])[0] != 0, "the flipped chunk must fail where it is decoded"
    rc, r, got, before = strided_call(emu, 2, bad, offset, run, stride, count, w, base)
    assert (rc, r) == (0, len(good)) and got[:r] == good and got[r:] == before[r:]
    for j in (0, 2):  # in a needed chunk: its code, and exactly the bytes with phi(t) < p_j
        rc, r, got, before = strided_call(emu, 2, _flip(case.frame, j), offset, run, stride, count, w, base)
        assert rc != 0 and r == committed_below(offset, run, stride, w, s[j]) == (j // 2) * run, (j, rc, r)
        assert got[:r] == good[:r] and got[r:] == before[r:], j
    for j in range(3):  # a corrupt header, in a gap too, is reported after the bytes before it are committed
        rc, r, got, before = strided_call(emu, 2, _with_header(case.frame, j, orig=-5), offset, run, stride, count, w, base)
        assert rc == MALFORMED and r == committed_below(offset, run, stride, w, s[j]) == ((j + 1) // 2) * run, (j, rc, r)
        assert got[:r] == good[:r] and got[r:] == before[r:], j
    # a header at or beyond `end` is never read
    rc, r, got, before = strided_call(emu, 2, _with_header(case.frame, 1, orig=-5), offset, 100, 300, 3, 300, slice_base(case, offset, 100, 300, 3, 300))
    assert (rc, r) == (0, 300) and got[:r] == want_strided(case, offset, 100, 300, 3, 300) and got[r:] == before[r:]


def test_strided_calls_launch_the_cm_stage_for_the_needed_chunks_only(emu, monkeypatch):
    """Five chunks.  Runs in chunks 0, 2 and 4: with windows of two chunks the needed chunks fill ceil(3 / 2) = 2 windows, the full decode
    ceil(5 / 2) = 3.  Runs in chunks 1 and 4, two chunks in the gap: with windows of one chunk 2 launches, where the full decode takes 5."""
    ref = require_ref().lib
    case = Case(ref, BS, 1, 0, stream_for(BS, blocks=4))
    assert len(case.sizes) == 5
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    emu.bz3_hip_debug_cm_launches(1)
    check_strided(emu, case, 10, 100, 2 * BS, 3)
    assert emu.bz3_hip_debug_cm_launches(1) == 2
    check_strided(emu, case, 0, case.T, case.T, 1)
    assert emu.bz3_hip_debug_cm_launches(1) == 3
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "1")
    check_strided(emu, case, BS + 10, 100, 3 * BS, 2)
    assert emu.bz3_hip_debug_cm_launches(1) == 2


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_invalid_periods_and_partial_overlap_are_refused_before_any_write(emu):
    case = Case(require_ref().lib, BS + 3, 4, 1, stream_for(BS + 3, blocks=1))
    for offset, run, stride, count in ((0, 10, 9, 2), (0, 10, 0, 2), (0, 2 ** 33, 2 ** 33, 2 ** 31), (U64 - 50, 10, 20, 4), (U64 - 5, 10, 20, 1), (5, 3, U64 // 2, 4)):
        rc, r, got, before = strided_call(emu, 4, case.frame, offset, run, stride, count, 64, room=64)
        assert (rc, r) == (INIT, 0) and got == before, (offset, run, stride, count)
    rc, r, got, before = strided_call(emu, 3, case.frame, 0, 10, 20, 2, 64, room=64)  # a bad element size
    assert (rc, r) == (INIT, 0) and got == before
    assert strided_call(emu, 4, case.frame, 0, 10, 5, 1, 64, room=64)[:2] == (0, 10)  # count == 1: stride < run is no violation
    assert strided_call(emu, 4, case.frame, U64, 0, 0, 7, 64, room=64)[:2] == (0, 0)  # W = 0: nothing else of the period is looked at
    assert strided_call(emu, 4, case.frame[:12], 0, 10, 20, 2, 64, room=64)[:2] == (MALFORMED, 0)
    # out overlaps the base without being it: BZ3_ERR_INIT, nothing written; the overlap is judged on w = count * run = 1000 bytes
    arena = _buf(b"\xa5" * 4096)
    sl = slice_base(case, 0, 100, 300, 10, 1000)
    C.memmove(arena, sl, 1000)
    before = bytes(arena)
    for off in (1, 16, 999):
        osz = C.c_size_t(4000)
        assert emu.bz3_hip_decompress_device_strided(4, _buf(case.frame), len(case.frame), 0, 100, 300, 10, arena, 4000, C.byref(arena, off), C.byref(osz)) == INIT
        assert bytes(arena) == before and osz.value == 0
    osz = C.c_size_t(4000)
    assert emu.bz3_hip_decompress_device_strided(4, _buf(case.frame), len(case.frame), 0, 100, 300, 10, arena, 4000, C.byref(arena, 1000), C.byref(osz)) == 0  # adjacent: fine
    assert osz.value == 1000 and bytes(arena)[1000:2000] == want_strided(case, 0, 100, 300, 10, 1000) and bytes(arena)[:1000] == sl


# ---- many -----------------------------------------------------------------------------------------------------------------------
def many_call(lib, ks, frames, params, caps, bases, in_place):
    """Per frame (rc, *out_size, out[0, w + GUARD) after, before).  bases[i]: None or the base's bytes of the slice."""
    n = len(frames)
    ws = [min(c, p[1] * p[3]) for c, p in zip(caps, params)]
    ins = [_buf(f) for f in frames]
    befores = [((bytes(bases[i]) + b"\xa5" * (ws[i] + GUARD))[: ws[i] + GUARD]) if in_place[i] else b"\xa5" * (ws[i] + GUARD) for i in range(n)]
    outs = [_buf(b) for b in befores]
    bbufs = [outs[i] if in_place[i] else None if bases[i] is None else _buf(bases[i]) for i in range(n)]
    out_sizes, rcs = (C.c_size_t * n)(*caps), (C.c_int * n)(*([77] * n))
    bp = (C.c_void_p * n)(*[None if b is None else C.addressof(b) for b in bbufs])
    bsz = (C.c_size_t * n)(*[0 if bases[i] is None else ws[i] if in_place[i] else len(bases[i]) for i in range(n)])
    rc = lib.bz3_hip_decompress_device_strided_many(n, None if ks is None else (C.c_uint32 * n)(*ks), _vp(ins), (C.c_size_t * n)(*map(len, frames)),
                                                    (C.c_uint64 * (4 * n))(*[v for p in params for v in p]), bp, bsz, _vp(outs), out_sizes, rcs)
    return rc, [(rcs[i], out_sizes[i], bytes(outs[i])[: ws[i] + GUARD], befores[i]) for i in range(n)]


def test_many_strided_requests_equal_their_single_calls(emu, monkeypatch):
    """Mixed periods (strided, contiguous, W = 0), element sizes and bases (none, separate, in place) in one call at windows of three
    chunks, one frame given twice with two different slices; then the same with one frame corrupt: no other frame's result changes."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    ref = require_ref().lib
    bs = BS + 3
    cases = [Case(ref, bs, k, wb, stream_for(bs, blocks=nb, last=last), seed=190 + i) for i, (k, wb, nb, last) in enumerate(((2, 1, 1, 777), (1, 0, 0, 50), (8, 1, 2, 1234), (4, 0, 0, 100)))]
    # (case, (offset, run, stride, count), *out_size, in place)
    plan = [(0, (bs - 30, 60, 200, 3), 10 ** 6, 0), (1, (0, 10, 10, 10 ** 5), 10 ** 6, 0), (2, (10, 5000, 2 * bs, 2), 10 ** 6, 1), (2, (2 * bs + 7, 64, 128, 20), 64 * 20 - 9, 0),
            (3, (7, 5, 11, 30), 10 ** 6, 0), (0, (5, 0, 9, 9), 50, 0), (0, (bs + 1, 3, bs, 1), 10 ** 6, 1)]
    ks = [cases[c].k for c, *_ in plan]
    frames = [cases[c].frame for c, *_ in plan]
    params = [p for _, p, _, _ in plan]
    caps = [cap for *_, cap, _ in plan]
    in_place = [bool(ip) for *_, ip in plan]
    bases = [slice_base(cases[c], *p, cap) for c, p, cap, _ in plan]
    rc, got = many_call(emu, ks, frames, params, caps, bases, in_place)
    assert rc == 0
    for i, (c, p, cap, ip) in enumerate(plan):
        want = want_strided(cases[c], *p, cap)
        assert got[i][:2] == (0, len(want)) and got[i][2][: len(want)] == want and got[i][2][len(want) :] == got[i][3][len(want) :], i
        assert got[i][:3] == strided_call(emu, ks[i], frames[i], *p, cap, bases[i], in_place[i])[:3], ("single call", i)
    frames2 = list(frames)
    frames2[2] = frames2[3] = _flip(frames[2], 2)  # chunk 2 holds the second run of frame 2 and every run of frame 3
    rc2, got2 = many_call(emu, ks, frames2, params, caps, bases, in_place)
    assert rc2 == got2[2][0] != 0 and got2[2][1] == 5000 and (got2[3][0], got2[3][1]) == (got2[2][0], 0)
    for i in (2, 3):
        assert got2[i][:3] == strided_call(emu, ks[i], frames2[i], *params[i], caps[i], bases[i], in_place[i])[:3]
    assert [g for i, g in enumerate(got2) if i not in (2, 3)] == [g for i, g in enumerate(got) if i not in (2, 3)]


def test_many_whole_call_errors(emu):
    ref = require_ref().lib
    frame = _ref_compress(ref, BS, b"abcdefgh" * 100)[1]
    full = b"abcdefgh" * 100

    def call(ks=(1, 1), n=2, params=((0, 2, 8, 50), (1, 3, 8, 50)), null_params=False):
        ins = [_buf(frame), _buf(frame)]
        outs = [_buf(b"\xa5" * 300), _buf(b"\xa5" * 300)]
        out_sizes, rcs = (C.c_size_t * 2)(300, 300), (C.c_int * 2)(77, 77)
        rc = emu.bz3_hip_decompress_device_strided_many(n, None if ks is None else (C.c_uint32 * 2)(*ks), _vp(ins), (C.c_size_t * 2)(len(frame), len(frame)),
                                                        None if null_params else (C.c_uint64 * 8)(*[v for p in params for v in p]), None, None, _vp(outs), out_sizes, rcs)
        return rc, list(rcs), list(out_sizes), [bytes(o) for o in outs]

    untouched = [b"\xa5" * 300] * 2
    assert call() == (0, [0, 0], [100, 150], [b"ab" * 50 + b"\xa5" * 200, b"bcd" * 50 + b"\xa5" * 150])
    assert call(ks=None)[:3] == (0, [0, 0], [100, 150])  # elem_sizes == NULL: 1 for every frame
    assert call(ks=(1, 3)) == (INIT, [INIT, INIT], [0, 0], untouched)  # a bad element size
    assert call(params=((0, 2, 8, 50), (1, 3, 2, 50))) == (INIT, [INIT, INIT], [0, 0], untouched)  # one invalid period fails the whole call
    assert call(null_params=True) == (INIT, [INIT, INIT], [0, 0], untouched)
    assert call(n=-1)[0] == INIT
    assert emu.bz3_hip_decompress_device_strided_many(0, None, None, None, None, None, None, None, None, None) == 0
    assert emu.bz3_hip_decompress_device_strided_many(2, None, None, None, None, None, None, None, None, None) == INIT
    assert full[1:4] == b"bcd"
