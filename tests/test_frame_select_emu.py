"""CPU tests of the index decode calls (include/bz3_hip.h bz3_hip_decompress_device_select[_many], the select merge of
bzip3_amd/csrc/planes.hpp through bz3_hip_debug_select, the walk with a piece table of frame.hpp) under the fiber emulation of the HIP
execution model (tests/emu).

The oracle of a request is always full[phi(t)], phi written out from its definition in bz3_hip.h with numpy: `full` is the reference's
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
from test_frame_range_emu import GUARD, INIT, MALFORMED, TILE, U64, Case, _flip, _with_header, range_call, stream_for
from test_frame_strided_emu import strided_call

HERE = os.path.dirname(os.path.abspath(__file__))
DST_COUNTS = (0, 1, 17, 4079, 4080, 4081, 8160, 8161)  # destination elements: the tile edges
PIECE_COUNTS = (2, 3, 64, 65, 1000)  # the binary search's edges


@pytest.fixture(scope="module")
def emu():
    if os.environ.get("BZ3_EMU_LIB"):
        return bzip3_amd._declare(C.CDLL(os.environ["BZ3_EMU_LIB"]))
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


# ---- phi ------------------------------------------------------------------------------------------------------------------------
def period_bytes(pieces, x):
    """For the bytes x (an int64 array, x >= 0) of the concatenated wanted bytes of periods: (period, byte of the period), from the
    definition: x = q L + r, j the piece with P_j <= r < P_{j+1}, the byte s_j + (r - P_j)."""
    s = np.array([p[0] for p in pieces], dtype=np.int64)
    lens = np.array([p[1] for p in pieces], dtype=np.int64)
    ends = np.cumsum(lens)  # P_1 .. P_m
    L = int(ends[-1])
    q, r = x // L, x % L
    j = np.searchsorted(ends, r, side="right")
    return q, s[j] + (r - (ends[j] - lens[j]))


def total(pieces):
    return sum(l for _, l in pieces)


def phi(offset, stride, pieces, w):
    q, b = period_bytes(pieces, np.arange(w, dtype=np.int64))
    return offset + q * stride + b


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def chunk_bytes(rel, stride, q0, r0, nbytes, pieces):
    """c(u) for u < nbytes, from the definition in planes.hpp (rel a signed int here)."""
    q, b = period_bytes(pieces, r0 + np.arange(nbytes, dtype=np.int64))
    return rel + (q0 + q) * stride + b


def piece_lengths(k):
    return sorted({v for v in (1, k - 1, k, k + 1, 15, 16, 17, 16 * k - 1, 16 * k, 16 * k + 1) if v > 0})


def piece_list(rng, m, k, long=0):
    """m pieces with lengths of piece_lengths mixed within the list (`long`: every eighth one some tiles long), gaps of 1, k and 16, now
    and then an empty piece and two neighbours that touch."""
    lens, out, at = piece_lengths(k), [], int(rng.integers(0, 40))
    for j in range(m):
        l = int(lens[int(rng.integers(0, len(lens)))])
        if long and j % 8 == 3:
            l = long + int(rng.integers(0, 2 * k))
        if m > 3 and j % 11 == 5:
            l = 0
        out.append((at, l))
        at += l + (0 if m > 3 and j % 13 == 7 else (1, k, 16)[int(rng.integers(0, 3))])
    return out


def place(rng, pieces, k, nbytes, end_mode, r0=None, q0=None, slack=0):
    """(n, rel, stride, q0, r0) of a segment of nbytes destination bytes over `pieces`, r0 > 0 where the list allows it: the chunk has n bytes and
    the segment's last chunk byte is its last (end_mode 0: the chunk has no tail), the one before its last (1), or lies inside its tail (2)."""
    L, E = total(pieces), pieces[-1][0] + pieces[-1][1]
    stride = E + (0, 1, k, 16)[int(rng.integers(0, 4))]
    q0 = int(rng.integers(0, 5)) if q0 is None else q0
    r0 = int(rng.integers(min(1, L - 1), L)) if r0 is None else r0
    if nbytes == 0:
        return 64 * k + int(rng.integers(0, k)), 0, stride, q0, r0
    f = chunk_bytes(0, stride, q0, r0, nbytes, pieces)
    first, last = int(f[0]), int(f[-1])
    rel = int(rng.integers(0, 40)) - first  # c(0) = a small number
    end = rel + last + 1  # one past the last chunk byte
    if k > 1 and end_mode == 0:
        rel += -end % k
    elif k > 1 and end_mode == 2:
        rel += (k // 2 - end) % k
    end = rel + last + 1
    n = end + (1 if end_mode == 1 else 0) + slack
    assert k == 1 or end_mode != 2 or (n // k) * k <= end - 1 < n
    return n, rel, stride, q0, r0


def select_case(call, rng, spec, alloc, in_place=False):
    """spec: (slot, base, dst alignment mod 16, n, k, has base, rel, stride, q0, r0, nbytes, pieces) per segment, one after the other with
    gaps.  alloc(array) -> (object for the hook, address, numpy reader); call(src, base, dst, table, n, pieces, n_pieces) -> rc.  The whole
    destination is compared against a 0xA5 fill (in place: the base) with the expected writes, the inputs against themselves."""
    room_s = sum(s[3] for s in spec) + 56 * len(spec) + 64
    room_d = sum(s[10] for s in spec) + 56 * len(spec) + 64
    src_np = rng.integers(0, 256, size=room_s, dtype=np.uint8)
    base_np = rng.integers(0, 256, size=room_d, dtype=np.uint8)
    src, base = alloc(src_np), alloc(base_np)
    dst = base if in_place else alloc(np.full(room_d, 0xA5, dtype=np.uint8))
    want = base_np.copy() if in_place else np.full(room_d, 0xA5, dtype=np.uint8)
    table, flat, offs = [], [], [0, 0, 0]
    addrs = (src[1], base[1], dst[1])
    for a_s, a_b, a_d, n, k, has_base, rel, stride, q0, r0, nbytes, pieces in spec:
        for j, al in enumerate((a_s, a_b, a_d)):
            offs[j] += (al - (addrs[j] + offs[j])) % 16
        if in_place:
            offs[1] = offs[2] = max(offs[1], offs[2])
        s, bo, d = offs
        table += [s, bo if has_base else NO_BASE, d, n, k | 0x100, rel % 2 ** 64, stride, q0, r0, nbytes, len(flat) // 2, len(pieces)]
        flat += [v for p in pieces for v in p]
        if nbytes:
            c = chunk_bytes(rel, stride, q0, r0, nbytes, pieces)
            assert 0 <= int(c[0]) and int(c[-1]) < n and bool(np.all(np.diff(c) > 0))
            x = merge_k(src_np[s : s + n], k)[c]
            want[d : d + nbytes] = D_inv(x, base_np[bo : bo + nbytes]) if has_base else x
        offs[0] += n + int(rng.integers(0, 40))
        offs[1] += nbytes + int(rng.integers(1, 40))
        offs[2] += nbytes + int(rng.integers(1, 40))  # at least one untouched byte between destination segments
    assert offs[0] <= room_s - 16 and max(offs[1:]) <= room_d - 16
    t = (C.c_uint64 * max(1, len(table)))(*table)
    pc = (C.c_uint64 * max(1, len(flat)))(*flat)
    assert call(src[0], base[0], dst[0], t, len(table) // 12, pc, len(flat) // 2) == 0
    bad = np.nonzero(dst[2]() != want)[0]
    assert bad.size == 0, ("bytes differ at", bad[:8], [table[12 * i : 12 * i + 12] for i in range(len(spec)) if any(table[12 * i + 2] <= b < table[12 * i + 2] + table[12 * i + 9] for b in bad[:8])][:2])
    assert np.array_equal(src[2](), src_np), "the source was written"
    if not in_place:
        assert np.array_equal(base[2](), base_np), "the base was written"


def sweep_specs_select(rng, k, has_base, counts=DST_COUNTS, alignments=True):
    """One launch per destination count: every m of PIECE_COUNTS with mixed piece lengths (m = 64, 65, 1000 with long pieces too, so that
    the 16-byte path and the byte path alternate), each with the three ends, plus 0..k-1 bytes beyond the elements; r0 > 0, and segments that
    span several periods wherever the destination is longer than a period.  Then (`alignments`) each of the three alignments through all 16
    values with the other two random, on two tiles and a little."""
    for elems in counts:
        spec = []
        for m in PIECE_COUNTS:
            for end_mode in range(3):
                for long in (0, 16 * k * 20):
                    pieces = piece_list(rng, m, k, long)
                    nbytes = elems * k + (int(rng.integers(0, k)) if elems else 0)
                    spec.append(_seg(rng, pieces, k, has_base, nbytes, end_mode))
        yield spec
    if not alignments:
        return
    spec = []
    for which in range(3):
        for al16 in range(16):
            al = [_r16(rng), _r16(rng), _r16(rng)]
            al[which] = al16
            pieces = piece_list(rng, 7, k, 16 * k * int(rng.integers(2, 30)))
            seg = _seg(rng, pieces, k, has_base, (2 * TILE + int(rng.integers(1, 300))) * k + int(rng.integers(0, k)), al16 % 3)
            spec.append((*al, *seg[3:]))
    yield spec


def _seg(rng, pieces, k, has_base, nbytes, end_mode, **kw):
    n, rel, stride, q0, r0 = place(rng, pieces, k, nbytes, end_mode, **kw)
    return (_r16(rng), _r16(rng), _r16(rng), n, k, has_base, rel, stride, q0, r0, nbytes, pieces)


def mixed_spec_select(rng):
    """One launch that holds select segments, uniform lists (a strided byte set that reaches the select kernel), clipped (a share inside one
    piece) and whole (one piece that is the chunk) segments of every k, with and without a base."""
    spec = []
    for _ in range(2):
        for k in (1, 2, 4, 8):
            for has in (0, 1):
                spec.append(_seg(rng, piece_list(rng, int(rng.integers(2, 40)), k, 16 * k * 9), k, has, int(rng.integers(600, 9000)) * k + int(rng.integers(0, k)), int(rng.integers(0, 3))))
                run, gap = int(rng.integers(1, 50 * k)), int(rng.integers(1, 100))
                uniform = [(j * (run + gap), run) for j in range(5)]
                spec.append(_seg(rng, uniform, k, has, int(rng.integers(600, 9000)) * k, int(rng.integers(0, 3))))
                n = int(rng.integers(600, 9000)) * k + int(rng.integers(0, k))
                a, b = sorted(int(v) for v in rng.integers(0, n + 1, size=2))
                spec.append((_r16(rng), _r16(rng), _r16(rng), n, k, has, 0, n + 50, 0, a, b - a, [(0, n), (n + 7, 3)]))  # inside one piece: clipped (k = 1: plain)
                spec.append((_r16(rng), _r16(rng), _r16(rng), n, k, has, -5, n + 50, 0, 0, n, [(5, n), (n + 7, 3)]))  # one piece, the whole chunk
    return spec


def in_place_spec_select(rng, sizes=(17, 4079, 4081, 9000, 70_001)):
    return [_seg(rng, piece_list(rng, (3, 64, 5, 65, 2)[i], k, 16 * k * 12 if i % 2 else 0), k, 1, e * k + int(rng.integers(0, k)), i % 3) for k in (1, 2, 4, 8) for i, e in enumerate(sizes)]


@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("elems", DST_COUNTS)
def test_select_kernel_every_piece_count_and_end(emu, elems, k, has_base):
    rng = np.random.default_rng(900 + 100 * elems + 10 * k + has_base)
    for spec in sweep_specs_select(rng, k, has_base, counts=(elems,), alignments=False):
        select_case(emu.bz3_hip_debug_select, rng, spec, _host_alloc)


@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_select_kernel_every_alignment(emu, k, has_base):
    rng = np.random.default_rng(900 + 10 * k + has_base)
    for spec in sweep_specs_select(rng, k, has_base, counts=()):
        select_case(emu.bz3_hip_debug_select, rng, spec, _host_alloc)


def test_select_kernel_periods_and_first_bytes(emu):
    """Segments that start at byte 0 and at the last byte of a period, at a large q0 with a negative rel, that span many short periods, and a
    period of more than 2^31 wanted bytes (the lane compares instead of dividing)."""
    rng = np.random.default_rng(91)
    spec = []
    for k in (1, 2, 4, 8):
        pieces = piece_list(rng, 3, k)
        L = total(pieces)
        for r0, q0 in ((0, 0), (L - 1, 0), (1, 2 ** 20), (L // 2, 7)):
            spec.append(_seg(rng, pieces, k, k % 4 == 0, 5000 * k + 1, int(rng.integers(0, 3)), r0=r0, q0=q0))
    select_case(emu.bz3_hip_debug_select, rng, spec, _host_alloc)
    # the long period: only the bytes around its end are in the chunk (rel moves them there)
    for k in (1, 4):
        big = [(0, 16 * k + 3), (16 * k + 9, 2 ** 31 + 5)]
        L, stride = total(big), 16 * k + 9 + 2 ** 31 + 5 + 2
        r0, nbytes = L - 40 * k, 40 * k + 16 * k + 3  # the end of piece 1, then piece 0 of the next period, whole
        f = chunk_bytes(0, stride, 0, r0, nbytes, big)
        rel = 3 * k - int(f[0])
        n = rel + int(f[-1]) + 1 + k
        select_case(emu.bz3_hip_debug_select, rng, [(_r16(rng), _r16(rng), _r16(rng), n, k, 1, rel, stride, 0, r0, nbytes, big)], _host_alloc)


def test_select_kernel_mixed_segments_in_one_launch(emu):
    rng = np.random.default_rng(92)
    select_case(emu.bz3_hip_debug_select, rng, mixed_spec_select(rng), _host_alloc)
    select_case(emu.bz3_hip_debug_select, rng, [], _host_alloc)


def test_select_kernel_in_place(emu):
    rng = np.random.default_rng(93)
    select_case(emu.bz3_hip_debug_select, rng, in_place_spec_select(rng), _host_alloc, in_place=True)


def test_debug_select_rejects_bad_arguments(emu):
    buf = _buf(b"", 256)
    call = emu.bz3_hip_debug_select
    pieces = [(3, 2), (11, 4), (20, 0), (21, 1)]  # L = 7, the last piece ends at 22
    pc = (C.c_uint64 * 8)(*[v for p in pieces for v in p])
    assert call(buf, buf, buf, None, -1, pc, 4) == INIT
    assert call(buf, buf, buf, None, 0, pc, 4) == 0
    ok = (0, 0, 128, 100, 2 | 0x100, 0, 30, 0, 1, 15, 0, 4)  # r0 = 1: bytes 4, 11..14, 21, 33, 34, 41.., the last one c(14) = 60 + 4 = 64
    assert int(chunk_bytes(0, 30, 0, 1, 15, pieces)[-1]) == 64
    one = lambda *t: call(buf, buf, buf, (C.c_uint64 * 12)(*t), 1, pc, 4)  # noqa: E731
    for mode in (0, 2, 3 | 0x100, 16 | 0x100, 2 | 0x300, 2 | 0x900):  # the split direction, bad element sizes, stray bits
        assert one(*ok[:4], mode, *ok[5:]) == INIT
    for length in (64, 10, 0, 2 ** 31):  # the last chunk byte is not below len; len >= 2^31
        assert one(*ok[:3], length, *ok[4:]) == INIT
    for rel, stride, q0, r0, nbytes, first, m in ((2 ** 64 - 5, 30, 0, 1, 15, 0, 4),  # c(0) < 0
                                                  (0, 21, 0, 1, 15, 0, 4),  # the list runs past the stride and the segment spans two periods
                                                  (0, 30, 0, 7, 15, 0, 4),  # r0 >= L
                                                  (0, 30, 2 ** 63, 1, 15, 0, 4), (0, U64, 1, 1, 15, 0, 4),  # c does not fit
                                                  (0, 30, 0, 1, 15, 1, 4), (0, 30, 0, 1, 15, 5, 0),  # pieces beyond the array
                                                  (0, 30, 0, 0, 1, 2, 1), (0, 30, 0, 0, 1, 0, 0)):  # L == 0 with nbytes > 0
        assert one(*ok[:5], rel, stride, q0, r0, nbytes, first, m) == INIT, (rel, stride, q0, r0, nbytes, first, m)
    for bad in ([(3, 2), (4, 4)], [(11, 4), (3, 2)], [(3, U64 - 1), (U64, 0)]):  # overlapping, descending, s + l overflows
        assert call(buf, buf, buf, (C.c_uint64 * 12)(*ok[:10], 0, 2), 1, (C.c_uint64 * 4)(*[v for p in bad for v in p]), 2) == INIT, bad
    assert call(buf, buf, buf, (C.c_uint64 * 12)(*ok), 1, None, 4) == INIT
    assert bytes(buf) == bytes(256)
    assert call(buf, None, buf, (C.c_uint64 * 12)(0, NO_BASE, 128, 65, *ok[4:]), 1, pc, 4) == 0  # (the last byte is the chunk's last)
    assert one(*ok[:9], 0, 0, 0) == 0  # nbytes == 0: nothing else of the tuple is looked at but its list


# ---- frames -------------------------------------------------------------------------------------------------------------------
def want_select(case, offset, stride, count, pieces, cap):
    """The bytes the contract asks for: full[phi(t)] for t < w with phi(t) < T."""
    w = min(cap, count * total(pieces))
    if w == 0:
        return b""
    idx = phi(offset, stride, pieces, w)
    assert bool(np.all(np.diff(idx) > 0))
    return bytes(np.frombuffer(case.full, dtype=np.uint8)[idx[idx < case.T]])


def index_base(case, offset, stride, count, pieces, cap):
    """The base's bytes of the index set, in output order (zeros where phi(t) runs past T)."""
    if case.base is None:
        return None
    w = min(cap, count * total(pieces))
    if w == 0:
        return b"\0"
    idx = phi(offset, stride, pieces, w)
    padded = np.concatenate([np.frombuffer(case.base, dtype=np.uint8), np.zeros(int(idx.max()) + 1, dtype=np.uint8)])
    return bytes(padded[idx])


def _pieces_arg(pieces):
    return (C.c_uint64 * max(1, 2 * len(pieces)))(*[v for p in pieces for v in p])


def select_call(lib, k, frame, offset, stride, count, pieces, cap, base=None, in_place=False, room=None, alloc=_buf):
    """(rc, *out_size, the bytes of out[0, room + GUARD) after the call, what they were before).  base: the base's bytes of the index set."""
    room = (min(cap, count * total(pieces)) if room is None else room) + GUARD
    before = (bytes(base) + b"\xa5" * room)[:room] if in_place else b"\xa5" * room
    out = alloc(before)
    b = out if in_place else None if base is None else alloc(base)
    osz = C.c_size_t(cap)
    rc = lib.bz3_hip_decompress_device_select(k, alloc(frame), len(frame), offset, stride, count, len(pieces), _pieces_arg(pieces), b,
                                              0 if base is None else room - GUARD if in_place else len(base), out, C.byref(osz))
    return rc, osz.value, bytes(out)[:room], before


def check_select(lib, case, offset, stride, count, pieces, cap=None, in_place=False, call=select_call):
    cap = count * total(pieces) if cap is None else cap
    base = index_base(case, offset, stride, count, pieces, cap)
    rc, r, got, before = call(lib, case.k, case.frame, offset, stride, count, pieces, cap, base, in_place and base is not None)
    want = want_select(case, offset, stride, count, pieces, cap)
    assert (rc, r) == (0, len(want)), (offset, stride, count, pieces[:4], cap, rc, r, len(want))
    assert got[:r] == want, ("bytes differ", offset, stride, count, pieces[:4], cap)
    assert got[r:] == before[r:], ("wrote beyond the index set", offset, stride, count, pieces[:4], cap)


def frame_requests(case):
    """(offset, stride, count, pieces, *out_size or None).  Chunk 4 is the short one: what needs no full chunk is asked of it, because a full
    chunk costs the emulator about a second."""
    s, bs, T = case.starts, case.bs, case.T
    yield 10, 0, 1, [(s[j] + 100 + j, 50 + j) for j in range(5)] + [(s[4] + 700, 1), (s[4] + 702, 33)], None  # pieces in every chunk; one period longer than the frame (its stride is not looked at)
    yield s[4] + 3, 100, 10, [(0, 5), (7, 1), (20, 33), (60, 40)], None  # a period shorter than a chunk; its last piece touches the next period's first
    yield 50, 4 * bs, 2, [(0, 100), (2 * bs + 10, 60), (3 * bs, 0)], None  # chunk 1 in a gap inside a period, chunk 3 between two periods; past T in the end
    yield s[4] - 30, 300, 3, [(0, 60), (100, 17)], None  # a piece across a chunk boundary, and more behind it
    for cap in (400 - 23, 170, 200, 30, 50, 51):  # *out_size inside a piece, at a piece end, at a period end, inside and at the end of the first piece, one beyond
        yield s[4] + 7, 300, 4, [(0, 50), (60, 20), (100, 30)], cap
    yield T - 700, 500, 3, [(0, 100), (200, 150)], None  # past T: short
    yield T + 5, 50, 4, [(0, 10), (20, 10)], None  # wholly past T
    yield 5, 9, 4, [], None  # m == 0
    yield 5, 9, 4, [(5, 0), (9, 0)], None  # L == 0
    yield 5, 9, 0, [(0, 2), (5, 2)], None  # count == 0


@pytest.mark.parametrize("with_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("bs", [BS, BS + 3])
def test_select_requests_of_a_frame_match_the_reference(emu, bs, k, with_base, monkeypatch):
    """Four full blocks of 65 KiB (65 KiB + 3: every block starts inside an element and has a tail) and a short one; windows of two chunks."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    case = Case(require_ref().lib, bs, k, with_base, stream_for(bs, blocks=4))
    assert len(case.sizes) == 5 and case.sizes[:4] == [bs] * 4
    for offset, stride, count, pieces, cap in frame_requests(case):
        check_select(emu, case, offset, stride, count, pieces, cap)
    if with_base:
        check_select(emu, case, case.starts[4] + 5, 200, 5, [(0, 60), (61, 3), (100, 64)], in_place=True)


def test_requests_that_normalise_to_one_piece_are_the_strided_call(emu, monkeypatch):
    """Bytes, rc and *out_size of the strided call, for a good frame and for one with a corrupt chunk: a single piece, neighbours that join
    to one, lists with empty pieces; count == 1 with several pieces is the concatenation of its range calls."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    bs = BS + 3
    case = Case(require_ref().lib, bs, 4, 1, stream_for(bs, blocks=2))
    s = case.starts
    for frame in (case.frame, _flip(case.frame, 1)):
        # (offset, stride, count, pieces, *out_size), the strided request (offset, run, stride, count) it is
        for (offset, stride, count, pieces, cap), strided in (((s[2] - 50, 300, 3, [(7, 100)], 10 ** 9), (s[2] - 43, 100, 300, 3)),  # a single piece
                                                              ((s[2] - 48, 100, 7, [(0, 30), (30, 50), (80, 20)], 10 ** 9), (s[2] - 48, 100, 100, 7)),  # neighbours that join (and fill the period)
                                                              ((s[2] - 48, 40, 14, [(3, 0), (5, 4), (9, 6), (15, 0), (39, 0)], 101), (s[2] - 43, 10, 40, 14)),  # both, *out_size inside a run
                                                              ((case.T - 10, 8, 4, [(0, 0), (0, 8)], 64), (case.T - 10, 8, 8, 4)),  # past T
                                                              ((s[2] + 1, 7, 1, [(2, 300)], 10 ** 9), (s[2] + 3, 300, 7, 1)), ((0, 16, 0, [(0, 16)], 64), (0, 16, 16, 0)),
                                                              ((s[2] - 20, 500, 3, [(0, 100), (200, 50)], 64), (s[2] - 20, 100, 500, 3))):  # *out_size leaves the first piece alone
            w = min(cap, count * total(pieces))
            base = index_base(case, offset, stride, count, pieces, cap)
            got = select_call(emu, 4, frame, offset, stride, count, pieces, cap, base, room=w)
            ref = strided_call(emu, 4, frame, *strided, cap, base, room=w)
            assert got == ref, (offset, stride, count, pieces, cap, got[:2], ref[:2])
        pieces = [(s[2] - 40, 100), (s[2] + 200, 7), (s[2] + 300, 64)]
        base = index_base(case, 3, 0, 1, pieces, 10 ** 9)
        rc, r, got, before = select_call(emu, 4, frame, 3, 0, 1, pieces, 10 ** 9, base)
        cat, at, code = b"", 0, 0
        for a, l in pieces:
            prc, pr, pgot, _ = range_call(emu, 4, frame, 3 + a, l, base[at : at + l])
            cat += pgot[:pr]
            at += l
            if prc != 0:
                code = prc
                break
        assert (rc, r) == (code, len(cat)) and got[:r] == cat and got[r:] == before[r:], (rc, r, code, len(cat))


# ---- skipping is real -----------------------------------------------------------------------------------------------------------
def committed_below(offset, stride, pieces, w, p):
    """The number of t < w with phi(t) < p."""
    return int((phi(offset, stride, pieces, w) < p).sum())


def test_corrupt_chunks_in_the_gaps_are_skipped_and_needed_ones_commit_a_prefix(emu, monkeypatch):
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    ref = require_ref().lib
    bs = BS + 3
    case = Case(ref, bs, 2, 1, stream_for(bs, blocks=2))
    s = case.starts
    offset, stride, count, pieces = 100, 2 * bs, 2, [(0, 500), (600, 700)]  # chunks 0 and 2 (the short one cuts the second period); chunk 1 lies in the gap between the periods
    w = count * total(pieces)
    base = index_base(case, offset, stride, count, pieces, w)
    good = want_select(case, offset, stride, count, pieces, w)
    assert 1200 < len(good) < w
    bad = _flip(case.frame, 1)  # a corrupt payload in a gap is not noticed
    assert range_call(emu, 2, bad, s[1], 50, base[:50])[0] != 0, "the flipped chunk must fail where it is decoded"
    rc, r, got, before = select_call(emu, 2, bad, offset, stride, count, pieces, w, base)
    assert (rc, r) == (0, len(good)) and got[:r] == good and got[r:] == before[r:]
    for j in (0, 2):  # in a needed chunk: its code, and exactly the bytes with phi(t) < p_j
        rc, r, got, before = select_call(emu, 2, _flip(case.frame, j), offset, stride, count, pieces, w, base)
        assert rc != 0 and r == committed_below(offset, stride, pieces, w, s[j]) == (j // 2) * 1200, (j, rc, r)
        assert got[:r] == good[:r] and got[r:] == before[r:], j
    for j in range(3):  # a corrupt header, in a gap too, is reported after the bytes before it are committed
        rc, r, got, before = select_call(emu, 2, _with_header(case.frame, j, orig=-5), offset, stride, count, pieces, w, base)
        assert rc == MALFORMED and r == committed_below(offset, stride, pieces, w, s[j]) == ((j + 1) // 2) * 1200, (j, rc, r)
        assert got[:r] == good[:r] and got[r:] == before[r:], j
    # a gap between two pieces of ONE period: chunk 1 again, and a failing chunk 2 commits the first piece alone
    pieces = [(0, 500), (2 * bs + 10, 300)]
    w = total(pieces)
    base = index_base(case, offset, 0, 1, pieces, w)
    good = want_select(case, offset, 0, 1, pieces, w)
    rc, r, got, before = select_call(emu, 2, bad, offset, 0, 1, pieces, w, base)
    assert (rc, r) == (0, 800) and got[:r] == good and got[r:] == before[r:]
    rc, r, got, before = select_call(emu, 2, _flip(case.frame, 2), offset, 0, 1, pieces, w, base)
    assert rc != 0 and r == 500 and got[:r] == good[:r] and got[r:] == before[r:]
    # a header at or beyond `end` is never read
    small = [(0, 100), (150, 50)]
    rc, r, got, before = select_call(emu, 2, _with_header(case.frame, 1, orig=-5), offset, 300, 3, small, 450, index_base(case, offset, 300, 3, small, 450))
    assert (rc, r) == (0, 450) and got[:r] == want_select(case, offset, 300, 3, small, 450) and got[r:] == before[r:]


def test_select_calls_decode_a_chunk_once_however_many_pieces_it_holds(emu, monkeypatch):
    """Five chunks.  Pieces in chunks 0, 2 and 4 with windows of two chunks: 2 CM launches, the full decode takes 3.  Windows of one chunk:
    three pieces in chunk 1 and one in chunk 3 take 2 launches; the same four pieces as four range entries of one _many call take 4."""
    ref = require_ref().lib
    case = Case(ref, BS, 1, 0, stream_for(BS, blocks=4))
    assert len(case.sizes) == 5
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    emu.bz3_hip_debug_cm_launches(1)
    check_select(emu, case, 10, 0, 1, [(0, 100), (2 * BS + 5, 100), (4 * BS, 100)])
    assert emu.bz3_hip_debug_cm_launches(1) == 2
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "1")
    pieces = [(BS + 10, 100), (BS + 500, 64), (2 * BS - 300, 200), (3 * BS + 7, 100)]
    check_select(emu, case, 0, 0, 1, pieces)
    assert emu.bz3_hip_debug_cm_launches(1) == 2
    n = len(pieces)
    ins, outs = [_buf(case.frame) for _ in pieces], [_buf(b"", l) for _, l in pieces]
    out_sizes, rcs = (C.c_size_t * n)(*[l for _, l in pieces]), (C.c_int * n)()
    assert emu.bz3_hip_decompress_device_range_many(n, None, _vp(ins), (C.c_size_t * n)(*[len(case.frame)] * n), (C.c_uint64 * n)(*[a for a, _ in pieces]), None, None, _vp(outs),
                                                    out_sizes, rcs) == 0
    assert b"".join(bytes(o) for o in outs) == want_select(case, 0, 0, 1, pieces, 10 ** 9)
    assert emu.bz3_hip_debug_cm_launches(1) == 4


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_invalid_piece_lists_and_partial_overlap_are_refused_before_any_write(emu):
    case = Case(require_ref().lib, BS + 3, 4, 1, stream_for(BS + 3, blocks=1))
    for offset, stride, count, pieces in ((0, 100, 2, [(0, 10), (5, 10)]), (0, 100, 2, [(20, 10), (0, 10)]), (0, 100, 1, [(0, 10), (9, 0)]),  # overlapping, descending
                                          (0, 25, 2, [(0, 10), (20, 6)]), (0, 0, 2, [(0, 1), (2, 1)]),  # the last piece past the stride with count > 1
                                          (0, 100, 2, [(0, 10), (200, 0)]), (U64 - 50, 20, 1, [(0, 5), (60, 0)]),  # ... an empty last piece counts as given: past the stride, past 2^64
                                          (0, 2 ** 40, 2, [(5, U64 - 3), (U64, 0)]), (0, U64, 2, [(0, 2 ** 63), (2 ** 63 + 1, 2 ** 63 - 2)]),  # s + l; L fits, count L does not
                                          (0, 2 ** 34, 2 ** 31, [(0, 2 ** 32), (2 ** 33, 2 ** 32)]),  # count L
                                          (U64 - 50, 20, 4, [(0, 5), (10, 5)]), (U64 - 5, 20, 1, [(0, 2), (4, 2)]), (5, U64 // 2, 4, [(0, 1), (2, 1)])):  # the last byte
        rc, r, got, before = select_call(emu, 4, case.frame, offset, stride, count, pieces, 64, room=64)
        assert (rc, r) == (INIT, 0) and got == before, (offset, stride, count, pieces)
    rc, r, got, before = select_call(emu, 3, case.frame, 0, 100, 2, [(0, 10), (20, 10)], 64, room=64)  # a bad element size
    assert (rc, r) == (INIT, 0) and got == before
    out, osz = _buf(b"\xa5" * 64), C.c_size_t(64)
    assert emu.bz3_hip_decompress_device_select(4, _buf(case.frame), len(case.frame), 0, 100, 2, 2, None, None, 0, out, C.byref(osz)) == INIT  # NULL pieces with m > 0
    assert osz.value == 0 and bytes(out) == b"\xa5" * 64
    assert emu.bz3_hip_decompress_device_select(4, _buf(case.frame), len(case.frame), 0, 100, 2, 0, None, None, 0, out, C.byref(osz)) == 0  # m == 0: the header alone
    assert osz.value == 0 and bytes(out) == b"\xa5" * 64
    assert select_call(emu, 4, case.frame, 0, 5, 1, [(0, 10), (20, 10)], 64, room=64)[:2] == (0, 20)  # count == 1: a stride below the list's end is no violation
    assert select_call(emu, 4, case.frame, U64, 0, 7, [(U64, 0)], 64, room=64)[:2] == (0, 0)  # L == 0: nothing else of the request is looked at
    for pieces in ([], [(3, 0)]):
        assert select_call(emu, 4, case.frame[:12], 0, 20, 2, pieces, 64, room=64)[:2] == (MALFORMED, 0)  # ... but the frame header
        assert select_call(emu, 4, b"XZ3v1" + case.frame[5:], 0, 20, 2, pieces, 64, room=64)[:2] == (MALFORMED, 0)
    # out overlaps the base without being it: BZ3_ERR_INIT, nothing written; the overlap is judged on w = count * L = 1000 bytes
    arena = _buf(b"\xa5" * 4096)
    pieces = [(0, 60), (100, 40)]
    sl = index_base(case, 0, 300, 10, pieces, 1000)
    C.memmove(arena, sl, 1000)
    before = bytes(arena)
    for off in (1, 16, 999):
        osz = C.c_size_t(4000)
        assert emu.bz3_hip_decompress_device_select(4, _buf(case.frame), len(case.frame), 0, 300, 10, 2, _pieces_arg(pieces), arena, 4000, C.byref(arena, off), C.byref(osz)) == INIT
        assert bytes(arena) == before and osz.value == 0
    osz = C.c_size_t(4000)
    assert emu.bz3_hip_decompress_device_select(4, _buf(case.frame), len(case.frame), 0, 300, 10, 2, _pieces_arg(pieces), arena, 4000, C.byref(arena, 1000), C.byref(osz)) == 0  # adjacent: fine
    assert osz.value == 1000 and bytes(arena)[1000:2000] == want_select(case, 0, 300, 10, pieces, 1000) and bytes(arena)[:1000] == sl


# ---- many -----------------------------------------------------------------------------------------------------------------------
def many_call(lib, ks, frames, params, lists, caps, bases, in_place):
    """Per frame (rc, *out_size, out[0, w + GUARD) after, before).  params[i] = (offset, stride, count); bases[i]: None or the base's bytes
    of the index set."""
    n = len(frames)
    ws = [min(c, p[2] * total(l)) for c, p, l in zip(caps, params, lists)]
    ins = [_buf(f) for f in frames]
    befores = [((bytes(bases[i]) + b"\xa5" * (ws[i] + GUARD))[: ws[i] + GUARD]) if in_place[i] else b"\xa5" * (ws[i] + GUARD) for i in range(n)]
    outs = [_buf(b) for b in befores]
    bbufs = [outs[i] if in_place[i] else None if bases[i] is None else _buf(bases[i]) for i in range(n)]
    out_sizes, rcs = (C.c_size_t * n)(*caps), (C.c_int * n)(*([77] * n))
    bp = (C.c_void_p * n)(*[None if b is None else C.addressof(b) for b in bbufs])
    bsz = (C.c_size_t * n)(*[0 if bases[i] is None else ws[i] if in_place[i] else len(bases[i]) for i in range(n)])
    arrs = [_pieces_arg(l) for l in lists]
    pp = (C.POINTER(C.c_uint64) * n)(*[C.cast(a, C.POINTER(C.c_uint64)) if l else None for a, l in zip(arrs, lists)])
    rc = lib.bz3_hip_decompress_device_select_many(n, None if ks is None else (C.c_uint32 * n)(*ks), _vp(ins), (C.c_size_t * n)(*map(len, frames)),
                                                   (C.c_uint64 * (4 * n))(*[v for p, l in zip(params, lists) for v in (*p, len(l))]), pp, bp, bsz, _vp(outs), out_sizes, rcs)
    return rc, [(rcs[i], out_sizes[i], bytes(outs[i])[: ws[i] + GUARD], befores[i]) for i in range(n)]


def test_many_select_requests_equal_their_single_calls(emu, monkeypatch):
    """Piece lists, requests that normalise to a strided, a contiguous and an empty one, element sizes and bases (none, separate, in place)
    in one call at windows of three chunks, so that one launch gathers select, strided and clipped segments; one frame given twice with
    two different index sets; then the same with one frame corrupt: no other frame's result changes."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    ref = require_ref().lib
    bs = BS + 3
    cases = [Case(ref, bs, k, wb, stream_for(bs, blocks=nb, last=last), seed=290 + i) for i, (k, wb, nb, last) in enumerate(((2, 1, 1, 777), (1, 0, 0, 50), (8, 1, 2, 1234), (4, 0, 0, 100)))]
    # (case, (offset, stride, count), pieces, *out_size, in place)
    plan = [(0, (bs - 30, 200, 3), [(0, 40), (41, 19), (100, 7)], 10 ** 6, 0), (1, (0, 10, 5), [(0, 4), (4, 6)], 10 ** 6, 0), (2, (10, 2 * bs, 2), [(0, 3000), (4000, 2000)], 10 ** 6, 1),
            (2, (2 * bs + 7, 128, 20), [(0, 16), (20, 30), (64, 18)], 64 * 20 - 9, 0), (3, (7, 11, 9), [(0, 2), (3, 1), (5, 2)], 10 ** 6, 0), (0, (5, 9, 9), [], 50, 0),
            (0, (bs + 1, 300, 4), [(2, 3), (5, 0), (9, 60)], 10 ** 6, 1), (3, (3, 20, 4), [(1, 8)], 10 ** 6, 0)]
    ks = [cases[c].k for c, *_ in plan]
    frames = [cases[c].frame for c, *_ in plan]
    params = [p for _, p, *_ in plan]
    lists = [l for _, _, l, *_ in plan]
    caps = [cap for *_, cap, _ in plan]
    in_place = [bool(ip) for *_, ip in plan]
    bases = [index_base(cases[c], *p, l, cap) for c, p, l, cap, _ in plan]
    rc, got = many_call(emu, ks, frames, params, lists, caps, bases, in_place)
    assert rc == 0
    for i, (c, p, l, cap, ip) in enumerate(plan):
        want = want_select(cases[c], *p, l, cap)
        assert got[i][:2] == (0, len(want)) and got[i][2][: len(want)] == want and got[i][2][len(want) :] == got[i][3][len(want) :], i
        assert got[i][:3] == select_call(emu, ks[i], frames[i], *p, l, cap, bases[i], in_place[i])[:3], ("single call", i)
    frames2 = list(frames)
    frames2[2] = frames2[3] = _flip(frames[2], 2)  # chunk 2 holds the second period of frame 2 and every piece of frame 3
    rc2, got2 = many_call(emu, ks, frames2, params, lists, caps, bases, in_place)
    assert rc2 == got2[2][0] != 0 and got2[2][1] == 5000 and (got2[3][0], got2[3][1]) == (got2[2][0], 0)
    for i in (2, 3):
        assert got2[i][:3] == select_call(emu, ks[i], frames2[i], *params[i], lists[i], caps[i], bases[i], in_place[i])[:3]
    assert [g for i, g in enumerate(got2) if i not in (2, 3)] == [g for i, g in enumerate(got) if i not in (2, 3)]


def test_many_whole_call_errors(emu):
    ref = require_ref().lib
    frame = _ref_compress(ref, BS, b"abcdefgh" * 100)[1]

    def call(ks=(1, 1), n=2, params=((0, 8, 50), (1, 8, 50)), lists=([(0, 1), (2, 1)], [(0, 2), (5, 1)]), null_params=False, null_pieces=False, null_list=False):
        ins = [_buf(frame), _buf(frame)]
        outs = [_buf(b"\xa5" * 300), _buf(b"\xa5" * 300)]
        out_sizes, rcs = (C.c_size_t * 2)(300, 300), (C.c_int * 2)(77, 77)
        arrs = [_pieces_arg(l) for l in lists]
        pp = (C.POINTER(C.c_uint64) * 2)(C.cast(arrs[0], C.POINTER(C.c_uint64)), None if null_list else C.cast(arrs[1], C.POINTER(C.c_uint64)))
        rc = emu.bz3_hip_decompress_device_select_many(n, None if ks is None else (C.c_uint32 * 2)(*ks), _vp(ins), (C.c_size_t * 2)(len(frame), len(frame)),
                                                       None if null_params else (C.c_uint64 * 8)(*[v for p, l in zip(params, lists) for v in (*p, len(l))]),
                                                       None if null_pieces else pp, None, None, _vp(outs), out_sizes, rcs)
        return rc, list(rcs), list(out_sizes), [bytes(o) for o in outs]

    untouched = [b"\xa5" * 300] * 2
    assert call() == (0, [0, 0], [100, 150], [b"ac" * 50 + b"\xa5" * 200, b"bcg" * 50 + b"\xa5" * 150])
    assert call(ks=None)[:3] == (0, [0, 0], [100, 150])  # elem_sizes == NULL: 1 for every frame
    assert call(ks=(1, 3)) == (INIT, [INIT, INIT], [0, 0], untouched)  # a bad element size
    assert call(lists=([(0, 1), (2, 1)], [(0, 2), (1, 1)])) == (INIT, [INIT, INIT], [0, 0], untouched)  # one invalid list fails the whole call
    assert call(null_params=True) == (INIT, [INIT, INIT], [0, 0], untouched)
    assert call(null_pieces=True) == (INIT, [INIT, INIT], [0, 0], untouched)
    assert call(null_list=True) == (INIT, [INIT, INIT], [0, 0], untouched)
    assert call(lists=([(0, 1), (2, 1)], []), null_list=True)[:3] == (0, [0, 0], [100, 0])  # m == 0: its list is not looked at
    assert call(n=-1)[0] == INIT
    assert emu.bz3_hip_decompress_device_select_many(0, None, None, None, None, None, None, None, None, None, None) == 0
    assert emu.bz3_hip_decompress_device_select_many(2, None, None, None, None, None, None, None, None, None, None) == INIT


@pytest.mark.parametrize("window", [2, 8])
def test_one_call_holds_every_request_form(emu, window, monkeypatch):
    """Five frames of element size 4 in one _many call, two of them with a base: a one-run range, the whole tensor, a two-run strided request,
    a two-piece select request and a select request with w <= l_0.  Every frame is a full block of 65 KiB + 3 and a short one, and every
    request but the whole tensor lies in the short chunk.  Windows of two chunks gather (clipped, whole), (whole, strided) and (select,
    clipped) in one launch each; a window of eight gathers all six chunks, so that ONE launch holds whole, clipped, strided and select
    segments side by side, each with the parameters of its own kind.  Every output is the numpy slice full[phi(t)] of the reference decode."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", str(window))
    ref = require_ref().lib
    bs = BS + 3
    plain, based = (Case(ref, bs, 4, wb, stream_for(bs, blocks=1, last=6001), seed=310 + wb) for wb in (0, 1))
    assert plain.sizes == [bs, 6001]
    # (case, (offset, stride, count), pieces, *out_size)
    plan = [(based, (bs + 10, 0, 1), [(0, 777)], 10 ** 6),  # one run inside chunk 1
            (plain, (0, 0, 1), [(0, plain.T)], 10 ** 6),  # the whole tensor: both chunks, whole
            (plain, (bs + 5, 1000, 2), [(3, 401)], 10 ** 6),  # two runs
            (based, (bs + 100, 2000, 2), [(0, 300), (650, 130)], 10 ** 6),  # two pieces
            (plain, (bs + 9, 900, 3), [(4, 500), (600, 100)], 333)]  # w <= l_0: the range (offset + 4, 333)
    params, lists, caps = [p for _, p, _, _ in plan], [l for *_, l, _ in plan], [cap for *_, cap in plan]
    bases = [index_base(c, *p, l, cap) for c, p, l, cap in plan]
    rc, got = many_call(emu, [4] * len(plan), [c.frame for c, *_ in plan], params, lists, caps, bases, [False] * len(plan))
    assert rc == 0
    for i, (c, p, l, cap) in enumerate(plan):
        want = want_select(c, *p, l, cap)
        assert len(want) == min(cap, p[2] * total(l)) > 0, i
        assert got[i][:2] == (0, len(want)), (i, got[i][:2])
        assert got[i][2][: len(want)] == want, ("bytes differ", i)
        assert got[i][2][len(want) :] == got[i][3][len(want) :], ("wrote beyond the request", i)
