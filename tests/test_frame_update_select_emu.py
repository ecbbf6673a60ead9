"""CPU tests of the index update (include/bz3_hip.h bz3_hip_update_device_select[_many], the select split of bzip3_amd/csrc/planes.hpp through
bz3_hip_debug_patch_select, update_frames of api_frames.hip with a request per frame) under the fiber emulation of the HIP execution model
(tests/emu).

The oracle of an update is always the reference's frame of the updated bytes: f' == bz3_compress(bs, S(D(x'))), with S, D and phi written in numpy
from their definitions (test_frame_planes_emu, test_frame_delta_emu, test_frame_select_emu), never the library under test.  The oracle of the
kernel is the numpy model select_patch_model of the formula in planes.hpp ("Select split"), applied to a slot that starts as random bytes.

BZ3_EMU_LIB=<path> runs the module on another build of the emulator library, as test_frame_update_emu does."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bzip3_amd
from oracle_lib import require_ref
from test_frame_delta_emu import NO_BASE, D, D_inv, _buf, _chunks, _host_alloc, _r16, _with_chunk
from test_frame_planes_emu import BS, _ref_decompress, _vp
from test_frame_range_emu import TILE, U64, _flip, _with_header
from test_frame_select_emu import DST_COUNTS, PIECE_COUNTS, _pieces_arg, _seg, chunk_bytes, phi, piece_list, total
from test_frame_update_emu import FILL, INIT, LAST, MALFORMED, TOO_BIG, Case, pattern, update_call

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu():
    if os.environ.get("BZ3_EMU_LIB"):
        return bzip3_amd._declare(C.CDLL(os.environ["BZ3_EMU_LIB"]))
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def select_patch_model(old, k, c, new):
    """The slot `old` (split_k of a chunk of len(old) bytes) after a select split: chunk byte c[u] gets new[u]; it lives at (c % k) m + c / k
    below m k and at c in the tail; every other byte as it was."""
    out = old.copy()
    m = len(old) // k
    out[np.where(c < m * k, (c % k) * m + c // k, c)] = new
    return out


def patch_select_case(call, rng, spec, alloc):
    """spec: (src, base, slot alignment mod 16, n, k, has base, rel, stride, q0, r0, nbytes, pieces) per segment (test_frame_select_emu._seg), one
    after the other with gaps: the slot has n bytes, src and base nbytes.  alloc(array) -> (object for the hook, address, numpy reader);
    call(src, base, dst, table, n, pieces, n_pieces) -> rc.  The slots and the guard bytes around them start as random bytes and the whole
    destination is compared against the model, the inputs against themselves."""
    room_s = sum(s[10] for s in spec) + 56 * len(spec) + 64
    room_d = sum(s[3] for s in spec) + 56 * len(spec) + 64
    src_np = rng.integers(0, 256, size=room_s, dtype=np.uint8)
    base_np = rng.integers(0, 256, size=room_s, dtype=np.uint8)
    dst_np = rng.integers(0, 256, size=room_d, dtype=np.uint8)
    src, base, dst = alloc(src_np), alloc(base_np), alloc(dst_np)
    want = dst_np.copy()
    table, flat, offs = [], [], [0, 0, 0]
    addrs = (src[1], base[1], dst[1])
    for a_s, a_b, a_d, n, k, has_base, rel, stride, q0, r0, nbytes, pieces in spec:
        for j, al in enumerate((a_s, a_b, a_d)):
            offs[j] += (al - (addrs[j] + offs[j])) % 16
        s, bo, d = offs
        table += [s, bo if has_base else NO_BASE, d, n, k, rel % 2 ** 64, stride, q0, r0, nbytes, len(flat) // 2, len(pieces)]
        flat += [v for p in pieces for v in p]
        if nbytes:
            c = chunk_bytes(rel, stride, q0, r0, nbytes, pieces)
            assert 0 <= int(c[0]) and int(c[-1]) < n and bool(np.all(np.diff(c) > 0))
            new = src_np[s : s + nbytes]
            want[d : d + n] = select_patch_model(dst_np[d : d + n], k, c, D(new, base_np[bo : bo + nbytes]) if has_base else new)
        offs[0] += nbytes + int(rng.integers(1, 40))
        offs[1] += nbytes + int(rng.integers(1, 40))
        offs[2] += n + int(rng.integers(1, 40))  # guard bytes between the slots
    assert max(offs[:2]) <= room_s - 16 and offs[2] <= room_d - 16
    t = (C.c_uint64 * max(1, len(table)))(*table)
    pc = (C.c_uint64 * max(1, len(flat)))(*flat)
    assert call(src[0], base[0], dst[0], t, len(table) // 12, pc, len(flat) // 2) == 0
    bad = np.nonzero(dst[2]() != want)[0]
    assert bad.size == 0, ("bytes differ at", bad[:8], [table[12 * i : 12 * i + 12] for i in range(len(spec)) if any(table[12 * i + 2] <= b < table[12 * i + 2] + table[12 * i + 3] for b in bad[:8])][:2])
    assert np.array_equal(src[2](), src_np) and np.array_equal(base[2](), base_np), "an input was written"


def sweep_specs_patch_select(rng, k, has_base, counts=DST_COUNTS, alignments=True):
    """One launch per source count (DST_COUNTS elements of k bytes, plus 0..k-1 bytes): every m of PIECE_COUNTS with piece lengths below, at and
    above 16 elements mixed within the list, lengths that are no multiple of k among them (m = 64, 65, 1000 with long pieces too, so that the
    16-element path and the byte path alternate), each with the three ends: the last byte is the chunk's last without a tail, the one before its
    last, inside its tail of len % k bytes.  r0 > 0, q0 > 0 and several periods wherever the source is longer than a period.  Then (`alignments`)
    each of the three alignments through all 16 values with the other two random, on two tiles and a little."""
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


def mixed_spec_patch_select(rng):
    """One launch that holds select splits, uniform lists, clipped splits (a share inside one piece) and whole splits (one piece that is the
    chunk) at every k, with and without a base."""
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


def periods_spec_patch_select(rng):
    """Segments that start at byte 0 and at the last byte of a period, in the middle of a piece at a large q0 with a negative rel, and that span
    many short periods (three and more)."""
    spec = []
    for k in (1, 2, 4, 8):
        pieces = piece_list(rng, 3, k)
        L = total(pieces)
        for r0, q0 in ((0, 0), (L - 1, 0), (1, 2 ** 20), (L // 2, 7)):
            spec.append(_seg(rng, pieces, k, k % 4 == 0, 5000 * k + 1, int(rng.integers(0, 3)), r0=r0, q0=q0))
        three = [(0, 40 * k), (50 * k + 1, 16 * k), (90 * k, 3)]  # exactly three periods, the first entered in the middle of a piece
        spec.append(_seg(rng, three, k, 1, 2 * total(three) + 30 * k, 1, r0=10 * k + 1, q0=2))
    return spec


@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("elems", DST_COUNTS)
def test_select_split_every_piece_count_and_end(emu, elems, k, has_base):
    rng = np.random.default_rng(1100 + 100 * elems + 10 * k + has_base)
    for spec in sweep_specs_patch_select(rng, k, has_base, counts=(elems,), alignments=False):
        patch_select_case(emu.bz3_hip_debug_patch_select, rng, spec, _host_alloc)


@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_select_split_every_alignment(emu, k, has_base):
    rng = np.random.default_rng(1100 + 10 * k + has_base)
    for spec in sweep_specs_patch_select(rng, k, has_base, counts=()):
        patch_select_case(emu.bz3_hip_debug_patch_select, rng, spec, _host_alloc)


def test_select_split_periods_and_first_bytes(emu):
    rng = np.random.default_rng(111)
    patch_select_case(emu.bz3_hip_debug_patch_select, rng, periods_spec_patch_select(rng), _host_alloc)


def test_select_split_mixed_segments_in_one_launch(emu):
    rng = np.random.default_rng(112)
    patch_select_case(emu.bz3_hip_debug_patch_select, rng, mixed_spec_patch_select(rng), _host_alloc)
    patch_select_case(emu.bz3_hip_debug_patch_select, rng, [], _host_alloc)


def debug_patch_select_rejects(call):
    buf = _buf(b"", 256)
    pieces = [(3, 2), (11, 4), (20, 0), (21, 1)]  # L = 7, the last piece ends at 22
    pc = (C.c_uint64 * 8)(*[v for p in pieces for v in p])
    assert call(buf, buf, buf, None, -1, pc, 4) == INIT
    assert call(buf, buf, buf, None, 0, pc, 4) == 0
    ok = (0, 0, 128, 100, 2, 0, 30, 0, 1, 15, 0, 4)  # the last chunk byte is c(14) = 64
    assert int(chunk_bytes(0, 30, 0, 1, 15, pieces)[-1]) == 64
    one = lambda *t: call(buf, buf, buf, (C.c_uint64 * 12)(*t), 1, pc, 4)  # noqa: E731
    for mode in (0, 3, 16, 2 | 0x100, 2 | 0x200, 2 | 0x800):  # bad element sizes, the inverse bit, stray bits
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
    assert one(*ok[:9], 0, 0, 0) == 0  # nbytes == 0: nothing else of the tuple is looked at but its list
    assert bytes(buf) == bytes(256)


def test_debug_patch_select_rejects_bad_arguments(emu):
    debug_patch_select_rejects(emu.bz3_hip_debug_patch_select)


# ---- frames -------------------------------------------------------------------------------------------------------------------
def index_update(case, offset, stride, count, pieces, seed=9):
    """(data, the base's bytes of the index set or None, the frame the update must give, the phi(t) of the request)."""
    W = count * total(pieces)
    idx = phi(offset, stride, pieces, W) if W else np.zeros(0, dtype=np.int64)
    d2 = np.frombuffer(pattern(W, seed), dtype=np.uint8)
    d = np.frombuffer(case.d, dtype=np.uint8).copy()
    d[idx] = d2
    expect = case.expect(bytes(d))
    if case.base is None:
        return bytes(d2), None, expect, idx
    rows = np.frombuffer(case.base, dtype=np.uint8)[idx]
    return bytes(D_inv(d2, rows)), bytes(rows), expect, idx


def default_cap(lib, frame):
    return len(frame) + int.from_bytes(frame[9:13], "little") * lib.bz3_bound(BS)


def select_update_call(lib, k, frame, offset, stride, count, pieces, data, base=None, cap=None, alloc=_buf, w=None):
    """(rc, *out_size, out[0, cap) after the call).  base: the base's bytes of the index set."""
    cap = default_cap(lib, frame) if cap is None else cap
    out = alloc(bytes([FILL]) * cap)
    osz = C.c_size_t(cap)
    rc = lib.bz3_hip_update_device_select(k, alloc(frame), len(frame), offset, stride, count, len(pieces), _pieces_arg(pieces), alloc(data), len(data) if w is None else w,
                                          None if base is None else alloc(base), out, C.byref(osz))
    return rc, osz.value, bytes(out)[:cap]


def touched_chunks(case, idx):
    return sorted({j for j, (p, o) in enumerate(zip(case.starts, case.sizes)) if o > 0 and bool(np.any((idx >= p) & (idx < p + o)))})


def check_select_update(lib, case, offset, stride, count, pieces, frame=None, want=None, call=select_update_call):
    data, rows, expect, idx = index_update(case, offset, stride, count, pieces)
    rc, size, out = call(lib, case.k, case.frame if frame is None else frame, offset, stride, count, pieces, data, rows)
    want = expect if want is None else want(expect)
    assert (rc, size) == (0, len(want)), (offset, stride, count, pieces[:4], rc, size, len(want))
    assert out[:size] == want, ("frames differ", offset, stride, count, pieces[:4])
    assert out[size:] == bytes([FILL]) * (len(out) - size), ("wrote beyond the frame", offset, stride, count, pieces[:4])
    return out[:size], idx


def refused_select(lib, k, frame, offset, stride, count, pieces, data, code, base=None, cap=None, call=select_update_call, **kw):
    rc, size, out = call(lib, k, frame, offset, stride, count, pieces, data, base, cap, **kw)
    assert (rc, size) == (code, 0), (rc, size, code, offset, stride, count, pieces[:4])
    assert out == bytes([FILL]) * len(out), "a refused call wrote to out"


def frame_requests(case):
    """(offset, stride, count, pieces) for a frame of full chunks of BS bytes and a short one of LAST."""
    s, z, T, n = case.starts, case.sizes, case.T, len(case.sizes)
    yield 10, 0, 1, [(100, 50), (300, 7), (1000, 64), (1100, 1)]  # scattered rows inside one chunk
    yield 3, 0, 1, [(s[j] + 100 + j, 50 + j) for j in range(n)]  # rows in every chunk
    if n > 1:
        yield 0, 0, 1, [(5, 9), (s[1] - 30, 60), (s[1] + 200, 16)]  # a piece that straddles a chunk boundary
        yield 0, 0, 1, [(s[1] - 40, 40), (s[1] + 100, 10)]  # a piece that ends exactly at a chunk boundary
    yield 3, 4096, (T - 3 - 120) // 4096 + 1, [(0, 24), (100, 17)]  # a column: every period touches, every chunk is cut
    yield 7, 100, 12, [(20, 33)]  # one piece per period: the strided update
    yield 0, 0, 1, [(0, T)]  # the whole tensor as one piece
    yield 5, 9, 4, []  # W == 0: m == 0
    yield 5, 9, 4, [(5, 0), (9, 0)]  # L == 0
    yield U64, 9, 0, [(0, 2), (5, 2)]  # count == 0: the offset is not looked at


def frames_match_reference(lib, k, chunks, call):
    case = Case(require_ref().lib, k, chunks)
    assert case.sizes == [BS] * (chunks - 1) + [LAST]
    old = _chunks(case.frame)
    for offset, stride, count, pieces in frame_requests(case):
        got, idx = check_select_update(lib, case, offset, stride, count, pieces, call=call)
        new, t = _chunks(got), touched_chunks(case, idx)
        assert all(new[j] == old[j] for j in range(chunks) if j not in t), ("an untouched chunk changed", offset, stride, count)
        if idx.size == 0:
            assert got == case.frame


@pytest.mark.parametrize("chunks", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_index_updates_of_a_frame_match_the_reference(emu, k, chunks, monkeypatch):
    """Blocks of 65 KiB, a short last chunk that is no multiple of k, windows of two chunks: f' is the reference's frame of S(x') byte for byte,
    nothing beyond it is written and the untouched chunks are those of f."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    frames_match_reference(emu, k, chunks, select_update_call)


def delta_frames_match_reference(lib, k, call):
    case = Case(require_ref().lib, k, 2, with_base=True)
    for offset, stride, count, pieces in ((BS - 400, 100, 9, [(0, 20), (40, 33)]), (3, 0, 1, [(0, 1), (2, 1)]), (0, 0, 1, [(0, BS - 1), (BS, LAST)])):
        check_select_update(lib, case, offset, stride, count, pieces, call=call)


@pytest.mark.parametrize("k", [1, 4])
def test_index_updates_of_a_delta_frame(emu, k):
    """f is a delta frame and `base` holds the base's bytes of the index set: the expectation is the reference's frame of S(D(x', b))."""
    delta_frames_match_reference(emu, k, select_update_call)


def covered_and_corrupt_chunks(lib, call):
    ref = require_ref().lib
    case = Case(ref, 2, 5)
    s = case.starts
    # chunk 2 is covered whole by a piece that cuts chunks 1 and 3; chunk 0 is cut by a small piece; chunk 4 is untouched
    req = (0, 0, 1, [(10, 5), (s[2] - 50, BS + 120)])
    for j in (2, 4):  # a covered chunk is rebuilt from data alone, an untouched one carried over: neither is decoded
        bad = _flip(case.frame, j)
        assert _ref_decompress(ref, bad, case.T)[0] != 0
        blk, orig = _chunks(bad)[j]
        check_select_update(lib, case, *req, frame=bad, want=(lambda f: f) if j == 2 else (lambda f: _with_chunk(f, j, blk, orig)), call=call)
    data, _, _, _ = index_update(case, *req)
    for j in (0, 1, 3):  # a corrupt cut chunk: the decoder's code, nothing written
        bad = _flip(case.frame, j)
        code = _ref_decompress(ref, bad, case.T)[0]
        assert code != 0
        refused_select(lib, 2, bad, *req, data, code, call=call)


def test_covered_chunks_are_not_decoded_and_corrupt_cut_chunks_fail(emu):
    covered_and_corrupt_chunks(emu, select_update_call)


NORMAL_FORMS = (  # (offset, stride, count, pieces), the range (offset, w) it is
    ((50, 300, 1, [(7, 100)]), (57, 100)),  # a single piece, one period
    ((BS - 48, 100, 7, [(0, 30), (30, 50), (80, 20)]), (BS - 48, 700)),  # neighbours that join and fill the period
    ((BS - 43, 10, 14, [(0, 0), (0, 4), (4, 6), (10, 0)]), (BS - 43, 140)),  # empty pieces dropped, stride == L
    ((0, 0, 1, [(0, 0), (BS + 3, 500), (BS + 503, 1)]), (BS + 3, 501)),  # count == 1 with a stride of 0
    ((9, 64, 3, [(0, 64)]), (9, 192)),  # the piece is the period
)


def normal_forms_are_the_range_update(lib, call, range_call):
    """Byte-identical results and the same number of CM launches, for a good frame and for one with a corrupt cut chunk."""
    case = Case(require_ref().lib, 4, 2)
    for frame in (case.frame, _flip(case.frame, 0)):
        for (offset, stride, count, pieces), (lo, w) in NORMAL_FORMS:
            data = pattern(w, 9)
            lib.bz3_hip_debug_cm_launches(1)
            got = call(lib, 4, frame, offset, stride, count, pieces, data, cap=default_cap(lib, frame))
            n_sel = lib.bz3_hip_debug_cm_launches(1)
            ref = range_call(lib, 4, frame, lo, data, cap=default_cap(lib, frame))
            assert got == ref and n_sel == lib.bz3_hip_debug_cm_launches(1), (offset, stride, count, pieces, got[:2], ref[:2])


def test_requests_in_range_form_are_the_range_update(emu):
    normal_forms_are_the_range_update(emu, select_update_call, update_call)


def decode_once(lib, call):
    """Chunk 0 holds 670 pieces over 67 periods, chunk 1 ten: one CM decode launch and one encode launch, as for the one-piece request that
    touches the same two chunks."""
    case = Case(require_ref().lib, 2, 2)
    lib.bz3_hip_debug_cm_launches(1)
    check_select_update(lib, case, 11, 1000, 68, [(20 * j, 3 + j) for j in range(10)], call=call)
    many = lib.bz3_hip_debug_cm_launches(1)
    check_select_update(lib, case, 11, 0, 1, [(0, 40), (BS, 40)], call=call)
    assert many == lib.bz3_hip_debug_cm_launches(1) == 2


def test_a_chunk_with_many_pieces_is_decoded_once(emu):
    decode_once(emu, select_update_call)


INVALID_LISTS = ((0, 100, 2, [(0, 10), (5, 10)]), (0, 100, 2, [(20, 10), (0, 10)]), (0, 100, 1, [(0, 10), (9, 0)]),  # overlapping, descending
                 (0, 25, 2, [(0, 10), (20, 6)]), (0, 0, 2, [(0, 1), (2, 1)]),  # the last piece past the stride with count > 1
                 (0, 100, 2, [(0, 10), (200, 0)]), (U64 - 50, 20, 1, [(0, 5), (60, 0)]),  # ... an empty last piece counts as given
                 (0, 2 ** 40, 2, [(5, U64 - 3), (U64, 0)]), (0, U64, 2, [(0, 2 ** 63), (2 ** 63 + 1, 2 ** 63 - 2)]),  # s + l; L fits, count L does not
                 (0, 2 ** 34, 2 ** 31, [(0, 2 ** 32), (2 ** 33, 2 ** 32)]),  # count L
                 (U64 - 50, 20, 4, [(0, 5), (10, 5)]), (U64 - 5, 20, 1, [(0, 2), (4, 2)]), (5, U64 // 2, 4, [(0, 1), (2, 1)]))  # the last byte


def update_refusals(lib, call):
    ref = require_ref().lib
    case = Case(ref, 2, 2)
    T, frame = case.T, case.frame
    data = pattern(64, 9)
    for offset, stride, count, pieces in INVALID_LISTS:  # every invalid list of the decode contract, whatever w is
        W = count * total(pieces)
        refused_select(lib, 2, frame, offset, stride, count, pieces, data, INIT, call=call, w=W if W <= 64 else 64)
    req = (BS - 300, 200, 3, [(0, 40), (100, 24)])  # W = 192, cuts both chunks
    data = pattern(192, 9)
    for w in (191, 0):  # w != W (a longer w would name bytes behind the buffer and is not run)
        refused_select(lib, 2, frame, *req, data, INIT, call=call, w=w)
    refused_select(lib, 2, frame, 5, 9, 4, [], b"x", INIT, call=call)  # W == 0 with w == 1
    refused_select(lib, 3, frame, *req, data, INIT, call=call)  # a bad element size
    refused_select(lib, 2, frame, T - 523, 200, 3, [(0, 40), (100, 24)], data, TOO_BIG, call=call)  # phi(W - 1) == T
    assert call(lib, 2, frame, T - 524, 200, 3, [(0, 40), (100, 24)], data)[0] == 0  # phi(W - 1) == T - 1
    refused_select(lib, 2, frame, T, 200, 3, [(0, 40), (100, 24)], data, TOO_BIG, call=call)
    need = 13 + 8 + ref.bz3_bound(BS) + 8 + ref.bz3_bound(LAST)
    refused_select(lib, 2, frame, *req, data, TOO_BIG, cap=need - 1, call=call)
    rc, size, out = call(lib, 2, frame, *req, data, cap=need)
    assert (rc, out[:size]) == (0, index_update(case, *req)[2]) and out[size:] == bytes([FILL]) * (need - size)
    refused_select(lib, 2, frame, 5, 9, 4, [], b"", TOO_BIG, cap=len(frame) - 1, call=call)
    assert call(lib, 2, frame, 5, 9, 4, [], b"", cap=len(frame))[:2] == (0, len(frame))
    refused_select(lib, 2, _with_header(frame, 1, orig=-5), 10, 0, 1, [(0, 100), (200, 92)], data, MALFORMED, call=call)  # a malformed header behind the request
    refused_select(lib, 2, frame[:12], 5, 9, 4, [], b"", MALFORMED, call=call)
    return case, req, data


def test_refusals_leave_out_untouched(emu):
    ref = require_ref().lib
    case, req, data = update_refusals(emu, select_update_call)
    frame, pieces = case.frame, _pieces_arg(req[3])
    arena = _buf(bytes([FILL]) * (4 * len(frame) + 4 * BS))
    cap = len(frame) + 3 * ref.bz3_bound(BS)
    C.memmove(arena, frame, len(frame))
    before = bytes(arena)
    for in_off, out_off in ((0, len(frame) - 1), (0, 0)):  # out overlaps in
        osz = C.c_size_t(cap)
        assert emu.bz3_hip_update_device_select(2, C.byref(arena, in_off), len(frame), *req[:3], 2, pieces, _buf(data), len(data), None, C.byref(arena, out_off), C.byref(osz)) == INIT
        assert osz.value == 0 and bytes(arena) == before
    arena2 = _buf(bytes([FILL]) * (cap + 2000))
    C.memmove(C.byref(arena2, cap - 1), data, len(data))
    before = bytes(arena2)
    for which in ("data", "base"):
        osz = C.c_size_t(cap)
        inside = C.byref(arena2, cap - 1)
        rc = emu.bz3_hip_update_device_select(2, _buf(frame), len(frame), *req[:3], 2, pieces, inside if which == "data" else _buf(data), len(data),
                                              inside if which == "base" else None, arena2, C.byref(osz))
        assert rc == INIT and osz.value == 0 and bytes(arena2) == before, which
    osz = C.c_size_t(cap)  # adjacent: fine
    assert emu.bz3_hip_update_device_select(2, _buf(frame), len(frame), *req[:3], 2, pieces, C.byref(arena2, cap), len(data), None, arena2, C.byref(osz)) == 0
    assert emu.bz3_hip_update_device_select(2, _buf(frame), len(frame), *req[:3], 2, pieces, _buf(data), len(data), None, arena2, None) == INIT
    osz = C.c_size_t(cap)
    assert emu.bz3_hip_update_device_select(2, _buf(frame), len(frame), *req[:3], 2, None, _buf(data), len(data), None, arena2, C.byref(osz)) == INIT  # NULL pieces with m > 0
    assert osz.value == 0


# ---- many ---------------------------------------------------------------------------------------------------------------------
def many_call(lib, ks, frames, params, lists, datas, bases, caps=None, alloc=_buf, addr=C.addressof):
    """Per frame (rc, *out_size, out[0, cap) after).  params[i] = (offset, stride, count)."""
    n = len(frames)
    caps = [default_cap(lib, f) for f in frames] if caps is None else caps
    ins, dbufs = [alloc(f) for f in frames], [alloc(d) for d in datas]
    bbufs = [None if b is None else alloc(b) for b in bases]
    outs = [alloc(bytes([FILL]) * c) for c in caps]
    out_sizes, rcs = (C.c_size_t * n)(*caps), (C.c_int * n)(*([77] * n))
    vp = lambda bufs: (C.c_void_p * n)(*[None if b is None else addr(b) for b in bufs])  # noqa: E731
    arrs = [_pieces_arg(l) for l in lists]
    pp = (C.POINTER(C.c_uint64) * n)(*[C.cast(a, C.POINTER(C.c_uint64)) if l else None for a, l in zip(arrs, lists)])
    rc = lib.bz3_hip_update_device_select_many(n, (C.c_uint32 * n)(*ks), vp(ins), (C.c_size_t * n)(*map(len, frames)),
                                               (C.c_uint64 * (4 * n))(*[v for p, l in zip(params, lists) for v in (*p, len(l))]), pp, vp(dbufs), (C.c_size_t * n)(*map(len, datas)),
                                               vp(bbufs), vp(outs), out_sizes, rcs)
    return rc, [(rcs[i], out_sizes[i], bytes(outs[i])[: caps[i]]) for i in range(n)]


def many_equal_single_calls(lib, many_call, single_call):
    """One call holds a range-form request, a one-piece (strided) one, many-piece ones with and without a base, W == 0, and a frame whose cut
    chunk is corrupt: every frame has its single call's result, the good ones the reference's frame, and the failing one leaves the others
    alone."""
    ref = require_ref().lib
    cases = [Case(ref, k, chunks, wb, seed=40 + i) for i, (k, chunks, wb) in enumerate(((2, 2, 0), (1, 1, 1), (8, 3, 0), (4, 2, 1), (4, 1, 0), (2, 2, 0)))]
    plan = [((BS - 30, 0, 1), [(0, 100)]), ((7, 50, 9), [(3, 20)]), ((BS - 100, 3500, 20), [(0, 64), (70, 9), (200, 128)]), ((5, BS, 2), [(0, 16), (40, 40), (90, 1)]), ((5, 9, 0), [(0, 1), (3, 1)]),
            ((BS - 10, 100, 2), [(0, 4), (8, 9)])]
    frames = [c.frame for c in cases]
    frames[5] = _flip(frames[5], 1)
    ks, params, lists = [c.k for c in cases], [p for p, _ in plan], [l for _, l in plan]
    ups = [index_update(c, *p, l) for c, (p, l) in zip(cases, plan)]
    datas, bases = [u[0] for u in ups], [u[1] for u in ups]
    rc, got = many_call(lib, ks, frames, params, lists, datas, bases)
    bad_code = _ref_decompress(ref, frames[5], cases[5].T)[0]
    assert rc == bad_code != 0
    for i in range(6):
        assert got[i] == single_call(lib, ks[i], frames[i], *params[i], lists[i], datas[i], bases[i]), ("single call", i)
        if i < 5:
            assert got[i][0] == 0 and got[i][2][: got[i][1]] == ups[i][2], i
    assert got[5][:2] == (bad_code, 0) and got[5][2] == bytes([FILL]) * len(got[5][2])
    assert got[4][2][: got[4][1]] == frames[4]


def test_many_updates_equal_their_single_calls(emu, monkeypatch):
    """Windows of two chunks: the column update of the three-chunk frame has its cut chunks in different windows, and its chunks share windows
    with the neighbouring frames'."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    many_equal_single_calls(emu, many_call, select_update_call)


def every_request_form(case_for):
    """(cases, params, lists) of five frames of element size 4 and six chunks, two of them with a base (case_for(with_base, seed) makes a case): a
    one-run range, the whole tensor, a two-run request with one piece per period, a two-piece request, and a two-piece request of which every
    chunk holds bytes of one piece alone.  Their patch segments are a clipped split, six whole splits, a select split over a one-piece table, a
    select split, and two clipped splits that come from a piece table."""
    plain, based = case_for(False, 61), case_for(True, 62)
    s = plain.starts
    assert plain.sizes == based.sizes == [BS] * 5 + [LAST]
    plan = [(based, (s[2] + 100, 0, 1), [(0, 777)]),  # one run inside chunk 2
            (plain, (0, 0, 1), [(0, plain.T)]),  # the whole tensor: every chunk covered
            (plain, (s[1] + 5, 1000, 2), [(3, 401)]),  # two runs
            (based, (s[3] + 100, 2000, 2), [(0, 300), (650, 130)]),  # two pieces
            (plain, (s[4] + 9, 0, 1), [(4, 500), (BS + 20, 100)])]  # one piece in chunk 4, the other in chunk 5
    return [c for c, _, _ in plan], [p for _, p, _ in plan], [l for *_, l in plan]


@pytest.mark.parametrize("window", [2, 16])
def test_one_call_holds_every_request_form(emu, window, monkeypatch):
    """The write mirror of test_frame_select_emu's test of this name: the five requests of every_request_form in one _many call.  Windows of two
    chunks patch the eleven touched chunks in six launches; a window of sixteen patches them in ONE launch, which then holds whole, clipped and
    select splits side by side, each with the parameters of its own kind.  Every resulting frame is the reference's frame of the updated bytes."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", str(window))
    ref = require_ref().lib
    cases, params, lists = every_request_form(lambda wb, seed: Case(ref, 4, 6, wb, seed=seed))
    ups = [index_update(c, *p, l) for c, p, l in zip(cases, params, lists)]
    assert sorted(len(touched_chunks(c, u[3])) for c, u in zip(cases, ups)) == [1, 1, 1, 2, 6]
    rc, got = many_call(emu, [4] * 5, [c.frame for c in cases], params, lists, [u[0] for u in ups], [u[1] for u in ups])
    assert rc == 0
    for i, ((code, size, out), (_, _, expect, _)) in enumerate(zip(got, ups)):
        assert (code, size) == (0, len(expect)), (i, code, size, len(expect))
        assert out[:size] == expect, ("frames differ", i)
        assert out[size:] == bytes([FILL]) * (len(out) - size), ("wrote beyond the frame", i)


def test_many_whole_call_errors(emu):
    case = Case(require_ref().lib, 1, 1)
    data = pattern(40, 9)
    many = emu.bz3_hip_update_device_select_many
    assert many(0, None, None, None, None, None, None, None, None, None, None, None) == 0
    assert many(2, None, None, None, None, None, None, None, None, None, None, None) == INIT
    untouched = lambda got: all(g[:2] == (INIT, 0) and g[2] == bytes([FILL]) * len(g[2]) for g in got)  # noqa: E731
    good = ((0, 100, 2), [(0, 15), (20, 5)])
    rc, got = many_call(emu, [1, 3], [case.frame] * 2, [good[0]] * 2, [good[1]] * 2, [data] * 2, [None] * 2)  # a bad element size fails the whole call
    assert rc == INIT and untouched(got)
    rc, got = many_call(emu, [1, 1], [case.frame] * 2, [good[0], (0, 100, 2)], [good[1], [(0, 15), (10, 5)]], [data] * 2, [None] * 2)  # one invalid list
    assert rc == INIT and untouched(got)
    rc, got = many_call(emu, [1, 1], [case.frame] * 2, [good[0]] * 2, [good[1]] * 2, [data, data[:39]], [None] * 2)  # one w != W
    assert rc == INIT and untouched(got)
    # elem_sizes and bases NULL: k = 1, no base; params NULL; pieces NULL
    cap = default_cap(emu, case.frame)
    pp = (C.POINTER(C.c_uint64) * 1)(C.cast(_pieces_arg(good[1]), C.POINTER(C.c_uint64)))
    for params, lists, code in (((C.c_uint64 * 4)(*good[0], 2), pp, 0), (None, pp, INIT), ((C.c_uint64 * 4)(*good[0], 2), None, INIT)):
        ins, dbuf, outs = [_buf(case.frame)], [_buf(data)], [_buf(bytes([FILL]) * cap)]
        out_sizes, rcs = (C.c_size_t * 1)(cap), (C.c_int * 1)(77)
        assert many(1, None, _vp(ins), (C.c_size_t * 1)(len(case.frame)), params, lists, _vp(dbuf), (C.c_size_t * 1)(len(data)), None, _vp(outs), out_sizes, rcs) == code
        if code == 0:
            assert rcs[0] == 0 and bytes(outs[0])[: out_sizes[0]] == index_update(case, *good[0], good[1])[2]
        else:
            assert rcs[0] == INIT and out_sizes[0] == 0 and bytes(outs[0]) == bytes([FILL]) * cap
