"""CPU tests of the range calls (include/bz3_hip.h bz3_hip_decompress_device_range[_many], the clipped merge of
bzip3_amd/csrc/planes.hpp through bz3_hip_debug_range, the skipping walk of frame.hpp) under the fiber emulation of the HIP execution
model (tests/emu).

The oracle of a range is always full[offset : offset + w]: `full` is the reference's bz3_decompress (oracle/_ref/libbz3ref.so), numpy
merge_k per chunk and numpy D_inv, never the library under test.  For frames with a broken chunk the expectation is written out from
the definition in bz3_hip.h (range_model), with the reference deciding every chunk it decodes.

BZ3_EMU_LIB=<path> runs the module on another build of the emulator library, as test_frame_delta_emu does (the sanitizer build of
tests/sanitize_emu.sh); every buffer handed to the library comes from that module's _buf and lies inside a larger allocation."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

import bzip3_amd
import mutants
from oracle_lib import require_ref
from test_frame_delta_emu import NO_BASE, D_inv, _base_for, _buf, _chunks, _host_alloc, _r16, _with_chunk
from test_frame_planes_emu import BS, COUNTS, _ref_compress, _ref_decompress, _vp, chunk_sizes, merge_k, per_block

HERE = os.path.dirname(os.path.abspath(__file__))
INIT, MALFORMED, TRUNCATED = bzip3_amd.BZ3_ERR_INIT, bzip3_amd.BZ3_ERR_MALFORMED_HEADER, bzip3_amd.BZ3_ERR_TRUNCATED_DATA
U64 = 2 ** 64 - 1
TILE = 4080  # planes.hpp PLANES_TILE_ELEMS
EDGE_COUNTS = (4079, 4080, 4081, 4095, 4096, 4097, 8159, 8160, 8161)
ALL_COUNTS = tuple(dict.fromkeys(COUNTS + EDGE_COUNTS))


@pytest.fixture(scope="module")
def emu():
    if os.environ.get("BZ3_EMU_LIB"):
        return bzip3_amd._declare(C.CDLL(os.environ["BZ3_EMU_LIB"]))
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def clip_points(elems, tail, k):
    """The a and b of the sweep for a chunk of elems * k + tail bytes."""
    s, mk = elems * k + tail, elems * k
    pts = {0, 1, k - 1, k, k + 1, 15, 16, 17, mk - 1, mk, s - 1, s}
    for t in (TILE, 2 * TILE):
        pts |= {t * k - 1, t * k, t * k + 1}
    return sorted(p for p in pts if 0 <= p <= s)


def clip_pairs(elems, tail, k):
    pts = clip_points(elems, tail, k)
    return [(a, b) for i, a in enumerate(pts) for b in pts[i:]]


def lay_out_range(rng, spec, addrs, src_np, base_np):
    """spec: (slot, base, dst alignment mod 16, elements, tail bytes, k, has base, a, b) per segment, one after the other with gaps;
    the base and dst alignments are those of the clip's first byte.  Returns the hook's table and the expected writes."""
    table, writes, offs = [], [], [0, 0, 0]
    for a_s, a_b, a_d, elems, tail, k, has_base, a, b in spec:
        n = elems * k + tail
        for j, al in enumerate((a_s, a_b, a_d)):
            offs[j] += (al - (addrs[j] + offs[j])) % 16
        s, bo, d = offs
        table += [s, bo if has_base else NO_BASE, d, n, k | 0x100, a, b]
        x = merge_k(src_np[s : s + n], k)[a:b]
        writes.append((d, D_inv(x, base_np[bo : bo + b - a]) if has_base else x))
        offs[0] += n + int(rng.integers(0, 40))
        offs[1] += b - a + int(rng.integers(1, 40))
        offs[2] += b - a + int(rng.integers(1, 40))  # at least one untouched byte between destination segments
    return table, writes, offs


def range_case(call, rng, spec, alloc):
    """alloc(array) -> (object for the hook, address, numpy reader); call(src, base, dst, table, n) -> rc.  The whole destination is
    compared against a 0xA5 fill with the expected writes, the inputs against themselves."""
    room_s = sum(e * k + t for _, _, _, e, t, k, _, _, _ in spec) + 56 * len(spec) + 64
    room_d = sum(b - a for *_, a, b in spec) + 56 * len(spec) + 64
    src_np = rng.integers(0, 256, size=room_s, dtype=np.uint8)
    base_np = rng.integers(0, 256, size=room_d, dtype=np.uint8)
    src, base, dst = alloc(src_np), alloc(base_np), alloc(np.full(room_d, 0xA5, dtype=np.uint8))
    want = np.full(room_d, 0xA5, dtype=np.uint8)
    table, writes, ends = lay_out_range(rng, spec, (src[1], base[1], dst[1]), src_np, base_np)
    assert ends[0] <= room_s - 16 and max(ends[1:]) <= room_d - 16
    for off, b in writes:
        want[off : off + len(b)] = b
    t = (C.c_uint64 * max(1, len(table)))(*table)
    assert call(src[0], base[0], dst[0], t, len(table) // 7) == 0
    bad = np.nonzero(dst[2]() != want)[0]
    assert bad.size == 0, ("bytes differ at", bad[:8], table[:14])
    assert np.array_equal(src[2](), src_np) and np.array_equal(base[2](), base_np), "an input was written"


def sweep_specs_range(rng, k, has_base, counts=ALL_COUNTS, alignments=True):
    """One launch per element count and tail length 0..k-1: every pair a <= b of clip_points, all at random alignments; then
    (`alignments`) each of the three alignments through all 16 values with the other two random, on a chunk of three tiles clipped at
    random interior bytes."""
    for elems in counts:
        for tail in range(k):
            yield [(_r16(rng), _r16(rng), _r16(rng), elems, tail, k, has_base, a, b) for a, b in clip_pairs(elems, tail, k)]
    if not alignments:
        return
    spec = []
    for which in range(3):
        for al16 in range(16):
            al = [_r16(rng), _r16(rng), _r16(rng)]
            al[which] = al16
            elems, tail = 2 * TILE + int(rng.integers(1, 300)), int(rng.integers(0, k))
            a, b = sorted(int(v) for v in rng.integers(0, elems * k + tail + 1, size=2))
            spec.append((*al, elems, tail, k, has_base, a, b))
    yield spec


def mixed_spec_range(rng):
    """One launch that holds clipped, whole and plain (k = 1) segments of every k, with and without a base."""
    spec = []
    for _ in range(3):
        for k in (1, 2, 4, 8):
            for has in (0, 1):
                elems, tail = int(rng.integers(20, 9000)), int(rng.integers(0, k))
                s = elems * k + tail
                a, b = sorted(int(v) for v in rng.integers(0, s + 1, size=2))
                spec.append((_r16(rng), _r16(rng), _r16(rng), elems, tail, k, has, a, b))  # clipped
                spec.append((_r16(rng), _r16(rng), _r16(rng), elems, tail, k, has, 0, s))  # whole
    return spec


def in_place_range_case(call, rng, alloc, sizes=(1, 17, 4079, 4081, 9000, 70_001)):
    """dst == base: (merge_k(src)[a:b] + dst) written over dst, every k, several tiles."""
    spec = []
    for k in (1, 2, 4, 8):
        for e in sizes:
            tail = int(rng.integers(0, k))
            a, b = sorted(int(v) for v in rng.integers(0, e * k + tail + 1, size=2))
            spec.append((_r16(rng), _r16(rng), e, tail, k, a, b))
    room_s = sum(e * k + t for _, _, e, t, k, _, _ in spec) + 56 * len(spec) + 64
    src_np = rng.integers(0, 256, size=room_s, dtype=np.uint8)
    old = rng.integers(0, 256, size=room_s, dtype=np.uint8)
    src, dst = alloc(src_np), alloc(old)
    want, table, offs = old.copy(), [], [0, 0]
    for a_s, a_d, elems, tail, k, a, b in spec:
        n = elems * k + tail
        offs[0] += (a_s - (src[1] + offs[0])) % 16
        offs[1] += (a_d - (dst[1] + offs[1])) % 16
        s, d = offs
        table += [s, d, d, n, k | 0x100, a, b]
        want[d : d + b - a] = D_inv(merge_k(src_np[s : s + n], k)[a:b], old[d : d + b - a])
        offs[0] += n + int(rng.integers(1, 40))
        offs[1] += b - a + int(rng.integers(1, 40))
    assert max(offs) <= room_s - 16
    t = (C.c_uint64 * len(table))(*table)
    assert call(src[0], dst[0], dst[0], t, len(table) // 7) == 0
    bad = np.nonzero(dst[2]() != want)[0]
    assert bad.size == 0, ("bytes differ at", bad[:8])
    assert np.array_equal(src[2](), src_np)


@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("elems", ALL_COUNTS)
def test_range_kernel_every_clip_pair_at_every_tail(emu, elems, k, has_base):
    rng = np.random.default_rng(500 + 100 * elems + 10 * k + has_base)
    for spec in sweep_specs_range(rng, k, has_base, counts=(elems,), alignments=False):
        range_case(emu.bz3_hip_debug_range, rng, spec, _host_alloc)


@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_range_kernel_every_alignment(emu, k, has_base):
    rng = np.random.default_rng(500 + 10 * k + has_base)
    for spec in sweep_specs_range(rng, k, has_base, counts=()):
        range_case(emu.bz3_hip_debug_range, rng, spec, _host_alloc)


def test_range_kernel_mixed_segments_in_one_launch(emu):
    rng = np.random.default_rng(52)
    range_case(emu.bz3_hip_debug_range, rng, mixed_spec_range(rng), _host_alloc)
    range_case(emu.bz3_hip_debug_range, rng, [], _host_alloc)


def test_range_kernel_in_place(emu):
    in_place_range_case(emu.bz3_hip_debug_range, np.random.default_rng(53), _host_alloc)


def test_debug_range_rejects_bad_arguments(emu):
    buf = _buf(b"", 64)
    assert emu.bz3_hip_debug_range(buf, buf, buf, None, -1) == INIT
    assert emu.bz3_hip_debug_range(buf, buf, buf, None, 0) == 0
    for mode in (0, 2, 3 | 0x100, 16 | 0x100, 2 | 0x300, 2 | 0x200):  # the split direction, bad element sizes, stray bits
        assert emu.bz3_hip_debug_range(buf, buf, buf, (C.c_uint64 * 7)(0, 0, 32, 8, mode, 0, 8), 1) == INIT
    for a, b in ((5, 4), (0, 9), (9, 9)):  # a <= b <= len
        assert emu.bz3_hip_debug_range(buf, buf, buf, (C.c_uint64 * 7)(0, 0, 32, 8, 2 | 0x100, a, b), 1) == INIT
    assert bytes(buf) == bytes(64)


# ---- frames -------------------------------------------------------------------------------------------------------------------
def stream_for(bs, blocks=5, last=1234):
    """`blocks` full blocks and a short one of repetitive bytes (LZP collapses them, so the emulated CM stage stays small)."""
    rng = np.random.default_rng(4)
    unit = bytes(rng.integers(0, 256, size=997, dtype=np.uint8))
    n = blocks * bs + last
    return (unit * (n // 997 + 1))[:n]


class Case:
    """A frame the reference made of `stream`, and what it decodes to: full = D_inv(merge_k per chunk of the reference's
    bz3_decompress, base)."""

    def __init__(self, ref, bs, k, with_base, stream, seed=70):
        self.k, self.bs = k, bs
        rc, self.frame = _ref_compress(ref, bs, stream)
        assert rc == 0
        rc, sx = _ref_decompress(ref, self.frame, len(stream) + 16)
        assert rc == 0 and sx == stream
        self.sizes = chunk_sizes(self.frame, len(sx))
        self.starts = [sum(self.sizes[:j]) for j in range(len(self.sizes))]
        self.T = len(sx)
        self.X = per_block(merge_k, sx, self.sizes, k)
        self.base = _base_for(self.T, seed + k) if with_base else None
        self.full = bytes(D_inv(self.X, self.base)) if with_base else self.X

    def want(self, offset, w):
        return self.full[offset : offset + w]


GUARD = 24


def range_call(lib, k, frame, offset, w, base=None, in_place=False, alloc=_buf):
    """(rc, *out_size, the bytes of out[0, w + GUARD) after the call, what they were before).  base: the base's bytes of the range."""
    room = w + GUARD
    before = (bytes(base) + b"\xa5" * room)[:room] if in_place else b"\xa5" * room
    out = alloc(before)
    b = out if in_place else None if base is None else alloc(base)
    osz = C.c_size_t(w)
    rc = lib.bz3_hip_decompress_device_range(k, alloc(frame), len(frame), offset, b, 0 if base is None else w if in_place else len(base), out, C.byref(osz))
    return rc, osz.value, bytes(out)[:room], before


def check_range(lib, case, offset, w, in_place=False):
    base = None if case.base is None else case.base[offset : offset + w] if in_place else (case.base[offset : offset + w] + bytes(w))[:w]
    rc, r, got, before = range_call(lib, case.k, case.frame, offset, w, base, in_place)
    want = case.want(offset, w)
    assert (rc, r) == (0, len(want)), (offset, w, rc, r)
    assert got[:r] == want, ("bytes differ", offset, w)
    assert got[r:] == before[r:], ("wrote beyond the range", offset, w)


def frame_ranges(case):
    T = case.T
    yield 0, T
    yield 0, T + 100  # end beyond T: a short read
    yield 5, 0
    for p in case.starts[1:]:
        for o in (p - 1, p, p + 1):
            yield o, 3  # offset at the boundary - 1, +0, +1
        for e in (p - 1, p, p + 1):
            yield e - 2, 2  # end at them
    yield case.starts[2] + 7, 1
    yield case.starts[1] - 5, case.sizes[1] + case.sizes[2] + 9  # two whole chunks between two clipped ones
    for o in (T - 1, T, T + 5):
        yield o, 9
    yield T - 3, U64  # offset + w overflows


@pytest.mark.parametrize("with_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_ranges_of_a_frame_match_the_reference(emu, k, with_base, monkeypatch):
    """65 KiB + 7: every block starts inside an element and has a tail; five full blocks and a short one; windows of two chunks."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    bs = BS + 7
    case = Case(require_ref().lib, bs, k, with_base, stream_for(bs))
    assert len(case.sizes) == 6 and case.sizes[:5] == [bs] * 5
    for offset, w in frame_ranges(case):
        if w == U64:  # (no buffer of that size: the capacity is a number to the call, which writes r bytes)
            # with a base, in place: two separate buffers of 2^64 bytes each would overlap whatever their addresses
            before = ((case.base[offset:] if with_base else b"") + b"\xa5" * 64)[:64]
            out = _buf(before)
            osz = C.c_size_t(U64)
            rc = emu.bz3_hip_decompress_device_range(k, _buf(case.frame), len(case.frame), offset, out if with_base else None, U64 if with_base else 0, out, C.byref(osz))
            assert (rc, osz.value) == (0, case.T - offset) and bytes(out)[: osz.value] == case.full[offset:] and bytes(out)[osz.value :] == before[osz.value :]
        else:
            check_range(emu, case, offset, w)


def test_range_over_a_base_slice_in_place_and_partial_overlap(emu):
    bs = BS + 7
    case = Case(require_ref().lib, bs, 4, 1, stream_for(bs, blocks=2))
    offset, w = bs - 100, bs + 300  # clipped, whole, clipped
    check_range(emu, case, offset, w, in_place=True)
    check_range(emu, case, 3, 50, in_place=True)
    # out overlaps the base without being it: BZ3_ERR_INIT, nothing written
    arena = _buf(b"\xa5" * 4096)
    C.memmove(arena, case.base[:1000], 1000)
    before = bytes(arena)
    for off in (1, 16, 999):
        osz = C.c_size_t(1000)
        assert emu.bz3_hip_decompress_device_range(4, _buf(case.frame), len(case.frame), 0, arena, 1000, C.byref(arena, off), C.byref(osz)) == INIT
        assert bytes(arena) == before
    osz = C.c_size_t(1000)
    assert emu.bz3_hip_decompress_device_range(4, _buf(case.frame), len(case.frame), 0, arena, 1000, C.byref(arena, 1000), C.byref(osz)) == 0  # adjacent: fine
    assert osz.value == 1000 and bytes(arena)[1000:2000] == case.full[:1000] and bytes(arena)[:1000] == case.base[:1000]


# ---- skipping is real -----------------------------------------------------------------------------------------------------------
def _le32s(b):
    return struct.unpack("<i", b)[0]


def range_model(ref, frame, k, offset, w, base=None):
    """(rc, committed bytes) of a range call from the definition in bz3_hip.h; the reference decodes every chunk that is decoded, alone
    in a frame of its own."""
    if len(frame) < 13 or frame[:5] != b"BZ3v1":
        return MALFORMED, b""
    bs, nb = struct.unpack("<II", frame[5:13])
    if not 65 * 1024 <= bs <= 511 << 20:
        return INIT, b""
    end, out, off, p, rc = min(offset + w, U64), b"", 13, 0, 0
    for _ in range(nb if w else 0):
        if p >= end:
            break
        left = len(frame) - off
        if left < 8:
            rc = MALFORMED
            break
        size, orig = _le32s(frame[off : off + 4]), _le32s(frame[off + 4 : off + 8])
        if size < 0 or size > bs:
            rc = MALFORMED
            break
        if left < size + 8:
            rc = TRUNCATED
            break
        if orig < 0:
            rc = MALFORMED
            break
        if orig > 0 and p + orig > offset:
            one = frame[:9] + struct.pack("<I", 1) + frame[off : off + 8 + size]
            rc, sx = _ref_decompress(ref, one, orig)
            if rc != 0:
                break
            out += bytes(merge_k(sx, k))[max(offset - p, 0) : min(end - p, orig)]
        off += 8 + size
        p += orig
    return rc, out if base is None else bytes(D_inv(out, base[: len(out)]))


def check_model(lib, ref, frame, k, offset, w, base=None, label=None):
    rc, r, got, before = range_call(lib, k, frame, offset, w, base)
    want = range_model(ref, frame, k, offset, w, base)
    assert (rc, got[:r]) == want, (label, offset, w, rc, want[0], r, len(want[1]))
    assert got[r:] == before[r:], ("wrote beyond the committed bytes", label)
    return rc, r


def _flip(frame, j, at=40):
    """`frame` with one payload byte of chunk j flipped."""
    blk, orig = _chunks(frame)[j]
    return _with_chunk(frame, j, blk[:at] + bytes([blk[at] ^ 0x40]) + blk[at + 1 :], orig)


def test_corrupt_chunks_outside_the_range_are_skipped(emu):
    ref = require_ref().lib
    bs = BS + 7
    case = Case(ref, bs, 2, 1, stream_for(bs, blocks=3))
    s = case.starts
    offset, w = s[1] + 10, bs - 20  # inside chunk 1
    for j in (0, 2, 3):  # wholly before the range, wholly after it
        bad = _flip(case.frame, j)
        assert _ref_decompress(ref, bad, case.T)[0] != 0
        full_rc, committed, _, _ = _full_call(emu, case.k, bad, case.base, case.T)
        assert full_rc != 0 and committed == s[j], "the full call must fail at the flipped chunk"
        rc, r, got, before = range_call(emu, case.k, bad, offset, w, case.base[offset : offset + w])
        assert (rc, r) == (0, w) and got[:w] == case.want(offset, w) and got[w:] == before[w:], j


def _full_call(lib, k, frame, base, room):
    out = _buf(b"\xa5" * room)
    osz = C.c_size_t(room)
    rc = lib.bz3_hip_decompress_device_delta(k, _buf(frame), None if base is None else _buf(base), 0 if base is None else len(base), out, len(frame), C.byref(osz))
    return rc, osz.value, bytes(out)[: osz.value], out


def test_corrupt_chunk_inside_the_range(emu):
    """A flipped payload byte at chunk j of the range: the full call's code, the range bytes of the chunks before j, the rest untouched."""
    ref = require_ref().lib
    bs = BS + 7
    case = Case(ref, bs, 4, 1, stream_for(bs, blocks=3))
    s = case.starts
    offset, w = s[1] - 50, 50 + bs + 70  # chunks 0 (clipped), 1 (whole), 2 (clipped)
    for j in (0, 1, 2):
        bad = _flip(case.frame, j)
        full_rc = _full_call(emu, case.k, bad, case.base, case.T)[0]
        rc, r, got, before = range_call(emu, case.k, bad, offset, w, case.base[offset : offset + w])
        want_r = max(0, min(s[j], offset + w) - offset)
        assert rc == full_rc != 0 and r == want_r, (j, rc, full_rc, r, want_r)
        assert got[:r] == case.want(offset, r) and got[r:] == before[r:], j
        assert (rc, got[:r]) == range_model(ref, bad, case.k, offset, w, case.base[offset : offset + w])


def _with_header(frame, j, size=None, orig=None):
    """`frame` with the size / original size fields of chunk j's header overwritten (the payload stays)."""
    off = 13
    for _ in range(j):
        off += 8 + int.from_bytes(frame[off : off + 4], "little")
    f = bytearray(frame)
    if size is not None:
        f[off : off + 4] = struct.pack("<i", size)
    if orig is not None:
        f[off + 4 : off + 8] = struct.pack("<i", orig)
    return bytes(f)


def test_header_mutants_before_inside_and_beyond_the_range(emu):
    """Chunk headers broken in the three ways the walk checks, and tests/mutants.py's mutated blocks, at every chunk of a frame: before
    the range they are reported with 0 bytes written (a header) or not noticed (a payload), inside it after the chunks before them are
    committed, at or beyond its end not at all."""
    ref = require_ref().lib
    bs = BS + 7
    case = Case(ref, bs, 2, 0, stream_for(bs, blocks=3))
    s, frame = case.starts, case.frame
    offset, w = s[1] + 5, bs + 20  # chunks 1 and 2; chunk 0 lies before the range, chunk 3 beyond its end
    cut = len(frame) - 10
    for j in range(4):
        for label, bad in (("size<0", _with_header(frame, j, size=-1)), ("size>bs", _with_header(frame, j, size=bs + 1)), ("orig<0", _with_header(frame, j, orig=-5)),
                           ("truncated", _with_header(frame[:cut], j, size=bs))):
            rc, r = check_model(emu, ref, bad, 2, offset, w, label=(label, j))
            if j == 0:
                assert rc != 0 and r == 0, (label, j)
            elif j == 3:
                assert (rc, r) == (0, w), (label, j)
            else:
                assert rc in (MALFORMED, TRUNCATED) and r == max(0, s[j] - offset), (label, j, rc, r)
    blocks = _chunks(frame)
    for (blk, orig), it in zip(mutants.mutants([b for b, _ in blocks], [o for _, o in blocks], 20, seed=11), range(20)):
        j = it % 4
        orig = orig if 0 < orig <= bs else blocks[j][1]
        bad = _with_chunk(frame, j, blk, orig)
        if orig != blocks[j][1] and j < 3:
            continue  # (another original size moves the chunks behind it: the header mutants above cover headers)
        rc, r = check_model(emu, ref, bad, 2, offset, w, label=("mutant", it, j))
        if j in (0, 3):
            assert (rc, r) == (0, w), ("a chunk outside the range was noticed", it, j)


def test_range_calls_launch_the_cm_stage_for_their_chunks_only(emu, monkeypatch):
    """Six frames of four chunks, windows of three, each range inside one chunk: two CM launches; the full decode takes eight."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    ref = require_ref().lib
    case = Case(ref, BS, 1, 0, stream_for(BS, blocks=3))
    assert len(case.sizes) == 4
    n = 6
    offs = [case.starts[i % 4] + 100 + i for i in range(n)]
    ws = [min(500, case.T - o) for o in offs]
    ins = [_buf(case.frame) for _ in range(n)]
    outs = [_buf(b"\xa5" * (w + GUARD)) for w in ws]
    out_sizes, rcs = (C.c_size_t * n)(*ws), (C.c_int * n)(*([77] * n))
    emu.bz3_hip_debug_cm_launches(1)
    assert emu.bz3_hip_decompress_device_range_many(n, None, _vp(ins), (C.c_size_t * n)(*[len(case.frame)] * n), (C.c_uint64 * n)(*offs), None, None, _vp(outs), out_sizes, rcs) == 0
    assert emu.bz3_hip_debug_cm_launches(1) == 2
    for i in range(n):
        assert (rcs[i], out_sizes[i]) == (0, ws[i]) and bytes(outs[i]) == case.want(offs[i], ws[i]) + b"\xa5" * GUARD
    outs = [_buf(b"", case.T) for _ in range(n)]
    out_sizes = (C.c_size_t * n)(*[case.T] * n)
    assert emu.bz3_hip_decompress_device_delta_many(n, None, _vp(ins), (C.c_size_t * n)(*[len(case.frame)] * n), None, None, _vp(outs), out_sizes, rcs) == 0
    assert emu.bz3_hip_debug_cm_launches(1) == 8
    assert all(bytes(o) == case.full for o in outs)


def synthetic_frame(ref, empty, payload):
    """A frame header that announces empty + 1 chunks, `empty` chunk headers (size 0, orig 0), then the one chunk of the one-block frame
    the reference makes of `payload`."""
    rc, one = _ref_compress(ref, BS, payload)
    assert rc == 0 and int.from_bytes(one[9:13], "little") == 1
    return one[:9] + struct.pack("<I", empty + 1) + bytes(8 * empty) + one[13:]


def test_five_thousand_empty_chunks_before_the_data(emu):
    """More skipped chunks than the walk has records, none of them decoded."""
    ref = require_ref().lib
    payload = stream_for(BS, blocks=0, last=3000)
    frame = synthetic_frame(ref, 5000, payload)
    emu.bz3_hip_debug_cm_launches(1)
    rc, r, got, before = range_call(emu, 1, frame, 0, 3000)
    assert (rc, r) == (0, 3000) and got[:r] == payload and got[r:] == before[r:]
    assert emu.bz3_hip_debug_cm_launches(1) == 1
    rc, r, got, before = range_call(emu, 2, frame, 2999, 10)
    assert (rc, r) == (0, 1) and got[:1] == bytes(merge_k(payload, 2))[2999:] and got[1:] == before[1:]


# ---- many -----------------------------------------------------------------------------------------------------------------------
def many_call(lib, ks, frames, offsets, ws, bases, in_place, alloc=_buf):
    """Per frame (rc, *out_size, out[0, w + GUARD) after, before).  bases[i]: None or the base's bytes of the range."""
    n = len(frames)
    ins = [alloc(f) for f in frames]
    befores = [((bytes(bases[i]) + b"\xa5" * (ws[i] + GUARD))[: ws[i] + GUARD]) if in_place[i] else b"\xa5" * (ws[i] + GUARD) for i in range(n)]
    outs = [alloc(b) for b in befores]
    bbufs = [outs[i] if in_place[i] else None if bases[i] is None else alloc(bases[i]) for i in range(n)]
    out_sizes, rcs = (C.c_size_t * n)(*ws), (C.c_int * n)(*([77] * n))
    bp = (C.c_void_p * n)(*[None if b is None else C.addressof(b) for b in bbufs])
    bsz = (C.c_size_t * n)(*[0 if bases[i] is None else ws[i] if in_place[i] else len(bases[i]) for i in range(n)])
    rc = lib.bz3_hip_decompress_device_range_many(n, (C.c_uint32 * n)(*ks), _vp(ins), (C.c_size_t * n)(*map(len, frames)), (C.c_uint64 * n)(*offsets), bp, bsz, _vp(outs),
                                                  out_sizes, rcs)
    return rc, [(rcs[i], out_sizes[i], bytes(outs[i])[: ws[i] + GUARD], befores[i]) for i in range(n)]


def test_many_ranges_equal_their_single_calls(emu, monkeypatch):
    """Frames with different k, offsets, bases (none, separate, in place) and lengths, an empty frame and a w = 0 frame, windows of three
    chunks; then the same with one frame corrupt: no other frame's result changes."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    ref = require_ref().lib
    bs = BS + 7
    cases = [Case(ref, bs, k, wb, stream_for(bs, blocks=nb, last=last), seed=90 + i)
             for i, (k, wb, nb, last) in enumerate(((2, 1, 2, 777), (1, 0, 1, 50), (8, 1, 3, 1234), (4, 0, 0, 100), (4, 1, 2, 9)))]
    empty = _ref_compress(ref, bs, b"")[1]
    plan = [(0, bs - 30, 100, 0), (1, 0, 10 ** 6, 0), (2, 2 * bs - 1, bs + 2, 1), (3, 7, 50, 0), (4, bs + 1, bs + 100, 1), (0, 5, 0, 0), (2, 10, 70_000, 0), (1, bs + 49, 9, 0)]
    ks = [cases[c].k for c, *_ in plan] + [2]
    frames = [cases[c].frame for c, *_ in plan] + [empty]
    offsets = [o for _, o, _, _ in plan] + [0]
    ws = [w for _, _, w, _ in plan] + [40]
    in_place = [bool(ip) for *_, ip in plan] + [False]
    bases = [None if cases[c].base is None else (cases[c].base[o : o + w] + bytes(w))[:w] for c, o, w, _ in plan] + [None]
    rc, got = many_call(emu, ks, frames, offsets, ws, bases, in_place)
    assert rc == 0
    for i, (c, o, w, ip) in enumerate(plan):
        want = cases[c].want(o, w)
        assert got[i][:2] == (0, len(want)) and got[i][2][: len(want)] == want and got[i][2][len(want) :] == got[i][3][len(want) :], i
        assert got[i][:3] == range_call(emu, ks[i], frames[i], o, w, bases[i], in_place[i])[:3], ("single call", i)
    assert got[-1][:3] == (0, 0, b"\xa5" * (40 + GUARD))
    # one corrupt frame (chunk 2 of the 8-byte frame, inside its range) changes no other frame's result
    frames2 = list(frames)
    frames2[2] = _flip(frames[2], 2)
    rc2, got2 = many_call(emu, ks, frames2, offsets, ws, bases, in_place)
    assert rc2 == got2[2][0] != 0 and got2[2][1] == 1
    assert got2[2][:3] == range_call(emu, ks[2], frames2[2], offsets[2], ws[2], bases[2], in_place[2])[:3]
    assert [g for i, g in enumerate(got2) if i != 2] == [g for i, g in enumerate(got) if i != 2]


def test_many_whole_call_errors(emu):
    ref = require_ref().lib
    frame = _ref_compress(ref, BS, b"abc" * 100)[1]
    n = 2

    def call(ks=(1, 1), outs=None, n=n, offsets=(0, 0)):
        ins = [_buf(frame), _buf(frame)]
        outs = outs or [_buf(b"\xa5" * 300), _buf(b"\xa5" * 300)]
        out_sizes, rcs = (C.c_size_t * 2)(300, 300), (C.c_int * 2)(77, 77)
        rc = emu.bz3_hip_decompress_device_range_many(n, (C.c_uint32 * 2)(*ks), _vp(ins), (C.c_size_t * 2)(len(frame), len(frame)), (C.c_uint64 * 2)(*offsets), None, None,
                                                      _vp(outs), out_sizes, rcs)
        return rc, list(rcs), list(out_sizes), [bytes(o) for o in outs]

    assert call() == (0, [0, 0], [300, 300], [b"abc" * 100] * 2)
    assert call(ks=(1, 3)) == (INIT, [INIT, INIT], [0, 0], [b"\xa5" * 300] * 2)  # a bad element size
    assert call(n=-1)[0] == INIT
    assert emu.bz3_hip_decompress_device_range_many(0, None, None, None, None, None, None, None, None, None) == 0
    assert emu.bz3_hip_decompress_device_range_many(2, None, None, None, None, None, None, None, None, None) == INIT
    # offsets == NULL: offset 0 for every frame
    ins, outs = [_buf(frame)], [_buf(b"\xa5" * 10)]
    out_sizes, rcs = (C.c_size_t * 1)(10), (C.c_int * 1)(77)
    assert emu.bz3_hip_decompress_device_range_many(1, None, _vp(ins), (C.c_size_t * 1)(len(frame)), None, None, None, _vp(outs), out_sizes, rcs) == 0
    assert (rcs[0], out_sizes[0], bytes(outs[0])) == (0, 10, (b"abc" * 4)[:10])
    # a frame shorter than its header, alone and beside a good one
    rc, r, got, before = range_call(emu, 1, frame[:12], 0, 10)
    assert (rc, r) == (MALFORMED, 0) and got == before
