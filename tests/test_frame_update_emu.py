"""CPU tests of the range update (include/bz3_hip.h bz3_hip_update_device_range[_many], the clipped split of bzip3_amd/csrc/planes.hpp through
bz3_hip_debug_patch, update_frames of api_frames.hip) under the fiber emulation of the HIP execution model (tests/emu).

The oracle of an update is always the reference's frame of the updated bytes: f' == bz3_compress(bs, S(x')), with S, D and the clipped split's
formula written in numpy from their definitions in bz3_hip.h (test_frame_planes_emu, test_frame_delta_emu, patch_model here), never the library
under test.

BZ3_EMU_LIB=<path> runs the module on another build of the emulator library, as test_frame_delta_emu does; every buffer handed to the library
comes from that module's _buf and lies inside a larger allocation."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

import bzip3_amd
from oracle_lib import require_ref
from test_frame_delta_emu import NO_BASE, D, D_inv, _base_for, _buf, _chunks, _host_alloc, _r16, _with_chunk
from test_frame_planes_emu import BS, COUNTS, S, _ref_compress, _ref_decompress, _vp, merge_k, per_block
from test_frame_range_emu import EDGE_COUNTS, TILE, _flip, _with_header, clip_points

HERE = os.path.dirname(os.path.abspath(__file__))
INIT, MALFORMED, TOO_BIG = bzip3_amd.BZ3_ERR_INIT, bzip3_amd.BZ3_ERR_MALFORMED_HEADER, bzip3_amd.BZ3_ERR_DATA_TOO_BIG
ALL_COUNTS = tuple(dict.fromkeys(COUNTS + EDGE_COUNTS))
FILL = 0xA5


@pytest.fixture(scope="module")
def emu():
    if os.environ.get("BZ3_EMU_LIB"):
        return bzip3_amd._declare(C.CDLL(os.environ["BZ3_EMU_LIB"]))
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def patch_model(old, k, a, b, new):
    """The slot `old` (split_k of a chunk of len(old) bytes) after a clipped split: dst[q m + e] = new[e k + q - a] for a <= e k + q < b below
    m k, the tail bytes in place; every other byte as it was."""
    out = old.copy()
    m = len(old) // k
    c = np.arange(a, b)
    at = np.where(c < m * k, (c % k) * m + c // k, c)
    out[at] = new
    return out


def lay_out_patch(rng, spec, addrs, src_np, base_np, dst_np):
    """spec: (src, base, slot alignment mod 16, elements, tail bytes, k, has base, a, b) per segment, one after the other with gaps; the src and
    base alignments are those of the clip's first byte.  Returns the hook's table and the expected destination."""
    table, want, offs = [], dst_np.copy(), [0, 0, 0]
    for a_s, a_b, a_d, elems, tail, k, has_base, a, b in spec:
        n = elems * k + tail
        for j, al in enumerate((a_s, a_b, a_d)):
            offs[j] += (al - (addrs[j] + offs[j])) % 16
        s, bo, d = offs
        table += [s, bo if has_base else NO_BASE, d, n, k, a, b]
        new = src_np[s : s + b - a]
        want[d : d + n] = patch_model(dst_np[d : d + n], k, a, b, D(new, base_np[bo : bo + b - a]) if has_base else new)
        offs[0] += b - a + int(rng.integers(1, 40))
        offs[1] += b - a + int(rng.integers(1, 40))
        offs[2] += n + int(rng.integers(1, 40))  # guard bytes between the slots
    return table, want, offs


def patch_case(call, rng, spec, alloc):
    """alloc(array) -> (object for the hook, address, numpy reader); call(src, base, dst, table, n) -> rc.  The slots and the guard bytes around
    them start as random bytes and the whole destination is compared against the model; the inputs against themselves."""
    room_s = sum(b - a for *_, a, b in spec) + 56 * len(spec) + 64
    room_d = sum(e * k + t for _, _, _, e, t, k, _, _, _ in spec) + 56 * len(spec) + 64
    src_np = rng.integers(0, 256, size=room_s, dtype=np.uint8)
    base_np = rng.integers(0, 256, size=room_s, dtype=np.uint8)
    dst_np = rng.integers(0, 256, size=room_d, dtype=np.uint8)
    src, base, dst = alloc(src_np), alloc(base_np), alloc(dst_np)
    table, want, ends = lay_out_patch(rng, spec, (src[1], base[1], dst[1]), src_np, base_np, dst_np)
    assert max(ends[:2]) <= room_s - 16 and ends[2] <= room_d - 16
    t = (C.c_uint64 * max(1, len(table)))(*table)
    assert call(src[0], base[0], dst[0], t, len(table) // 7) == 0
    bad = np.nonzero(dst[2]() != want)[0]
    assert bad.size == 0, ("bytes differ at", bad[:8], table[:14])
    assert np.array_equal(src[2](), src_np) and np.array_equal(base[2](), base_np), "an input was written"


def sweep_specs_patch(rng, k, has_base, counts=ALL_COUNTS, alignments=True):
    """One launch per element count and tail length 0..k-1: every pair a < b of clip_points, all at random alignments; then (`alignments`) each
    of the three alignments through all 16 values with the other two random, on a chunk of two tiles and more clipped at random interior bytes."""
    for elems in counts:
        for tail in range(k):
            pts = clip_points(elems, tail, k)
            spec = [(_r16(rng), _r16(rng), _r16(rng), elems, tail, k, has_base, a, b) for i, a in enumerate(pts) for b in pts[i + 1 :]]
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
            a, b = sorted(int(v) for v in rng.integers(0, elems * k + tail + 1, size=2))
            spec.append((*al, elems, tail, k, has_base, a, b))
    yield spec


def mixed_spec_patch(rng):
    """One launch that holds clipped splits, whole splits, plain copies (k = 1, no base) and delta copies (k = 1 with a base) of every k."""
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


@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("elems", ALL_COUNTS)
def test_patch_kernel_every_clip_pair_at_every_tail(emu, elems, k, has_base):
    rng = np.random.default_rng(700 + 100 * elems + 10 * k + has_base)
    for spec in sweep_specs_patch(rng, k, has_base, counts=(elems,), alignments=False):
        patch_case(emu.bz3_hip_debug_patch, rng, spec, _host_alloc)


@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_patch_kernel_every_alignment(emu, k, has_base):
    rng = np.random.default_rng(700 + 10 * k + has_base)
    for spec in sweep_specs_patch(rng, k, has_base, counts=()):
        patch_case(emu.bz3_hip_debug_patch, rng, spec, _host_alloc)


def test_patch_kernel_mixed_segments_in_one_launch(emu):
    rng = np.random.default_rng(72)
    patch_case(emu.bz3_hip_debug_patch, rng, mixed_spec_patch(rng), _host_alloc)
    patch_case(emu.bz3_hip_debug_patch, rng, [], _host_alloc)


def test_debug_patch_rejects_bad_arguments(emu):
    buf = _buf(b"", 64)
    assert emu.bz3_hip_debug_patch(buf, buf, buf, None, -1) == INIT
    assert emu.bz3_hip_debug_patch(buf, buf, buf, None, 0) == 0
    for mode in (0, 3, 16, 2 | 0x100, 2 | 0x200):  # bad element sizes, the inverse direction, stray bits
        assert emu.bz3_hip_debug_patch(buf, buf, buf, (C.c_uint64 * 7)(0, 0, 32, 8, mode, 0, 8), 1) == INIT
    for a, b in ((5, 4), (0, 9), (9, 9)):  # a <= b <= len
        assert emu.bz3_hip_debug_patch(buf, buf, buf, (C.c_uint64 * 7)(0, 0, 32, 8, 2, a, b), 1) == INIT
    assert bytes(buf) == bytes(64)


# ---- frames -------------------------------------------------------------------------------------------------------------------
LAST = 1235  # the short last chunk: no multiple of 2, 4 or 8


def pattern(n, seed):
    """n bytes of period 1000 (a multiple of every k, so every byte plane of it is periodic too: LZP collapses them and the emulated CM stage
    stays small)."""
    unit = bytes(np.random.default_rng(seed).integers(0, 256, size=1000, dtype=np.uint8))
    return (unit * (n // 1000 + 1))[:n]


class Case:
    """A frame the reference made: f = bz3_compress(bs, S(d)), d = D(x, base) (d = x without a base), of `chunks` chunks of which the last is
    LAST bytes."""

    def __init__(self, ref, k, chunks, with_base=False, bs=BS, seed=3, total=None):
        self.ref, self.k, self.bs = ref, k, bs
        n = (chunks - 1) * bs + LAST if total is None else total
        self.d = pattern(n, seed)
        self.base = _base_for(n, seed + 50) if with_base else None
        self.x = bytes(D_inv(self.d, self.base)) if with_base else self.d
        self.frame = self.expect(self.d)
        self.sizes = [o for _, o in _chunks(self.frame)]
        self.starts = [sum(self.sizes[:j]) for j in range(len(self.sizes))]
        self.T = sum(self.sizes)

    def expect(self, d):
        rc, f = _ref_compress(self.ref, self.bs, S(d, self.bs, self.k, self.ref.bz3_bound))
        assert rc == 0
        return f

    def updated(self, offset, w, seed=9):
        """(data, the base's bytes of the range or None, the frame the update must give)."""
        d2 = pattern(w, seed)
        d = self.d[:offset] + d2 + self.d[offset + w :]
        if self.base is None:
            return d2, None, self.expect(d)
        rows = self.base[offset : offset + w]
        return bytes(D_inv(d2, rows)), rows, self.expect(d)

    def touched(self, offset, w):
        return [j for j, (p, o) in enumerate(zip(self.starts, self.sizes)) if w > 0 and o > 0 and p < offset + w and p + o > offset]

    def need(self, offset, w):
        t = self.touched(offset, w)
        return 13 + sum(8 + (self.ref.bz3_bound(o) if j in t else len(blk)) for j, (blk, o) in enumerate(_chunks(self.frame)))


def update_call(lib, k, frame, offset, data, base=None, cap=None, alloc=_buf):
    """(rc, *out_size, out[0, cap) after the call).  base: the base's bytes of the range."""
    cap = len(frame) + (len(data) // BS + 2) * lib.bz3_bound(BS) if cap is None else cap
    out = alloc(bytes([FILL]) * cap)
    osz = C.c_size_t(cap)
    rc = lib.bz3_hip_update_device_range(k, alloc(frame), len(frame), offset, alloc(data), len(data), None if base is None else alloc(base), out, C.byref(osz))
    return rc, osz.value, bytes(out)[:cap]


def check_update(lib, case, offset, w, frame=None, want=None, call=update_call):
    data, rows, expect = case.updated(offset, w)
    rc, size, out = call(lib, case.k, case.frame if frame is None else frame, offset, data, rows)
    want = expect if want is None else want(expect)
    assert (rc, size) == (0, len(want)), (offset, w, rc, size, len(want))
    assert out[:size] == want, ("frames differ", offset, w)
    assert out[size:] == bytes([FILL]) * (len(out) - size), ("wrote beyond the frame", offset, w)
    return out[:size]


def refused(lib, k, frame, offset, data, code, base=None, cap=None, call=update_call):
    rc, size, out = call(lib, k, frame, offset, data, base, cap)
    assert (rc, size) == (code, 0), (rc, size, code)
    assert out == bytes([FILL]) * len(out), "a refused call wrote to out"


def frame_ranges(case):
    T, s, z = case.T, case.starts, case.sizes
    yield T // 2, 1  # one byte
    yield 100, 1100  # inside one chunk
    j = min(1, len(z) - 1)
    yield s[j], z[j]  # exactly one chunk
    if len(z) > 1:
        yield s[1] - 1, 2  # across a chunk boundary by one byte on either side
    yield 0, 777
    yield T - 300, 300
    yield 0, T
    yield 5, 0
    if len(z) >= 5:
        yield s[1] - 7, 3 * z[1]  # four chunks, the first and the last of them cut: more than a window of two or three


def frames_match_reference(lib, k, chunks, call, decode):
    """decode(lib, k, frame, room) -> (rc, the bytes bz3_hip_decompress_device_planes commits)."""
    case = Case(require_ref().lib, k, chunks)
    assert case.sizes == [BS] * (chunks - 1) + [LAST]
    old = _chunks(case.frame)
    for offset, w in frame_ranges(case):
        got = check_update(lib, case, offset, w, call=call)
        new, t = _chunks(got), case.touched(offset, w)
        assert all(new[j] == old[j] for j in range(chunks) if j not in t), ("an untouched chunk changed", offset, w)
        if w == 0:
            assert got == case.frame
        if (offset, w) in ((0, case.T), (100, 1100)):  # round trip: f' decodes to x'
            data = case.updated(offset, w)[0]
            assert decode(lib, k, got, case.T + 16) == (0, case.d[:offset] + data + case.d[offset + w :])


def host_decode(lib, k, frame, room):
    back = _buf(b"", room)
    bsz = C.c_size_t(room)
    rc = lib.bz3_hip_decompress_device_planes(k, _buf(frame), back, len(frame), C.byref(bsz))
    return rc, C.string_at(back, bsz.value)


@pytest.mark.parametrize("chunks", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_updates_of_a_frame_match_the_reference(emu, k, chunks, monkeypatch):
    """Blocks of 65 KiB, a short last chunk that is no multiple of k, windows of two chunks: f' is the reference's frame of S(x') byte for byte,
    nothing beyond it is written, the untouched chunks are those of f, and f' decodes to x'."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    frames_match_reference(emu, k, chunks, update_call, host_decode)


def delta_frames_match_reference(lib, k, call):
    case = Case(require_ref().lib, k, 2, with_base=True)
    for offset, w in ((BS - 40, 90), (3, 1), (0, case.T), (BS, LAST)):
        check_update(lib, case, offset, w, call=call)


@pytest.mark.parametrize("k", [1, 4])
def test_updates_of_a_delta_frame(emu, k):
    """f is a delta frame and `base` holds the range's bytes: the expectation is the reference's frame of S(D(x', b))."""
    delta_frames_match_reference(emu, k, update_call)


def untouched_chunks_are_not_decoded(lib, call):
    ref = require_ref().lib
    case = Case(ref, 2, 5)
    offset, w = case.starts[2] + 10, BS + 20  # cuts chunks 2 and 3
    for j in (0, 1, 4):
        bad = _flip(case.frame, j)
        assert _ref_decompress(ref, bad, case.T)[0] != 0
        blk, orig = _chunks(bad)[j]
        check_update(lib, case, offset, w, frame=bad, want=lambda f: _with_chunk(f, j, blk, orig), call=call)
    data, _, _ = case.updated(offset, w)
    for j in (2, 3):
        bad = _flip(case.frame, j)
        code = _ref_decompress(ref, bad, case.T)[0]
        assert code != 0
        refused(lib, 2, bad, offset, data, code, call=call)
    # a covered chunk is rebuilt from the new bytes alone: its old payload is not looked at either
    bad = _flip(case.frame, 1)
    check_update(lib, case, case.starts[1], BS, frame=bad, call=call)


def test_untouched_chunks_are_not_decoded(emu):
    """A flipped payload byte in an untouched chunk: the reference refuses the frame, the update returns BZ3_OK and carries the corrupt chunk
    over verbatim.  In a cut chunk: the decoder's code, nothing written."""
    untouched_chunks_are_not_decoded(emu, update_call)


def empty_last_chunk_is_copied(lib, call):
    case = Case(require_ref().lib, 4, 2, total=2 * BS)
    assert case.sizes == [BS, 0] and case.T == BS
    old = _chunks(case.frame)
    for offset, w in ((0, BS), (BS - 10, 10), (7, 0)):
        got = check_update(lib, case, offset, w, call=call)
        assert _chunks(got)[1] == old[1]
    refused(lib, 4, case.frame, BS - 1, b"ab", TOO_BIG, call=call)


def test_empty_last_chunk_is_copied_verbatim(emu):
    """A stream of exactly two blocks: the reference codes its (sic) last block from 0 bytes; the update copies that chunk."""
    empty_last_chunk_is_copied(emu, update_call)


def update_errors(lib, call):
    """(case, data) for the caller's own overlap checks."""
    ref = require_ref().lib
    case = Case(ref, 2, 2)
    T, frame = case.T, case.frame
    data = pattern(500, 9)
    refused(lib, 2, frame, T - 499, data, TOO_BIG, call=call)  # offset + w > T
    refused(lib, 2, frame, 2 ** 64 - 4, data, TOO_BIG, call=call)  # offset + w overflows
    refused(lib, 2, frame, T, b"x", TOO_BIG, call=call)
    offset = BS - 100  # cuts both chunks
    need = case.need(offset, 500)
    assert need == 13 + 2 * (8 + ref.bz3_bound(BS)) - ref.bz3_bound(BS) + ref.bz3_bound(LAST)
    refused(lib, 2, frame, offset, data, TOO_BIG, cap=need - 1, call=call)
    rc, size, out = call(lib, 2, frame, offset, data, cap=need)
    assert (rc, out[:size]) == (0, case.updated(offset, 500)[2]) and out[size:] == bytes([FILL]) * (need - size)
    need0 = case.need(0, 0)
    assert need0 == len(frame)
    refused(lib, 2, frame, 0, b"", TOO_BIG, cap=need0 - 1, call=call)
    assert call(lib, 2, frame, 0, b"", cap=need0)[:2] == (0, need0)
    # a malformed header in a chunk BEHIND the range is reported: here the update is stricter than range decode
    for bad in (_with_header(frame, 1, orig=-5), _with_header(frame, 1, size=-1), _with_header(frame, 1, size=BS + 1)):
        refused(lib, 2, bad, 10, data, MALFORMED, call=call)
    refused(lib, 2, frame[: len(frame) - 10], 10, data, bzip3_amd.BZ3_ERR_TRUNCATED_DATA, call=call)
    refused(lib, 2, frame[:12], 0, b"", MALFORMED, call=call)  # in_size < 13
    refused(lib, 2, b"XZ3v1" + frame[5:], 0, data, MALFORMED, call=call)
    refused(lib, 3, frame, 0, data, INIT, call=call)  # a bad element size
    return case, data


def test_update_errors_leave_out_untouched(emu):
    ref = require_ref().lib
    case, data = update_errors(emu, update_call)
    frame = case.frame
    # overlaps of out with in, data and base
    arena = _buf(bytes([FILL]) * (4 * len(frame) + 4 * BS))
    cap = len(frame) + 3 * ref.bz3_bound(BS)
    C.memmove(arena, frame, len(frame))
    before = bytes(arena)
    for in_off, out_off in ((0, len(frame) - 1), (0, 0)):
        osz = C.c_size_t(cap)
        assert emu.bz3_hip_update_device_range(2, C.byref(arena, in_off), len(frame), 10, _buf(data), len(data), None, C.byref(arena, out_off), C.byref(osz)) == INIT
        assert osz.value == 0 and bytes(arena) == before
    arena2 = _buf(bytes([FILL]) * (cap + 2000))
    C.memmove(C.byref(arena2, cap - 1), data, len(data))
    before = bytes(arena2)
    for which in ("data", "base"):
        osz = C.c_size_t(cap)
        inside = C.byref(arena2, cap - 1)
        rc = emu.bz3_hip_update_device_range(2, _buf(frame), len(frame), 10, inside if which == "data" else _buf(data), len(data), inside if which == "base" else None, arena2,
                                             C.byref(osz))
        assert rc == INIT and osz.value == 0 and bytes(arena2) == before, which
    osz = C.c_size_t(cap)  # adjacent: fine
    assert emu.bz3_hip_update_device_range(2, _buf(frame), len(frame), 10, C.byref(arena2, cap), len(data), None, arena2, C.byref(osz)) == 0
    assert emu.bz3_hip_update_device_range(2, _buf(frame), len(frame), 10, _buf(data), len(data), None, arena2, None) == INIT


# ---- many ---------------------------------------------------------------------------------------------------------------------
def many_call(lib, ks, frames, offsets, datas, bases, caps=None):
    n = len(frames)
    caps = [len(f) + (len(d) // BS + 2) * lib.bz3_bound(BS) for f, d in zip(frames, datas)] if caps is None else caps
    ins, dbufs = [_buf(f) for f in frames], [_buf(d) for d in datas]
    bbufs = [None if b is None else _buf(b) for b in bases]
    outs = [_buf(bytes([FILL]) * c) for c in caps]
    out_sizes, rcs = (C.c_size_t * n)(*caps), (C.c_int * n)(*([77] * n))
    bp = (C.c_void_p * n)(*[None if b is None else C.addressof(b) for b in bbufs])
    rc = lib.bz3_hip_update_device_range_many(n, (C.c_uint32 * n)(*ks), _vp(ins), (C.c_size_t * n)(*map(len, frames)), (C.c_uint64 * n)(*offsets), _vp(dbufs),
                                              (C.c_size_t * n)(*map(len, datas)), bp, _vp(outs), out_sizes, rcs)
    return rc, [(rcs[i], out_sizes[i], bytes(outs[i])[: caps[i]]) for i in range(n)]


def many_equal_single_calls(emu, many_call, update_call):
    ref = require_ref().lib
    cases = [Case(ref, k, chunks, wb, seed=20 + i) for i, (k, chunks, wb) in enumerate(((2, 2, 0), (1, 1, 1), (8, 5, 0), (4, 2, 1), (4, 1, 0), (2, 2, 0)))]
    plan = [(BS - 30, 100), (7, 300), (BS + 5, 2 * BS), (0, cases[3].T), (5, 0), (BS - 1, 2)]
    frames = [c.frame for c in cases]
    frames[5] = _flip(frames[5], 1)
    ks, offsets = [c.k for c in cases], [o for o, _ in plan]
    ups = [c.updated(o, w) for c, (o, w) in zip(cases, plan)]
    datas, bases = [u[0] for u in ups], [u[1] for u in ups]
    rc, got = many_call(emu, ks, frames, offsets, datas, bases)
    bad_code = _ref_decompress(ref, frames[5], cases[5].T)[0]
    assert rc == bad_code != 0
    for i in range(6):
        assert got[i] == update_call(emu, ks[i], frames[i], offsets[i], datas[i], bases[i]), ("single call", i)
        if i < 5:
            assert got[i][0] == 0 and got[i][2][: got[i][1]] == ups[i][2], i
    assert got[5][:2] == (bad_code, 0) and got[5][2] == bytes([FILL]) * len(got[5][2])
    assert got[4][2][: got[4][1]] == frames[4]


def test_many_updates_equal_their_single_calls(emu, monkeypatch):
    """Six frames of mixed k in one call, two with a base, one with w == 0, one whose cut chunk is corrupt; windows of three chunks."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    many_equal_single_calls(emu, many_call, update_call)


def one_chunk_updates_share_launches(emu, many_call):
    ref = require_ref().lib
    case = Case(ref, 2, 2)
    n = 6
    for (offset, w), launches in (((100 + 0, 50), 2), ((0, BS), 1)):  # six cut chunks: one decode and one encode launch; six covered ones: one encode launch
        data, _, expect = case.updated(offset, w)
        emu.bz3_hip_debug_cm_launches(1)
        rc, got = many_call(emu, [2] * n, [case.frame] * n, [offset] * n, [data] * n, [None] * n)
        assert emu.bz3_hip_debug_cm_launches(1) == launches
        assert rc == 0 and all(g[0] == 0 and g[2][: g[1]] == expect for g in got)


def test_many_one_chunk_updates_share_their_cm_launches(emu):
    one_chunk_updates_share_launches(emu, many_call)


def test_many_whole_call_errors(emu):
    case = Case(require_ref().lib, 1, 1)
    data = pattern(40, 9)
    assert emu.bz3_hip_update_device_range_many(0, None, None, None, None, None, None, None, None, None, None) == 0
    assert emu.bz3_hip_update_device_range_many(2, None, None, None, None, None, None, None, None, None, None) == INIT
    rc, got = many_call(emu, [1, 3], [case.frame] * 2, [0, 0], [data] * 2, [None] * 2)  # a bad element size fails the whole call
    assert rc == INIT and all(g[:2] == (INIT, 0) and g[2] == bytes([FILL]) * len(g[2]) for g in got)
    # offsets, elem_sizes and bases NULL: offset 0, k = 1, no base
    cap = len(case.frame) + 2 * emu.bz3_bound(BS)
    ins, dbuf, outs = [_buf(case.frame)], [_buf(data)], [_buf(bytes([FILL]) * cap)]
    out_sizes, rcs = (C.c_size_t * 1)(cap), (C.c_int * 1)(77)
    assert emu.bz3_hip_update_device_range_many(1, None, _vp(ins), (C.c_size_t * 1)(len(case.frame)), None, _vp(dbuf), (C.c_size_t * 1)(len(data)), None, _vp(outs), out_sizes, rcs) == 0
    assert rcs[0] == 0 and bytes(outs[0])[: out_sizes[0]] == case.expect(data + case.d[len(data) :])
