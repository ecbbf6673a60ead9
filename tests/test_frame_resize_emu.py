"""CPU tests of the resize (include/bz3_hip.h bz3_hip_resize_device[_many], the replane segment of bzip3_amd/csrc/planes.hpp through
bz3_hip_debug_replane, resize_frames of api_frames.hip) under the fiber emulation of the HIP execution model (tests/emu).

The oracle of a resize is always the reference's frame of the new bytes: f' == bz3_compress(block_size, S(x')), with S, D and pos written in
numpy from their definitions in bz3_hip.h (test_frame_planes_emu, test_frame_delta_emu, replane_model here), never the library under test.

BZ3_EMU_LIB=<path> runs the module on another build of the emulator library, as test_frame_update_emu does."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bzip3_amd
from oracle_lib import require_ref
from test_frame_delta_emu import D_inv, _base_for, _buf, _chunks, _host_alloc, _r16, _with_chunk
from test_frame_planes_emu import BS, S, _ref_decompress, _vp
from test_frame_range_emu import TILE, _flip, _with_header, clip_points
from test_frame_update_emu import ALL_COUNTS, FILL, INIT, LAST, MALFORMED, TOO_BIG, Case, pattern

HERE = os.path.dirname(os.path.abspath(__file__))
BS2 = 133_120  # the block size of the cases in which the effective block size changes (bz3_hip.h, "Resize")


@pytest.fixture(scope="module")
def emu():
    if os.environ.get("BZ3_EMU_LIB"):
        return bzip3_amd._declare(C.CDLL(os.environ["BZ3_EMU_LIB"]))
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def pos(c, length, k):
    """Where split_k keeps byte c of a chunk of `length` bytes: (c % k)(L / k) + c / k below (L / k) k, c in the tail."""
    m = length // k
    return np.where(c < m * k, (c % k) * m + c // k, c)


def replane_model(dst, src, k, len_old, len_new, a):
    """dst[pos(c; len_new)] = src[pos(c; len_old)] for c < a, and no other byte of dst."""
    out = dst.copy()
    c = np.arange(a)
    out[pos(c, len_new, k)] = src[pos(c, len_old, k)]
    return out


def replane_case(call, rng, spec, alloc):
    """spec: (src alignment, dst alignment mod 16, len_old, len_new, k, a) per segment, one after the other with guard bytes between them.
    alloc(array) -> (object for the hook, address, numpy reader); call(src, dst, table, n) -> rc.  The slots and the guard bytes start as random
    bytes; the whole destination allocation is compared with the model, the source with itself."""
    room_s = sum(s[2] for s in spec) + 56 * len(spec) + 64
    room_d = sum(s[3] for s in spec) + 56 * len(spec) + 64
    src_np = rng.integers(0, 256, size=room_s, dtype=np.uint8)
    dst_np = rng.integers(0, 256, size=room_d, dtype=np.uint8)
    src, dst = alloc(src_np), alloc(dst_np)
    table, want, so, do = [], dst_np.copy(), 0, 0
    for a_s, a_d, len_old, len_new, k, a in spec:
        so += (a_s - (src[1] + so)) % 16
        do += (a_d - (dst[1] + do)) % 16
        table += [so, do, len_old, len_new, k, a]
        want[do : do + len_new] = replane_model(dst_np[do : do + len_new], src_np[so : so + len_old], k, len_old, len_new, a)
        so += len_old + int(rng.integers(1, 40))
        do += len_new + int(rng.integers(1, 40))
    assert so <= room_s - 16 and do <= room_d - 16
    t = (C.c_uint64 * max(1, len(table)))(*table)
    assert call(src[0], dst[0], t, len(table) // 6) == 0
    bad = np.nonzero(dst[2]() != want)[0]
    assert bad.size == 0, ("bytes differ at", bad[:8], table[:12])
    assert np.array_equal(src[2](), src_np), "the source was written"


def new_lengths(rng, len_old, a, k):
    """New lengths below, equal to and above the old one that hold a kept bytes; the plane stride changes by every residue mod 16 over a sweep."""
    out = [len_old, len_old + int(rng.integers(1, 40)), len_old + k * int(rng.integers(16, 5000)) + int(rng.integers(0, k))]
    if a < len_old:
        out += [int(rng.integers(a, len_old)), a]
    return out


def sweep_specs_replane(rng, k, counts=ALL_COUNTS, alignments=True):
    """One launch per old element count and tail length 0..k-1: every a of clip_points with new lengths below, equal to and above the old one, at
    random alignments; then (`alignments`) the source alignment, the destination alignment and the change of the plane stride through all 16
    values each with the others random, on a chunk of two copy tiles and more per plane."""
    for elems in counts:
        for tail in range(k):
            len_old = elems * k + tail
            spec = [(_r16(rng), _r16(rng), len_old, ln, k, a) for a in clip_points(elems, tail, k) for ln in new_lengths(rng, len_old, a, k)]
            if spec:
                yield spec
    if not alignments:
        return
    spec = []
    for which in range(3):
        for v in range(16):
            al = [_r16(rng), _r16(rng), _r16(rng)]
            al[which] = v
            elems, tail = 2 * 16384 + int(rng.integers(1, 300)), int(rng.integers(0, k))
            len_old = elems * k + tail
            a = int(rng.integers(len_old - 40 * k, len_old + 1))
            spec.append((al[0], al[1], len_old, len_old + k * (16 + al[2]) + int(rng.integers(0, k)), k, a))
    yield spec


def mixed_spec_replane(rng):
    spec = []
    for _ in range(3):
        for k in (1, 2, 4, 8):
            len_old = int(rng.integers(20, 9000)) * k + int(rng.integers(0, k))
            a = int(rng.integers(0, len_old + 1))
            spec.append((_r16(rng), _r16(rng), len_old, a + int(rng.integers(0, 9000)), k, a))
    return spec


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_replane_kernel_every_count_tail_and_kept_size(emu, k):
    rng = np.random.default_rng(900 + k)
    for spec in sweep_specs_replane(rng, k, alignments=False):
        replane_case(emu.bz3_hip_debug_replane, rng, spec, _host_alloc)


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_replane_kernel_every_alignment(emu, k):
    rng = np.random.default_rng(910 + k)
    for spec in sweep_specs_replane(rng, k, counts=()):
        replane_case(emu.bz3_hip_debug_replane, rng, spec, _host_alloc)


def test_replane_kernel_mixed_element_sizes_in_one_launch(emu):
    rng = np.random.default_rng(92)
    replane_case(emu.bz3_hip_debug_replane, rng, mixed_spec_replane(rng), _host_alloc)
    replane_case(emu.bz3_hip_debug_replane, rng, [], _host_alloc)


def test_debug_replane_rejects_bad_arguments(emu):
    buf, dst = _buf(b"", 64), _buf(b"", 64)
    assert emu.bz3_hip_debug_replane(buf, dst, None, -1) == INIT
    assert emu.bz3_hip_debug_replane(buf, dst, None, 0) == 0
    for mode in (0, 3, 16, 2 | 0x100):  # bad element sizes, stray bits
        assert emu.bz3_hip_debug_replane(buf, dst, (C.c_uint64 * 6)(0, 0, 8, 8, mode, 4), 1) == INIT
    for len_old, len_new, a in ((8, 16, 9), (16, 8, 9)):  # a <= min(len_old, len_new)
        assert emu.bz3_hip_debug_replane(buf, dst, (C.c_uint64 * 6)(0, 0, len_old, len_new, 2, a), 1) == INIT
    assert bytes(dst) == bytes(64)


# ---- frames -------------------------------------------------------------------------------------------------------------------
def eff(bs, t, bound):
    """The effective block size of src/libbz3.c:877-878."""
    return max(65 * 1024, bound(t) if bs > t else bs)


def resize_cap(lib, bs, frame, keep, w):
    total = (keep if keep < 1 << 40 else 0) + w  # (a keep no frame holds: the call is refused whatever the room)
    b = eff(bs, total, lib.bz3_bound)
    return 13 + len(frame) + (-(-total // b) + 1) * (8 + lib.bz3_bound(b))


def resize_call(lib, bs, k, frame, keep, data, base=None, cap=None, alloc=_buf):
    """(rc, *out_size, out[0, cap) after the call).  base: the base's bytes of the appended range."""
    cap = resize_cap(lib, bs, frame, keep, len(data)) if cap is None else cap
    out = alloc(bytes([FILL]) * cap)
    osz = C.c_size_t(cap)
    rc = lib.bz3_hip_resize_device(bs, k, alloc(frame), len(frame), keep, alloc(data), len(data), None if base is None else alloc(base), out, C.byref(osz))
    return rc, osz.value, bytes(out)[:cap]


def resized(case, keep, w, seed=9):
    """(data, the base's bytes of the appended range or None, the bytes the new frame codes)."""
    d2 = pattern(w, seed)
    d = case.d[:keep] + d2
    if case.base is None:
        return d2, None, d
    rows = _base_for(w, seed + 70)
    return bytes(D_inv(d2, rows)), rows, d


def check_resize(lib, case, keep, w, frame=None, want=None, call=resize_call):
    data, rows, d = resized(case, keep, w)
    b = eff(case.bs, keep + w, case.ref.bz3_bound)
    if keep + w >= b and (keep + w) % b == 0:  # the reference would drop a block: never written
        return refused(lib, case.bs, case.k, case.frame if frame is None else frame, keep, data, INIT, rows, call=call)
    expect = case.expect(d)
    rc, size, out = call(lib, case.bs, case.k, case.frame if frame is None else frame, keep, data, rows)
    want = expect if want is None else want(expect)
    assert (rc, size) == (0, len(want)), (keep, w, rc, size, len(want))
    assert out[:size] == want, ("frames differ", keep, w)
    assert out[size:] == bytes([FILL]) * (len(out) - size), ("wrote beyond the frame", keep, w)
    return out[:size]


def refused(lib, bs, k, frame, keep, data, code, base=None, cap=None, call=resize_call):
    rc, size, out = call(lib, bs, k, frame, keep, data, base, cap)
    assert (rc, size) == (code, 0), (rc, size, code)
    assert out == bytes([FILL]) * len(out), "a refused call wrote to out"


def keeps_of(case):
    T = case.T
    return sorted({0, 1, T // 2, max(T - LAST // 2, 0), T - 1, T, *case.starts})


def widths_of(case, keep, bs=BS):
    """0, 1, up to one byte short of the next boundary, across it; two and more new chunks behind the first, a middle and the last byte."""
    to_edge = bs - keep % bs
    return sorted({0, 1, to_edge - 1, to_edge + 1} | ({2 * bs + 17} if keep in (0, case.T // 2, case.T) else set()))


def frames_match_reference(lib, k, chunks, call):
    ref = require_ref().lib
    case = Case(ref, k, chunks)
    assert case.sizes == [BS] * (chunks - 1) + [LAST]
    old = _chunks(case.frame)
    for keep in keeps_of(case):
        for w in widths_of(case, keep):
            got = check_resize(lib, case, keep, w, call=call)
            if got is None:
                continue
            new = _chunks(got)
            for j, (blk, orig) in enumerate(old):  # an old chunk that lies inside the kept bytes and keeps its extent is carried over
                if case.starts[j] + orig <= keep and (orig == BS or w == 0):
                    assert new[j] == (blk, orig), ("a copied chunk changed", keep, w, j)
            if (keep, w) == (case.T, 0):
                assert got == case.frame
            if w == 2 * BS + 17:  # round trip: the reference decodes f' to S(x')
                d = resized(case, keep, w)[2]
                assert _ref_decompress(ref, got, len(d) + 16) == (0, S(d, case.bs, case.k, ref.bz3_bound))


@pytest.mark.parametrize("chunks", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_resizes_of_a_frame_match_the_reference(emu, k, chunks, monkeypatch):
    """Blocks of 65 KiB, a short last chunk that is no multiple of k, windows of two chunks: f' is the reference's frame of S(x') byte for byte,
    nothing beyond it is written, and the chunks inside the kept bytes are those of f."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    frames_match_reference(emu, k, chunks, resize_call)


def block_size_changes(lib, k, call):
    """The sizes of bz3_hip.h's table: block_size 133,120; T = 100,000 has the header block size 102,032, + 20,000 gives 122,432, + 40,000 more
    133,120 and two chunks; and back."""
    ref = require_ref().lib
    one = Case(ref, k, 1, bs=BS2, total=100_000)
    assert (int.from_bytes(one.frame[5:9], "little"), one.sizes) == (102_032, [100_000])
    got = check_resize(lib, one, 100_000, 20_000, call=call)  # grows below block_size
    assert (int.from_bytes(got[5:9], "little"), [o for _, o in _chunks(got)]) == (122_432, [120_000])
    got = check_resize(lib, one, 100_000, 60_000, call=call)  # grows across it
    assert (int.from_bytes(got[5:9], "little"), [o for _, o in _chunks(got)]) == (BS2, [BS2, 160_000 - BS2])
    check_resize(lib, one, 70_001, 0, call=call)  # one block, cut back
    check_resize(lib, one, 99_999, 100_001, call=call)
    two = Case(ref, k, 2, bs=BS2, total=160_000)
    assert (int.from_bytes(two.frame[5:9], "little"), two.sizes) == (BS2, [BS2, 160_000 - BS2])
    got = check_resize(lib, two, 120_000, 0, call=call)  # truncated from above block_size to below it
    assert (int.from_bytes(got[5:9], "little"), [o for _, o in _chunks(got)]) == (122_432, [120_000])
    check_resize(lib, two, 100_003, 777, call=call)
    check_resize(lib, two, BS2 + 5, 0, call=call)  # stays above it: chunk 0 is copied
    check_resize(lib, two, 0, 0, call=call)  # T' == 0: the reference's frame of no bytes
    check_resize(lib, Case(ref, k, 1, bs=BS2, total=0), 0, 5000, call=call)  # and from it


@pytest.mark.parametrize("k", [1, 2, 8])
def test_effective_block_size_changes(emu, k):
    block_size_changes(emu, k, resize_call)


def delta_frames_match_reference(lib, k, call):
    case = Case(require_ref().lib, k, 2, with_base=True)
    for keep, w in ((case.T, 90), (case.T, BS + 5), (BS - 40, 100), (BS + 7, 0), (3, 1)):
        check_resize(lib, case, keep, w, call=call)


@pytest.mark.parametrize("k", [1, 4])
def test_resizes_of_a_delta_frame(emu, k):
    """f is a delta frame and `base` holds the appended range's bytes: the expectation is the reference's frame of S(D(x', b))."""
    delta_frames_match_reference(emu, k, resize_call)


def copied_chunks_are_not_decoded(lib, call):
    ref = require_ref().lib
    case = Case(ref, 2, 5)
    for j in (0, 3):  # an append cuts the last chunk alone
        bad = _flip(case.frame, j)
        assert _ref_decompress(ref, bad, case.T)[0] != 0
        blk, orig = _chunks(bad)[j]
        check_resize(lib, case, case.T, 500, frame=bad, want=lambda f: _with_chunk(f, j, blk, orig), call=call)
    bad = _flip(case.frame, 4)
    code = _ref_decompress(ref, bad, case.T)[0]
    assert code != 0
    refused(lib, BS, 2, bad, case.T, pattern(500, 9), code, call=call)
    # a truncation inside chunk 2: chunks 0 and 1 are copied, 2 is cut, 3 and 4 are dropped unread
    keep = 2 * BS + 100
    for j in (1, 3, 4):
        bad = _flip(case.frame, j)
        check_resize(lib, case, keep, 0, frame=bad, want=(lambda f: _with_chunk(f, 1, *_chunks(bad)[1])) if j == 1 else None, call=call)
    bad = _flip(case.frame, 2)
    refused(lib, BS, 2, bad, keep, b"", _ref_decompress(ref, bad, case.T)[0], call=call)


def test_copied_chunks_are_not_decoded(emu):
    """A flipped payload byte in a copied chunk: BZ3_OK, and the corrupt chunk is carried over verbatim.  In the cut chunk: the decoder's code,
    nothing written."""
    copied_chunks_are_not_decoded(emu, resize_call)


def resize_errors(lib, call):
    """(case, data) for the caller's own overlap checks."""
    ref = require_ref().lib
    case = Case(ref, 2, 2)
    T, frame = case.T, case.frame
    data = pattern(500, 9)
    refused(lib, BS, 2, frame, T + 1, data, TOO_BIG, call=call)  # keep > T
    refused(lib, BS, 2, frame, 2 ** 64 - 4, data, TOO_BIG, call=call)  # keep + w overflows
    # irregular frames: a short middle chunk, an empty last chunk, a header block size that is not eff(block_size, T)
    three = Case(ref, 2, 3)
    blk, _ = _chunks(Case(ref, 2, 1, total=BS - 2).frame)[0]
    refused(lib, BS, 2, _with_chunk(three.frame, 1, blk, BS - 2), three.T - 2, data, INIT, call=call)
    quirk = Case(ref, 2, 2, total=2 * BS)
    assert quirk.sizes == [BS, 0]
    refused(lib, BS, 2, quirk.frame, BS, data, INIT, call=call)
    refused(lib, BS + 2, 2, frame, T, data, INIT, call=call)
    refused(lib, BS2, 2, frame, T, data, INIT, call=call)
    one = Case(ref, 2, 1, bs=BS2, total=100_000)
    refused(lib, BS2 + 2, 2, frame[:5] + (102_034).to_bytes(4, "little") + one.frame[9:], 100_000, data, INIT, call=call)
    more = frame[:9] + (3).to_bytes(4, "little") + frame[13:]  # a chunk count the frame does not hold: the walk's own error
    refused(lib, BS, 2, more, T, data, _ref_decompress(ref, more, T + BS)[0], call=call)
    # T' a multiple of B
    refused(lib, BS, 2, frame, T, pattern(2 * BS - T, 9), INIT, call=call)
    refused(lib, BS, 2, frame, BS, b"", INIT, call=call)
    # capacity
    need = 13 + 8 + len(_chunks(frame)[0][0]) + 8 + ref.bz3_bound(LAST + 500)
    refused(lib, BS, 2, frame, T, data, TOO_BIG, cap=need - 1, call=call)
    rc, size, out = call(lib, BS, 2, frame, T, data, cap=need)
    assert (rc, out[:size]) == (0, case.expect(case.d + data)) and out[size:] == bytes([FILL]) * (need - size)
    refused(lib, BS, 2, frame, T, b"", TOO_BIG, cap=len(frame) - 1, call=call)
    assert call(lib, BS, 2, frame, T, b"", cap=len(frame))[:2] == (0, len(frame))
    # a malformed chunk header behind keep is reported
    for bad in (_with_header(frame, 1, orig=-5), _with_header(frame, 1, size=-1), _with_header(frame, 1, size=BS + 1)):
        refused(lib, BS, 2, bad, 10, data, MALFORMED, call=call)
    refused(lib, BS, 2, frame[: len(frame) - 10], 10, data, bzip3_amd.BZ3_ERR_TRUNCATED_DATA, call=call)
    refused(lib, BS, 2, frame[:12], 0, b"", MALFORMED, call=call)  # in_size < 13
    refused(lib, BS, 2, b"XZ3v1" + frame[5:], 0, data, MALFORMED, call=call)
    refused(lib, BS, 3, frame, 0, data, INIT, call=call)  # a bad element size
    return case, data


def test_resize_errors_leave_out_untouched(emu):
    ref = require_ref().lib
    case, data = resize_errors(emu, resize_call)
    frame, T = case.frame, case.T
    # overlaps of out with in, data and base
    arena = _buf(bytes([FILL]) * (4 * len(frame) + 4 * BS))
    cap = len(frame) + 3 * ref.bz3_bound(BS)
    C.memmove(arena, frame, len(frame))
    before = bytes(arena)
    for in_off, out_off in ((0, len(frame) - 1), (0, 0)):
        osz = C.c_size_t(cap)
        assert emu.bz3_hip_resize_device(BS, 2, C.byref(arena, in_off), len(frame), T, _buf(data), len(data), None, C.byref(arena, out_off), C.byref(osz)) == INIT
        assert osz.value == 0 and bytes(arena) == before
    arena2 = _buf(bytes([FILL]) * (cap + 2000))
    C.memmove(C.byref(arena2, cap - 1), data, len(data))
    before = bytes(arena2)
    for which in ("data", "base"):
        osz = C.c_size_t(cap)
        inside = C.byref(arena2, cap - 1)
        rc = emu.bz3_hip_resize_device(BS, 2, _buf(frame), len(frame), T, inside if which == "data" else _buf(data), len(data), inside if which == "base" else None, arena2,
                                       C.byref(osz))
        assert rc == INIT and osz.value == 0 and bytes(arena2) == before, which
    osz = C.c_size_t(cap)  # adjacent: fine
    assert emu.bz3_hip_resize_device(BS, 2, _buf(frame), len(frame), T, C.byref(arena2, cap), len(data), None, arena2, C.byref(osz)) == 0
    assert emu.bz3_hip_resize_device(BS, 2, _buf(frame), len(frame), T, _buf(data), len(data), None, arena2, None) == INIT


# ---- many ---------------------------------------------------------------------------------------------------------------------
def many_call(lib, bss, ks, frames, keeps, datas, bases, caps=None):
    n = len(frames)
    caps = [resize_cap(lib, bs, f, keep, len(d)) for bs, f, keep, d in zip(bss, frames, keeps, datas)] if caps is None else caps
    ins, dbufs = [_buf(f) for f in frames], [_buf(d) for d in datas]
    bbufs = [None if b is None else _buf(b) for b in bases]
    outs = [_buf(bytes([FILL]) * c) for c in caps]
    out_sizes, rcs = (C.c_size_t * n)(*caps), (C.c_int * n)(*([77] * n))
    bp = (C.c_void_p * n)(*[None if b is None else C.addressof(b) for b in bbufs])
    rc = lib.bz3_hip_resize_device_many(n, (C.c_uint32 * n)(*bss), (C.c_uint32 * n)(*ks), _vp(ins), (C.c_size_t * n)(*map(len, frames)), (C.c_uint64 * n)(*keeps), _vp(dbufs),
                                        (C.c_size_t * n)(*map(len, datas)), bp, _vp(outs), out_sizes, rcs)
    return rc, [(rcs[i], out_sizes[i], bytes(outs[i])[: caps[i]]) for i in range(n)]


def many_equal_single_calls(lib, many_call, resize_call):
    ref = require_ref().lib
    shapes = ((2, 2, 0, BS, None), (1, 1, 1, BS, None), (8, 5, 0, BS, None), (4, 2, 1, BS, None), (4, 1, 0, BS2, 100_000), (2, 2, 0, BS, None), (2, 2, 0, BS, None))
    cases = [Case(ref, k, chunks, wb, bs=bs, seed=20 + i, total=total) for i, (k, chunks, wb, bs, total) in enumerate(shapes)]
    plan = [(cases[0].T, 100), (700, 300), (3 * BS + 5, 2 * BS), (cases[3].T, BS), (100_000, 60_000), (cases[5].T, 2), (cases[6].T, 0)]
    frames = [c.frame for c in cases]
    frames[5] = _flip(frames[5], 1)  # its cut chunk is corrupt
    bss, ks, keeps = [c.bs for c in cases], [c.k for c in cases], [keep for keep, _ in plan]
    ups = [resized(c, keep, w) for c, (keep, w) in zip(cases, plan)]
    datas, bases = [u[0] for u in ups], [u[1] for u in ups]
    rc, got = many_call(lib, bss, ks, frames, keeps, datas, bases)
    bad_code = _ref_decompress(ref, frames[5], cases[5].T)[0]
    assert rc == bad_code != 0
    for i in range(7):
        assert got[i] == resize_call(lib, bss[i], ks[i], frames[i], keeps[i], datas[i], bases[i]), ("single call", i)
        if i != 5:
            assert got[i][0] == 0 and got[i][2][: got[i][1]] == cases[i].expect(ups[i][2]), i
    assert got[5][:2] == (bad_code, 0) and got[5][2] == bytes([FILL]) * len(got[5][2])
    assert got[6][2][: got[6][1]] == frames[6]


def test_many_resizes_equal_their_single_calls(emu, monkeypatch):
    """Seven frames of mixed k and block size in one call, two with a base, one truncated, one whose block size changes, one copied verbatim,
    one whose cut chunk is corrupt; windows of three chunks."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    many_equal_single_calls(emu, many_call, resize_call)


def appends_share_launches(lib, many_call, n=64):
    ref = require_ref().lib
    case = Case(ref, 2, 2)
    data, _, d = resized(case, case.T, 50)
    lib.bz3_hip_debug_cm_launches(1)
    rc, got = many_call(lib, [BS] * n, [2] * n, [case.frame] * n, [case.T] * n, [data] * n, [None] * n)
    assert lib.bz3_hip_debug_cm_launches(1) <= 2  # one decode and one encode launch
    expect = case.expect(d)
    assert rc == 0 and all(g[0] == 0 and g[2][: g[1]] == expect for g in got)


def test_many_appends_share_their_cm_launches(emu):
    appends_share_launches(emu, many_call)


def test_many_whole_call_errors(emu):
    case = Case(require_ref().lib, 1, 1)
    data = pattern(40, 9)
    assert emu.bz3_hip_resize_device_many(0, None, None, None, None, None, None, None, None, None, None, None) == 0
    assert emu.bz3_hip_resize_device_many(2, None, None, None, None, None, None, None, None, None, None, None) == INIT
    rc, got = many_call(emu, [BS] * 2, [1, 3], [case.frame] * 2, [0, 0], [data] * 2, [None] * 2)  # a bad element size fails the whole call
    assert rc == INIT and all(g[:2] == (INIT, 0) and g[2] == bytes([FILL]) * len(g[2]) for g in got)
    # elem_sizes and bases NULL: k = 1, no base
    cap = resize_cap(emu, BS, case.frame, case.T, len(data))
    ins, dbuf, outs = [_buf(case.frame)], [_buf(data)], [_buf(bytes([FILL]) * cap)]
    out_sizes, rcs = (C.c_size_t * 1)(cap), (C.c_int * 1)(77)
    assert emu.bz3_hip_resize_device_many(1, (C.c_uint32 * 1)(BS), None, _vp(ins), (C.c_size_t * 1)(len(case.frame)), (C.c_uint64 * 1)(case.T), _vp(dbuf),
                                          (C.c_size_t * 1)(len(data)), None, _vp(outs), out_sizes, rcs) == 0
    assert rcs[0] == 0 and bytes(outs[0])[: out_sizes[0]] == case.expect(case.d + data)
