"""CPU tests of the sync (include/bz3_hip.h bz3_hip_sync_device[_many], k_diff_segments of bzip3_amd/csrc/planes.hpp through bz3_hip_debug_diff,
update_frames of api_frames.hip in its sync mode) under the fiber emulation of the HIP execution model (tests/emu).

The oracle of a sync is the reference's frame of the new bytes: f' == bz3_compress(bs, S_k(D(new, base))), with S and D written in numpy from their
definitions (test_frame_planes_emu, test_frame_delta_emu), and numpy's own comparison for the dirty chunks and the kernel's flags; never the library
under test.

BZ3_EMU_LIB=<path> runs the module on another build of the emulator library, as test_frame_update_emu does."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
from oracle_lib import require_ref
from test_frame_delta_emu import D, _buf, _chunks, _with_chunk
from test_frame_planes_emu import BS, _ref_decompress, _vp
from test_frame_range_emu import _flip, _with_header
from test_frame_update_emu import FILL, INIT, LAST, MALFORMED, TOO_BIG, Case, emu  # noqa: F401  (emu: the module's fixture)

# ---- the kernel ---------------------------------------------------------------------------------------------------------------
TILE_BYTES = 16 << 10  # COPY_TILE_GRANULES granules of 16 bytes
LENGTHS = (0, 1, 15, 16, 17, 31, 33, TILE_BYTES - 17, TILE_BYTES - 1, TILE_BYTES, TILE_BYTES + 1, TILE_BYTES + 17, 2 * TILE_BYTES + 5)
ALIGNS = (0, 7, 9)
BATCH = 256  # runs of one launch of the sweep


def _aligned_host(a):
    """(address, reader) of a 16-byte aligned host copy of the array."""
    raw = (C.c_uint8 * (len(a) + 32))()
    buf = (C.c_uint8 * max(1, len(a))).from_buffer(raw, (-C.addressof(raw)) % 16)
    view = np.frombuffer(buf, dtype=np.uint8)[: len(a)]
    view[:] = a
    return C.addressof(buf), lambda: view


def flip_points(n, al_a, al_b):
    """The run offsets at which the sweep flips one byte: the first and the last byte, the byte on each side of every 16-byte seam of either
    side's granules (the tile seams are among a's: a tile is 1024 of its granules), and the guard bytes just before and just behind the run."""
    pts = {-1, n}
    if n:
        pts |= {0, n - 1}
    for al in (al_a, al_b):
        for o in range((-al) % 16, n, 16):  # the byte at run offset o has the address al + o mod 16
            if o > 0:
                pts |= {o - 1, o}
    return sorted(pts)


def diff_case(call, rng, groups, alloc, exact=False):
    """groups: (alignment of a mod 16, of b, length, flips); one run of `a` per group and one run of `b` per entry of flips, which is None (equal
    runs between guard bytes that all differ) or the run offset of the one byte in which b differs from a, -1 and `length` being the guard bytes
    next to the run (every other guard byte is equal as well).  A run lies in a region of whole granules; exact: every region is an allocation
    of its own that holds exactly the aligned granules with a byte of the run, else a side's regions share one allocation and have a granule
    of guard bytes on either side.  alloc(array) -> (16-byte aligned address, reader).  The flags are compared with the flips, and a and b with
    themselves."""
    pad = 0 if exact else 16
    regions = ([], [])  # per side: (array, run offset)
    runs, want = [], []  # (index of a's region, of b's, length)
    for al_a, al_b, n, flips in groups:
        size = lambda al: 2 * pad + ((al + n + 15) // 16 * 16 if n else 0)  # noqa: E731
        ra = rng.integers(0, 256, size=size(al_a), dtype=np.uint8)
        sa, sb = pad + al_a, pad + al_b
        regions[0].append((ra, sa))
        lo, hi = -min(sa, sb), min(len(ra) - sa, size(al_b) - sb)  # the run offsets both regions hold
        same = rng.integers(0, 256, size=size(al_b), dtype=np.uint8)
        same[sb + lo : sb + hi] = ra[sa + lo : sa + hi]
        for f in flips:
            rb = same.copy()
            if f is None:
                rb[sb + lo : sb] ^= 0xFF
                rb[sb + n : sb + hi] ^= 0xFF
            else:
                assert lo <= f < hi, "the flipped byte lies outside the regions"
                rb[sb + f] ^= 1 << int(rng.integers(0, 8))
            regions[1].append((rb, sb))
            runs.append((len(regions[0]) - 1, len(regions[1]) - 1, n))
            want.append(int(f is not None and 0 <= f < n))
    addr, readers, before = ([], []), ([], []), ([], [])
    for side in (0, 1):
        if exact:
            for reg, start in regions[side]:
                a, r = alloc(reg)
                addr[side].append(a + start)
                readers[side].append(r)
                before[side].append(reg)
        else:
            whole = np.concatenate([reg for reg, _ in regions[side]]) if regions[side] else np.zeros(16, dtype=np.uint8)
            a, r = alloc(whole)
            off = 0
            for reg, start in regions[side]:
                addr[side].append(a + off + start)
                off += len(reg)
            readers[side].append(r)
            before[side].append(whole)
    a0, b0 = min(addr[0], default=0), min(addr[1], default=0)
    if not runs:
        a0, _ = alloc(np.zeros(16, dtype=np.uint8))
        b0 = a0
    table = [v for ia, ib, n in runs for v in (addr[0][ia] - a0, addr[1][ib] - b0, n)]
    flags = (C.c_uint32 * max(1, len(runs)))(*([7] * max(1, len(runs))))
    assert call(a0, b0, (C.c_uint64 * max(1, len(table)))(*table), len(runs), flags) == 0
    got = list(flags)[: len(runs)]
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, ("flags differ", [(i, runs[i], got[i], want[i]) for i in bad[:6]])
    for side in (0, 1):
        for r, was in zip(readers[side], before[side]):
            assert np.array_equal(r(), was), "an input was written"


def sweep_groups(n, al_a, al_b):
    """The equal runs, then every flip of flip_points, in launches of BATCH runs."""
    flips = [None] + flip_points(n, al_a, al_b)
    for i in range(0, len(flips), BATCH):
        yield [(al_a, al_b, n, flips[i : i + BATCH])]


def mixed_groups(rng):
    """One launch of 3 * len(LENGTHS) + 3 runs of all the lengths in which only every third differs, its neighbours being equal runs."""
    groups = []
    for i, n in enumerate(LENGTHS * 3 + (5000, 70000, 40)):
        f = int(rng.integers(0, n)) if i % 3 == 1 and n else None
        groups.append((ALIGNS[i % 3], ALIGNS[(i // 3) % 3], n, [f]))
    return groups


@pytest.mark.parametrize("al_b", ALIGNS)
@pytest.mark.parametrize("al_a", ALIGNS)
@pytest.mark.parametrize("n", LENGTHS)
def test_diff_kernel_every_seam_at_every_alignment_pair(emu, n, al_a, al_b):
    rng = np.random.default_rng(900 + 256 * n + 16 * al_a + al_b)
    for groups in sweep_groups(n, al_a, al_b):
        diff_case(emu.bz3_hip_debug_diff, rng, groups, _aligned_host)


def test_diff_kernel_mixed_launch_on_exact_allocations(emu):
    rng = np.random.default_rng(91)
    groups = mixed_groups(rng)
    assert sum(len(g[3]) for g in groups) >= 40
    diff_case(emu.bz3_hip_debug_diff, rng, groups, _aligned_host, exact=True)
    diff_case(emu.bz3_hip_debug_diff, rng, groups, _aligned_host)
    diff_case(emu.bz3_hip_debug_diff, rng, [], _aligned_host)


def test_debug_diff_rejects_bad_arguments(emu):
    buf = _buf(b"", 64)
    flags = (C.c_uint32 * 1)(7)
    assert emu.bz3_hip_debug_diff(buf, buf, None, -1, flags) == INIT
    assert emu.bz3_hip_debug_diff(buf, buf, None, 1, flags) == INIT
    assert emu.bz3_hip_debug_diff(buf, buf, (C.c_uint64 * 3)(0, 0, 8), 1, None) == INIT
    assert emu.bz3_hip_debug_diff(None, buf, (C.c_uint64 * 3)(0, 0, 8), 1, flags) == INIT
    assert emu.bz3_hip_debug_diff(buf, None, (C.c_uint64 * 3)(0, 0, 8), 1, flags) == INIT
    assert emu.bz3_hip_debug_diff(buf, buf, None, 0, None) == 0
    assert flags[0] == 7 and bytes(buf) == bytes(64)
    assert emu.bz3_hip_debug_diff(buf, buf, (C.c_uint64 * 3)(3, 3, 40), 1, flags) == 0 and flags[0] == 0  # a run against itself


# ---- frames -------------------------------------------------------------------------------------------------------------------
def change_sets(case):
    """(name, the byte offsets of the tensor that change), for a Case of test_frame_update_emu."""
    s, z, T, k = case.starts, case.sizes, case.T, case.k
    yield "none", []
    yield "first byte", [0]
    yield "last byte of the last chunk", [T - 1]
    if len(z) > 1:
        yield "either side of a chunk seam", [s[1] - 1, s[1]]
    yield "one byte in every chunk", [p + o // 3 for p, o in zip(s, z) if o]
    if k > 1:
        yield "one plane byte of one element", [s[-1] + 5 * k + k - 1]


def new_version(case, at):
    """(the new tensor, the frame the sync must give, numpy's count of the chunks that differ)."""
    x = np.frombuffer(case.x, dtype=np.uint8).copy()
    x[at] ^= 0x21
    d = bytes(x) if case.base is None else bytes(D(x, case.base))
    old = np.frombuffer(case.x, dtype=np.uint8)
    dirty = sum(1 for p, o in zip(case.starts, case.sizes) if o and not np.array_equal(x[p : p + o], old[p : p + o]))
    return bytes(x), case.expect(d), dirty


def sync_cap(lib, frame):
    """Room for every chunk coded again."""
    return 13 + len(_chunks(frame)) * (8 + lib.bz3_bound(BS))


def sync_call(lib, k, frame, data, old, base=None, cap=None, alloc=_buf):
    """(rc, *out_size, out[0, cap) after the call, *recoded).  `old is data`: one buffer for both."""
    cap = sync_cap(lib, frame) if cap is None else cap
    out = alloc(bytes([FILL]) * cap)
    osz, rec = C.c_size_t(cap), C.c_uint32(77)
    dbuf = alloc(data)
    obuf = dbuf if old is data else None if old is None else alloc(old)
    rc = lib.bz3_hip_sync_device(k, alloc(frame), len(frame), dbuf, obuf, len(data), None if base is None else alloc(base), out, C.byref(osz), C.byref(rec))
    return rc, osz.value, bytes(out)[:cap], rec.value


def refused(lib, k, frame, data, old, code, base=None, cap=None, call=sync_call):
    rc, size, out, rec = call(lib, k, frame, data, old, base, cap)
    assert (rc, size, rec) == (code, 0, 0), (rc, size, rec, code)
    assert out == bytes([FILL]) * len(out), "a refused call wrote to out"


def frames_match_reference(lib, k, chunks, with_base, call):
    case = Case(require_ref().lib, k, chunks, with_base=with_base)
    assert case.sizes == [BS] * (chunks - 1) + [LAST]
    old_chunks = _chunks(case.frame)
    for name, at in change_sets(case):
        new, want, dirty = new_version(case, at)
        lib.bz3_hip_debug_cm_launches(1)
        rc, size, out, rec = call(lib, k, case.frame, new, case.x, case.base)
        launches = lib.bz3_hip_debug_cm_launches(1)
        assert (rc, size) == (0, len(want)), (name, rc, size, len(want))
        assert out[:size] == want, ("frames differ", name)
        assert out[size:] == bytes([FILL]) * (len(out) - size), ("wrote beyond the frame", name)
        assert rec == dirty == len({j for j, (p, o) in enumerate(zip(case.starts, case.sizes)) for a in at if p <= a < p + o}), name
        assert launches == (1 if dirty else 0), (name, launches)
        clean = [j for j, (p, o) in enumerate(zip(case.starts, case.sizes)) if not any(p <= a < p + o for a in at)]
        assert all(_chunks(out[:size])[j] == old_chunks[j] for j in clean), ("a clean chunk changed", name)
        if not at:
            assert out[:size] == case.frame


@pytest.mark.parametrize("with_base", [False, True], ids=["plain", "base"])
@pytest.mark.parametrize("chunks", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_syncs_of_a_frame_match_the_reference(emu, k, chunks, with_base):
    """Blocks of 65 KiB and a short odd last chunk: f' is the reference's frame of S_k(D(new, base)) byte for byte, nothing beyond it is written,
    `recoded` is numpy's count, and the CM stage is launched once for a dirty set and not at all without one."""
    frames_match_reference(emu, k, chunks, with_base, sync_call)


def nothing_is_decoded(lib, call):
    ref = require_ref().lib
    case = Case(ref, 2, 5)
    new, want, dirty = new_version(case, [case.starts[2] + 10, case.starts[3] + 7])
    assert dirty == 2
    for j in range(5):  # a corrupt CLEAN chunk is carried over, a corrupt DIRTY chunk is replaced: BZ3_OK either way
        bad = _flip(case.frame, j)
        assert _ref_decompress(ref, bad, case.T)[0] != 0
        blk, orig = _chunks(bad)[j]
        rc, size, out, rec = call(lib, 2, bad, new, case.x)
        assert (rc, rec) == (0, 2) and out[:size] == (want if j in (2, 3) else _with_chunk(want, j, blk, orig)), j


def test_no_chunk_is_decoded(emu):
    nothing_is_decoded(emu, sync_call)


def sync_errors(lib, call):
    """(case, the new tensor, need) for the caller's own overlap checks."""
    ref = require_ref().lib
    case = Case(ref, 2, 2)
    new, want, _ = new_version(case, [BS + 3])  # the last chunk is dirty
    T, frame = case.T, case.frame
    for size in (T - 1, T + 1, 0):
        refused(lib, 2, frame, (new + b"z")[:size], (case.x + b"z")[:size], TOO_BIG, call=call)
    need = 13 + 8 + len(_chunks(frame)[0][0]) + 8 + ref.bz3_bound(LAST)
    refused(lib, 2, frame, new, case.x, TOO_BIG, cap=need - 1, call=call)
    rc, size, out, rec = call(lib, 2, frame, new, case.x, cap=need)
    assert (rc, rec, out[:size]) == (0, 1, want) and out[size:] == bytes([FILL]) * (need - size)
    refused(lib, 2, frame, new, case.x, TOO_BIG, cap=len(frame) - 1, call=call)  # (need >= the frame)
    refused(lib, 2, frame, case.x, case.x, TOO_BIG, cap=len(frame) - 1, call=call)  # nothing dirty: need == the frame
    assert call(lib, 2, frame, case.x, case.x, cap=len(frame))[:3] == (0, len(frame), frame)
    refused(lib, 2, frame, new, None, INIT, call=call)  # old == NULL
    # a malformed chunk header BEHIND the last dirty chunk is reported
    first, _, _ = new_version(case, [3])
    for bad in (_with_header(frame, 1, orig=-5), _with_header(frame, 1, size=-1), _with_header(frame, 1, size=BS + 1)):
        refused(lib, 2, bad, first, case.x, MALFORMED, call=call)
    refused(lib, 2, frame[: len(frame) - 10], first, case.x, bzip3_amd.BZ3_ERR_TRUNCATED_DATA, call=call)
    refused(lib, 2, frame[:12], new, case.x, MALFORMED, call=call)  # in_size < 13
    refused(lib, 3, frame, new, case.x, INIT, call=call)  # a bad element size
    return case, new, need


def test_sync_errors_leave_out_untouched(emu):
    case, new, need = sync_errors(emu, sync_call)
    frame, T = case.frame, case.T
    cap = sync_cap(emu, frame)
    base = bytes(T)
    # out overlapping each of in, data, old and base: the last byte of out[0, cap) is the input's first
    arena = _buf(bytes([FILL]) * (cap + len(frame) + T + 64))
    for which in range(4):
        given = [frame, new, case.x, base]
        C.memmove(C.byref(arena, cap - 1), given[which], len(given[which]))
        before = bytes(arena)
        args = [_buf(g) for g in given]
        args[which] = C.byref(arena, cap - 1)
        osz, rec = C.c_size_t(cap), C.c_uint32(77)
        assert emu.bz3_hip_sync_device(2, args[0], len(frame), args[1], args[2], T, args[3], arena, C.byref(osz), C.byref(rec)) == INIT, which
        assert (osz.value, rec.value) == (0, 0) and bytes(arena) == before, which
    osz = C.c_size_t(cap)  # adjacent: fine; data and old may overlap each other; recoded may be NULL
    C.memmove(C.byref(arena, cap), new, T)
    assert emu.bz3_hip_sync_device(2, _buf(frame), len(frame), C.byref(arena, cap), C.byref(arena, cap), T, None, arena, C.byref(osz), None) == 0
    assert bytes(arena)[: osz.value] == frame
    assert emu.bz3_hip_sync_device(2, _buf(frame), len(frame), _buf(new), _buf(case.x), T, None, arena, None, None) == INIT


def test_data_equal_to_old_is_the_verbatim_copy(emu):
    case = Case(require_ref().lib, 4, 2, with_base=True)
    emu.bz3_hip_debug_cm_launches(1)
    for old in (case.x, bytes(bytearray(case.x))):  # one buffer for both (sync_call), and two buffers with the same bytes
        rc, size, out, rec = sync_call(emu, 4, case.frame, case.x, old, case.base)
        assert (rc, rec, out[:size]) == (0, 0, case.frame)
    assert emu.bz3_hip_debug_cm_launches(1) == 0
    # a frame with an empty last chunk (a stream of exactly two blocks): the empty chunk is clean and copied
    two = Case(require_ref().lib, 4, 2, total=2 * BS)
    assert two.sizes == [BS, 0]
    new, want, dirty = new_version(two, [BS - 1])
    assert two.T == BS
    rc, size, out, rec = sync_call(emu, 4, two.frame, new[:BS], two.x[:BS])
    assert (rc, rec, dirty, out[:size]) == (0, 1, 1, want) and _chunks(out[:size])[1] == _chunks(two.frame)[1]


# ---- many ---------------------------------------------------------------------------------------------------------------------
def many_call(lib, ks, frames, datas, olds, bases, caps=None):
    n = len(frames)
    caps = [sync_cap(lib, f) for f in frames] if caps is None else caps
    ins, dbufs, obufs = [_buf(f) for f in frames], [_buf(d) for d in datas], [_buf(o) for o in olds]
    bbufs = [None if b is None else _buf(b) for b in bases]
    outs = [_buf(bytes([FILL]) * c) for c in caps]
    out_sizes, rcs, rec = (C.c_size_t * n)(*caps), (C.c_int * n)(*([77] * n)), (C.c_uint32 * n)(*([77] * n))
    bp = (C.c_void_p * n)(*[None if b is None else C.addressof(b) for b in bbufs])
    rc = lib.bz3_hip_sync_device_many(n, (C.c_uint32 * n)(*ks), _vp(ins), (C.c_size_t * n)(*map(len, frames)), _vp(dbufs), _vp(obufs), (C.c_size_t * n)(*map(len, datas)), bp,
                                      _vp(outs), out_sizes, rec, rcs)
    return rc, [(rcs[i], out_sizes[i], bytes(outs[i])[: caps[i]], rec[i]) for i in range(n)]


def many_equal_single_calls(lib, many_call, sync_call):
    ref = require_ref().lib
    cases = [Case(ref, k, chunks, wb, seed=40 + i) for i, (k, chunks, wb) in enumerate(((2, 2, 0), (1, 1, 1), (8, 5, 0), (4, 2, 1), (4, 1, 0)))]
    cases += [cases[0], cases[2]]  # the same `in` twice, with other changes; a failing frame among good ones
    plan = [[BS - 1, BS], [7], [3, 2 * BS + 5, 4 * BS + 9], [], [100], [5], [BS + 1]]
    news = [new_version(c, at) for c, at in zip(cases, plan)]
    frames, ks = [c.frame for c in cases], [c.k for c in cases]
    datas, olds, bases = [v[0] for v in news], [c.x for c in cases], [c.base for c in cases]
    datas[6] = datas[6][:-1]  # size != T
    olds[6] = olds[6][:-1]
    rc, got = many_call(lib, ks, frames, datas, olds, bases)
    assert rc == TOO_BIG
    for i in range(7):
        assert got[i] == sync_call(lib, ks[i], frames[i], datas[i], olds[i], bases[i]), ("single call", i)
        if i < 6:
            assert got[i][0] == 0 and got[i][2][: got[i][1]] == news[i][1] and got[i][3] == news[i][2] == len(plan[i]), i
    assert got[6][:2] == (TOO_BIG, 0) and got[6][2] == bytes([FILL]) * len(got[6][2]) and got[6][3] == 0
    assert got[3][2][: got[3][1]] == frames[3]


def test_many_syncs_equal_their_single_calls(emu, monkeypatch):
    """Seven frames of mixed k in one call, two with a base, one without a change, two of one `in`, one whose size is wrong; windows of three
    chunks, so that the dirty chunks of the call take more than one."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    many_equal_single_calls(emu, many_call, sync_call)


def dirty_chunks_share_launches(lib, many_call):
    ref = require_ref().lib
    case = Case(ref, 2, 2)
    n = 6
    for at, launches in (([5], 1), ([5, BS + 5], 1), ([], 0)):  # six, twelve and no dirty chunks: one encode launch, one, none; never a decode launch
        new, want, dirty = new_version(case, at)
        lib.bz3_hip_debug_cm_launches(1)
        rc, got = many_call(lib, [2] * n, [case.frame] * n, [new] * n, [case.x] * n, [None] * n)
        assert lib.bz3_hip_debug_cm_launches(1) == launches
        assert rc == 0 and all(g[0] == 0 and g[2][: g[1]] == want and g[3] == dirty for g in got)


def test_many_dirty_chunks_share_their_cm_launch(emu):
    dirty_chunks_share_launches(emu, many_call)


def test_many_whole_call_errors(emu):
    case = Case(require_ref().lib, 1, 1)
    new, want, _ = new_version(case, [9])
    assert emu.bz3_hip_sync_device_many(0, None, None, None, None, None, None, None, None, None, None, None) == 0
    assert emu.bz3_hip_sync_device_many(2, None, None, None, None, None, None, None, None, None, None, None) == INIT
    rc, got = many_call(emu, [1, 3], [case.frame] * 2, [new] * 2, [case.x] * 2, [None] * 2)  # a bad element size fails the whole call
    assert rc == INIT and all(g[:2] == (INIT, 0) and g[2] == bytes([FILL]) * len(g[2]) and g[3] == 0 for g in got)
    # elem_sizes, bases and recoded NULL: k = 1, no base, no count
    cap = sync_cap(emu, case.frame)
    ins, dbuf, obuf, outs = [_buf(case.frame)], [_buf(new)], [_buf(case.x)], [_buf(bytes([FILL]) * cap)]
    out_sizes, rcs = (C.c_size_t * 1)(cap), (C.c_int * 1)(77)
    assert emu.bz3_hip_sync_device_many(1, None, _vp(ins), (C.c_size_t * 1)(len(case.frame)), _vp(dbuf), _vp(obuf), (C.c_size_t * 1)(case.T), None, _vp(outs), out_sizes, None,
                                        rcs) == 0
    assert rcs[0] == 0 and bytes(outs[0])[: out_sizes[0]] == want
    for missing in (4, 5, 6):  # datas, olds and sizes are required
        args = [1, None, _vp(ins), (C.c_size_t * 1)(len(case.frame)), _vp(dbuf), _vp(obuf), (C.c_size_t * 1)(case.T), None, _vp(outs), (C.c_size_t * 1)(cap), None, rcs]
        args[missing] = None
        assert emu.bz3_hip_sync_device_many(*args) == INIT
