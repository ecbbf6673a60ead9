"""CPU tests of the delta frame calls (include/bz3_hip.h bz3_hip_compress_device_delta[_many] / bz3_hip_decompress_device_delta[_many],
bz3_hip_crc32c_device, the delta tiles of bzip3_amd/csrc/planes.hpp through bz3_hip_debug_delta) under the fiber emulation of the HIP
execution model (tests/emu).

D(x, b)[i] = (x[i] - b[i]) mod 256 and its inverse are written here in numpy from the definition in bz3_hip.h; split_k / merge_k / S
come from test_frame_planes_emu (numpy as well); the reference is oracle/_ref/libbz3ref.so.

BZ3_EMU_LIB=<path> runs the module on another build of the emulator library (the sanitizer build of tests/sanitize_emu.sh, with its
LD_PRELOAD and options; `-s` shows a sanitizer report that pytest's capture would hide).  For that build every buffer handed to the
library here lies inside a larger allocation: the segment kernels load the whole aligned 16-byte granules that hold a segment's
first and last byte (device allocations are granule-aligned and padded; a ctypes array of the exact size is not)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bzip3_amd
import mutants
from oracle_lib import require_ref
from test_frame_planes_emu import BS, COUNTS, S, _five, _ref_compress, _ref_decompress, _vp, chunk_sizes, merge_k, per_block, split_k

HERE = os.path.dirname(os.path.abspath(__file__))
NO_BASE = 2 ** 64 - 1
INIT, TOO_BIG = bzip3_amd.BZ3_ERR_INIT, bzip3_amd.BZ3_ERR_DATA_TOO_BIG


@pytest.fixture(scope="module")
def emu():
    if os.environ.get("BZ3_EMU_LIB"):
        return bzip3_amd._declare(C.CDLL(os.environ["BZ3_EMU_LIB"]))
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


def _buf(data, room=None):
    """A ctypes uint8 array of max(1, room or len(data)) bytes holding `data`, with 16 bytes of the same allocation on either side."""
    n = max(1, len(data) if room is None else room)
    b = (C.c_uint8 * n).from_buffer((C.c_uint8 * (n + 32))(), 16)
    if len(data):
        C.memmove(b, bytes(data), len(data))
    return b


# ---- the transform, from its definition -------------------------------------------------------------------------------------
def _u8(b):
    return b if isinstance(b, np.ndarray) else np.frombuffer(bytes(b), dtype=np.uint8)


def D(x, b):
    """D(x, b)[i] = (x[i] - b[i]) mod 256."""
    return ((_u8(x).astype(np.int16) - _u8(b).astype(np.int16)) % 256).astype(np.uint8)


def D_inv(d, b):
    return ((_u8(d).astype(np.int16) + _u8(b).astype(np.int16)) % 256).astype(np.uint8)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def lay_out3(rng, spec, addrs, src_np, base_np):
    """spec: (src, base, dst alignment mod 16, elements, tail bytes, k, inverse, has base) per segment, one after the other with gaps.
    Returns the hook's table and the expected writes [(dst_off, bytes)]."""
    table, writes, offs = [], [], [0, 0, 0]
    for a_s, a_b, a_d, elems, tail, k, inverse, has_base in spec:
        n = elems * k + tail
        for j, a in enumerate((a_s, a_b, a_d)):
            offs[j] += (a - (addrs[j] + offs[j])) % 16
        s, b, d = offs
        table += [s, b if has_base else NO_BASE, d, n, k | (inverse << 8)]
        x, base = src_np[s : s + n], base_np[b : b + n] if has_base else np.zeros(n, dtype=np.uint8)
        writes.append((d, D_inv(merge_k(x, k), base) if inverse else split_k(D(x, base), k)))
        for j in range(3):
            offs[j] += n + int(rng.integers(1, 40))  # at least one untouched byte between destination segments
    return table, writes, max(offs)


def spec_room3(spec):
    return sum(e * k + t for _, _, _, e, t, k, _, _ in spec) + 80 * len(spec) + 64


def delta_case(call, rng, spec, alloc):
    """alloc(room, fill) -> (object for the hook, address, numpy reader); call(src, base, dst, table, n) -> rc."""
    room = spec_room3(spec)
    src_np = rng.integers(0, 256, size=room, dtype=np.uint8)
    base_np = rng.integers(0, 256, size=room, dtype=np.uint8)
    src, base, dst = alloc(src_np), alloc(base_np), alloc(np.full(room, 0xA5, dtype=np.uint8))
    want = np.full(room, 0xA5, dtype=np.uint8)
    table, writes, end = lay_out3(rng, spec, (src[1], base[1], dst[1]), src_np, base_np)
    assert end <= room - 16
    for off, b in writes:
        want[off : off + len(b)] = b
    t = (C.c_uint64 * max(1, len(table)))(*table)
    assert call(src[0], base[0], dst[0], t, len(table) // 5) == 0
    bad = np.nonzero(dst[2]() != want)[0]
    assert bad.size == 0, ("bytes differ at", bad[:8], spec[:2], table[:10])
    assert np.array_equal(src[2](), src_np) and np.array_equal(base[2](), base_np), "an input was written"


def _r16(rng):
    return int(rng.integers(0, 16))


def sweep_specs3(rng, k, inverse, big=200_000):
    """At every edge element count with every tail length: each of the three alignments through all 16 values with the other two
    random, and 48 random triples (one launch per count); then random segments up to `big` bytes."""
    for elems in COUNTS:
        spec = []
        for tail in range(k):
            for which in range(3):
                for a in range(16):
                    al = [_r16(rng), _r16(rng), _r16(rng)]
                    al[which] = a
                    spec.append((*al, elems, tail, k, inverse, 1))
            spec += [(_r16(rng), _r16(rng), _r16(rng), elems, tail, k, inverse, 1) for _ in range(48 // k)]
        yield spec
    spec = [(_r16(rng), _r16(rng), _r16(rng), int(rng.integers(0, big // k)), int(rng.integers(0, k)), k, inverse, 1) for _ in range(4)]
    spec += [(_r16(rng), _r16(rng), _r16(rng), int(rng.integers(0, 300)), int(rng.integers(0, k)), k, inverse, 1) for _ in range(40)]
    yield spec


def mixed_spec3(rng):
    """One launch that holds plain, planes-only and delta segments of every k in both directions."""
    return [(_r16(rng), _r16(rng), _r16(rng), int(rng.integers(0, 9000)), int(rng.integers(0, k)), k, inv, has)
            for _ in range(3) for k in (1, 2, 4, 8) for inv in (0, 1) for has in (0, 1)]


def _host_alloc(a):
    buf = _buf(b"", len(a))
    view = np.frombuffer(buf, dtype=np.uint8)
    view[:] = a
    return buf, C.addressof(buf), lambda: view


@pytest.mark.parametrize("inverse", [0, 1], ids=["in", "out"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_delta_kernel_every_alignment_count_and_tail(emu, k, inverse):
    rng = np.random.default_rng(300 + 10 * k + inverse)
    for spec in sweep_specs3(rng, k, inverse):
        delta_case(emu.bz3_hip_debug_delta, rng, spec, _host_alloc)


def test_delta_kernel_mixed_segments_in_one_launch(emu):
    rng = np.random.default_rng(22)
    delta_case(emu.bz3_hip_debug_delta, rng, mixed_spec3(rng), _host_alloc)
    delta_case(emu.bz3_hip_debug_delta, rng, [], _host_alloc)


def in_place_case(call, rng, alloc, sizes=(0, 1, 17, 4079, 4080, 4081, 9000, 70_001)):
    """dst == base: merge_k(src) + dst written over dst, every k, several tiles, every destination alignment class touched."""
    spec = [(_r16(rng), 0, _r16(rng), e, int(rng.integers(0, k)), k, 1, 1) for k in (1, 2, 4, 8) for e in sizes]
    room = spec_room3(spec)
    src_np = rng.integers(0, 256, size=room, dtype=np.uint8)
    old = rng.integers(0, 256, size=room, dtype=np.uint8)
    src, dst = alloc(src_np), alloc(old)
    want, table, offs = old.copy(), [], [0, 0]
    for a_s, _, a_d, elems, tail, k, _, _ in spec:
        n = elems * k + tail
        offs[0] += (a_s - (src[1] + offs[0])) % 16
        offs[1] += (a_d - (dst[1] + offs[1])) % 16
        s, d = offs
        table += [s, d, d, n, k | 0x100]
        want[d : d + n] = D_inv(merge_k(src_np[s : s + n], k), old[d : d + n])
        offs[0] += n + int(rng.integers(1, 40))
        offs[1] += n + int(rng.integers(1, 40))
    assert max(offs) <= room - 16
    t = (C.c_uint64 * len(table))(*table)
    assert call(src[0], dst[0], dst[0], t, len(table) // 5) == 0
    bad = np.nonzero(dst[2]() != want)[0]
    assert bad.size == 0, ("bytes differ at", bad[:8])


def test_delta_kernel_in_place(emu):
    in_place_case(emu.bz3_hip_debug_delta, np.random.default_rng(23), _host_alloc)


def test_debug_delta_rejects_bad_arguments(emu):
    buf = _buf(b"", 64)
    assert emu.bz3_hip_debug_delta(buf, buf, buf, None, -1) == INIT
    assert emu.bz3_hip_debug_delta(buf, buf, buf, None, 0) == 0
    for mode in (0, 3, 16, 2 | 0x200):
        assert emu.bz3_hip_debug_delta(buf, buf, buf, (C.c_uint64 * 5)(0, 0, 32, 8, mode), 1) == INIT
    assert bytes(buf) == bytes(64)


def test_swar_bytes_against_numpy(emu):
    """sub_bytes / add_bytes on every pair of byte values, through a k = 1 segment of 65536 bytes each way."""
    x = np.repeat(np.arange(256, dtype=np.uint8), 256)
    b = np.tile(np.arange(256, dtype=np.uint8), 256)
    for inverse, want in ((0, D(x, b)), (1, D_inv(x, b))):
        src, base, dst = _host_alloc(x), _host_alloc(b), _host_alloc(np.zeros(65536, dtype=np.uint8))
        assert emu.bz3_hip_debug_delta(src[0], base[0], dst[0], (C.c_uint64 * 5)(0, 0, 0, 65536, 1 | (inverse << 8)), 1) == 0
        assert np.array_equal(dst[2](), want)


# ---- the checksum -------------------------------------------------------------------------------------------------------------
def crc32sum(init, data):
    """src/libbz3.c crc32sum from its definition: reflected CRC-32C (polynomial 0x82F63B78), state `init`, no inversion."""
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
        table.append(c)
    crc = init
    for byte in data:
        crc = table[(crc ^ byte) & 0xFF] ^ (crc >> 8)
    return crc


def test_crc32c_device_is_the_block_checksum(emu):
    rng = np.random.default_rng(5)
    data = bytes(rng.integers(0, 256, size=70_000, dtype=np.uint8))
    buf = _buf(data)
    crc = C.c_uint32(0)
    for off, n, init in ((0, 70_000, 1), (1, 69_999, 1), (2, 1, 1), (3, 2, 7), (3, 40_000, 0xDEADBEEF), (5, 0, 9), (0, 16385, 1)):
        assert emu.bz3_hip_crc32c_device(C.byref(buf, off), n, init, C.byref(crc)) == 0
        assert crc.value == crc32sum(init, data[off : off + n]) == emu.bz3_hip_stage_crc32c(_buf(data[off : off + n]), n, init), (off, n, init)
    # the published check value of CRC-32C ("123456789" with the usual all-ones init and final inversion)
    assert crc32sum(0xFFFFFFFF, b"123456789") ^ 0xFFFFFFFF == 0xE3069283
    assert emu.bz3_hip_crc32c_device(buf, 10, 1, None) == INIT


# ---- frames -------------------------------------------------------------------------------------------------------------------
def _base_for(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8))


def _x_for(d, base):
    """The input whose difference from `base` is `d` (so that what reaches the coder is as compressible as `d`)."""
    return bytes(D_inv(d, base))


def _compress_delta(lib, bs, k, x, base, cap=None):
    cap = lib.bz3_bound(len(x)) + 64 if cap is None else cap  # (room for the frame and chunk headers of a small incompressible input)
    dst = _buf(b"\xa5" * cap)
    osz = C.c_size_t(cap)
    rc = lib.bz3_hip_compress_device_delta(bs, k, _buf(x), None if base is None else _buf(base), dst, len(x), C.byref(osz))
    return rc, C.string_at(dst, osz.value)


def _decompress_delta(lib, k, frame, base, room, in_place=False):
    """(rc, committed bytes, the rest of out).  in_place: out is the base's own buffer."""
    b = None if base is None else _buf(base)
    out = b if in_place else _buf(b"\xa5" * room)
    osz = C.c_size_t(len(base) if in_place else room)
    rc = lib.bz3_hip_decompress_device_delta(k, _buf(frame), b, 0 if base is None else len(base), out, len(frame), C.byref(osz))
    return rc, C.string_at(out, osz.value), bytes(out)[osz.value : len(base) if in_place else room]


def _restore(ref, frame, k, base, room):
    """What a delta frame decodes to anywhere: the reference's bz3_decompress, merge_k per chunk, plus the base."""
    rc, sx = _ref_decompress(ref, frame, room)
    d = per_block(merge_k, sx, chunk_sizes(frame, len(sx)), k)
    return rc, bytes(D_inv(d, base[: len(d)]))


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_delta_frames_match_the_reference(emu, k, monkeypatch):
    """frame_cases' good inputs (five chunks, the exact multiple, 100 bytes, empty) against seeded bases, at an odd block size and
    windows of two blocks: the frame is the reference's frame of S_k(D(x, b)); the reference's decode, merged and added to the base
    in numpy, is x; the device decode is x, into a new buffer and over the base."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    ref = require_ref().lib
    bs = BS + 7
    five = _five(bs)
    for seed, d in enumerate((five, five[: 2 * bs], five[:100], b"")):
        base = _base_for(len(d), 40 + seed)
        x = _x_for(d, base)
        rc, frame = _compress_delta(emu, bs, k, x, base)
        assert (rc, frame) == _ref_compress(ref, bs, S(bytes(D(x, base)), bs, k, ref.bz3_bound)), (k, len(d))
        kept = x if len(x) % bs or not x else x[: len(x) - bs]  # src/libbz3.c:914 drops the last block of an exact multiple
        assert _restore(ref, frame, k, base, len(x) + 16) == (0, kept)
        assert _decompress_delta(emu, k, frame, base, len(x) + 16)[:2] == (0, kept)
        rc, got, rest = _decompress_delta(emu, k, frame, base, 0, in_place=True)
        assert (rc, got) == (0, kept) and rest == base[len(kept) :]


def test_identities(emu):
    """No base is the _planes call; a base of zeros gives the same frame; base == x gives the frame of zeros."""
    ref = require_ref().lib
    x = _five(BS)[: 2 * BS + 4321]
    for k in (1, 4):
        plain = _buf(b"", emu.bz3_bound(len(x)))
        psz = C.c_size_t(len(plain))
        assert emu.bz3_hip_compress_device_planes(BS, k, _buf(x), plain, len(x), C.byref(psz)) == 0
        want = C.string_at(plain, psz.value)
        assert _compress_delta(emu, BS, k, x, None) == (0, want)
        assert _compress_delta(emu, BS, k, x, bytes(len(x))) == (0, want)
        assert _compress_delta(emu, BS, k, x, x) == _ref_compress(ref, BS, bytes(len(x)))
        back = _buf(b"", len(x))
        bsz = C.c_size_t(len(x))
        assert emu.bz3_hip_decompress_device_planes(k, _buf(want), back, len(want), C.byref(bsz)) == 0
        assert _decompress_delta(emu, k, want, None, len(x))[:2] == (0, C.string_at(back, bsz.value)) == (0, x)
        assert _decompress_delta(emu, k, want, bytes(len(x)), len(x))[:2] == (0, x)


# ---- many ---------------------------------------------------------------------------------------------------------------------
def _many_compress(lib, bs, ks, xs, bases):
    n = len(xs)
    ins, caps = [_buf(x) for x in xs], [lib.bz3_bound(len(x)) + 64 for x in xs]
    bbufs = [None if b is None else _buf(b) for b in bases]
    outs = [_buf(b"\xa5" * c) for c in caps]
    out_sizes, rcs = (C.c_size_t * n)(*caps), (C.c_int * n)(*([77] * n))
    bp = (C.c_void_p * n)(*[None if b is None else C.addressof(b) for b in bbufs])
    rc = lib.bz3_hip_compress_device_delta_many(bs, n, (C.c_uint32 * n)(*ks), _vp(ins), bp, (C.c_size_t * n)(*map(len, xs)), _vp(outs), out_sizes, rcs)
    return rc, list(rcs), [C.string_at(o, s) for o, s in zip(outs, out_sizes)]


def _many_decompress(lib, ks, frames, bases, rooms, in_place):
    """Per frame (rc, committed bytes, the rest of its out).  in_place[i]: frame i decodes over its base's buffer."""
    n = len(frames)
    ins = [_buf(f) for f in frames]
    bbufs = [None if b is None else _buf(b) for b in bases]
    outs = [bbufs[i] if in_place[i] else _buf(b"\xa5" * rooms[i]) for i in range(n)]
    caps = [len(bases[i]) if in_place[i] else rooms[i] for i in range(n)]
    out_sizes, rcs = (C.c_size_t * n)(*caps), (C.c_int * n)(*([77] * n))
    bp = (C.c_void_p * n)(*[None if b is None else C.addressof(b) for b in bbufs])
    rc = lib.bz3_hip_decompress_device_delta_many(n, (C.c_uint32 * n)(*ks), _vp(ins), (C.c_size_t * n)(*map(len, frames)), bp,
                                                  (C.c_size_t * n)(*[0 if b is None else len(b) for b in bases]), _vp(outs), out_sizes, rcs)
    return rc, [(rcs[i], C.string_at(outs[i], out_sizes[i]), bytes(outs[i])[out_sizes[i] : caps[i]]) for i in range(n)]


def _mixed():
    five = _five(BS)
    ds = [five, b"", five[: 2 * BS + 9], five[: BS + 7], b"abcdefghij" * 10, five[: 3 * BS + 5], b"xyz", five[:40_001]]
    ks = [2, 8, 1, 4, 4, 8, 2, 1]
    bases = [_base_for(len(d), 60 + i) if i % 3 != 1 else None for i, d in enumerate(ds)]
    xs = [d if b is None else _x_for(d, b) for d, b in zip(ds, bases)]
    return xs, ks, bases


@pytest.mark.parametrize("window", ["2", "3"])
def test_many_with_and_without_bases_across_windows(emu, monkeypatch, window):
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", window)
    ref = require_ref().lib
    xs, ks, bases = _mixed()
    rc, rcs, frames = _many_compress(emu, BS, ks, xs, bases)
    assert rc == 0 and rcs == [0] * len(xs)
    for i, (x, k, b) in enumerate(zip(xs, ks, bases)):
        assert (0, frames[i]) == _compress_delta(emu, BS, k, x, b), ("single call", i)
        d = x if b is None else bytes(D(x, b))
        assert (0, frames[i]) == _ref_compress(ref, BS, S(d, BS, k, ref.bz3_bound)), ("reference", i)
    in_place = [b is not None and i % 2 == 0 for i, b in enumerate(bases)]
    rc, got = _many_decompress(emu, ks, frames, bases, [len(x) + 16 for x in xs], in_place)
    assert rc == 0
    for i, (x, b) in enumerate(zip(xs, bases)):
        assert got[i][:2] == (0, x), i
        assert got[i][2] == (b[len(x) :] if in_place[i] else b"\xa5" * 16), ("wrote beyond the decoded bytes", i)


def _chunks(frame):
    out, off = [], 13
    for _ in range(int.from_bytes(frame[9:13], "little")):
        size, orig = int.from_bytes(frame[off : off + 4], "little"), int.from_bytes(frame[off + 4 : off + 8], "little")
        out.append((frame[off + 8 : off + 8 + size], orig))
        off += 8 + size
    return out


def _with_chunk(frame, j, block, orig):
    """`frame` with chunk j replaced by (block, orig)."""
    cs = _chunks(frame)
    cs[j] = (block, orig)
    return frame[:13] + b"".join(len(b).to_bytes(4, "little") + int(o).to_bytes(4, "little") + b for b, o in cs)


def test_many_isolates_mutants(emu, monkeypatch):
    """Good delta frames between frames whose second or third chunk is a mutant of tests/mutants.py: every frame has its single call's
    code and committed bytes, the committed bytes are x (not D), and the rest of out is untouched (in place: still the base)."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    ref = require_ref().lib
    five = _five(BS)[: 2 * BS + 777]
    frames, ks, bases, xs = [], [], [], []
    for i, k in enumerate((1, 4, 8)):
        base = _base_for(len(five), 80 + i)
        x = _x_for(five, base)
        rc, f = _compress_delta(emu, BS, k, x, base)
        assert rc == 0
        frames.append(f), ks.append(k), bases.append(base), xs.append(x)
    blocks = [c for f in frames for c in _chunks(f)[1:3]]
    muts = list(mutants.mutants([b for b, _ in blocks], [o for _, o in blocks], 2 * len(frames), seed=7))
    all_frames, all_ks, all_bases, names = [], [], [], []
    for i, f in enumerate(frames):
        for j in (1, 2):
            blk, orig = muts[2 * i + j - 1]
            all_frames.append(_with_chunk(f, j, blk, min(orig, BS))), all_ks.append(ks[i]), all_bases.append(bases[i]), names.append(("mutant", i, j))
        all_frames.append(f), all_ks.append(ks[i]), all_bases.append(bases[i]), names.append(("good", i, 0))
    n = len(all_frames)
    for in_place in ([q % 2 == 0 for q in range(n)], [False] * n):  # every frame's neighbours of the other kind; all out of place
        rooms = [len(five) + 16] * n
        rc, got = _many_decompress(emu, all_ks, all_frames, all_bases, rooms, in_place)
        failed = 0
        for q, (kind, i, j) in enumerate(names):
            single = _decompress_delta(emu, all_ks[q], all_frames[q], all_bases[q], rooms[q], in_place=in_place[q])
            assert got[q] == single, (q, kind, got[q][0], single[0], len(got[q][1]), len(single[1]))
            code, committed, rest = got[q]
            assert committed == xs[i][: len(committed)], (q, "the committed bytes are not x")
            assert rest == (all_bases[q][len(committed) :] if in_place[q] else b"\xa5" * (rooms[q] - len(committed))), (q, "out was touched beyond the committed bytes")
            # the code and the committed size are the reference's for the same frame
            rrc, sx = _ref_decompress(ref, all_frames[q], rooms[q])
            assert (code, len(committed)) == (rrc, len(sx)), (q, kind, code, rrc)
            if kind == "good":
                assert code == 0 and committed == xs[i]
            failed += code != 0
        assert failed >= len(frames), "the mutants did not fail"
        assert rc == next(g[0] for g in got if g[0] != 0)


# ---- arguments ----------------------------------------------------------------------------------------------------------------
def test_base_too_short(emu):
    """A base shorter than the decoded size: the chunks that fit are committed, the next one is BZ3_ERR_DATA_TOO_BIG."""
    ref = require_ref().lib
    five = _five(BS)
    base = _base_for(len(five), 90)
    x = _x_for(five, base)
    rc, frame = _compress_delta(emu, BS, 2, x, base)
    assert rc == 0
    short = base[: 3 * BS - 1]
    want = _ref_decompress(ref, frame, len(short))  # the reference with an output of that size: its code and committed size
    for in_place in (False, True):
        rc, got, rest = _decompress_delta(emu, 2, frame, short, len(five) + 16, in_place=in_place)
        assert (rc, len(got)) == (TOO_BIG, 2 * BS) == (want[0], len(want[1]))
        assert got == x[: 2 * BS] and rest == (short[2 * BS :] if in_place else b"\xa5" * (len(five) + 16 - 2 * BS))


def test_overlap_and_null_arguments(emu):
    x = _five(BS)[:5000]
    base = _base_for(len(x), 91)
    rc, frame = _compress_delta(emu, BS, 1, x, base)
    assert rc == 0
    arena = _buf(b"\xa5" * 40_000)
    at = lambda off: C.byref(arena, off)  # noqa: E731
    # decode: out overlaps the base without being it
    C.memmove(at(0), base, len(base))
    before = bytes(arena)
    for off in (1, 16, len(base) - 1):
        osz = C.c_size_t(len(x))
        assert emu.bz3_hip_decompress_device_delta(1, _buf(frame), at(0), len(base), at(off), len(frame), C.byref(osz)) == INIT
        assert bytes(arena) == before
    osz = C.c_size_t(len(x))
    assert emu.bz3_hip_decompress_device_delta(1, _buf(frame), at(0), len(base), at(len(base)), len(frame), C.byref(osz)) == 0  # adjacent: fine
    assert C.string_at(at(len(base)), osz.value) == x
    # compress: the coded frame overlaps the base or the input
    cap = emu.bz3_bound(len(x))
    arena2 = _buf(b"\xa5" * 40_000)
    C.memmove(arena2, x, len(x))
    C.memmove(C.byref(arena2, 10_000), base, len(base))
    before = bytes(arena2)
    for out_off in (len(x) - 1, 10_000 - cap + 1, 10_000 + len(base) - 1):
        osz = C.c_size_t(cap)
        assert emu.bz3_hip_compress_device_delta(BS, 1, arena2, C.byref(arena2, 10_000), C.byref(arena2, out_off), len(x), C.byref(osz)) == INIT
        assert bytes(arena2) == before
    # _many: one bad frame fails the whole call before any write
    xs, ks, bases = [x, x], [1, 1], [base, base]
    n = 2
    ins, bb = [_buf(x), _buf(x)], [_buf(base), _buf(base)]
    out0 = _buf(b"\xa5" * cap)
    out_sizes, rcs = (C.c_size_t * n)(cap, cap), (C.c_int * n)(77, 77)
    outs = (C.c_void_p * n)(C.addressof(out0), C.addressof(bb[1]) + 5)
    assert emu.bz3_hip_compress_device_delta_many(BS, n, (C.c_uint32 * n)(*ks), _vp(ins), _vp(bb), (C.c_size_t * n)(len(x), len(x)), outs, out_sizes, rcs) == INIT
    assert list(rcs) == [INIT, INIT] and list(out_sizes) == [0, 0] and bytes(out0) == b"\xa5" * cap and bytes(bb[1]) == base
    fr = [_buf(frame), _buf(frame)]
    out_sizes, rcs = (C.c_size_t * n)(len(x), len(x)), (C.c_int * n)(77, 77)
    outs = (C.c_void_p * n)(C.addressof(out0), C.addressof(bb[1]) + 5)
    assert emu.bz3_hip_decompress_device_delta_many(n, (C.c_uint32 * n)(*ks), _vp(fr), (C.c_size_t * n)(len(frame), len(frame)), _vp(bb),
                                                    (C.c_size_t * n)(len(base), len(base)), outs, out_sizes, rcs) == INIT
    assert list(rcs) == [INIT, INIT] and list(out_sizes) == [0, 0] and bytes(out0) == b"\xa5" * cap and bytes(bb[1]) == base
    # bases without base_sizes; n == 0 touches nothing; a bad element size
    out_sizes, rcs = (C.c_size_t * n)(len(x), len(x)), (C.c_int * n)(77, 77)
    assert emu.bz3_hip_decompress_device_delta_many(n, None, _vp(fr), (C.c_size_t * n)(len(frame), len(frame)), _vp(bb), None, _vp([out0, out0]), out_sizes, rcs) == INIT
    assert emu.bz3_hip_compress_device_delta_many(BS, 0, None, None, None, None, None, None, None) == 0
    assert emu.bz3_hip_decompress_device_delta_many(0, None, None, None, None, None, None, None, None) == 0
    osz = C.c_size_t(cap)
    assert emu.bz3_hip_compress_device_delta(BS, 3, _buf(x), _buf(base), out0, len(x), C.byref(osz)) == INIT
    assert bytes(out0) == b"\xa5" * cap
    # NULL bases / NULL entries are the _planes call
    rc, rcs, frames = _many_compress(emu, BS, [4, 4], [x, x], [None, base])
    plain = _buf(b"", cap)
    psz = C.c_size_t(cap)
    assert emu.bz3_hip_compress_device_planes(BS, 4, _buf(x), plain, len(x), C.byref(psz)) == 0
    assert rc == 0 and frames[0] == C.string_at(plain, psz.value) != frames[1]
