"""CPU tests of the byte-plane frame calls (include/bz3_hip.h bz3_hip_compress_device_planes[_many] /
bz3_hip_decompress_device_planes[_many], the split / merge kernel of bzip3_amd/csrc/planes.hpp through bz3_hip_debug_planes) under the
fiber emulation of the HIP execution model (tests/emu), and of bzip3_amd._lossless_block_size (pure Python).

split_k / merge_k and S (split_k of every block bz3_compress cuts the input into) are written here in numpy from their definition
in bz3_hip.h, independent of the product; the reference is oracle/_ref/libbz3ref.so."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bzip3_amd
import frame_cases
from oracle_lib import require_ref

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTS = (0, 1, 15, 16, 17, 31, 4095, 4097)
KiB65, MiB511 = 65 * 1024, 511 << 20
BS = KiB65


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


# ---- the transform, from its definition -------------------------------------------------------------------------------------
def split_k(b, k):
    """split_k(b)[q m + e] = b[e k + q]; the tail of len(b) % k bytes stays in place."""
    b = np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b
    m = len(b) // k
    return np.concatenate([b[: m * k].reshape(m, k).T.reshape(-1), b[m * k :]])


def merge_k(b, k):
    b = np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b
    m = len(b) // k
    return np.concatenate([b[: m * k].reshape(k, m).T.reshape(-1), b[m * k :]])


def block_sizes(n, block_size, bound):
    """The sizes of the blocks bz3_compress(block_size, n bytes) codes (src/libbz3.c:877-878, :892-914), the (sic) short last one included."""
    bs = block_size
    if bs > n:
        bs = bound(n)  # :877
    bs = max(bs, KiB65)  # :878
    nb = n // bs + (1 if n % bs else 0)
    return bs, [n % bs if j == nb - 1 else bs for j in range(nb)]


def per_block(f, data, sizes, k):
    data = np.frombuffer(bytes(data), dtype=np.uint8)
    out, off = [], 0
    for s in sizes:
        out.append(f(data[off : off + s], k))
        off += s
    out.append(data[off:])  # what :914 drops is in no block
    return np.concatenate(out).tobytes()


def S(data, block_size, k, bound):
    return per_block(split_k, data, block_sizes(len(data), block_size, bound)[1], k)


def S_inv(data, block_size, k, bound):
    return per_block(merge_k, data, block_sizes(len(data), block_size, bound)[1], k)


def chunk_sizes(frame, committed):
    """The original sizes of the chunks of `frame` that lie within `committed` decoded bytes, read from its chunk headers."""
    sizes, off, total = [], 13, 0
    while off + 8 <= len(frame):
        size, orig = int.from_bytes(frame[off : off + 4], "little"), int.from_bytes(frame[off + 4 : off + 8], "little")
        if total + orig > committed or total == committed:
            break
        sizes.append(orig)
        total += orig
        off += 8 + size
    assert total == committed, ("the committed bytes are not whole chunks", total, committed)
    return sizes


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def lay_out(rng, spec, src_addr, dst_addr, src_np):
    """spec: (src alignment mod 16, dst alignment mod 16, elements, tail bytes, k, inverse) per segment, one after the other with
    gaps.  Returns the hook's table and the expected writes [(dst_off, bytes)]."""
    table, writes, s_off, d_off = [], [], 0, 0
    for a_s, a_d, elems, tail, k, inverse in spec:
        n = elems * k + tail
        s_off += (a_s - (src_addr + s_off)) % 16
        d_off += (a_d - (dst_addr + d_off)) % 16
        table += [s_off, d_off, n, k | (inverse << 8)]
        writes.append((d_off, (merge_k if inverse else split_k)(src_np[s_off : s_off + n], k)))
        s_off += n + int(rng.integers(0, 40))
        d_off += n + int(rng.integers(1, 40))  # at least one untouched byte between destination segments
    return table, writes, max(s_off, d_off)


def spec_room(spec):
    return sum(e * k + t for _, _, e, t, k, _ in spec) + 80 * len(spec) + 64


def _planes_case(lib, rng, spec):
    room = spec_room(spec)
    src, dst = (C.c_uint8 * room)(), (C.c_uint8 * room)()
    src_np, dst_np = np.frombuffer(src, dtype=np.uint8), np.frombuffer(dst, dtype=np.uint8)
    src_np[:] = rng.integers(0, 256, size=room, dtype=np.uint8)
    dst_np[:] = 0xA5
    want = dst_np.copy()
    table, writes, end = lay_out(rng, spec, C.addressof(src), C.addressof(dst), src_np)
    assert end <= room - 16
    for off, b in writes:
        want[off : off + len(b)] = b
    t = (C.c_uint64 * max(1, len(table)))(*table)
    assert lib.bz3_hip_debug_planes(src, dst, t, len(table) // 4) == 0
    bad = np.nonzero(dst_np != want)[0]
    assert bad.size == 0, ("bytes differ at", bad[:8], spec[:2], table[:8])


def sweep_specs(rng, k, inverse):
    """Every source x destination alignment mod 16 at the edge element counts with every tail length (one launch per count), then
    random segments up to ~200 KB."""
    for elems in COUNTS:
        yield [(a, b, elems, tail, k, inverse) for a in range(16) for b in range(16) for tail in range(k)]
    spec = [(int(rng.integers(0, 16)), int(rng.integers(0, 16)), int(rng.integers(0, 200_000 // k)), int(rng.integers(0, k)), k, inverse) for _ in range(4)]
    spec += [(int(rng.integers(0, 16)), int(rng.integers(0, 16)), int(rng.integers(0, 300)), int(rng.integers(0, k)), k, inverse) for _ in range(40)]
    yield spec


def mixed_spec(rng):
    """One launch that mixes k = 1, 2, 4, 8 in both directions."""
    return [(int(rng.integers(0, 16)), int(rng.integers(0, 16)), int(rng.integers(0, 9000)), int(rng.integers(0, k)), k, inv)
            for _ in range(6) for k in (1, 2, 4, 8) for inv in (0, 1)]


@pytest.mark.parametrize("inverse", [0, 1], ids=["split", "merge"])
@pytest.mark.parametrize("k", [2, 4, 8])
def test_planes_kernel_every_alignment_count_and_tail(emu, k, inverse):
    rng = np.random.default_rng(100 + 10 * k + inverse)
    for spec in sweep_specs(rng, k, inverse):
        _planes_case(emu, rng, spec)


def test_planes_kernel_mixed_element_sizes_in_one_launch(emu):
    rng = np.random.default_rng(21)
    _planes_case(emu, rng, mixed_spec(rng))
    _planes_case(emu, rng, [])


def test_debug_planes_rejects_bad_arguments(emu):
    buf = (C.c_uint8 * 64)()
    INIT = bzip3_amd.BZ3_ERR_INIT
    assert emu.bz3_hip_debug_planes(buf, buf, None, -1) == INIT
    assert emu.bz3_hip_debug_planes(buf, buf, None, 0) == 0
    for mode in (0, 3, 16, 2 | 0x200):
        assert emu.bz3_hip_debug_planes(buf, buf, (C.c_uint64 * 4)(0, 32, 8, mode), 1) == INIT
    assert bytes(buf) == bytes(64)


# ---- frames -------------------------------------------------------------------------------------------------------------------
def _buf(data, room=None):
    n = max(1, len(data) if room is None else room)
    b = (C.c_uint8 * n)()
    if len(data):
        C.memmove(b, bytes(data), len(data))
    return b


class PlanesFrames:
    """libbz3.h's frame API as frame_cases.check calls it, conjugated: bz3_compress(data) is the planes call on S^-1(data), so the
    frame must be the reference's frame of data; bz3_decompress(frame) is S of what the planes call commits, per committed chunk."""

    def __init__(self, lib, k):
        self.lib, self.k = lib, k
        self.bz3_bound = lib.bz3_bound

    def bz3_compress(self, bs, data, out, n, osz):
        src = _buf(S_inv(bytes(data[:n]), bs, self.k, self.lib.bz3_bound))
        return self.lib.bz3_hip_compress_device_planes(bs, self.k, src, out, n, osz)

    def bz3_decompress(self, frame, out, n, osz):
        room = osz._obj.value
        rc = self.lib.bz3_hip_decompress_device_planes(self.k, _buf(frame[:n]), out, n, osz)
        if rc != 0 and osz._obj.value == room and rc in (bzip3_amd.BZ3_ERR_INIT, bzip3_amd.BZ3_ERR_MALFORMED_HEADER) and (n < 13 or frame[:5] != b"BZ3v1" or rc == bzip3_amd.BZ3_ERR_INIT):
            return rc  # refused at the frame header: *out_size is not written, as in the reference
        got = C.string_at(out, osz._obj.value)
        back = per_block(split_k, got, chunk_sizes(bytes(frame[:n]), len(got)), self.k)
        C.memmove(out, back, len(back))
        return rc


def _five(bs):
    rng = np.random.default_rng(4)
    unit = bytes(rng.integers(0, 256, size=997, dtype=np.uint8))  # repetitive: LZP collapses it, so the emulated CM stage stays small
    return (unit * (5 * bs // 997 + 2))[: 4 * bs + 1234]


@pytest.mark.parametrize("k", [2, 4])
def test_planes_frames_match_the_reference(emu, k):
    """Good frames, the empty and the 100-byte input, the exact multiple, the 15 malformed frames and the short output."""
    frame_cases.check(PlanesFrames(emu, k), _five(BS), BS)


@pytest.mark.parametrize("k", [2, 4])
def test_planes_frames_at_an_odd_block_size(emu, k, monkeypatch):
    """65 KiB + 7: blocks start in the middle of an element and every block has a tail; windows of two blocks."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    bs = BS + 7
    frame_cases.check(PlanesFrames(emu, k), _five(bs), bs)


def _ref_compress(ref, bs, data):
    out = (C.c_uint8 * (ref.bz3_bound(len(data)) + 64))()
    osz = C.c_size_t(len(out))
    rc = ref.bz3_compress(bs, data, out, len(data), C.byref(osz))
    return rc, bytes(out[: osz.value])


def _ref_decompress(ref, frame, room):
    out = (C.c_uint8 * max(1, room))()
    osz = C.c_size_t(room)
    rc = ref.bz3_decompress(frame, out, len(frame), C.byref(osz))
    return rc, C.string_at(out, osz.value)


def _vp(bufs):
    return (C.c_void_p * len(bufs))(*[C.addressof(b) for b in bufs])


def _many_compress(lib, bs, ks, datas):
    n = len(datas)
    ins = [_buf(d) for d in datas]
    caps = [lib.bz3_bound(len(d)) for d in datas]
    outs = [_buf(b"\xa5" * c) for c in caps]
    out_sizes = (C.c_size_t * n)(*caps)
    rcs = (C.c_int * n)(*([77] * n))
    rc = lib.bz3_hip_compress_device_planes_many(bs, n, (C.c_uint32 * n)(*ks), _vp(ins), (C.c_size_t * n)(*map(len, datas)), _vp(outs), out_sizes, rcs)
    return rc, list(rcs), list(out_sizes), outs


def _many_decompress(lib, ks, frames, rooms):
    n = len(frames)
    ins = [_buf(f) for f in frames]
    outs = [_buf(b"\xa5" * r) for r in rooms]
    out_sizes = (C.c_size_t * n)(*rooms)
    rcs = (C.c_int * n)(*([77] * n))
    rc = lib.bz3_hip_decompress_device_planes_many(n, (C.c_uint32 * n)(*ks), _vp(ins), (C.c_size_t * n)(*map(len, frames)), _vp(outs), out_sizes, rcs)
    return rc, list(rcs), list(out_sizes), outs


def _single_compress(lib, bs, k, data):
    dst = _buf(b"", lib.bz3_bound(len(data)))
    osz = C.c_size_t(lib.bz3_bound(len(data)))
    rc = lib.bz3_hip_compress_device_planes(bs, k, _buf(data), dst, len(data), C.byref(osz))
    return rc, C.string_at(dst, osz.value)


def _mixed():
    five = _five(BS)
    rng = np.random.default_rng(9)
    steps = np.cumsum(rng.integers(1, 9, size=3 * BS // 8 + 11)).astype("<i8").tobytes()  # more than two blocks of int64
    datas = [five, b"", steps, five[: 2 * BS], b"abcdefghij" * 10, five[: BS + 7], b"xyz", five[: 3 * BS + 5], five[:40_001]]
    ks = [2, 8, 8, 4, 4, 1, 8, 4, 2]
    return datas, ks


def test_many_mixed_element_sizes_across_windows(emu, monkeypatch):
    """Frames of k = 1, 2, 4, 8 in one call, windows of 3 blocks that cut through frames: each equals its single call and the
    reference's frame of S(x); decoding gives x back.  One corrupt frame in the middle does not change its neighbours."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    ref = require_ref().lib
    datas, ks = _mixed()
    rc, rcs, sizes, outs = _many_compress(emu, BS, ks, datas)
    assert rc == 0 and rcs == [0] * len(datas)
    frames = [C.string_at(o, s) for o, s in zip(outs, sizes)]
    for i, (d, k) in enumerate(zip(datas, ks)):
        assert (0, frames[i]) == _single_compress(emu, BS, k, d), ("single call", i)
        assert (0, frames[i]) == _ref_compress(ref, BS, S(d, BS, k, ref.bz3_bound)), ("reference", i)
    # what decodes is what the reference decodes from the frame, merged per chunk (an exact multiple loses its last block: :914)
    rooms = [len(d) + 16 for d in datas]
    want = []
    for f, k, r in zip(frames, ks, rooms):
        rrc, sx = _ref_decompress(ref, f, r)
        want.append((rrc, per_block(merge_k, sx, chunk_sizes(f, len(sx)), k)))
    rc, rcs, sizes, outs = _many_decompress(emu, ks, frames, rooms)
    got = [(r, C.string_at(o, s)) for r, o, s in zip(rcs, outs, sizes)]
    assert rc == 0 and got == want
    for i, d in enumerate(datas):
        assert got[i][1] == (d if len(d) % BS or not d else d[: len(d) - BS]), i
        assert bytes(outs[i][sizes[i] : rooms[i]]) == b"\xa5" * (rooms[i] - sizes[i]), ("wrote beyond the decoded bytes", i)
    # frame 2 (three chunks, k = 8) with a flipped byte in its second chunk
    bad = bytearray(frames[2])
    second = 13 + 8 + int.from_bytes(bad[13:17], "little")
    bad[second + 8 + 40] ^= 0x40
    frames2 = frames[:2] + [bytes(bad)] + frames[3:]
    rrc, sx = _ref_decompress(ref, bytes(bad), rooms[2])
    assert rrc != 0
    want2 = list(want)
    want2[2] = (rrc, per_block(merge_k, sx, chunk_sizes(bytes(bad), len(sx)), 8))
    rc, rcs, sizes, outs = _many_decompress(emu, ks, frames2, rooms)
    assert rc == rrc and [(r, C.string_at(o, s)) for r, o, s in zip(rcs, outs, sizes)] == want2


@pytest.mark.parametrize("bad_k", [3, 16, 0])
def test_bad_element_size_fails_the_whole_call_before_any_write(emu, bad_k):
    INIT = bzip3_amd.BZ3_ERR_INIT
    datas = [_five(BS)[:5000], _five(BS)[:7000], b"abc"]
    for ks in ([bad_k, 2, 4], [2, 4, bad_k]):
        rc, rcs, sizes, outs = _many_compress(emu, BS, ks, datas)
        assert rc == INIT and rcs == [INIT] * 3 and sizes == [0] * 3
        assert all(bytes(o) == b"\xa5" * len(o) for o in outs)
        frames = [_ref_compress(require_ref().lib, BS, d)[1] for d in datas]
        rc, rcs, sizes, outs = _many_decompress(emu, ks, frames, [len(d) for d in datas])
        assert rc == INIT and rcs == [INIT] * 3 and sizes == [0] * 3
        assert all(bytes(o) == b"\xa5" * len(o) for o in outs)
    data = datas[0]
    dst = _buf(b"\xa5" * emu.bz3_bound(len(data)))
    osz = C.c_size_t(len(dst))
    assert emu.bz3_hip_compress_device_planes(BS, bad_k, _buf(data), dst, len(data), C.byref(osz)) == INIT
    assert bytes(dst) == b"\xa5" * len(dst)
    frame = _ref_compress(require_ref().lib, BS, data)[1]
    back = _buf(b"\xa5" * len(data))
    osz = C.c_size_t(len(data))
    assert emu.bz3_hip_decompress_device_planes(bad_k, _buf(frame), back, len(frame), C.byref(osz)) == INIT
    assert bytes(back) == b"\xa5" * len(data)


def test_element_size_one_is_the_plain_call(emu):
    for data in (_five(BS), _five(BS)[: 2 * BS], b""):
        n = len(data)
        cap = emu.bz3_bound(n)
        a, b = _buf(b"", cap), _buf(b"", cap)
        sa, sb = C.c_size_t(cap), C.c_size_t(cap)
        assert emu.bz3_hip_compress_device(BS, _buf(data), a, n, C.byref(sa)) == 0
        assert emu.bz3_hip_compress_device_planes(BS, 1, _buf(data), b, n, C.byref(sb)) == 0
        assert C.string_at(a, sa.value) == C.string_at(b, sb.value)
        frame = C.string_at(a, sa.value)
        x, y = _buf(b"", n + 16), _buf(b"", n + 16)
        sx, sy = C.c_size_t(n + 16), C.c_size_t(n + 16)
        assert emu.bz3_hip_decompress_device(_buf(frame), x, len(frame), C.byref(sx)) == 0
        assert emu.bz3_hip_decompress_device_planes(1, _buf(frame), y, len(frame), C.byref(sy)) == 0
        assert C.string_at(x, sx.value) == C.string_at(y, sy.value)


# ---- the lossless block size (pure Python) ------------------------------------------------------------------------------------
def _bound(n):
    return n + n // 50 + 32  # bz3_bound, include/libbz3.h


@pytest.mark.parametrize("planes", [1, 2, 4, 8])
@pytest.mark.parametrize("requested", [KiB65, 1 << 20, 16 << 20, MiB511])
def test_lossless_block_size(planes, requested):
    assert _bound(12345) == require_ref().lib.bz3_bound(12345)
    for nbytes in {0, 1, requested - planes, requested, requested + planes, 2 * requested, 37 * requested, KiB65, MiB511}:
        bs = bzip3_amd._lossless_block_size(nbytes, requested, planes)
        assert bs % planes == 0 and bs >= KiB65, (nbytes, bs)
        assert nbytes == 0 or nbytes % bs != 0 or bs > nbytes, (nbytes, bs)
        eff, sizes = block_sizes(nbytes, bs, _bound)  # the reference's own arithmetic
        assert eff <= MiB511 and sum(sizes) == nbytes, (nbytes, bs, eff)
        # as close to the request as the conditions allow: no multiple of `planes` between the two satisfies them
        step = -planes if bs < requested else planes
        for cand in range(requested - requested % planes if bs < requested else requested + (-requested) % planes, bs, step):
            if cand < KiB65:
                continue
            ceff, csizes = block_sizes(nbytes, cand, _bound)
            assert not (ceff <= MiB511 and sum(csizes) == nbytes and (nbytes == 0 or nbytes % cand != 0 or cand > nbytes)), (nbytes, bs, cand)


@pytest.mark.parametrize("planes", [1, 8])
def test_lossless_block_size_between_the_bound_and_the_request(planes):
    """501 MiB < nbytes < request: one block would be bz3_bound(nbytes) > 511 MiB, so the size drops below nbytes at once (no long walk)."""
    nbytes = (505 << 20) + 3
    bs = bzip3_amd._lossless_block_size(nbytes, MiB511, planes)
    assert bs == nbytes - nbytes % planes - (planes if nbytes % planes == 0 else 0) and bs % planes == 0
    eff, sizes = block_sizes(nbytes, bs, _bound)
    assert eff <= MiB511 and sum(sizes) == nbytes
