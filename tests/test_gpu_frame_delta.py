"""-m gpu: delta frames on a real device (include/bz3_hip.h bz3_hip_*_device_delta[_many], bz3_hip_crc32c_device, the delta tiles of
bzip3_amd/csrc/planes.hpp; the `base` arguments of bzip3_amd's tensor calls), compared with the real reference on S(D(x, b)), with D
from the numpy of test_frame_delta_emu."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
from oracle_lib import require_ref
from test_frame_delta_emu import D, D_inv, delta_case, in_place_case, mixed_spec3, sweep_specs3, _r16
from test_frame_planes_emu import S, chunk_sizes, merge_k, per_block
from test_gpu_frame_planes import DTYPES, _host, _make, _raw, _ref_frame

pytestmark = pytest.mark.gpu
MiB = 1 << 20
BS = MiB


def _gpu_alloc(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t.data_ptr(), t.data_ptr(), lambda: t.cpu().numpy()


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def test_delta_kernel_on_the_gpu(gpu_lib):
    """The emulator suite's sweep (k = 1, 2, 4, 8, both directions, the three alignments, edge counts and tails), segments of
    megabytes, the mixed launch and the in-place launch, on device memory."""
    rng = np.random.default_rng(33)
    for k in (1, 2, 4, 8):
        for inverse in (0, 1):
            for spec in sweep_specs3(rng, k, inverse):
                delta_case(gpu_lib.bz3_hip_debug_delta, rng, spec, _gpu_alloc)
            delta_case(gpu_lib.bz3_hip_debug_delta, rng,
                       [(_r16(rng), _r16(rng), _r16(rng), int(rng.integers(MiB, 9 * MiB)) // k, int(rng.integers(0, k)), k, inverse, 1) for _ in range(4)], _gpu_alloc)
    delta_case(gpu_lib.bz3_hip_debug_delta, rng, mixed_spec3(rng), _gpu_alloc)
    in_place_case(gpu_lib.bz3_hip_debug_delta, rng, _gpu_alloc)
    in_place_case(gpu_lib.bz3_hip_debug_delta, rng, _gpu_alloc, sizes=(3 * MiB + 5, 1_000_003))


# ---- byte tensors against the reference -----------------------------------------------------------------------------------------
def _pair(n, seed, step=1e-3, dtype="float32"):
    """(x, base) as uint8 GPU tensors: base ~ N(0, 0.02) of `dtype`, x = base + N(0, step * 0.02) rounded to the dtype."""
    import torch

    g = torch.Generator().manual_seed(seed)
    b = torch.randn(n, generator=g) * 0.02
    x = b + torch.randn(n, generator=g) * (0.02 * step)
    dt = getattr(torch, dtype)
    return x.to(dt).to("cuda:0").view(torch.uint8), b.to(dt).to("cuda:0").view(torch.uint8)


def _restore(frame, k, base):
    """What a delta frame decodes to anywhere: the reference's bz3_decompress, merge_k per chunk, plus the base."""
    ref = require_ref().lib
    out = (C.c_uint8 * max(1, len(base)))()
    osz = C.c_size_t(len(base))
    assert ref.bz3_decompress(frame, out, len(frame), C.byref(osz)) == 0
    sx = C.string_at(out, osz.value)
    return bytes(D_inv(per_block(merge_k, sx, chunk_sizes(frame, len(sx)), k), base[: len(sx)]))


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_delta_frames_match_the_reference(gpu_lib, k):
    """Several blocks of 1 MiB + 7 (every block starts inside an element and has a tail): the frame is the reference's frame of
    S_k(D(x, b)), it decodes anywhere to x, and on the device to x in a new tensor and over the base."""
    import torch

    bs = BS + 7
    x, base = _pair(800_001, 7 + k)
    xb, bb = _host(x), _host(base)
    frame = bzip3_amd.compress_tensor(x, bs, planes=k, base=base)
    assert _host(frame) == _ref_frame(bs, S(bytes(D(xb, bb)), bs, k, gpu_lib.bz3_bound))
    assert _restore(_host(frame), k, bb) == xb
    assert _host(x) == xb and _host(base) == bb, "an input was written"
    assert torch.equal(bzip3_amd.decompress_tensor(frame, planes=k, base=base), x)
    over = base.clone()
    got = bzip3_amd.decompress_tensor(frame, out=over, planes=k, base=over)
    assert got.data_ptr() == over.data_ptr() and torch.equal(over, x)


def test_identities(gpu_lib):
    import torch

    x, _ = _pair(700_001, 3)
    for k in (1, 4):
        plain = _host(bzip3_amd.compress_tensor(x, BS, planes=k))
        assert _host(bzip3_amd.compress_tensor(x, BS, planes=k, base=torch.zeros_like(x))) == plain
        assert _host(bzip3_amd.compress_tensor(x, BS, planes=k, base=x.clone())) == _ref_frame(BS, bytes(x.numel()))


def test_many_with_and_without_bases(gpu_lib, monkeypatch):
    """Frames with and without bases and different k in one call, windows of 3 blocks that cut through frames: each equals its single
    call; decoding (some over their bases) restores every tensor."""
    import torch

    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    pairs = [_pair(n, 20 + i) for i, n in enumerate((600_000, 1, 300_001, 0, 70_000, 1_000_003))]
    xs = [p[0] for p in pairs]
    bases = [p[1] if i % 3 != 1 else None for i, p in enumerate(pairs)]
    ks = [4, 1, 2, 8, 1, 8]
    frames = bzip3_amd.compress_tensors(xs, BS, planes=ks, bases=bases)
    for x, k, b, f in zip(xs, ks, bases, frames):
        assert _host(f) == _host(bzip3_amd.compress_tensor(x, BS, planes=k, base=b))
        d = _host(x) if b is None else bytes(D(_host(x), _host(b)))
        assert _host(f) == _ref_frame(BS, S(d, BS, k, gpu_lib.bz3_bound))
    keep = [None if b is None else b.clone() for b in bases]
    outs = [keep[i] if keep[i] is not None and i % 2 == 0 else torch.empty_like(x) for i, x in enumerate(xs)]
    backs = bzip3_amd.decompress_tensors(frames, outs, planes=ks, bases=keep)
    assert all(torch.equal(b, x) for b, x in zip(backs, xs))
    assert all(o.data_ptr() == b.data_ptr() for o, b in zip(outs, backs) if o.numel())


def test_corrupt_frame_in_place_commits_whole_chunks_and_leaves_the_base(gpu_lib):
    """A flipped byte in the second of three chunks, decoded over the base: BZ3_ERR_CRC-class failure, the first chunk is x, the rest
    of the tensor is still the base; the neighbours in the same call are untouched by it."""
    import torch

    x, base = _pair(700_000, 31)
    frame = bzip3_amd.compress_tensor(x, BS, planes=4, base=base).clone()
    f = _host(frame)
    second = 13 + 8 + int.from_bytes(f[13:17], "little")
    bad = frame.clone()
    bad[second + 8 + 40] ^= 0x40
    over, over2 = base.clone(), base.clone()
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.decompress_tensors([frame, bad, frame], [torch.empty_like(x), over, over2], planes=4, bases=[base, over, over2])
    assert e.value.index == 1 and e.value.codes[0] == 0 and e.value.codes[2] == 0
    assert torch.equal(e.value.outs[0], x) and torch.equal(over2, x)
    n = e.value.outs[1].numel()
    assert n == BS and torch.equal(over[:n], x[:n]) and torch.equal(over[n:], base[n:])


def test_arguments(gpu_lib):
    """Base too short, partial overlap, a host pointer as base, n = 0, through the C calls."""
    import torch

    INIT = bzip3_amd.BZ3_ERR_INIT
    x, base = _pair(700_000, 41)  # 2.8 MB: three chunks at 1 MiB
    frame = bzip3_amd.compress_tensor(x, BS, planes=2, base=base)
    vp = C.c_void_p
    # too short: two chunks fit
    short = base[: x.numel() - 1].clone()
    out = torch.full((x.numel(),), 0xA5, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.decompress_tensor(frame, out=out, planes=2, base=short)
    assert e.value.code == bzip3_amd.BZ3_ERR_DATA_TOO_BIG and e.value.out.numel() == 2 * BS
    assert torch.equal(out[: 2 * BS], x[: 2 * BS]) and bool((out[2 * BS :] == 0xA5).all())
    # partial overlap: nothing written
    arena = torch.cat([base, torch.full((BS,), 0xA5, dtype=torch.uint8, device="cuda:0")])
    before = arena.clone()
    torch.cuda.synchronize()
    for off in (1, 16, base.numel() - 1):
        osz = C.c_size_t(arena.numel() - off)
        rc = gpu_lib.bz3_hip_decompress_device_delta(2, vp(frame.data_ptr()), vp(arena.data_ptr()), base.numel(), vp(arena.data_ptr() + off), frame.numel(), C.byref(osz))
        assert rc == INIT and torch.equal(arena, before)
    # compress: the coded frame may overlap neither the input nor the base
    cap = gpu_lib.bz3_bound(x.numel())
    big = torch.cat([x, torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda:0")])
    before = big.clone()
    torch.cuda.synchronize()
    osz = C.c_size_t(cap)
    assert gpu_lib.bz3_hip_compress_device_delta(BS, 2, vp(big.data_ptr()), vp(base.data_ptr()), vp(big.data_ptr() + x.numel() - 1), x.numel(), C.byref(osz)) == INIT
    assert torch.equal(big, before)
    # a host pointer as base
    host = (C.c_uint8 * x.numel())()
    osz = C.c_size_t(cap)
    dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert gpu_lib.bz3_hip_compress_device_delta(BS, 2, vp(x.data_ptr()), host, vp(dst.data_ptr()), x.numel(), C.byref(osz)) == INIT
    osz = C.c_size_t(x.numel())
    assert gpu_lib.bz3_hip_decompress_device_delta(2, vp(frame.data_ptr()), host, x.numel(), vp(out.data_ptr()), frame.numel(), C.byref(osz)) == INIT
    assert bool((dst == 0xA5).all())
    # n = 0
    assert gpu_lib.bz3_hip_compress_device_delta_many(BS, 0, None, None, None, None, None, None, None) == 0
    assert gpu_lib.bz3_hip_decompress_device_delta_many(0, None, None, None, None, None, None, None, None) == 0
    assert bzip3_amd.compress_tensors([], bases=[]) == [] and bzip3_amd.decompress_tensors([], bases=None) == []


def test_crc32c_device(gpu_lib):
    import torch

    x, _ = _pair(100_003, 51)
    h = _host(x)
    for off, n in ((0, x.numel()), (1, 70_000), (3, 5), (2, 0)):
        assert bzip3_amd.base_crc(x[off : off + n]) == gpu_lib.bz3_hip_stage_crc32c(h[off : off + n], n, 1), (off, n)


# ---- typed tensors ------------------------------------------------------------------------------------------------------------
def _special(dtype, numel, seed):
    """_make plus NaNs with payloads, -0.0 and infinities for the float dtypes."""
    import torch

    x = _make(dtype, numel, seed)
    if x.dtype.is_floating_point and numel >= 8:
        x[0], x[1], x[2], x[3] = float("nan"), -0.0, float("inf"), float("-inf")
        bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]
        x.view(bits)[4] = -2  # all ones but the lowest bit: a NaN with a full payload and the sign set
    return x


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_tensor_against_a_base_round_trips(gpu_lib, dtype):
    """Every dtype of DEFAULT_PLANES' kinds, with NaN payloads, -0.0, infinities, 0-d, empty and non-contiguous input: bit-exact, the
    frame is the reference's frame of S(D(x, b)) at the default planes (1; float64: 8), the inputs are untouched."""
    import torch

    for seed, (shape, numel) in enumerate([((0,), 0), ((), 1), ((300, 500), 150_000), ((2 * BS // 8,), 2 * BS // 8)]):
        base = _special(dtype, numel, 60 + seed).reshape(shape)
        x = _special(dtype, numel, 70 + seed).reshape(shape)
        if numel > 100:
            x = torch.where(torch.rand(shape, device=x.device) < 0.9, base, x)  # most elements unchanged
        keep_x, keep_b = _raw(x), _raw(base)
        p = bzip3_amd.pack_tensor(x, BS, base=base)
        want_planes = 8 if dtype == "float64" else 1  # the one dtype whose planes are more than 3 % smaller after D at every step measured
        assert p.delta and p.planes == want_planes and p.base_crc == gpu_lib.bz3_hip_stage_crc32c(keep_b, len(keep_b), 1)
        assert "delta" in repr(p)
        assert _host(p.frame) == _ref_frame(p.block_size, S(bytes(D(keep_x, keep_b)), p.block_size, want_planes, gpu_lib.bz3_bound)), (dtype, shape)
        y = bzip3_amd.unpack_tensor(p, base=base)
        assert y.dtype == x.dtype and y.shape == x.shape and _raw(y) == keep_x
        assert _raw(x) == keep_x and _raw(base) == keep_b
        forced = bzip3_amd.pack_tensor(x, BS, planes=min(8, max(1, x.element_size())), base=base)
        assert _raw(bzip3_amd.unpack_tensor(forced, base=base)) == keep_x
    xt = _make(dtype, 300 * 500, 5, (300, 500)).t()
    bt = _make(dtype, 300 * 500, 6, (500, 300))
    assert not xt.is_contiguous()
    assert _raw(bzip3_amd.unpack_tensor(bzip3_amd.pack_tensor(xt, BS, base=bt), base=bt)) == _raw(xt)
    bn = _make(dtype, 300 * 500, 7, (300, 500)).t()  # a non-contiguous base, on both sides
    assert not bn.is_contiguous()
    assert _raw(bzip3_amd.unpack_tensor(bzip3_amd.pack_tensor(xt, BS, base=bn), base=bn)) == _raw(xt)


def test_plain_packed_tensor_keeps_its_defaults(gpu_lib):
    x = _make("float32", 1000, 1)
    p = bzip3_amd.pack_tensor(x, BS)
    assert p.delta is False and p.base_crc is None and p.planes == 4
    q = bzip3_amd.PackedTensor(p.frame, p.dtype, p.shape, p.planes, p.block_size, p.nbytes)  # the constructor of before
    assert q.delta is False and q.base_crc is None and _raw(bzip3_amd.unpack_tensor(q)) == _raw(x)


def test_pack_state_dict_against_a_base_dict(gpu_lib):
    """A missing name and a reshaped tensor are packed without a base; inplace=True returns the base's own storage."""
    import torch

    sd = {"a.w": _make("bfloat16", 1024 * 512, 1, (1024, 512)), "a.b": _make("float32", 1024, 2), "new": _make("float32", 5000, 3),
          "reshaped": _make("float16", 6000, 4, (60, 100)), "ids": _make("int64", 70_001, 5), "empty": _make("float32", 0, 6, (0, 3))}
    base = {"a.w": _make("bfloat16", 1024 * 512, 11, (1024, 512)), "a.b": sd["a.b"].clone(), "reshaped": _make("float16", 6000, 14, (100, 60)),
            "ids": sd["ids"] + 1, "empty": _make("float32", 0, 6, (0, 3)), "unused": _make("float32", 10, 7)}
    packed = bzip3_amd.pack_state_dict(sd, BS, base=base)
    assert list(packed) == list(sd)
    assert {k: p.delta for k, p in packed.items()} == {"a.w": True, "a.b": True, "new": False, "reshaped": False, "ids": True, "empty": True}
    for k, p in packed.items():
        assert p.planes == (1 if p.delta else bzip3_amd.default_planes(sd[k].dtype)), k
        one = bzip3_amd.pack_tensor(sd[k], BS, base=base[k] if p.delta else None)
        assert _host(one.frame) == _host(p.frame) and one.base_crc == p.base_crc, k
    back = bzip3_amd.unpack_state_dict(packed, base=base)
    assert all(_raw(back[k]) == _raw(sd[k]) for k in sd)
    assert all(back[k].data_ptr() != base[k].data_ptr() for k in sd if packed[k].delta and sd[k].numel())
    with pytest.raises(ValueError):
        bzip3_amd.unpack_state_dict(packed)  # no base
    ptrs = {k: v.data_ptr() for k, v in base.items()}
    keep_unused = _raw(base["unused"])
    back = bzip3_amd.unpack_state_dict(packed, base=base, inplace=True)
    for k in sd:
        assert _raw(back[k]) == _raw(sd[k]), k
        if packed[k].delta:
            assert back[k] is base[k] and back[k].data_ptr() == ptrs[k], k
    assert _raw(base["unused"]) == keep_unused and _raw(base["reshaped"]) != _raw(sd["reshaped"])


def test_wrong_base_is_refused_before_anything_is_written(gpu_lib):
    import torch

    x, base = _make("float32", 300_000, 1), _make("float32", 300_000, 2)
    p = bzip3_amd.pack_tensor(x, BS, base=base)
    other = base.clone()
    other[1234] += 1
    out = torch.full_like(x, 7.0)
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor(p, out=out, base=other)
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor(p, out=out, base=base[:-1])  # another size, also with the check off
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor(p, out=out, base=base[:-1], check_base=False)
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor(p, out=out)
    assert bool((out == 7.0).all())
    keep = other.clone()
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor(p, out=other, base=other)  # in place: the base is still what it was
    assert torch.equal(other, keep)
    # check_base=False skips the read: the codec cannot tell, and returns x + (other - base) byte-wise without an error
    y = bzip3_amd.unpack_tensor(p, base=other, check_base=False)
    want = D_inv(D(_raw(x), _raw(base)), _raw(other))
    assert _raw(y) == bytes(want) and _raw(y) != _raw(x)
    p.base_crc = None  # a record without a checksum is decoded as it is
    assert _raw(bzip3_amd.unpack_tensor(p, base=base)) == _raw(x)


def test_base_argument_errors(gpu_lib):
    import torch

    x = _make("float32", 1000, 1)
    with pytest.raises(TypeError):
        bzip3_amd.pack_tensor(x, BS, base=x.cpu())
    with pytest.raises(TypeError):
        bzip3_amd.pack_tensor(x, BS, base=[0.0] * 1000)
    with pytest.raises(ValueError):
        bzip3_amd.pack_tensor(x, BS, base=x[:-1])
    with pytest.raises(ValueError):
        bzip3_amd.pack_tensor(x, BS, base=x.to(torch.float64))
    raw = x.view(torch.uint8)
    with pytest.raises(TypeError):
        bzip3_amd.compress_tensor(raw, BS, base=raw.cpu())
    with pytest.raises(ValueError):
        bzip3_amd.compress_tensor(raw, BS, base=raw[:-1])
    with pytest.raises(ValueError):
        bzip3_amd.compress_tensors([raw, raw], BS, bases=[raw])
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            bzip3_amd.pack_tensor(x, BS, base=x.to("cuda:1"))


def test_bfloat16_step_sizes_are_the_references(gpu_lib):
    """A bfloat16 tensor one step of 1e-3 sigma from its base, packed with and without the base: the device frames have the sizes the
    reference gives for S(D(x, b)) and for x.  (What the ratio is, is the reference's business: none is asserted.)"""
    import torch

    x, base = _pair(1 << 20, 77, step=1e-3, dtype="bfloat16")
    xt, bt = x.view(torch.bfloat16), base.view(torch.bfloat16)
    with_base, alone = bzip3_amd.pack_tensor(xt, BS, base=bt), bzip3_amd.pack_tensor(xt, BS)
    ref_delta = _ref_frame(with_base.block_size, S(bytes(D(_host(x), _host(base))), with_base.block_size, with_base.planes, gpu_lib.bz3_bound))
    ref_alone = _ref_frame(alone.block_size, S(_host(x), alone.block_size, alone.planes, gpu_lib.bz3_bound))
    print(f"bfloat16, step 1e-3 sigma: {x.numel()} bytes, alone {len(ref_alone)}, against the base {len(ref_delta)}")
    assert with_base.frame.numel() == len(ref_delta) and alone.frame.numel() == len(ref_alone)
    assert _raw(bzip3_amd.unpack_tensor(with_base, base=bt)) == _host(x)
