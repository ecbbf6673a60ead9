"""-m gpu: byte-plane frames and typed tensors on a real device (include/bz3_hip.h bz3_hip_*_device_planes[_many], the split / merge
kernel of bzip3_amd/csrc/planes.hpp; bzip3_amd.pack_tensor / unpack_tensor / pack_state_dict / unpack_state_dict), compared with the
real reference on S(x), the input with every block split into byte planes by the numpy of test_frame_planes_emu."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import bzip3_amd
from oracle_lib import require_ref
from test_frame_planes_emu import S, lay_out, mixed_spec, spec_room, sweep_specs

pytestmark = pytest.mark.gpu
MiB = 1 << 20


def _ref_frame(bs, data):
    ref = require_ref().lib
    out = (C.c_uint8 * (ref.bz3_bound(len(data)) + 64))()
    osz = C.c_size_t(len(out))
    assert ref.bz3_compress(bs, data, out, len(data), C.byref(osz)) == 0
    return bytes(out[: osz.value])


def _host(t):
    return bytes(t.cpu().numpy()) if t.numel() else b""


def _raw(x):
    """The bytes of a tensor, through numpy on the host (independent of the product's view logic)."""
    import torch

    x = x.detach().cpu().contiguous()
    if x.dtype == torch.bfloat16:
        return x.view(torch.int16).numpy().tobytes()
    return x.numpy().tobytes()


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def test_planes_kernel_on_the_gpu(gpu_lib):
    """The emulator suite's sweep of the split / merge kernel (every alignment x edge element count x tail, k = 2, 4, 8, both
    directions, a mixed launch), on torch tensors, plus segments of megabytes."""
    import torch

    rng = np.random.default_rng(31)

    def case(spec):
        room = spec_room(spec)
        src = torch.from_numpy(rng.integers(0, 256, size=room, dtype=np.uint8)).to("cuda:0")
        dst = torch.full((room,), 0xA5, dtype=torch.uint8, device="cuda:0")
        src_np, want = src.cpu().numpy(), dst.cpu().numpy().copy()
        table, writes, end = lay_out(rng, spec, src.data_ptr(), dst.data_ptr(), src_np)
        assert end <= room - 16
        for off, b in writes:
            want[off : off + len(b)] = b
        torch.cuda.synchronize()
        t = (C.c_uint64 * max(1, len(table)))(*table)
        assert gpu_lib.bz3_hip_debug_planes(src.data_ptr(), dst.data_ptr(), t, len(table) // 4) == 0
        bad = np.nonzero(dst.cpu().numpy() != want)[0]
        assert bad.size == 0, ("bytes differ at", bad[:8], spec[:2])

    for k in (2, 4, 8):
        for inverse in (0, 1):
            for spec in sweep_specs(rng, k, inverse):
                case(spec)
            case([(int(rng.integers(0, 16)), int(rng.integers(0, 16)), int(rng.integers(MiB, 9 * MiB)) // k, int(rng.integers(0, k)), k, inverse) for _ in range(4)])
    case(mixed_spec(rng))


# ---- typed tensors ------------------------------------------------------------------------------------------------------------
BS = MiB
DTYPES = ["bfloat16", "float16", "float32", "float64", "int32", "int64", "int8", "bool", "complex64"]


def _make(dtype, numel, seed, shape=None):
    import torch

    g = torch.Generator().manual_seed(seed)
    dt = getattr(torch, dtype)
    if dt.is_floating_point or dt.is_complex:
        x = (torch.randn(numel, generator=g, dtype=torch.float64 if dt == torch.float64 else torch.float32) * 0.02)
        if dt.is_complex:
            x = torch.complex(x, torch.randn(numel, generator=g) * 0.02)
        x = x.to(dt)
    elif dt == torch.bool:
        x = torch.rand(numel, generator=g) < 0.1
    elif dt == torch.int8:
        x = torch.randint(-20, 20, (numel,), generator=g, dtype=dt)
    else:
        x = torch.cumsum(torch.randint(1, 9, (numel,), generator=g, dtype=torch.int64), 0).to(dt)
    return x.reshape(shape if shape is not None else (numel,)).to("cuda:0")


@pytest.mark.parametrize("forced", [False, True], ids=["default_planes", "planes_elem_size"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_tensor_round_trip(gpu_lib, dtype, forced):
    """0, 1 and 1000 x 1001 elements and exactly 2 x block_size bytes (the size at which the byte API drops a block): same tensor
    back, the frame is the reference's frame of S(x) at the block size really used, the input is untouched."""
    import torch

    esize = torch.empty(0, dtype=getattr(torch, dtype)).element_size()
    planes = min(esize, 8) if forced else None
    cases = [((0,), 0), ((), 1), ((1,), 1), ((1000, 1001), 1000 * 1001), ((2 * BS // esize,), 2 * BS // esize)]
    for seed, (shape, numel) in enumerate(cases):
        x = _make(dtype, numel, seed, shape)
        keep = x.clone()
        p = bzip3_amd.pack_tensor(x, BS, planes=planes)
        k = planes if forced else bzip3_amd.DEFAULT_PLANES[dtype]
        assert p.planes == k and p.dtype == x.dtype and tuple(p.shape) == tuple(x.shape) and p.nbytes == numel * esize
        assert p.block_size == bzip3_amd._lossless_block_size(p.nbytes, BS, k)
        assert p.frame.dtype == torch.uint8 and p.frame.device == x.device
        raw = _raw(keep)
        assert _host(p.frame) == _ref_frame(p.block_size, S(raw, p.block_size, k, gpu_lib.bz3_bound)), (dtype, shape, "frame differs from the reference's on S(x)")
        y = bzip3_amd.unpack_tensor(p)
        assert y.dtype == x.dtype and y.shape == x.shape and y.device == x.device
        assert _raw(y) == raw and torch.equal(y, keep), (dtype, shape)
        assert _raw(x) == raw, "pack_tensor wrote to its input"
    out = torch.empty_like(keep)
    assert bzip3_amd.unpack_tensor(p, out=out) is out and _raw(out) == raw


def test_pack_tensor_takes_non_contiguous_input_and_refuses_the_cpu(gpu_lib):
    import torch

    x = _make("float32", 300 * 500, 3, (300, 500)).t()
    assert not x.is_contiguous()
    y = bzip3_amd.unpack_tensor(bzip3_amd.pack_tensor(x, BS))
    assert y.shape == x.shape and torch.equal(y, x)
    with pytest.raises(TypeError):
        bzip3_amd.pack_tensor(x.cpu())
    p = bzip3_amd.pack_tensor(x, BS)
    p.nbytes += 4
    p.shape = (300 * 500 + 1,)
    with pytest.raises(ValueError):
        bzip3_amd.unpack_tensor(p)
    with pytest.raises(ValueError):
        bzip3_amd.compress_tensor(x.contiguous().view(torch.uint8).flatten(), BS, planes=3)


def test_compress_tensor_planes_is_the_c_call(gpu_lib):
    """compress_tensor(s) with planes: uint8 in and out, the frames of the reference on S(x); planes=1 stays today's frame."""
    import torch

    xs = [_make("float32", 700_001, 5).view(torch.uint8).flatten(), _make("int64", 300_000, 6).view(torch.uint8).flatten(), _make("int8", 1234, 7).view(torch.uint8).flatten()]
    ks = [4, 8, 2]
    frames = bzip3_amd.compress_tensors(xs, BS, planes=ks)
    for x, k, f in zip(xs, ks, frames):
        assert _host(f) == _ref_frame(BS, S(_host(x), BS, k, gpu_lib.bz3_bound))
        assert _host(f) == _host(bzip3_amd.compress_tensor(x, BS, planes=k))
        assert torch.equal(bzip3_amd.decompress_tensor(f, planes=k), x)
    backs = bzip3_amd.decompress_tensors(frames, planes=ks)
    assert all(torch.equal(b, x) for b, x in zip(backs, xs))
    assert _host(bzip3_amd.compress_tensor(xs[0], BS)) == _host(bzip3_amd.compress_tensor(xs[0], BS, planes=1)) == _ref_frame(BS, _host(xs[0]))


def _model_dict():
    """~40 tensors shaped like a small mixed-precision checkpoint: 64 B to 8 MiB, several dtypes, some sizes multiples of 1 MiB."""
    sd, seed = {}, 100
    for layer in range(4):
        for name, dtype, shape in (("attn.w", "bfloat16", (1024, 1024)), ("attn.b", "bfloat16", (1024,)), ("mlp.w", "float16", (512, 1000)),
                                   ("mlp.master", "float32", (1024, 2048)), ("mlp.exp_avg_sq", "float32", (512, 1000)), ("ln.w", "float32", (16,)),
                                   ("ids", "int64", (70_000 + layer,)), ("mask", "bool", (333, 77)), ("step", "int32", ()), ("q.scale", "float64", (257,))):
            seed += 1
            numel = int(np.prod(shape)) if shape else 1
            sd[f"layers.{layer}.{name}"] = _make(dtype, numel, seed, shape)
    sd["empty"] = _make("float32", 0, 1, (0, 3))
    return sd


def test_pack_state_dict(gpu_lib):
    import torch

    sd = _model_dict()
    assert len(sd) > 40
    gpu_lib.bz3_hip_debug_cm_launches(1)
    packed = bzip3_amd.pack_state_dict(sd, BS)
    launches = gpu_lib.bz3_hip_debug_cm_launches(1)
    assert 0 < launches < len(sd), (launches, len(sd))
    assert list(packed) == list(sd)
    back = bzip3_amd.unpack_state_dict(packed)
    for name, x in sd.items():
        p = packed[name]
        assert p.planes == bzip3_amd.DEFAULT_PLANES[str(x.dtype).replace("torch.", "")]
        y = back[name]
        assert y.dtype == x.dtype and y.shape == x.shape and _raw(y) == _raw(x), name
        one = bzip3_amd.pack_tensor(x, BS)
        assert one.block_size == p.block_size and _host(one.frame) == _host(p.frame), name
    forced = bzip3_amd.pack_state_dict({k: sd[k] for k in list(sd)[:10]}, BS, planes=2)
    assert all(p.planes == 2 for p in forced.values())
    assert all(_raw(v) == _raw(sd[k]) for k, v in bzip3_amd.unpack_state_dict(forced).items())
    assert bzip3_amd.pack_state_dict({}) == {} and bzip3_amd.unpack_state_dict({}) == {}


def test_one_block_of_256_mib_of_fp32(gpu_lib):
    """One launch of the split kernel at the benchmark's block size: the frame is the reference's frame of S(x), by digest."""
    x = _make("float32", MiB, 77).repeat(64)  # 64 M elements; the repeats let LZP shorten the block, so the CPU reference takes seconds, not minutes
    p = bzip3_amd.pack_tensor(x, 511 * MiB)  # larger than the tensor: one block (src/libbz3.c:877)
    assert p.planes == 4 and p.block_size == 511 * MiB
    raw = _raw(x)
    want = _ref_frame(p.block_size, S(raw, p.block_size, 4, gpu_lib.bz3_bound))
    got = _host(p.frame)
    assert len(got) == len(want) and hashlib.sha256(got).hexdigest() == hashlib.sha256(want).hexdigest()
    assert _raw(bzip3_amd.unpack_tensor(p)) == raw


# ---- compression evidence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int64_cumsum", "float32_normal"])
def test_planes_shrink_what_the_defaults_say_they_shrink(gpu_lib, kind):
    """With the reference library alone: the frame of S(x) is smaller than the frame of x for sorted 64-bit integers (k = 8) and
    N(0, 0.02) fp32 (k = 4), 2 M elements at 1 MiB blocks.  Then the product's frames have the reference's lengths."""
    import torch

    rng = np.random.default_rng(2024)
    n = 2_000_000
    if kind == "int64_cumsum":
        k, raw = 8, np.cumsum(rng.integers(1, 9, size=n)).astype("<i8").tobytes()
    else:
        k, raw = 4, (rng.standard_normal(n) * 0.02).astype("<f4").tobytes()
    bs = bzip3_amd._lossless_block_size(len(raw), BS, k)
    ref = require_ref().lib
    plain, planes = _ref_frame(bs, raw), _ref_frame(bs, S(raw, bs, k, ref.bz3_bound))
    print(f"{kind}: {len(raw)} bytes, interleaved {len(plain)}, byte planes {len(planes)}")
    assert len(planes) < len(plain)
    x = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda:0")
    assert bzip3_amd.compress_tensor(x, bs, planes=k).numel() == len(planes)
    assert bzip3_amd.compress_tensor(x, bs).numel() == len(plain)
