"""-m gpu: the batched checksum on a real device (include/bz3_hip.h bz3_hip_crc32c_device_many; bzip3_amd.crc32c_tensors), the content
checksum of packed tensors (PackedTensor.crc, `checksum=` / `verify=`), checkpoint files (save_packed / load_packed) and chains of them
(check_chain / unpack_chain).  The yardstick of every checksum is bz3_hip_stage_crc32c of the host bytes (the block codec's kernels on a
buffer of its own) and, for the small buffers, the bitwise CRC of test_crc_many_emu."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
from test_crc_many_emu import SEG, SIZES, crc_ref
from test_gpu_frame_planes import _host, _raw

pytestmark = pytest.mark.gpu
KiB, MiB = 1 << 10, 1 << 20
INIT, OK = bzip3_amd.BZ3_ERR_INIT, bzip3_amd.BZ3_OK
BS = 128 * KiB


def _call(lib, ptrs, sizes, inits, fill=0xDEAD0000):
    n = len(ptrs)
    crcs = (C.c_uint32 * max(1, n))(*([fill + i for i in range(n)] or [0]))
    rc = lib.bz3_hip_crc32c_device_many(n, (C.c_void_p * max(1, n))(*ptrs), (C.c_size_t * max(1, n))(*sizes),
                                        None if inits is None else (C.c_uint32 * max(1, n))(*inits), crcs)
    return rc, list(crcs)[:n]


def _stage(lib, data, init=1):
    return lib.bz3_hip_stage_crc32c(data, len(data), init)


@pytest.fixture(scope="module")
def arena(gpu_lib):
    """16 MiB of random bytes on cuda:0 and the same on the host."""
    import torch

    host = np.random.default_rng(2024).integers(0, 256, size=16 * MiB, dtype=np.uint8)
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    return dev, host.tobytes()


def test_sweep_big_and_small_buffers_in_one_call(gpu_lib, arena):
    """The emulator suite's sizes at every start address mod 4 with four start states, five buffers of 1 to 3 MiB of odd sizes at odd
    offsets of one allocation and 300 small ones: one call."""
    import torch

    dev, host = arena
    rng = np.random.default_rng(11)
    base = dev.data_ptr()
    assert base % 4 == 0
    spec = []  # (offset, size, init)
    for align in range(4):
        for n in SIZES:
            for init in (0, 1, 0xFFFFFFFF, int(rng.integers(0, 2 ** 32))):
                spec.append((64 + align, n, init))
    big = [(1 * MiB + 1, MiB + 1, 1), (3 * MiB + 3, 3 * MiB - 5, 1), (6 * MiB + 7, 2 * MiB + 255, 7), (9 * MiB + 2, MiB + SEG + 259, 0), (11 * MiB + 5, 2 * MiB + 12345, 0xFFFFFFFF)]
    small = [(int(rng.integers(0, 15 * MiB)), int(rng.integers(0, 3000)), int(rng.integers(0, 2 ** 32))) for _ in range(300)]
    spec = spec + big + small
    order = rng.permutation(len(spec))
    spec = [spec[i] for i in order]
    before = dev.clone()
    torch.cuda.synchronize()
    rc, got = _call(gpu_lib, [base + o for o, _, _ in spec], [n for _, n, _ in spec], [i for _, _, i in spec])
    assert rc == OK
    for (o, n, init), g in zip(spec, got):
        data = host[o : o + n]
        assert g == _stage(gpu_lib, data, init), (o, n, hex(init))
        if n <= 3000:
            assert g == crc_ref(init, data), (o, n, hex(init))
    assert torch.equal(dev, before), "the call wrote to a buffer"
    # inits == NULL is 1 everywhere; zero-size buffers with a NULL pointer among device buffers
    rc, got = _call(gpu_lib, [base + 3, None, base + MiB + 1, None], [70_001, 0, 5, 0], None)
    assert rc == OK and got == [_stage(gpu_lib, host[3:70_004]), 1, crc_ref(1, host[MiB + 1 : MiB + 6]), 1]


def test_launch_count_on_the_device(gpu_lib, arena):
    dev, host = arena
    base = dev.data_ptr()
    counts = []
    for n in (1, 300):
        sizes = [1 + (37 * i) % 900 for i in range(n)]
        gpu_lib.bz3_hip_debug_crc_launches(1)
        rc, got = _call(gpu_lib, [base + 5 * i for i in range(n)], sizes, None)
        counts.append(gpu_lib.bz3_hip_debug_crc_launches(1))
        assert rc == OK and got == [crc_ref(1, host[5 * i : 5 * i + s]) for i, s in enumerate(sizes)]
    assert counts[0] == counts[1] and 1 <= counts[0] <= 3, counts
    # buffers of several segments: still the same count for 1 and for 300
    counts = []
    for n in (1, 300):
        gpu_lib.bz3_hip_debug_crc_launches(1)
        rc, _ = _call(gpu_lib, [base + 3 + 7 * i for i in range(n)], [2 * SEG + 100 + i for i in range(n)], None)
        counts.append(gpu_lib.bz3_hip_debug_crc_launches(1))
        assert rc == OK
    assert counts[0] == counts[1] and 1 <= counts[0] <= 3, counts


def test_a_host_pointer_among_device_buffers(gpu_lib, arena):
    dev, host = arena
    base = dev.data_ptr()
    on_host = (C.c_uint8 * 4096)()
    rc, got = _call(gpu_lib, [base, C.addressof(on_host), base + 100], [1000, 4096, 1000], None, fill=0xABCD0000)
    assert rc == INIT and got == [0xABCD0000, 0xABCD0001, 0xABCD0002], "crcs was written"
    rc, got = _call(gpu_lib, [C.addressof(on_host)], [16], None, fill=0xABCD0000)
    assert rc == INIT and got == [0xABCD0000]
    # of size 0 it is never looked at
    rc, got = _call(gpu_lib, [base, C.addressof(on_host)], [10, 0], [1, 9])
    assert rc == OK and got == [crc_ref(1, host[:10]), 9]


def test_buffers_on_two_gpus(gpu_lib):
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    a = torch.arange(200, dtype=torch.uint8, device="cuda:0")
    b = torch.arange(200, dtype=torch.uint8, device="cuda:1")
    torch.cuda.synchronize(0)
    torch.cuda.synchronize(1)
    rc, got = _call(gpu_lib, [a.data_ptr(), b.data_ptr()], [200, 200], None, fill=0xABCD0000)
    assert rc == INIT and got == [0xABCD0000, 0xABCD0001]
    with pytest.raises(ValueError):
        bzip3_amd.crc32c_tensors([a, b])
    assert bzip3_amd.crc32c_tensors([b, b[3:50]]) == [crc_ref(1, bytes(range(200))), crc_ref(1, bytes(range(3, 50)))]


def test_crc32c_tensors(gpu_lib, arena):
    import torch

    dev, host = arena
    assert bzip3_amd.crc32c_tensors([]) == []
    ts = [dev[1:70_002], dev[:0], dev[5 * MiB + 3 : 6 * MiB + 4], dev[1:70_002], torch.empty(0, dtype=torch.uint8, device="cuda:0")]
    got = bzip3_amd.crc32c_tensors(ts)
    assert all(isinstance(c, int) for c in got)
    assert got == [_stage(gpu_lib, host[1:70_002]), 1, _stage(gpu_lib, host[5 * MiB + 3 : 6 * MiB + 4]), _stage(gpu_lib, host[1:70_002]), 1]
    assert got[:4] == [bzip3_amd.base_crc(t) for t in ts[:4]]
    assert bzip3_amd.crc32c_tensors(ts[:2], inits=[5, 6]) == [_stage(gpu_lib, host[1:70_002], 5), 6]
    with pytest.raises(ValueError):
        bzip3_amd.crc32c_tensors(ts[:2], inits=[5])
    for bad in (dev.cpu()[:10], dev[:16].view(torch.int32), dev[:64:2], host[:10]):
        with pytest.raises(TypeError):
            bzip3_amd.crc32c_tensors([dev[:4], bad])


# ---- packed tensors -----------------------------------------------------------------------------------------------------------
def _state_dict(n, seed, lo=64 * KiB, hi=256 * KiB):
    """n float32 tensors of lo to hi bytes of N(0, 0.02), of odd element counts, on cuda:0."""
    import torch

    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i in range(n):
        numel = int(torch.randint(lo // 4, hi // 4, (1,), generator=g)) | 1
        sd[f"t{i}"] = (torch.randn(numel, generator=g) * 0.02).to("cuda:0")
    return sd


def _step(sd, seed, step=1e-3):
    import torch

    g = torch.Generator().manual_seed(seed)
    return {k: v + (torch.randn(v.numel(), generator=g) * (0.02 * step)).to(v.device).reshape(v.shape).to(v.dtype) for k, v in sd.items()}


def test_pack_40_tensors_against_a_base_dict(gpu_lib):
    import torch

    base = _state_dict(40, 1)
    sd = _step(base, 2)
    for k in ("t3", "t17", "t39"):  # three without a base
        del base[k]
    gpu_lib.bz3_hip_debug_crc_launches(1)
    packed = bzip3_amd.pack_state_dict(sd, BS, base=base)
    assert 1 <= gpu_lib.bz3_hip_debug_crc_launches(1) <= 3
    plain = bzip3_amd.pack_state_dict(sd, BS, base=base, checksum=False)
    for k, p in packed.items():
        want_base = _stage(gpu_lib, _raw(base[k])) if k in base else None
        assert p.delta == (k in base) and p.base_crc == want_base, k
        assert p.crc == _stage(gpu_lib, _raw(sd[k])) == bzip3_amd.base_crc(sd[k].view(torch.uint8)), k
        q = plain[k]
        assert q.crc is None and q.base_crc == want_base and _host(q.frame) == _host(p.frame), k
        assert (q.planes, q.block_size, q.nbytes, q.delta) == (p.planes, p.block_size, p.nbytes, p.delta)
    gpu_lib.bz3_hip_debug_crc_launches(1)
    back = bzip3_amd.unpack_state_dict(packed, base=base, check_base=True)
    assert 1 <= gpu_lib.bz3_hip_debug_crc_launches(1) <= 3
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    back = bzip3_amd.unpack_state_dict(packed, base=base, check_base=False, verify=True)
    assert 1 <= gpu_lib.bz3_hip_debug_crc_launches(1) <= 3
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    # the same for the rows path: all bases in one call, the same error for the first offender before anything is decoded
    gpu_lib.bz3_hip_debug_crc_launches(1)
    rows = bzip3_amd.unpack_state_dict(packed, base=base, rows={"t0": (0, 100), "t3": (5, 9)})
    assert 1 <= gpu_lib.bz3_hip_debug_crc_launches(1) <= 3
    assert torch.equal(rows["t0"], sd["t0"][:100]) and torch.equal(rows["t3"], sd["t3"][5:9]) and torch.equal(rows["t5"], sd["t5"])
    wrong = dict(base)
    wrong["t8"], wrong["t20"] = base["t8"] + 1, base["t20"] + 1
    cm = gpu_lib.bz3_hip_debug_cm_launches(0)
    with pytest.raises(ValueError, match="base 't8'"):
        bzip3_amd.unpack_state_dict(packed, base=wrong, rows={"t0": (0, 100)})
    with pytest.raises(ValueError, match="base 8 "):
        bzip3_amd.unpack_state_dict(packed, base=wrong)
    assert gpu_lib.bz3_hip_debug_cm_launches(0) == cm, "something was decoded before the bases were checked"


def test_verify(gpu_lib):
    import torch

    base = _state_dict(2, 5)
    sd = _step(base, 6)
    other = _step(base, 7)
    p = bzip3_amd.pack_tensor(sd["t0"], BS, base=base["t0"])
    assert p.crc == _stage(gpu_lib, _raw(sd["t0"]))
    assert torch.equal(bzip3_amd.unpack_tensor(p, base=base["t0"], verify=True), sd["t0"])
    with pytest.raises(ValueError, match="checksum"):
        bzip3_amd.unpack_tensor(p, base=other["t0"], check_base=False, verify=True)
    noise = bzip3_amd.unpack_tensor(p, base=other["t0"], check_base=False)  # as before: other bytes and no error
    assert noise.shape == sd["t0"].shape and _raw(noise) != _raw(sd["t0"])
    # in place, the check comes after the write
    over = other["t0"].clone()
    with pytest.raises(ValueError, match="checksum"):
        bzip3_amd.unpack_tensor(p, out=over, base=over, check_base=False, verify=True)
    assert _raw(over) == _raw(noise)
    # a record without a checksum is not verified
    q = bzip3_amd.pack_tensor(sd["t0"], BS, base=base["t0"], checksum=False)
    assert q.crc is None and _raw(bzip3_amd.unpack_tensor(q, base=other["t0"], check_base=False, verify=True)) == _raw(noise)
    # the dict call names the tensor
    packed = bzip3_amd.pack_state_dict(sd, BS, base=base)
    with pytest.raises(ValueError, match="'t1'"):
        bzip3_amd.unpack_state_dict(packed, base={"t0": base["t0"], "t1": other["t1"]}, check_base=False, verify=True)
    with pytest.raises(ValueError, match="rows"):
        bzip3_amd.unpack_state_dict(packed, base=base, rows={"t0": (0, 10)}, verify=True)


def _every_dtype(seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, name in enumerate(bzip3_amd.DEFAULT_PLANES):
        dt = getattr(torch, name)
        shape = (37 + i, 501)
        if dt.is_complex:
            x = torch.complex(torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64)) * 0.02
        elif dt.is_floating_point:
            x = torch.randn(shape, generator=g, dtype=torch.float64) * 0.02
        elif dt == torch.bool:
            x = torch.rand(shape, generator=g) < 0.1
        elif dt == torch.uint8:
            x = torch.randint(0, 40, shape, generator=g)
        else:
            x = torch.randint(-20, 20, shape, generator=g)
        sd[name] = x.to(dt).to("cuda:0")
    sd["scalar"] = torch.tensor(3.5, device="cuda:0")
    sd["none"] = torch.empty((0, 3), dtype=torch.float16, device="cuda:0")
    return sd


def test_file_round_trip_every_dtype(gpu_lib, tmp_path):
    import torch

    sd = _every_dtype(8)
    assert set(bzip3_amd.DEFAULT_PLANES) <= set(sd)
    packed = bzip3_amd.pack_state_dict(sd, BS)
    path = str(tmp_path / "all.bz3t")
    bzip3_amd.save_packed(path, packed, {"step": 1})
    loaded = bzip3_amd.load_packed(path, "cuda:0")
    assert list(loaded) == list(sd)
    for k, p in loaded.items():
        q = packed[k]
        assert p.frame.device == q.frame.device and _host(p.frame) == _host(q.frame), k
        assert (p.dtype, tuple(p.shape), p.planes, p.block_size, p.nbytes, p.delta, p.base_crc, p.crc) == (q.dtype, tuple(q.shape), q.planes, q.block_size, q.nbytes, q.delta, q.base_crc, q.crc)
    back = bzip3_amd.unpack_state_dict(loaded, verify=True)
    for k, x in sd.items():
        assert back[k].dtype == x.dtype and back[k].shape == x.shape and _raw(back[k]) == _raw(x), k
    # frames saved from the CPU give the same file
    on_cpu = {k: bzip3_amd.PackedTensor(p.frame.cpu(), p.dtype, p.shape, p.planes, p.block_size, p.nbytes, p.delta, p.base_crc, p.crc) for k, p in packed.items()}
    bzip3_amd.save_packed(path + ".cpu", on_cpu, {"step": 1})
    assert open(path, "rb").read() == open(path + ".cpu", "rb").read()
    # a subset of the file, and rows of it
    some = bzip3_amd.load_packed(path, "cuda:0", names=["int64", "float32"])
    rows = bzip3_amd.unpack_state_dict(some, rows={"float32": (3, 20)})
    assert list(rows) == ["int64", "float32"]
    assert _raw(rows["float32"]) == _raw(sd["float32"][3:20]) and _raw(rows["int64"]) == _raw(sd["int64"])


def test_chain_of_three_checkpoints(gpu_lib, tmp_path):
    import torch

    sd0 = _state_dict(6, 40)
    sd1 = _step(sd0, 41)
    fresh = _state_dict(6, 44)
    sd1["t2"] = fresh["t2"]  # replaced whole
    sd2 = _step(sd1, 42)
    sd2["t4"] = fresh["t4"]
    steps = [bzip3_amd.pack_state_dict(sd0, BS),
             bzip3_amd.pack_state_dict(sd1, BS, base={k: v for k, v in sd0.items() if k != "t2"}),
             bzip3_amd.pack_state_dict(sd2, BS, base={k: v for k, v in sd1.items() if k != "t4"})]
    assert [sum(p.delta for p in s.values()) for s in steps] == [0, 5, 5]
    loaded = []
    for t, s in enumerate(steps):
        path = str(tmp_path / f"step{t}.bz3t")
        bzip3_amd.save_packed(path, s, {"step": t})
        loaded.append(bzip3_amd.load_packed(path, "cuda:0"))
    assert bzip3_amd.check_chain(loaded) == []
    got = bzip3_amd.unpack_chain(loaded)
    assert list(got) == list(sd2) and all(_raw(got[k]) == _raw(sd2[k]) for k in sd2)
    # step 1 swapped for a delta against other data: the chain breaks at its first link, before any decode
    broken = [loaded[0], bzip3_amd.pack_state_dict(sd1, BS, base=_step(sd0, 43)), loaded[2]]
    cm = gpu_lib.bz3_hip_debug_cm_launches(0)
    with pytest.raises(ValueError, match="step 1"):
        bzip3_amd.unpack_chain(broken)
    assert gpu_lib.bz3_hip_debug_cm_launches(0) == cm, "a frame was decoded before the chain was checked"
