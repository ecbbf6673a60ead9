"""-m gpu: the LZP encoder cases of tests/lzp_cases.py on the device -- the oracle's bytes and the driver's record from one stage call per
case, all of them as one batch (several driver workgroups in one launch, emission beside the other blocks' drivers), and the decoder's
targeted test, whose atomics run concurrently only here.  tests/test_lzp_cases.py holds the preconditions of the cases."""
import ctypes as C

import pytest

import bzip3_amd
import lzp_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return L.stage_cases()


@pytest.fixture(scope="module")
def batch(oracle, cases):
    """(block size, [(name, data, the oracle's block)]) -- computed once for both kinds of state."""
    bs = max(65 * 1024, max(len(d) for d in cases.values()))
    out = []
    for name in L.STAGE_NAMES:
        n, err, blk = oracle.encode_block(cases[name], bs)
        assert n > 0 and err == 0 and blk[8] & 2, name  # LZP applied (model & 2)
        out.append((name, cases[name], blk))
    return bs, out


@pytest.mark.parametrize("name", L.STAGE_NAMES)
def test_encoder_bytes_and_driver_record(gpu_lib, oracle, cases, name):
    L.check_encoder(bzip3_amd.StageApi(gpu_lib), oracle, name, cases[name])


def test_encoder_on_the_ends(gpu_lib, oracle):
    g = bzip3_amd.StageApi(gpu_lib)
    for name, d in L.ends().items():
        L.check_encoder(g, oracle, name, d)


@pytest.mark.parametrize("lean", [0, 1], ids=["classic", "lean"])
def test_all_cases_as_one_batch(gpu_lib, batch, lean):
    bs, blocks = batch
    n = len(blocks)
    try:
        assert gpu_lib.bz3_hip_set_lean_states(lean) == 0
        states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
        assert all(states)
        cap = gpu_lib.bz3_bound(bs) + 64
        bufs = [(C.c_uint8 * cap)() for _ in range(n)]
        for b, (_, d, _) in zip(bufs, blocks):
            C.memmove(b, d, len(d))
        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        sizes = (C.c_int32 * n)(*[len(d) for _, d, _ in blocks])
        gpu_lib.bz3_encode_blocks(states, ptrs, sizes, n)
        for k, (name, _, want) in enumerate(blocks):
            assert gpu_lib.bz3_last_error(states[k]) == 0, name
            assert bytes(bufs[k][: sizes[k]]) == want, name
        bsz = (C.c_size_t * n)(*[cap] * n)
        orig = (C.c_int32 * n)(*[len(d) for _, d, _ in blocks])
        gpu_lib.bz3_decode_blocks(states, ptrs, bsz, sizes, orig, n)
        for k, (name, d, _) in enumerate(blocks):
            assert gpu_lib.bz3_last_error(states[k]) == 0 and bytes(bufs[k][: len(d)]) == d, name
        for st in states:
            gpu_lib.bz3_free(st)
    finally:
        gpu_lib.bz3_hip_set_lean_states(0)


def test_lzp_decoder_chunks_alignments_and_caps_on_gpu(gpu_lib, oracle):
    """lzp_cases.check_decoder on the device: the atomicMax inserts of the bulk literals and the atomicExch at every sequencing point run
    concurrently only here (the emulator runs lanes one after the other)."""
    L.check_decoder(bzip3_amd.StageApi(gpu_lib), oracle)
