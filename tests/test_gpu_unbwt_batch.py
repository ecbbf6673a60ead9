"""GPU tests of the batched inverse BWT (bzip3_amd/csrc/unbwt.hip bwt_inverse_batch; the decoder's tail sends the blocks of a window through it in
runs of up to four).  The smallest shapes at which it can go wrong: jobs of unequal extent under one grid, a run shorter than the job table, a block
that fails in the middle of a run, and both stride regimes (every row a splitter below 2^17 rows, hashed splitters above) in one run."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
import datagen
from test_gpu_unbwt_strides import _cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def text_3mib():
    return datagen.text(3 << 20, seed=41)  # (seconds to generate: once for the module)


@pytest.fixture(scope="module")
def four_jobs(oracle, text_3mib):
    """The three 300,000-byte cases of test_gpu_unbwt_strides.py (text, wrong index, junk) and a text of 1,000 bytes: (name, bytes, index, expected)."""
    small = text_3mib[5000:6000]
    idx, u = oracle.bwt(small)
    want = oracle.unbwt(u, idx)
    assert want == (0, small)
    return _cases(oracle, text_3mib[1000000:1300000], 31) + [("text 1000", u, idx, want)]


@pytest.mark.parametrize("log_stride", (-1, 3, 8))
def test_four_jobs_in_one_run(gpu_lib, four_jobs, log_stride):
    g = bzip3_amd.StageApi(gpu_lib)
    gpu_lib.bz3_hip_debug_set_unbwt_log_stride(log_stride)
    try:
        rc, got = g.unbwt_many([(u, idx) for _, u, idx, _ in four_jobs])
        assert rc == 0
        for (name, _, _, want), b in zip(four_jobs, got):
            assert (0, b) == want, (name, log_stride)
    finally:
        gpu_lib.bz3_hip_debug_set_unbwt_log_stride(-1)


SIZES = (70000, 2 << 20, 300000, 1 << 20, (1 << 17) + 5, 500000, 2 << 20, 140000, 1500000, 70 * 1024)
BAD_INDEX, BAD_PAYLOAD, CHECKED = 4, 5, (0, 2)  # 128 KiB + 5 with a header index beyond its size; 500,000 with a flipped payload byte; 70,000 and 300,000


@pytest.mark.parametrize("lean", (0, 1))
def test_ragged_runs_with_a_failed_block_and_a_corrupted_one(gpu_lib, oracle, text_3mib, lean):
    """Ten blocks of 70 KB to 2 MiB, encoded and decoded in device memory: one window, runs of at most four.  Block 4's header index is raised beyond
    its size (BZ3_ERR_MALFORMED_HEADER in front of the inverse BWT: it drops out of its run); block 5's payload is corrupted, so its walk meets foreign
    cycles beside genuine jobs.  The oracle decides the error codes of the two damaged blocks, and sizes, codes and bytes of two others; the rest must be their own
    input.  What a FAILED block leaves in its buffer is not defined by the API, so the damaged blocks are held to their error code alone: this test shows
    that they do not disturb their neighbours, and the bytes a walk writes on input that is no genuine BWT are pinned by test_four_jobs_in_one_run (junk
    and wrong index against oracle.unbwt)."""
    import torch

    bs = 2 << 20
    blocks = [text_3mib[(i * 104729) % ((3 << 20) - n) :][:n] for i, n in enumerate(SIZES)]
    n = len(blocks)
    cap = gpu_lib.bz3_bound(bs) + 64
    dev = torch.device("cuda", 0)
    gpu_lib.bz3_hip_bind_device(0)
    assert gpu_lib.bz3_hip_set_lean_states(lean) == 0
    states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
    try:
        assert all(states)
        bufs = [torch.zeros(cap, dtype=torch.uint8, device=dev) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[b.data_ptr() for b in bufs])
        for b, d in zip(bufs, blocks):
            b[: len(d)] = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev)
        torch.cuda.synchronize()
        sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
        gpu_lib.bz3_hip_encode_blocks_device(states, ptrs, sizes, n)
        assert all(sizes[i] > 0 and gpu_lib.bz3_last_error(states[i]) == 0 for i in range(n))
        bufs[BAD_PAYLOAD][sizes[BAD_PAYLOAD] // 2] ^= 0x41
        wrong = torch.frombuffer(bytearray(int(len(blocks[BAD_INDEX]) + 1000).to_bytes(4, "little")), dtype=torch.uint8).to(dev)
        bufs[BAD_INDEX][4:8] = wrong  # the header's BWT index (bytes 4..7)
        torch.cuda.synchronize()
        looked_at = sorted(set(CHECKED) | {BAD_INDEX, BAD_PAYLOAD})
        coded = {i: bytes(bufs[i][: sizes[i]].cpu().numpy()) for i in looked_at}
        want = {i: oracle.decode_block(c, len(blocks[i]), bs) for i, c in coded.items()}
        assert want[BAD_INDEX][1] == bzip3_amd.BZ3_ERR_MALFORMED_HEADER and want[BAD_PAYLOAD][1] != 0
        assert all(want[i] == (len(blocks[i]), 0, blocks[i]) for i in CHECKED)
        bsz = (C.c_size_t * n)(*[cap] * n)
        orig = (C.c_int32 * n)(*[len(d) for d in blocks])
        gpu_lib.bz3_hip_decode_blocks_device(states, ptrs, bsz, sizes, orig, n)
        for i, d in enumerate(blocks):
            err = gpu_lib.bz3_last_error(states[i])
            if i in (BAD_INDEX, BAD_PAYLOAD):
                assert err == want[i][1], (i, err)
            else:
                assert err == 0 and bytes(bufs[i][: len(d)].cpu().numpy()) == d, (i, err)
    finally:
        for s in states:
            gpu_lib.bz3_free(s)
        gpu_lib.bz3_hip_set_lean_states(0)
        gpu_lib.bz3_hip_bind_device(-1)
        gpu_lib.bz3_hip_release_cached_memory()
