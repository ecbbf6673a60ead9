"""GPU tests of the batched forward BWT (bzip3_amd/csrc/bwt.hip bwt_forward_batch; the encoder's front end sends the blocks of a window through it
in runs of up to four).  The smallest shapes at which it can go wrong: jobs that take different paths of the sorter under one grid (done after pass 0,
one more window, rank doubling from a list overflow, from big rounds and from the tail kernel's give-up), jobs of unequal extent on the same path,
a run shorter than the job table, and blocks that leave a window before its runs (stored, failed)."""
import ctypes as C

import pytest

import bzip3_amd
import datagen
from test_gpu_unbwt_batch import SIZES

pytestmark = pytest.mark.gpu

MIXED = ("phrase3", "tile513", "aaaa", "phrase1")
MIXED2 = ("deeprep", "n2", "mixdeep", "group257")


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (bytes, oracle.bwt of them): once for the module."""
    c = datagen.suffix_sorter_cases()
    return {k: (c[k], oracle.bwt(c[k])) for k in MIXED + MIXED2}


@pytest.fixture(scope="module")
def text_3mib():
    return datagen.text(3 << 20, seed=41)


@pytest.mark.parametrize("names", (MIXED, MIXED2, MIXED[::-1]), ids=("mixed", "mixed2", "mixed reversed"))
def test_jobs_that_diverge_in_one_run(gpu_lib, cases, names):
    rc, got = bzip3_amd.StageApi(gpu_lib).bwt_many([cases[k][0] for k in names])
    assert rc == 0
    for k, r in zip(names, got):
        assert r == cases[k][1], k


def test_unequal_extents_on_one_path(gpu_lib, oracle, text_3mib):
    """Four text blocks of 300,000 bytes and one of 1,000: a run of four and a run of one; then the small one inside the run."""
    blocks = [text_3mib[k * 400000 :][:300000] for k in range(4)] + [text_3mib[5000:6000]]
    want = [oracle.bwt(b) for b in blocks]
    g = bzip3_amd.StageApi(gpu_lib)
    assert g.bwt_many(blocks) == (0, want)
    assert g.bwt_many(blocks[2:] + blocks[:1]) == (0, want[2:] + want[:1])


STORED, OVERSIZE, CHECKED = 3, 7, (0, 5, 11)


@pytest.mark.parametrize("lean", (0, 1))
def test_ten_blocks_and_two_that_leave_early(gpu_lib, oracle, text_3mib, lean):
    """Ten blocks of 70 KB to 2 MiB encoded in device memory, with a block of 40 bytes (stored) and one larger than its state's block size (it fails
    alone) among them: the oracle decides the coded bytes of the first, a middle and the last block, and all ten decode back to their input."""
    import torch

    bs = 2 << 20
    blocks = [text_3mib[(i * 104729) % ((3 << 20) - n) :][:n] for i, n in enumerate(SIZES)]
    blocks.insert(STORED, b"y" * 40)
    blocks.insert(OVERSIZE, text_3mib[: bs + 1])
    n = len(blocks)
    assert n == 12 and len(blocks[CHECKED[1]]) == SIZES[4] and blocks[CHECKED[2]] == blocks[-1]
    cap = gpu_lib.bz3_bound(bs + 1) + 64
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
        for i in range(n):
            if i == OVERSIZE:
                assert sizes[i] == -1 and gpu_lib.bz3_last_error(states[i]) == bzip3_amd.BZ3_ERR_DATA_TOO_BIG
            else:
                assert sizes[i] > 0 and gpu_lib.bz3_last_error(states[i]) == 0, i
        assert sizes[STORED] == 48
        for i in CHECKED:
            assert (sizes[i], 0, bytes(bufs[i][: sizes[i]].cpu().numpy())) == oracle.encode_block(blocks[i], bs), i
        keep = [i for i in range(n) if i != OVERSIZE]
        m = len(keep)
        st2 = (C.c_void_p * m)(*[states[i] for i in keep])
        p2 = (C.c_void_p * m)(*[ptrs[i] for i in keep])
        bsz = (C.c_size_t * m)(*[cap] * m)
        coded = (C.c_int32 * m)(*[sizes[i] for i in keep])
        orig = (C.c_int32 * m)(*[len(blocks[i]) for i in keep])
        gpu_lib.bz3_hip_decode_blocks_device(st2, p2, bsz, coded, orig, m)
        for i in keep:
            assert gpu_lib.bz3_last_error(states[i]) == 0 and bytes(bufs[i][: len(blocks[i])].cpu().numpy()) == blocks[i], i
    finally:
        for s in states:
            gpu_lib.bz3_free(s)
        gpu_lib.bz3_hip_set_lean_states(0)
        gpu_lib.bz3_hip_bind_device(-1)
        gpu_lib.bz3_hip_release_cached_memory()
