"""GPU tests of the inverse BWT (bzip3_amd/csrc/unbwt.hip): forced splitter strides and the rule through the stage hook, and the decoder's tail
with nothing waiting for the stream between the inverse BWTs of a window -- their scratch is reused in stream order, which the emulator's
synchronous streams cannot show -- on the plain stream (a batch of 24) and on the CU partition's masked stream (a batch of 128)."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
import datagen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def text_3mib():
    return datagen.text(3 << 20, seed=41)  # (seconds to generate: once for the module)


def _cases(oracle, text, seed, bwt=None):
    """bwt: who transforms the text (the oracle; its sorter needs seconds for 3 MiB, so the larger case passes the GPU's forward transform, pinned
    elsewhere) -- the expected bytes are oracle.unbwt's either way."""
    rng = np.random.default_rng(seed)
    n = len(text)
    idx, u = (bwt or oracle.bwt)(text)
    wrong = idx // 2 + 1 if idx // 2 + 1 != idx else idx // 2 + 2
    junk = bytes(rng.integers(0, 5, size=n, dtype=np.uint8))
    cases = [("text", u, idx), ("text, wrong index", u, wrong), ("junk", junk, int(rng.integers(1, n + 1)))]
    out = [(name, b, i, oracle.unbwt(b, i)) for name, b, i in cases]
    assert out[0][3] == (0, text)
    return out


@pytest.fixture(scope="module")
def cases_300k(oracle, text_3mib):
    return _cases(oracle, text_3mib[1000000:1300000], 31)


@pytest.mark.parametrize("log_stride", (0, 3, 5, 8, -1))
def test_forced_strides_and_the_rule(gpu_lib, cases_300k, log_stride):
    g = bzip3_amd.StageApi(gpu_lib)
    gpu_lib.bz3_hip_debug_set_unbwt_log_stride(log_stride)
    try:
        for name, u, idx, want in cases_300k:
            assert g.unbwt(u, idx) == want, (name, log_stride)
    finally:
        gpu_lib.bz3_hip_debug_set_unbwt_log_stride(-1)


def test_the_rule_at_3_mib(gpu_lib, oracle, text_3mib):
    g = bzip3_amd.StageApi(gpu_lib)
    gpu_lib.bz3_hip_debug_set_unbwt_log_stride(-1)
    for name, u, idx, want in _cases(oracle, text_3mib, 32, bwt=g.bwt):
        assert g.unbwt(u, idx) == want, name


def _round_trips(gpu_lib, oracle, blocks, bs, corrupt, checked):
    """Encode and decode `blocks` in device memory twice on fresh states.  The oracle decodes the coded blocks listed in `checked` and the corrupted
    one (its decoder runs at 3 MB/s: a few blocks of every kind, not the whole batch) and decides their sizes, error codes and plaintext; every other
    block must come back as its own input with error 0, which is what the oracle returns for any stream it accepts."""
    import torch

    n = len(blocks)
    cap = gpu_lib.bz3_bound(bs) + 64
    dev = torch.device("cuda", 0)
    gpu_lib.bz3_hip_bind_device(0)
    states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
    assert all(states)
    want = {}
    try:
        bufs = [torch.zeros(cap, dtype=torch.uint8, device=dev) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[b.data_ptr() for b in bufs])
        for trip in range(2):
            for b, d in zip(bufs, blocks):
                if len(d):
                    b[: len(d)] = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev)
            torch.cuda.synchronize()
            sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
            gpu_lib.bz3_hip_encode_blocks_device(states, ptrs, sizes, n)
            assert all(sizes[i] > 0 and gpu_lib.bz3_last_error(states[i]) == 0 for i in range(n)), trip
            where = sizes[corrupt] // 2
            bufs[corrupt][where] ^= 0x41
            torch.cuda.synchronize()
            if trip == 0:  # (the second trip codes the same bytes: asserted below)
                coded = {i: bytes(bufs[i][: sizes[i]].cpu().numpy()) for i in sorted(set(checked) | {corrupt})}
                want = {i: oracle.decode_block(c, len(blocks[i]), bs) for i, c in coded.items()}
                assert want[corrupt][1] != 0 and all(want[i][:2] == (len(blocks[i]), 0) and want[i][2] == blocks[i] for i in checked)
            else:
                assert all(bytes(bufs[i][: sizes[i]].cpu().numpy()) == c for i, c in coded.items())
            bsz = (C.c_size_t * n)(*[cap] * n)
            orig = (C.c_int32 * n)(*[len(d) for d in blocks])
            gpu_lib.bz3_hip_decode_blocks_device(states, ptrs, bsz, sizes, orig, n)
            for i, d in enumerate(blocks):
                err = gpu_lib.bz3_last_error(states[i])
                if i == corrupt:
                    assert err == want[i][1], (trip, i, err)
                else:
                    assert err == 0 and bytes(bufs[i][: len(d)].cpu().numpy()) == d, (trip, i, err)
    finally:
        for s in states:
            gpu_lib.bz3_free(s)
        gpu_lib.bz3_hip_bind_device(-1)
        gpu_lib.bz3_hip_release_cached_memory()


def test_stream_order_reuse_of_scratch(gpu_lib, oracle, text_3mib):
    """24 blocks of 1 MiB, 70 KiB and 3 MiB in turn (every inverse BWT takes the bytes its predecessor's kernels may still be using), two stored
    blocks of fewer than 64 bytes and one corrupted payload among them."""
    bs = 3 << 20
    big = text_3mib
    blocks = []
    for i in range(24):
        size = ((1 << 20), 70 * 1024, (3 << 20))[i % 3]
        o = (i * 104729) % ((3 << 20) - size + 1)
        blocks.append(big[o : o + size] if i % 3 != 2 else big[o:] + big[:o])
    blocks[5] = b"stored: 23 bytes of it."
    blocks[16] = b"x" * 63
    _round_trips(gpu_lib, oracle, blocks, bs, corrupt=10, checked=(3, 4, 5, 16, 20))  # 1 MiB corrupted; 1 MiB, 70 KiB, the stored ones, 3 MiB


def test_masked_stream_tail(gpu_lib, oracle, text_3mib):
    """128 blocks of 128 KiB: the decoder's tail takes the CU partition (batches of 128 or more), where the inverse BWT's lane target is that of
    the CUs left to the masked stream."""
    bs = 128 * 1024
    blocks = [text_3mib[(i * 24007) % ((3 << 20) - bs) :][:bs] for i in range(128)]
    _round_trips(gpu_lib, oracle, blocks, bs, corrupt=77, checked=(0, 31, 64, 127))
