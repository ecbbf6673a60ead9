"""-m gpu: the row-cache CM kernels with two and three workgroups on a CU, chosen by the automatic policy.

bench.py's 768 blocks per GPU are the only way the product reaches k_cm_encode_rows / k_cm_encode_rows3 and k_cm_decode_sync2 / k_cm_decode_sync3 (cm.hip):
cm_variant_for (api_internal.hpp) takes them when a batch has more CM jobs than the device has CUs, the three-per-CU pair above twice that.  The other -m gpu
tests force a variant with 4 to 9 blocks (every block has a CU to itself, and forcing switches the routing off) or stay at 140 blocks and below.  Here the
batches are as large as the policy asks: the SIMD claim of the encoders (HW_ID / XCC_ID, atomicOr on a word per CU, the swapped role when wave 0's SIMD is
taken, the release when more workgroups are launched than fit at once), the per-job spill areas and status words while neighbours share a CU's LDS, SIMDs and
barriers, routing and hand-back at the real CU count together with the CU partition and the tail rings of batches of 128 and more.  BZ3_HIP_CUS is NOT set:
real sharing of a CU is the point.  Inputs and expected counters: tests/cm_batch_cases.py (its preconditions are checked without a GPU by
tests/test_cm_batch_cases.py); expected bytes: the real reference (oracle/_ref) -- a run without it fails, it does not skip."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
import cm_batch_cases as cases

pytestmark = pytest.mark.gpu
_cache = {}


def _thresholds(lib):
    if "c" not in _cache:
        _cache["c"] = cases.thresholds(lib)
    return _cache["c"]


def _stage_input(oracle):
    """~48 KiB of BWT output of restricted-alphabet text (at most 37 byte values: no row cache ever evicts a row of it) and its coded bytes: one oracle call per
    direction, shared by the five cases."""
    if "stage" not in _cache:
        u = oracle.bwt(cases.restricted_text(48 * 1024 + 77, seed=9))[1]
        _cache["stage"] = (u, oracle.cm_encode(u))
    return _cache["stage"]


COPIES = {"c1-1": lambda c1, c2: c1 - 1, "c1": lambda c1, c2: c1, "c2-1": lambda c1, c2: c2 - 1, "c2": lambda c1, c2: c2,
          "3(c1-1)+40": lambda c1, c2: 3 * (c1 - 1) + 40}
VARIANT = {"c1-1": 0, "c1": 1, "c2-1": 1, "c2": 2, "3(c1-1)+40": 2}


@pytest.mark.parametrize("which", list(COPIES))
def test_each_variant_alone_through_the_stage_hooks(gpu_lib, oracle, monkeypatch, which):
    """`copies` identical CM jobs in ONE launch of the variant the automatic policy picks for that many (bz3_hip_stage_cm_encode_many / _decode_many; no
    hand-back, so this is the variant itself): one block per CU, the first batch with two on a CU, the last with two, the first with three, and more
    workgroups than fit at once.  Every copy must agree with copy 0 (BZ3_CM_MANY_CHECK: -2 otherwise) and copy 0 with the oracle."""
    monkeypatch.setenv("BZ3_CM_MANY_CHECK", "1")
    try:
        assert gpu_lib.bz3_hip_bind_device(0) == 0 and gpu_lib.bz3_hip_set_cm_mode(-1) == 0
        c1, c2 = _thresholds(gpu_lib)
        copies = COPIES[which](c1, c2)
        plain, coded = _stage_input(oracle)
        for e in (0, 1):
            assert gpu_lib.bz3_hip_cm_variant_for(0, copies, e) == VARIANT[which], (copies, e)
        out = (C.c_uint8 * (gpu_lib.bz3_bound(len(plain)) + 64))()
        got = C.c_int32(0)
        ms = gpu_lib.bz3_hip_stage_cm_encode_many(bzip3_amd._cbuf(plain, len(plain)), len(plain), out, C.byref(got), copies)
        assert ms >= 0, (copies, ms)
        assert got.value == len(coded) and C.string_at(out, got.value) == coded, copies
        back = (C.c_uint8 * len(plain))()
        ms = gpu_lib.bz3_hip_stage_cm_decode_many(bzip3_amd._cbuf(coded, len(coded)), len(coded), back, len(plain), copies, None)
        assert ms >= 0, (copies, ms)
        assert bytes(back) == plain, copies
    finally:
        gpu_lib.bz3_hip_bind_device(-1)


def _batch(lib, oracle, size):
    """The batch of one size with the reference's coded blocks: built once, shared by the two state kinds, never modified."""
    from oracle_lib import Bz3, require_ref

    c1, c2 = _thresholds(lib)
    if size not in _cache:
        ref = Bz3(require_ref().lib)
        _cache[size] = cases.build_batch(cases.batch_sizes(c1, c2)[size], c1, lambda d, bs: ref.encode_block(d, bs)[2], oracle)
    return _cache[size], c1


@pytest.mark.parametrize("states_kind", ["classic_host", "lean_device"])
@pytest.mark.parametrize("size", ["two_per_cu", "three_per_cu", "oversubscribed"])
def test_distinct_blocks_through_the_batch_path_under_the_automatic_policy(gpu_lib, oracle, size, states_kind):
    """c1 + 43, c2 + 39 and 3 (c1 - 1) + 40 CM jobs (~300 / 552 / 808 on MI355X), every block distinct, lengths 4 .. 96 KiB, through bz3_encode_blocks /
    bz3_decode_blocks with classic states and through the device entry points with lean states and the workspace kept (bench.py's configuration), mode auto,
    twice on the same states: every coded block equals the real reference's, every decode gives the plaintext back; on the second trip one bit of one
    fitting block's payload is flipped and that block alone reports the oracle's error.  Counters around each call, every expectation derived in
    cm_batch_cases from the library's rules and the reference's blocks: the routed count exactly, at least the two 128-value blocks handed back by the
    decoder, at most the blocks that are neither fitting nor routed handed back in either direction (so the row-cache kernels finished at least 60 % of the
    batch), two CM launches per direction."""
    import torch

    b, c1 = _batch(gpu_lib, oracle, size)
    b.check_distinct(c1 - 1)
    assert len(b.fitting) * 10 >= b.n_jobs * 6
    lean = states_kind == "lean_device"
    want_variant = 1 if size == "two_per_cu" else 2
    n, bs = b.n, cases.BLOCK_SIZE
    cap = gpu_lib.bz3_bound(bs) + 64
    stride = (cap + 255) & ~255
    flip, flip_at = b.flip_target(c1)
    host = np.zeros((n, stride), dtype=np.uint8)
    states = None
    try:
        assert gpu_lib.bz3_hip_bind_device(0) == 0 and gpu_lib.bz3_hip_set_cm_mode(-1) == 0
        assert gpu_lib.bz3_hip_set_lean_states(1 if lean else 0) == 0
        if lean:
            assert gpu_lib.bz3_hip_set_keep_workspace(1) == 0
            dev = torch.zeros((n, stride), dtype=torch.uint8, device="cuda:0")
            base = dev.data_ptr()
        else:
            base = host.ctypes.data
        states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
        assert all(states)
        ptrs = (C.c_void_p * n)(*[base + i * stride for i in range(n)])
        for e in (0, 1):
            assert gpu_lib.bz3_hip_cm_variant_for(0, b.n_jobs, e) == want_variant
        # (the routed blocks leave the row-cache launch: what is left must still take the same variant)
        assert gpu_lib.bz3_hip_cm_variant_for(0, b.n_jobs - len(b.routed_encode), 1) == want_variant
        assert gpu_lib.bz3_hip_cm_variant_for(0, b.n_jobs - len(b.routed_decode), 0) == want_variant

        def counters():
            return gpu_lib.bz3_hip_cm_blocks_given_up(), gpu_lib.bz3_hip_cm_blocks_routed_full(), gpu_lib.bz3_hip_debug_cm_launches(0)

        for trip in range(2):
            host[:] = 0
            for i, d in enumerate(b.blocks):
                host[i, : len(d)] = np.frombuffer(d, dtype=np.uint8)
            sizes = (C.c_int32 * n)(*[len(d) for d in b.blocks])
            k0 = counters()
            if lean:
                dev.copy_(torch.from_numpy(host))
                torch.cuda.synchronize()
                gpu_lib.bz3_hip_encode_blocks_device(states, ptrs, sizes, n)
                host[:] = dev.cpu().numpy()
            else:
                gpu_lib.bz3_encode_blocks(states, ptrs, sizes, n)
            k1 = counters()
            given, routed, launches = (k1[j] - k0[j] for j in range(3))
            print("%s %s trip %d encode: %d jobs, %d routed, %d given up (at most %d), %d CM launches"
                  % (size, states_kind, trip, b.n_jobs, routed, given, b.given_up_cap(len(b.routed_encode)), launches))
            for i in range(n):
                assert sizes[i] == len(b.want[i]) and host[i, : sizes[i]].tobytes() == b.want[i], (trip, i, b.kinds[i])
                assert len(b.blocks[i]) < 64 or gpu_lib.bz3_last_error(states[i]) == 0, (trip, i)
            assert routed == len(b.routed_encode), (trip, routed, b.routed_encode)
            assert 0 <= given <= b.given_up_cap(len(b.routed_encode)), (trip, given)
            assert launches == 2, (trip, launches)
            corrupt = trip == 1
            if corrupt:
                host[flip, flip_at] ^= 0x10
                if lean:
                    dev[flip, flip_at] ^= 0x10
                    torch.cuda.synchronize()
                mutant = host[flip, : sizes[flip]].tobytes()
                want_err = oracle.decode_block(mutant, len(b.blocks[flip]), bs)[1]
                assert want_err != 0
            bsz = (C.c_size_t * n)(*[cap] * n)
            orig = (C.c_int32 * n)(*[len(d) for d in b.blocks])
            if lean:
                gpu_lib.bz3_hip_decode_blocks_device(states, ptrs, bsz, sizes, orig, n)
                host[:] = dev.cpu().numpy()
            else:
                gpu_lib.bz3_decode_blocks(states, ptrs, bsz, sizes, orig, n)
            k2 = counters()
            given, routed, launches = (k2[j] - k1[j] for j in range(3))
            # (a corrupted payload decodes to arbitrary bytes: that one block is no fitting block any more and may be handed back too)
            cap_dec = b.given_up_cap(len(b.routed_decode)) + (1 if corrupt else 0)
            print("%s %s trip %d decode: %d jobs, %d routed, %d given up (at least 2, at most %d), %d CM launches"
                  % (size, states_kind, trip, b.n_jobs, routed, given, cap_dec, launches))
            for i, d in enumerate(b.blocks):
                if corrupt and i == flip:
                    assert gpu_lib.bz3_last_error(states[i]) == want_err, (gpu_lib.bz3_last_error(states[i]), want_err)
                else:
                    assert gpu_lib.bz3_last_error(states[i]) == 0 and host[i, : len(d)].tobytes() == d, (trip, i, b.kinds[i])
            assert routed == len(b.routed_decode), (trip, routed, b.routed_decode)
            assert 2 <= given <= cap_dec, (trip, given)
            assert launches == 2, (trip, launches)
    finally:
        if states is not None:
            for s_ in states:
                if s_:
                    gpu_lib.bz3_free(s_)
        gpu_lib.bz3_hip_set_keep_workspace(-1)
        gpu_lib.bz3_hip_set_lean_states(0)
        gpu_lib.bz3_hip_bind_device(-1)
        gpu_lib.bz3_hip_release_cached_memory()
