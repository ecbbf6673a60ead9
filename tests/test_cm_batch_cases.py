"""The preconditions of tests/test_gpu_cm_batches.py, checked without a GPU: what tests/cm_batch_cases.py generates for the largest batch (3 * 256 + 40 CM jobs,
the thresholds of a 256-CU device) has the properties its expected counters are derived from."""
import numpy as np
import pytest

import cm_batch_cases as cases

C1, C2 = 257, 513  # bz3_hip_cm_variant_for on MI355X (256 CUs): the GPU test scans the library for them


@pytest.fixture(scope="module")
def batch(ref_lib, oracle):
    n_jobs = cases.batch_sizes(C1, C2)["oversubscribed"]
    assert n_jobs == 808
    return cases.build_batch(n_jobs, C1, lambda d, bs: ref_lib.encode_block(d, bs)[2], oracle)


def test_batch_sizes_follow_the_thresholds():
    assert cases.batch_sizes(C1, C2) == {"two_per_cu": 300, "three_per_cu": 552, "oversubscribed": 808}
    assert C2 - 1 == 2 * (C1 - 1)


def test_fitting_blocks_fit_every_row_cache(batch):
    """At most 40 distinct byte values and model byte 0 (the CM input is a permutation of the block): at most 40 first touches, no eviction from a cache of
    44 rows or more, nothing outside the 40 most frequent values.  At least 60 % of the CM jobs are such blocks."""
    assert batch.n_jobs == 808 and batch.n == 810
    assert len(batch.fitting) * 10 >= batch.n_jobs * 6
    seen = set()
    for i in batch.fitting:
        d = batch.blocks[i]
        assert cases.MIN_LEN <= len(d) <= cases.MAX_LEN
        values = np.unique(np.frombuffer(d, dtype=np.uint8))
        assert len(values) <= cases.ROUTE_KEEP, (i, len(values))
        assert batch.want[i][8] == 0, i
        assert cases.outside_top(d) == 0
        seen.add(int(values.max()) >> 7)
    assert seen == {0, 1}  # rows below and above byte value 128
    assert not set(batch.fitting) & (set(batch.routed_encode) | set(batch.routed_decode))
    lens = sorted(len(batch.blocks[i]) for i in batch.jobs)
    assert lens[0] < 6 * 1024 and lens[-1] > 90 * 1024 and lens[-1] <= cases.MAX_LEN  # workgroups end at very different times


def test_specials_meet_their_size_conditions(batch, oracle):
    kinds = batch.kinds
    rand = [i for i in batch.jobs if kinds[i] == "rand"]
    v128 = [i for i in batch.jobs if kinds[i] == "v128"]
    assert len(rand) == 4 and len(v128) == 2
    for i in rand:  # routed in both directions
        assert i in batch.routed_encode and i in batch.routed_decode
    for i in v128:
        d = batch.blocks[i]
        model, before, payload, _ = cases.parse_header(batch.want[i])
        assert model == 0 and len(np.unique(np.frombuffer(d, dtype=np.uint8))) == 128
        assert cases.outside_top(d) * 4 > 2 * len(d)   # ~88 / 128 of the bytes lie outside the top 40: routed on encode
        assert i in batch.routed_encode
        assert payload * 10 < len(d) * 9                # shrinks by more than a tenth: the decoder does not route it ...
        assert i not in batch.routed_decode
        assert len(d) >= 32768                          # ... and 128 live rows in a cache of 96 or 56 miss far more often than 1024 + n / 32 times
    stored = [i for i in range(batch.n) if kinds[i] == "stored"]
    empty = [i for i in range(batch.n) if kinds[i] == "empty"]
    assert [len(batch.blocks[i]) for i in stored + empty] == [41, 0]
    assert all(cases.parse_header(batch.want[i])[0] == -1 for i in stored + empty)
    assert len(batch.jobs) == batch.n - 2 and not set(stored + empty) & set(batch.jobs)


def test_routing_counts_are_the_specials_plus_ordinary_blocks_that_meet_the_rule(batch):
    kinds = batch.kinds
    special_enc = [i for i in batch.jobs if kinds[i] in ("rand", "v128")]
    special_dec = [i for i in batch.jobs if kinds[i] == "rand"]
    extra_enc = [i for i in batch.routed_encode if i not in special_enc]
    extra_dec = [i for i in batch.routed_decode if i not in special_dec]
    assert all(kinds[i] == "ord" for i in extra_enc + extra_dec)
    assert len(batch.routed_encode) == 6 + len(extra_enc) and len(batch.routed_decode) == 4 + len(extra_dec)
    # what is left after routing still takes the three-per-CU kernels, and more workgroups than fit at once
    assert batch.n_jobs - len(batch.routed_encode) > 3 * (C1 - 1) and batch.n_jobs - len(batch.routed_decode) > 3 * (C1 - 1)
    assert batch.given_up_cap(len(batch.routed_decode)) >= 2
    models = [batch.want[i][8] for i in batch.jobs if kinds[i] == "ord"]
    assert any(m & 2 for m in models) and any(m & 4 for m in models)  # LZP and mRLE both applied somewhere


def test_blocks_that_may_share_a_cu_differ(batch):
    batch.check_distinct(C1 - 1)


def test_the_flipped_block_is_a_late_fitting_block_the_oracle_refuses(batch, oracle):
    i, at = batch.flip_target(C1)
    assert C1 <= i < batch.n_jobs and batch.kinds[i] == "fit"
    blk = batch.want[i]
    _, _, payload, head = cases.parse_header(blk)
    assert head <= at < head + payload
    mutant = blk[:at] + bytes([blk[at] ^ 0x10]) + blk[at + 1 :]
    n, err, _ = oracle.decode_block(mutant, len(batch.blocks[i]), cases.BLOCK_SIZE)
    assert err != 0 and n < 0
    assert oracle.decode_block(blk, len(batch.blocks[i]), cases.BLOCK_SIZE)[:2] == (len(batch.blocks[i]), 0)
