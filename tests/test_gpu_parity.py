"""-m gpu: the parity tests proper.  Everything goes through the C ABI of bzip3_amd/lib/libbzip3.so on a
real MI355X and is compared, bit for bit, with the oracle (and with oracle/_ref when it travelled)."""
import ctypes as C
import hashlib
import os
import struct

import numpy as np
import pytest

import bzip3_amd
import datagen

pytestmark = pytest.mark.gpu
GOLDEN = datagen.GOLDEN


def _cases():
    c = dict(datagen.nasty_cases())
    t = datagen.shakespeare()
    c["text1m"] = t[1000000 : 1000000 + (1 << 20)]
    c["rand256k"] = datagen.random_bytes(256 * 1024)
    c["lowent512k"] = datagen.low_entropy(512 * 1024)
    c["repeats1m"] = datagen.repeats(1 << 20)
    c["markov2m"] = datagen.text(2 << 20, seed=11, chains=256)
    return c


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_stage_parity(gpu_lib, oracle, name):
    d = CASES[name]
    g = bzip3_amd.StageApi(gpu_lib)
    for k in {len(d), max(0, len(d) - 1), max(0, len(d) - 3), min(len(d), 5)}:
        assert g.crc32c(d[:k]) == oracle.crc32c(d[:k])          # crc32sum
    e = oracle.mrle_encode(d)
    assert g.mrle_encode(d) == e                                 # mrlec
    assert g.mrle_decode(e, len(d)) == (0, d)                    # mrled
    for cut in (len(e) - 1, len(e) - 2, 40):
        if 32 <= cut <= len(e):
            a, b = g.mrle_decode(e, len(d), cut), oracle.mrle_decode(e, len(d), cut)
            assert a[0] == b[0] and (a[0] != 0 or a[1] == b[1])
    assert g.lzp_encode(d) == oracle.lzp_encode(d)               # lzp_compress
    n, z = oracle.lzp_encode(d)
    if n > 0:
        assert g.lzp_decode(z, len(d) + 100) == (len(d), d)      # lzp_decompress
        assert g.lzp_decode(z, len(d) // 2) == oracle.lzp_decode(z, len(d) // 2)
    if len(d) > 1:
        assert g.bwt(d) == oracle.bwt(d)                         # libsais_bwt
        idx, u = oracle.bwt(d)
        assert g.unbwt(u, idx) == (0, d)                         # libsais_unbwt
        c = oracle.cm_encode(u)
        assert g.cm_encode(u) == c                               # encode_bytes
        assert g.cm_decode(c, len(u)) == u                       # decode_bytes
        assert g.cm_decode(c[: len(c) // 2], len(u)) == oracle.cm_decode(c[: len(c) // 2], len(u))


@pytest.mark.parametrize("name", sorted(CASES))
def test_block_parity(gpu_lib, oracle, name):
    d = CASES[name]
    bs = max(65 * 1024, len(d))
    with bzip3_amd.State(bs, gpu_lib) as st:
        a = st.encode_block(d)
        assert a == oracle.encode_block(d, bs)
        r = st.decode_block(a[2], len(d))
        assert r[2] == d and (r[:2] == (len(d), 0) or len(d) == 0)


def test_golden_fixture_decodes_on_gpu(gpu_lib):
    # the reference's `make test` (Makefile.am:81-83) on the GPU path
    raw = open(os.path.join(GOLDEN, "shakespeare.txt.bz3"), "rb").read()
    bs, chunks = datagen.parse_chunks(raw)
    out = b""
    with bzip3_amd.State(bs, gpu_lib) as st:
        for comp, orig, blk in chunks:
            n, err, dec = st.decode_block(blk, orig)
            assert (n, err) == (orig, 0)
            out += dec
    assert hashlib.md5(out).hexdigest() == datagen.SHAKESPEARE_MD5


def test_cfg1_known_answer_on_gpu(gpu_lib, text):
    # BASELINE config 1: shakespeare.txt -b 8 -> the oracle's / reference's exact file bytes
    with bzip3_amd.State(8 << 20, gpu_lib) as st:
        n, err, blk = st.encode_block(text)
        assert (n, err) == (1229797, 0)
        f = b"BZ3v1" + struct.pack("<I", 8 << 20) + struct.pack("<II", len(blk), len(text)) + blk
        assert hashlib.md5(f).hexdigest() == "90bb3148f6a5bf00be8d682458dd15dd"
        assert st.decode_block(blk, len(text)) == (len(text), 0, text)
        t = st.timings()
        assert t["cm"] > 0


def test_cm_decode_of_arbitrary_bytes_matches_reference(gpu_lib, oracle):
    # decode_bytes (src/libbz3.c:436-494) is defined on ANY input; random / skewed bytes exercise improbable symbols,
    # renormalisation runs and the `code < low` states a stream that ends early produces.
    g = bzip3_amd.StageApi(gpu_lib)
    rng = np.random.default_rng(12)
    for size, n in ((0, 1000), (5, 70000), (50000, 200000), (300000, 400000)):
        junk = bytes(rng.integers(0, 256, size=size, dtype=np.uint8))
        assert g.cm_decode(junk, n) == oracle.cm_decode(junk, n)
    skew = bytes(rng.choice(np.array([0, 255, 1, 128], dtype=np.uint8), size=100000, p=[0.6, 0.3, 0.05, 0.05]))
    assert g.cm_decode(skew, 500000) == oracle.cm_decode(skew, 500000)


def test_unbwt_of_arbitrary_bytes_matches_reference(gpu_lib, oracle):
    # libsais_unbwt on input that is not a genuine BWT (a corrupted block): the bytes it leaves decide the error code
    g = bzip3_amd.StageApi(gpu_lib)
    rng = np.random.default_rng(22)
    for trial in range(40):
        n = int(rng.integers(2, 100)) if trial % 4 == 0 else int(rng.integers(100, 700000))
        k = [1, 2, 3, 256, 7][trial % 5]
        u = bytes(rng.integers(0, k, size=n, dtype=np.uint8))
        for idx in sorted({1, n, int(rng.integers(1, n + 1)), int(rng.integers(1, n + 1))}):
            assert g.unbwt(u, idx) == oracle.unbwt(u, idx), (n, k, idx)


def test_corrupted_payload_error_codes(gpu_lib, oracle, text):
    """Bit flips inside the coded payload: CM -> unBWT -> LZP -> mRLE -> CRC all run on garbage and the return value /
    last_error must still be the reference's (the oracle is pinned against it on the same cases, tests/test_oracle.py)."""
    bs = 65 * 1024
    with bzip3_amd.State(bs, gpu_lib) as st:
        for data in (text[:60000], (text[:500] * 200)[:66000], datagen.low_entropy(50000)):
            blk = oracle.encode_block(data, bs)[2]
            for pos in (20, 25, 40, 100, len(blk) // 2, len(blk) - 3):
                for bit in (1, 0x40):
                    if pos >= len(blk):
                        continue
                    m = blk[:pos] + bytes([blk[pos] ^ bit]) + blk[pos + 1 :]
                    assert st.decode_block(m, len(data))[:2] == oracle.decode_block(m, len(data), bs)[:2], (len(data), pos, bit)


def test_random_mixtures_encode_identically(gpu_lib, oracle):
    """40 random concatenations of text / runs / repeats / noise / low-entropy pieces (sizes 0 .. 300 KB): the encoded block
    is byte-identical to the oracle's and decodes back (every stage flag combination of :609-632 shows up)."""
    rng = np.random.default_rng(77)
    bs = 320 * 1024
    text = datagen.shakespeare()
    models = set()
    with bzip3_amd.State(bs, gpu_lib) as st:
        for trial in range(40):
            parts = []
            for _ in range(int(rng.integers(1, 6))):
                n = int(rng.integers(0, 60000))
                kind = int(rng.integers(0, 6))
                if kind == 0:
                    o = int(rng.integers(0, len(text) - n)); parts.append(text[o : o + n])
                elif kind == 1:
                    parts.append(bytes([int(rng.integers(0, 256))]) * n)
                elif kind == 2:
                    unit = bytes(rng.integers(0, 256, size=int(rng.integers(1, 300)), dtype=np.uint8)); parts.append((unit * (n // len(unit) + 1))[:n])
                elif kind == 3:
                    parts.append(bytes(rng.integers(0, 256, size=n, dtype=np.uint8)))
                elif kind == 4:
                    parts.append(bytes(rng.choice(np.array([0xF2, 0xFF, 0, 65], dtype=np.uint8), size=n)))
                else:
                    parts.append(datagen.low_entropy(n) if n else b"")
            d = b"".join(parts)[: bs]
            a, b = st.encode_block(d), oracle.encode_block(d, bs)
            assert a == b, (trial, len(d))
            if a[0] > 8 and len(d) >= 64:
                models.add(a[2][8])
            k, err, back = st.decode_block(a[2], len(d))
            assert (err == 0 and back == d) or len(d) == 0, (trial, len(d))
    assert len(models) >= 3, models


def test_mutated_blocks_decode_like_the_reference(gpu_lib, oracle):
    """Decoder hardening: 800 mutated blocks through the GPU path; return value, last_error and decoded
    bytes equal the oracle's, which test_oracle.py pins against the real reference on the same generator (1500 mutants)."""
    import mutants

    data = mutants.seeds()
    blocks = [oracle.encode_block(d, mutants.BS)[2] for d in data]
    for m, osz in mutants.mutants(blocks, [len(d) for d in data], 800):
        # a fresh state per block, like the oracle: some paths of the reference leave last_error untouched (:596-601, :691)
        a, b = bzip3_amd.decode_block(m, osz, mutants.BS, gpu_lib), oracle.decode_block(m, osz, mutants.BS)
        assert a[:2] == b[:2] and (a[0] < 0 or a[2] == b[2]), (len(m), osz, a[:2], b[:2])


def test_decoder_error_codes(gpu_lib, oracle, text):
    bs = 65 * 1024
    blk = oracle.encode_block(text[:30000], bs)[2]
    muts = [blk[: len(blk) // 2], blk[:4] + b"\0\0\0\0" + blk[8:], blk[:8] + b"\x7f" + blk[9:], blk[:20] + bytes([blk[20] ^ 1]) + blk[21:],
            blk[:4] + b"\xff\xff\xff\x7f" + blk[8:], blk[:4] + b"\xfb\xff\xff\xff" + blk[8:], b"\0" * 9, blk[:9]]
    with bzip3_amd.State(bs, gpu_lib) as st:
        for m in muts:
            assert st.decode_block(m, 30000)[:2] == oracle.decode_block(m, 30000, bs)[:2]
        for bsz, cs, osz in [(5, len(blk), 30000), (len(blk) - 1, len(blk), 30000), (70000, -5, 30000), (70000, len(blk), -1),
                             (70000, len(blk), 10 ** 9), (20000, len(blk), 30000), (70000, len(blk), 29999), (70000, len(blk), 30001)]:
            assert st.decode_block(blk, osz, buffer_size=bsz, comp_size=cs)[:2] == oracle.decode_block(blk, osz, bs, buffer_size=bsz, comp_size=cs)[:2]
        assert st.encode_block(b"x" * (bs + 1))[:2] == (-1, bzip3_amd.BZ3_ERR_DATA_TOO_BIG)
        # a good block still decodes after failures (state reuse)
        assert st.decode_block(blk, 30000) == (30000, 0, text[:30000])


def test_batch_api_host_buffers(gpu_lib, oracle, text):
    # bz3_encode_blocks / bz3_decode_blocks (src/libbz3.c:845-870): n independent (state, buffer) pairs
    bs = 1 << 20
    blocks = [text[i * 700000 : i * 700000 + 700000 - i * 1000] for i in range(5)] + [b"tiny", datagen.random_bytes(100000, seed=9)]
    n = len(blocks)
    states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
    assert all(states)
    cap = gpu_lib.bz3_bound(bs) + 64
    bufs = [(C.c_uint8 * cap)() for _ in range(n)]
    for b, d in zip(bufs, blocks):
        C.memmove(b, d, len(d))
    ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
    gpu_lib.bz3_encode_blocks(states, ptrs, sizes, n)
    for i, d in enumerate(blocks):
        assert gpu_lib.bz3_last_error(states[i]) == 0
        assert bytes(bufs[i][: sizes[i]]) == oracle.encode_block(d, bs)[2]
    bsz = (C.c_size_t * n)(*[cap] * n)
    orig = (C.c_int32 * n)(*[len(d) for d in blocks])
    gpu_lib.bz3_decode_blocks(states, ptrs, bsz, sizes, orig, n)
    for i, d in enumerate(blocks):
        assert gpu_lib.bz3_last_error(states[i]) == 0 and bytes(bufs[i][: len(d)]) == d
    for s in states:
        gpu_lib.bz3_free(s)


@pytest.mark.parametrize("pipe", [None, "1,4", "5,3", "6,2", "3,8"], ids=["auto", "w1s4", "w5s3", "w6s2", "w3s8"])
def test_front_end_and_tail_rings_on_gpu(gpu_lib, oracle, text, pipe, monkeypatch):
    """The encoder's front end and the decoder's tail run their serial LZP kernels on side streams over a ring of context slots
    (api_encode.hip encode_group / api_decode.hip decode_group).  Under the CPU emulator kernels run at launch, so only here do the side streams really
    overlap the group's stream: 40 blocks (LZP applied, declined, stored) through forced ring shapes -- windows of one block
    through four slots, a ragged last window through three, round 2's two slots of six, eight slots (all eight side streams: an experiment's
    shape; a GPU-filling batch's tail takes four slots of 16 blocks by default) -- and the automatic one, classic and lean states: the
    oracle's bytes both ways.  The CU partition (side streams on reserved CUs, whole-GPU kernels on the rest) is taken from 128 blocks on
    (round 6): test_large_lean_batch_default_rings_and_kept_workspace_on_gpu covers it."""
    for var in ("BZ3_HIP_LZP_PIPE", "BZ3_HIP_TAIL_PIPE"):
        if pipe:
            monkeypatch.setenv(var, pipe)
        else:
            monkeypatch.delenv(var, raising=False)
    bs = 1 << 20
    distinct = []
    for i in range(10):
        if i % 5 == 3:
            distinct.append(text[i * 50000 : i * 50000 + 60000] * 4 + text[900000:930000])  # long repeats: LZP applies (model & 2)
        elif i == 6:
            distinct.append(b"x" * 41)                                                       # stored (< 64 bytes)
        elif i == 4:
            distinct.append(datagen.random_bytes(150000, seed=4))                            # LZP declines (model 0)
        else:
            distinct.append(text[i * 90000 : i * 90000 + 180000 + 9000 * i])
    want = [oracle.encode_block(d, bs)[2] for d in distinct]
    assert {w[8] for w, d in zip(want, distinct) if len(d) >= 64} >= {0, 2}
    blocks = [distinct[(7 * k) % 10] for k in range(40)]
    n = len(blocks)
    try:
        for lean in (0, 1):
            assert gpu_lib.bz3_hip_set_lean_states(lean) == 0
            states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
            assert all(states)
            cap = gpu_lib.bz3_bound(bs) + 64
            bufs = [(C.c_uint8 * cap)() for _ in range(n)]
            for b, d in zip(bufs, blocks):
                C.memmove(b, d, len(d))
            ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
            sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
            gpu_lib.bz3_encode_blocks(states, ptrs, sizes, n)
            if pipe:
                w, q = (int(x) for x in pipe.split(","))
                ring = gpu_lib.bz3_hip_debug_front_end_ring()
                assert (ring & 0xFFFF, (ring >> 16) & 0xFF) == (w, q)
            for k in range(n):
                assert bytes(bufs[k][: sizes[k]]) == want[(7 * k) % 10], (lean, k)
            bsz = (C.c_size_t * n)(*[cap] * n)
            orig = (C.c_int32 * n)(*[len(d) for d in blocks])
            gpu_lib.bz3_decode_blocks(states, ptrs, bsz, sizes, orig, n)
            for k, d in enumerate(blocks):
                assert gpu_lib.bz3_last_error(states[k]) == 0 and bytes(bufs[k][: len(d)]) == d, (lean, k)
            for st in states:
                gpu_lib.bz3_free(st)
    finally:
        gpu_lib.bz3_hip_set_lean_states(0)


def test_suffix_sorter_paths_on_gpu(gpu_lib, oracle, monkeypatch):
    """Every path of the round-3 suffix sorter (bwt.hip; cases and what they exercise: datagen.suffix_sorter_cases) against the
    oracle's BWT, then the big groups forced down the deep path (bz3_hip_debug_bwt_big_rounds(0), test hook), then a 6 MiB text block whose
    anchor tiles run concurrently on all CUs (the emulator runs them one after the other)."""
    g = bzip3_amd.StageApi(gpu_lib)
    cases = datagen.suffix_sorter_cases()
    for name in sorted(cases):
        assert g.bwt(cases[name]) == oracle.bwt(cases[name]), name
    try:
        gpu_lib.bz3_hip_debug_bwt_big_rounds(0)
        for name in ("phrase1", "phrase3", "text300k"):
            assert g.bwt(cases[name]) == oracle.bwt(cases[name]), name
        gpu_lib.bz3_hip_debug_bwt_big_rounds(8)
        for name in ("mixdeep", "phrase3"):
            assert g.bwt(cases[name]) == oracle.bwt(cases[name]), name
    finally:
        gpu_lib.bz3_hip_debug_bwt_big_rounds(-1)
    d = datagen.text(6 << 20, seed=77, chains=4096)
    assert g.bwt(d) == oracle.bwt(d)


def test_batch_over_all_gpus_of_the_node(gpu_lib, oracle, text):
    """bz3_encode_blocks / bz3_decode_blocks with states on EVERY visible GPU (the reference forks a thread per block,
    src/libbz3.c:845-870): bz3_new round-robins the states over the devices, the batch is split into one group per GPU and the groups
    run at the same time (api.hip for_each_device_group).  Oracle bytes both ways, as many groups inside their group function at once
    as there are devices, and the batch takes no longer than 1.15 x the same per-GPU load (6 blocks of 4 MiB: > 3 s of codec time) on one GPU alone -- groups that ran one after the other would take ndev x.  Skipped on a 1-GPU lease:
    it costs nothing there, and it is the only hardware evidence of row (e) when the node has more."""
    import time

    ndev = gpu_lib.bz3_hip_device_count()
    if ndev < 2:
        pytest.skip("one visible GPU: the multi-device path needs at least two (the emulator suite runs it with two emulated devices)")
    bs = 4 << 20
    per_dev = 6
    pieces = [text[(i * 700001) % (len(text) - bs) :][:bs - 1000 * i] for i in range(per_dev * ndev)]

    def run(blocks):
        n = len(blocks)
        states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
        assert all(states)
        cap = gpu_lib.bz3_bound(bs) + 64
        bufs = [(C.c_uint8 * cap)() for _ in range(n)]
        for b, d in zip(bufs, blocks):
            C.memmove(b, d, len(d))
        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
        gpu_lib.bz3_hip_debug_peak_concurrent_groups(1)
        t0 = time.perf_counter()
        gpu_lib.bz3_encode_blocks(states, ptrs, sizes, n)
        t_enc = time.perf_counter() - t0
        peak_enc = gpu_lib.bz3_hip_debug_peak_concurrent_groups(1)
        coded = [bytes(bufs[i][: sizes[i]]) for i in range(n)]
        assert all(gpu_lib.bz3_last_error(states[i]) == 0 for i in range(n))
        bsz = (C.c_size_t * n)(*[cap] * n)
        orig = (C.c_int32 * n)(*[len(d) for d in blocks])
        t0 = time.perf_counter()
        gpu_lib.bz3_decode_blocks(states, ptrs, bsz, sizes, orig, n)
        t_dec = time.perf_counter() - t0
        peak_dec = gpu_lib.bz3_hip_debug_peak_concurrent_groups(1)
        assert all(gpu_lib.bz3_last_error(states[i]) == 0 and bytes(bufs[i][: len(d)]) == d for i, d in enumerate(blocks))
        devs = sorted(gpu_lib.bz3_hip_state_device(s) for s in states)
        for s in states:
            gpu_lib.bz3_free(s)
        return coded, t_enc + t_dec, min(peak_enc, peak_dec), devs

    gpu_lib.bz3_hip_bind_device(-1)  # round robin over the visible devices
    run(pieces[:ndev])               # first touch of every device (contexts, streams) outside the timed calls
    coded, t_all, peak, devs = run(pieces)
    assert devs == sorted(list(range(ndev)) * per_dev), devs
    assert peak == ndev, f"{peak} device groups ran at the same time, {ndev} devices"
    for d, c in zip(pieces, coded):
        assert c == oracle.encode_block(d, bs)[2]
    gpu_lib.bz3_hip_bind_device(0)
    _, t_one, _, devs1 = run(pieces[:per_dev])  # the same per-GPU load on one GPU
    gpu_lib.bz3_hip_bind_device(-1)
    assert set(devs1) == {0}
    assert t_one > 1.0, f"per-GPU load too small to tell overlap from serialisation ({t_one:.2f}s)"
    assert t_all < 1.15 * t_one, f"{ndev} GPUs x {per_dev} blocks took {t_all:.2f}s, one GPU x {per_dev} blocks {t_one:.2f}s"


def test_device_resident_api(gpu_lib, oracle, text):
    import torch

    bs = 2 << 20
    d = text[: 2 << 20]
    cap = gpu_lib.bz3_bound(bs) + 64
    buf = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    buf[: len(d)] = torch.frombuffer(bytearray(d), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    gpu_lib.bz3_hip_bind_device(0)
    with bzip3_amd.State(bs, gpu_lib) as st:
        n = gpu_lib.bz3_hip_encode_block_device(st.ptr, buf.data_ptr(), len(d))
        assert st.last_error == 0
        assert bytes(buf[:n].cpu().numpy()) == oracle.encode_block(d, bs)[2]
        m = gpu_lib.bz3_hip_decode_block_device(st.ptr, buf.data_ptr(), cap, n, len(d))
        assert (m, st.last_error) == (len(d), 0)
        assert bytes(buf[:m].cpu().numpy()) == d
    gpu_lib.bz3_hip_bind_device(-1)


def test_frame_api_round_trip_and_reference_interop(gpu_lib, text):
    from oracle_lib import require_ref

    data = text[:3000000]
    out = (C.c_uint8 * (gpu_lib.bz3_bound(len(data)) + 64))()
    osz = C.c_size_t(len(out))
    assert gpu_lib.bz3_compress(1 << 20, data, out, len(data), C.byref(osz)) == 0
    ref = require_ref()  # byte-identical frame (a -m gpu run without the real reference fails, it never skips the comparison)
    out2 = (C.c_uint8 * len(out))()
    osz2 = C.c_size_t(len(out2))
    assert ref.lib.bz3_compress(1 << 20, data, out2, len(data), C.byref(osz2)) == 0
    assert osz.value == osz2.value and bytes(out[: osz.value]) == bytes(out2[: osz2.value])
    back = (C.c_uint8 * (len(data) + 16))()
    bsz = C.c_size_t(len(back))
    assert gpu_lib.bz3_decompress(out, back, osz.value, C.byref(bsz)) == 0
    assert bytes(back[: bsz.value]) == data


def test_frame_api_multi_block_matches_reference(gpu_lib, text):
    """bz3_compress / bz3_decompress (src/libbz3.c:876-997) batch the blocks of a frame; frames, return codes and the
    bytes committed before an error must equal the reference's sequential loop (good + 15 malformed frames)."""
    import frame_cases

    frame_cases.check(gpu_lib, text[: 4 * 65 * 1024 + 1234], 65 * 1024)
    frame_cases.check(gpu_lib, (text * 3)[: 4 * (1 << 20) + 777], 1 << 20)


def test_large_block_round_trip_properties(gpu_lib, oracle):
    # size-independent properties at a size the oracle's BWT would not finish quickly: decode(encode(x)) == x,
    # the stored CRC is the oracle's CRC of x, header fields are self-consistent, and (when oracle/_ref
    # travelled) the bytes equal the real reference's.
    from oracle_lib import Bz3, require_ref

    n = int(os.environ.get("BZ3_TEST_LARGE_MIB", "24")) << 20
    d = datagen.text(n, seed=21, chains=4096)
    with bzip3_amd.State(n, gpu_lib) as st:
        m, err, blk = st.encode_block(d)
        assert err == 0 and 0 < m < n // 3
        assert struct.unpack("<I", blk[:4])[0] == oracle.crc32c(d)
        assert Bz3(require_ref().lib).encode_block(d, n)[2] == blk
        k, err, back = st.decode_block(blk, n)
        assert (k, err) == (n, 0) and back == d
        print("timings(decode, ms):", st.timings(), "bwt:", st.bwt_stats())


def test_full_size_blocks_256_32_511mib(gpu_lib, oracle):
    """BASELINE.json's block sizes in the default suite: one 256 MiB block (cfg3/cfg4), one 32 MiB block (cfg2) and the 511 MiB
    maximum (cfg5: the u32 index arithmetic of the suffix sorter at its largest n, src/libbz3.c:536) go through
    bz3_encode_blocks / bz3_decode_blocks as ONE batch (the serial CM launches overlap, so the test costs one 511 MiB block).
    Green means compared: the inputs are deterministic (tests/datagen.py) and tests/golden/full_size_digests.json holds their
    digests and the size + md5 of the REAL reference's coded bytes for them (recorded from the reference in round 2,
    profiles/r02_full_size_parity_*.log); both are asserted unconditionally.  In addition the real reference (oracle/_ref) encodes
    the same blocks on the host meanwhile and its bytes are compared byte for byte -- a run without oracle/_ref FAILS, it does
    not skip the comparison.  Then the batch is decoded and compared with the plaintext.  BZ3_TEST_NO_511=1 drops the 511 MiB
    block (builder-side quick runs only)."""
    import json
    import threading

    from oracle_lib import Bz3, require_ref

    golden = json.load(open(os.path.join(datagen.GOLDEN, "full_size_digests.json")))
    sizes_mib = [256, 32] + ([] if os.environ.get("BZ3_TEST_NO_511") == "1" else [511])
    seeds = {256: 31, 32: 32, 511: 33}
    blocks = [datagen.text(m << 20, seed=seeds[m], chains=65536) for m in sizes_mib]
    for m, d in zip(sizes_mib, blocks):
        g = golden[str(m)]
        assert (len(d), hashlib.md5(d).hexdigest()) == (g["plain_bytes"], g["plain_md5"]), "%d MiB: the deterministic input changed" % m
    ref = require_ref()
    want = {}

    def encode_on_host(k):
        want[k] = Bz3(ref.lib).encode_block(blocks[k], len(blocks[k]))

    threads = [threading.Thread(target=encode_on_host, args=(k,)) for k in range(len(blocks))]
    for t in threads:
        t.start()
    n = len(blocks)
    states = (C.c_void_p * n)(*[gpu_lib.bz3_new(len(d)) for d in blocks])
    assert all(states)
    caps = [gpu_lib.bz3_bound(len(d)) + 64 for d in blocks]
    bufs = [(C.c_uint8 * cap)() for cap in caps]
    for b, d in zip(bufs, blocks):
        C.memmove(b, d, len(d))
    ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
    gpu_lib.bz3_encode_blocks(states, ptrs, sizes, n)
    coded = []
    for i, d in enumerate(blocks):
        assert gpu_lib.bz3_last_error(states[i]) == 0 and 0 < sizes[i] < len(d) // 3, i
        coded.append(C.string_at(bufs[i], sizes[i]))
        assert struct.unpack("<I", coded[i][:4])[0] == oracle.crc32c(d)
        g = golden[str(sizes_mib[i])]
        assert (sizes[i], hashlib.md5(coded[i]).hexdigest()) == (g["coded_bytes"], g["coded_md5"]), \
            "%d MiB block: coded bytes differ from the committed digest of the reference's output" % sizes_mib[i]
    for t in threads:
        t.join()
    for i in range(n):
        m, err, blk = want[i]
        assert (sizes[i], 0) == (m, err) and coded[i] == blk, "%d MiB block differs from the reference" % sizes_mib[i]
        print("%d MiB block: %d bytes, md5 %s, byte-identical to the reference" % (sizes_mib[i], m, hashlib.md5(blk).hexdigest()))
    bsz = (C.c_size_t * n)(*caps)
    orig = (C.c_int32 * n)(*[len(d) for d in blocks])
    gpu_lib.bz3_decode_blocks(states, ptrs, bsz, sizes, orig, n)
    for i, d in enumerate(blocks):
        assert gpu_lib.bz3_last_error(states[i]) == 0, i
        assert C.string_at(bufs[i], len(d)) == d, "%d MiB block: decode differs from the plaintext" % sizes_mib[i]
    tm = (C.c_float * 8)()
    gpu_lib.bz3_hip_last_timings(states[0], tm)
    print("timings(decode of the 256 MiB block, ms):", [round(x, 1) for x in tm[:6]])
    for s in states:
        gpu_lib.bz3_free(s)
    gpu_lib.bz3_hip_release_cached_memory()


# ---- opt-in machinery (row-cache kernels, lean states): after everything the default path needs ----------------------------------
def test_cm_row_cache_kernels_on_gpu(gpu_lib, oracle, text):
    """The row-cache CM kernels (two workgroups per CU; bz3_hip_set_cm_mode(1)) must produce the bytes of the oracle:
    stage hooks on BWT output of text (fits the cache), on a 150-symbol source (slots are recycled through the spill
    area), on random bytes (given up by the kernel, coded again by the full-model kernel) and on a truncated stream;
    then a host-buffer batch that mixes text and random blocks."""
    g = bzip3_amd.StageApi(gpu_lib)
    rng = np.random.default_rng(12)
    def zipf(nsym, a, n):
        p = 1.0 / np.arange(1, nsym + 1) ** a
        return bytes(rng.permutation(256)[:nsym].astype(np.uint8)[rng.choice(nsym, size=n, p=p / p.sum())])

    wide = zipf(150, 1.2, 400000)  # 4 % of the bytes outside the 96 / 112 cached rows: thrashes, may be given up
    inputs = {"text": oracle.bwt(text[2000000 : 2000000 + (1 << 20)])[1], "wide150": wide, "wide130": zipf(130, 2.5, 400000),
              "rand": datagen.random_bytes(200000, seed=3), "lowent": oracle.bwt(datagen.low_entropy(300000))[1], "tiny": b"abracadabra"}
    given_up = {"text": 0, "wide130": 0, "rand": 2, "lowent": 0, "tiny": 0}
    try:
        assert gpu_lib.bz3_hip_set_cm_mode(1) == 0
        for name, d in inputs.items():
            c = oracle.cm_encode(d)
            n0 = gpu_lib.bz3_hip_cm_blocks_given_up()
            assert g.cm_encode(d) == c, name
            assert g.cm_decode(c, len(d)) == d, name
            if name in given_up:
                assert gpu_lib.bz3_hip_cm_blocks_given_up() - n0 == given_up[name], name
            cut = c[: len(c) // 3]
            assert g.cm_decode(cut, len(d)) == oracle.cm_decode(cut, len(d)), name
        bs = 1 << 20
        blocks = [text[i * 500000 : i * 500000 + 400000] for i in range(6)] + [datagen.random_bytes(150000, seed=5), b"tiny", wide[:300000]]
        n = len(blocks)
        states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
        assert all(states)
        cap = gpu_lib.bz3_bound(bs) + 64
        bufs = [(C.c_uint8 * cap)() for _ in range(n)]
        for b, d in zip(bufs, blocks):
            C.memmove(b, d, len(d))
        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
        gpu_lib.bz3_encode_blocks(states, ptrs, sizes, n)
        for i, d in enumerate(blocks):
            assert gpu_lib.bz3_last_error(states[i]) == 0
            assert bytes(bufs[i][: sizes[i]]) == oracle.encode_block(d, bs)[2], i
        bsz = (C.c_size_t * n)(*[cap] * n)
        orig = (C.c_int32 * n)(*[len(d) for d in blocks])
        gpu_lib.bz3_decode_blocks(states, ptrs, bsz, sizes, orig, n)
        for i, d in enumerate(blocks):
            assert gpu_lib.bz3_last_error(states[i]) == 0 and bytes(bufs[i][: len(d)]) == d, i
        for s in states:
            gpu_lib.bz3_free(s)
    finally:
        gpu_lib.bz3_hip_set_cm_mode(-1)


def test_lean_states_on_gpu(gpu_lib, oracle, text):
    """Lean states (bz3_hip_set_lean_states): no per-state swap buffer, the CM encoder works in place in the caller's
    buffer, the CM decoder reads a staged copy of the payload, the tail runs in windows.  Same bytes, return values and
    error codes: block parity on every case, a batch, the device-resident entry points, 300 mutated blocks, and small
    caller buffers (the LZP decoder writes into the caller's buffer instead of a bz3_bound-sized swap buffer)."""
    import mutants

    try:
        assert gpu_lib.bz3_hip_set_lean_states(1) == 0
        for mode in (-1, 1):
            assert gpu_lib.bz3_hip_set_cm_mode(mode) == 0
            for name in sorted(CASES):
                d = CASES[name]
                bs = max(65 * 1024, len(d))
                with bzip3_amd.State(bs, gpu_lib) as st:
                    a = st.encode_block(d)
                    assert a == oracle.encode_block(d, bs), (mode, name)
                    r = st.decode_block(a[2], len(d))
                    assert (r[:2] == (len(d), 0) or len(d) == 0) and r[2] == d, (mode, name)
        assert gpu_lib.bz3_hip_set_cm_mode(-1) == 0
        # batch through the host-buffer API
        bs = 1 << 20
        blocks = [text[i * 700000 : i * 700000 + 700000 - i * 1000] for i in range(5)] + [b"tiny", datagen.random_bytes(300000, seed=9), b""]
        n = len(blocks)
        states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
        assert all(states)
        cap = gpu_lib.bz3_bound(bs) + 64
        bufs = [(C.c_uint8 * cap)() for _ in range(n)]
        for b, d in zip(bufs, blocks):
            C.memmove(b, d, len(d))
        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
        gpu_lib.bz3_encode_blocks(states, ptrs, sizes, n)
        for i, d in enumerate(blocks):
            assert bytes(bufs[i][: sizes[i]]) == oracle.encode_block(d, bs)[2], i
        bsz = (C.c_size_t * n)(*[cap] * n)
        orig = (C.c_int32 * n)(*[len(d) for d in blocks])
        gpu_lib.bz3_decode_blocks(states, ptrs, bsz, sizes, orig, n)
        for i, d in enumerate(blocks):
            assert bytes(bufs[i][: len(d)]) == d, i
        for s in states:
            gpu_lib.bz3_free(s)
        # hostile input
        data = mutants.seeds()
        enc = [oracle.encode_block(d, mutants.BS)[2] for d in data]
        for m, osz in mutants.mutants(enc, [len(d) for d in data], 300, seed=77):
            a, b = bzip3_amd.decode_block(m, osz, mutants.BS, gpu_lib), oracle.decode_block(m, osz, mutants.BS)
            assert a[:2] == b[:2] and (a[0] < 0 or a[2] == b[2]), (len(m), osz, a[:2], b[:2])
        # caller buffers smaller than bz3_bound(block_size)
        plain = (text[:3000] * 4) + text[5000:9000]
        blk = oracle.encode_block(plain, mutants.BS)[2]
        k = len(plain)
        with bzip3_amd.State(mutants.BS, gpu_lib) as st:
            for bsz_, cs, osz in [(k, len(blk), k), (k + 1, len(blk), k), (len(blk), len(blk), k), (k - 1, len(blk), k), (k, len(blk), k - 1),
                                  (k // 2, len(blk), k // 2), (70000, len(blk), k), (5, len(blk), k)]:
                assert st.decode_block(blk, osz, buffer_size=bsz_, comp_size=cs)[:2] == oracle.decode_block(blk, osz, mutants.BS, buffer_size=bsz_, comp_size=cs)[:2]
    finally:
        gpu_lib.bz3_hip_set_lean_states(0)
        gpu_lib.bz3_hip_set_cm_mode(-1)
        gpu_lib.bz3_hip_release_cached_memory()


def test_large_lean_batch_default_rings_and_kept_workspace_on_gpu(gpu_lib, oracle, text):
    """The defaults for GPU-filling batches, at a size a test can afford: 140 lean blocks (>= 128: the decoder's tail takes its four-slot ring -- windows of 30
    blocks since round 6 -- on the CU partition, LZP decoders on the 64 reserved CUs, whole-GPU kernels on the others) through the batch API, twice, with the
    workspace KEPT between the calls (bz3_hip_set_keep_workspace(1): the decode call reuses the encode call's arena and carves the swap buffers of its tail
    windows from it).  Blocks of text with long repeats (LZP and mRLE on), a random block, a tiny and an empty one; on the second trip one payload is
    corrupted: that block fails its CRC, its neighbours do not.  (140 blocks are fewer than an MI355X has CUs: the batch takes the whole-model CM
    kernels, one block per CU, and nothing is routed, the random block neither.  Batches that take the row-cache variants, with routing and hand-back:
    tests/test_gpu_cm_batches.py.)"""
    n = 140
    bs = 128 * 1024
    blocks = []
    for i in range(n):
        if i == 7:
            blocks.append(datagen.random_bytes(90000, seed=3))
        elif i == 19:
            blocks.append(b"tiny")
        elif i == 23:
            blocks.append(b"")
        else:
            o = (i * 37123) % 4000000
            blocks.append(text[o : o + 40000 + 13 * i] + text[o + 100 : o + 20100] + b"\xf2" * (i % 5) + b"q" * (300 + i))
    want = [oracle.encode_block(d, bs)[2] for d in blocks]
    try:
        assert gpu_lib.bz3_hip_set_lean_states(1) == 0 and gpu_lib.bz3_hip_set_keep_workspace(1) == 0
        states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
        assert all(states)
        cap = gpu_lib.bz3_bound(bs) + 64
        for trip in range(2):
            bufs = [(C.c_uint8 * cap)() for _ in range(n)]
            for b, d in zip(bufs, blocks):
                C.memmove(b, d, len(d))
            ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
            sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
            gpu_lib.bz3_encode_blocks(states, ptrs, sizes, n)
            for i in range(n):
                assert bytes(bufs[i][: sizes[i]]) == want[i], (trip, i)
            if trip == 1:
                bufs[50][sizes[50] // 2] ^= 0x41
            bsz = (C.c_size_t * n)(*[cap] * n)
            orig = (C.c_int32 * n)(*[len(d) for d in blocks])
            gpu_lib.bz3_decode_blocks(states, ptrs, bsz, sizes, orig, n)
            for i, d in enumerate(blocks):
                if trip == 1 and i == 50:
                    assert gpu_lib.bz3_last_error(states[i]) != 0
                else:
                    assert gpu_lib.bz3_last_error(states[i]) == 0 and bytes(bufs[i][: len(d)]) == d, (trip, i)
        for s_ in states:
            gpu_lib.bz3_free(s_)
    finally:
        gpu_lib.bz3_hip_set_keep_workspace(-1)
        gpu_lib.bz3_hip_set_lean_states(0)
        gpu_lib.bz3_hip_release_cached_memory()


def test_zz_three_blocks_per_cu_variants_on_gpu(gpu_lib, oracle, text):
    """The 44/56-row kernels (mode 2: three blocks per CU), the 96-row pair (1) and the whole-model pair (0) through the stage hooks:
    same bytes as the oracle on text, a source that recycles slots, random bytes (given up, recoded by the full-model kernel) and a
    truncated stream."""
    g = bzip3_amd.StageApi(gpu_lib)
    rng = np.random.default_rng(13)
    p = 1.0 / np.arange(1, 91) ** 2.0
    wide = bytes(rng.permutation(256)[:90].astype(np.uint8)[rng.choice(90, size=300000, p=p / p.sum())])
    inputs = {"text": oracle.bwt(text[3000000 : 3000000 + (1 << 20)])[1], "wide90": wide, "rand": datagen.random_bytes(150000, seed=4), "tiny": b"abracadabra"}
    try:
        for mode in (2, 1, 0):
            assert gpu_lib.bz3_hip_set_cm_mode(mode) == 0
            for name, d in inputs.items():
                c = oracle.cm_encode(d)
                assert g.cm_encode(d) == c, (mode, name)
                assert g.cm_decode(c, len(d)) == d, (mode, name)
                assert g.cm_decode(c[: len(c) // 3], len(d)) == oracle.cm_decode(c[: len(c) // 3], len(d)), (mode, name)
    finally:
        gpu_lib.bz3_hip_set_cm_mode(-1)


@pytest.mark.gpu
def test_zz_calibrated_text_stays_on_the_three_per_cu_kernels(gpu_lib, oracle):
    """Round 4's regression: text with digits and markup (tests/datagen.py ENWIK_NOISE, the enwik8 calibration of bench.py's workload)
    misses the 44 / 56-row caches of the three-blocks-per-CU CM kernels on ~0.3 % of its bytes; rounds 1-3 gave a block up beyond 0.4 %,
    so a whole batch of such blocks was coded twice.  Now: beyond 3 % (stages.hpp CM_MISS_BASE / CM_MISS_SHIFT).  Four blocks of 6 MiB
    through the row-cache kernels of both directions: oracle bytes, nothing given up; a binary block in the same batch still is."""
    bs = 6 << 20
    blocks = [datagen.text(bs, seed=60 + i, chains=4096, noise=datagen.ENWIK_NOISE) for i in range(4)] + [datagen.random_bytes(1 << 20, seed=9)]
    n = len(blocks)
    try:
        assert gpu_lib.bz3_hip_set_cm_mode(2) == 0
        states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
        assert all(states)
        cap = gpu_lib.bz3_bound(bs) + 64
        bufs = [(C.c_uint8 * cap)() for _ in range(n)]
        for b, d in zip(bufs, blocks):
            C.memmove(b, d, len(d))
        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
        g0 = gpu_lib.bz3_hip_cm_blocks_given_up()
        gpu_lib.bz3_encode_blocks(states, ptrs, sizes, n)
        g1 = gpu_lib.bz3_hip_cm_blocks_given_up()
        for i, d in enumerate(blocks):
            assert gpu_lib.bz3_last_error(states[i]) == 0
            assert bytes(bufs[i][: sizes[i]]) == oracle.encode_block(d, bs)[2], i
        bsz = (C.c_size_t * n)(*[cap] * n)
        orig = (C.c_int32 * n)(*[len(d) for d in blocks])
        gpu_lib.bz3_decode_blocks(states, ptrs, bsz, sizes, orig, n)
        g2 = gpu_lib.bz3_hip_cm_blocks_given_up()
        for i, d in enumerate(blocks):
            assert gpu_lib.bz3_last_error(states[i]) == 0 and bytes(bufs[i][: len(d)]) == d, i
        assert (g1 - g0, g2 - g1) == (1, 1), (g1 - g0, g2 - g1)  # the random block only
        for s in states:
            gpu_lib.bz3_free(s)
    finally:
        gpu_lib.bz3_hip_set_cm_mode(-1)


def test_kept_workspace_leaves_the_headroom_to_the_host_program(gpu_lib, text):
    """the headroom rule (include/bz3_hip.h bz3_hip_set_workspace_headroom).  The device is filled with ballast until only a few GiB are
    free -- less than a full ring of LZP contexts would take --, then a lean batch goes through encode and decode with the workspace KEPT.  After each call
    at least `headroom` bytes are free and a torch allocation of that size succeeds (round 5: the kept workspace took every byte and the host program's next
    48 MiB allocation failed); the ring shrank to make that true; the round trip is the identity and the coded bytes equal a run without memory pressure."""
    import torch

    GiB = 1 << 30
    dev = torch.device("cuda", 0)
    bs = 16 << 20
    n = 40
    base = (text * 4)[:bs]
    cap = gpu_lib.bz3_bound(bs) + 64
    headroom = 2 * GiB
    gpu_lib.bz3_hip_bind_device(0)
    gpu_lib.bz3_hip_release_cached_memory()
    src = torch.frombuffer(bytearray(base), dtype=torch.uint8).to(dev)
    bufs = []
    for k in range(n):
        b = torch.zeros(cap, dtype=torch.uint8, device=dev)
        b[:bs] = torch.roll(src, 4099 * k)
        bufs.append(b)
    plain = [b[:bs].clone() for b in bufs[:3]]
    need, ctx = gpu_lib.bz3_hip_debug_workspace_bytes(bs, 0), gpu_lib.bz3_hip_debug_workspace_bytes(bs, 1)
    ballast = None
    try:
        assert gpu_lib.bz3_hip_set_lean_states(1) == 0 and gpu_lib.bz3_hip_set_keep_workspace(1) == 0
        gpu_lib.bz3_hip_set_workspace_headroom(headroom)
        states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
        assert all(states)
        ptrs = (C.c_void_p * n)(*[b.data_ptr() for b in bufs])

        def round_trip():
            sizes = (C.c_int32 * n)(*[bs] * n)
            gpu_lib.bz3_hip_encode_blocks_device(states, ptrs, sizes, n)
            assert all(sizes[i] > 0 and gpu_lib.bz3_last_error(states[i]) == 0 for i in range(n))
            free_enc = torch.cuda.mem_get_info(dev)[0]
            ring = gpu_lib.bz3_hip_debug_front_end_ring()
            coded = [bytes(bufs[i][: sizes[i]].cpu().numpy()) for i in (0, 1, n - 1)]
            bsz = (C.c_size_t * n)(*[cap] * n)
            orig = (C.c_int32 * n)(*[bs] * n)
            gpu_lib.bz3_hip_decode_blocks_device(states, ptrs, bsz, sizes, orig, n)
            assert all(gpu_lib.bz3_last_error(states[i]) == 0 for i in range(n))
            free_dec = torch.cuda.mem_get_info(dev)[0]
            for i in range(3):
                assert torch.equal(bufs[i][:bs], plain[i]), i
            return free_enc, free_dec, (ring & 0xFFFF, (ring >> 16) & 0xFF), coded

        _, _, shape0, coded0 = round_trip()  # plenty of memory: the ring takes its full shape, 4 slots of 8
        assert shape0 == (8, 4), shape0
        gpu_lib.bz3_hip_release_cached_memory()
        torch.cuda.empty_cache()
        # ballast: leave the stages' scratch + 12 contexts (with a swap buffer each) + the headroom free -- a full ring would be 32 contexts
        leave = need + 12 * (ctx + cap) + headroom + (1 * GiB)
        free0 = torch.cuda.mem_get_info(dev)[0]
        assert free0 > leave + GiB
        ballast = torch.empty(free0 - leave, dtype=torch.uint8, device=dev)
        gpu_lib.bz3_hip_debug_headroom_events(1, None)
        free_enc, free_dec, shape1, coded1 = round_trip()
        assert coded1 == coded0  # the bytes do not depend on the ring's shape
        assert shape1[0] * shape1[1] < 32 and shape1[0] * shape1[1] >= 8, shape1  # the ring shrank instead of eating the headroom
        assert free_enc >= headroom and free_dec >= headroom, (free_enc, free_dec)
        assert gpu_lib.bz3_hip_debug_cached_bytes(0) > need  # ... and the workspace is still kept
        x = torch.empty(headroom - (64 << 20), dtype=torch.uint8, device=dev)  # what the host program was promised is really there
        x.fill_(1)
        torch.cuda.synchronize()
        del x
        rel = C.c_uint(0)
        trims = gpu_lib.bz3_hip_debug_headroom_events(0, C.byref(rel))
        assert rel.value == 0, (trims, rel.value)  # sized right: the rule did not have to throw the workspace away
        # a headroom nobody can honour beside the ballast: the library then holds NOTHING when the call returns
        gpu_lib.bz3_hip_set_workspace_headroom(leave + 8 * GiB)
        round_trip()
        assert gpu_lib.bz3_hip_debug_cached_bytes(0) == 0
        for s_ in states:
            gpu_lib.bz3_free(s_)
    finally:
        del ballast
        gpu_lib.bz3_hip_set_workspace_headroom(-1)
        gpu_lib.bz3_hip_set_keep_workspace(-1)
        gpu_lib.bz3_hip_set_lean_states(0)
        gpu_lib.bz3_hip_release_cached_memory()
        gpu_lib.bz3_hip_bind_device(-1)
        torch.cuda.empty_cache()


@pytest.mark.parametrize("pipe", [None, "1,4", "5,3", "6,2"], ids=["auto", "w1s4", "w5s3", "w6s2"])
def test_two_thread_front_end_on_gpu(gpu_lib, oracle, text, pipe, monkeypatch):
    """Round 6: the encoder's front end on two host threads and two streams (bz3_hip_set_front_end_duo(1); api_encode.hip encode_group) -- only on the GPU do the
    two streams really overlap.  120 blocks of up to 1.5 MiB (LZP applied, declined, stored, random), classic and lean states, three encode calls in a row
    (the later ones reuse the pool's swap buffers, which phase A may only touch behind phase B's events), forced ring shapes: the oracle's bytes, and the
    decoder gives the plaintext back."""
    if pipe:
        monkeypatch.setenv("BZ3_HIP_LZP_PIPE", pipe)
    else:
        monkeypatch.delenv("BZ3_HIP_LZP_PIPE", raising=False)
    bs = 1536 * 1024
    distinct = []
    for i in range(12):
        if i % 5 == 3:
            distinct.append(text[i * 50000 : i * 50000 + 60000] * 5 + text[900000:930000])
        elif i == 6:
            distinct.append(b"x" * 41)
        elif i == 4:
            distinct.append(datagen.random_bytes(300000, seed=4))
        else:
            distinct.append(text[i * 90000 : i * 90000 + 400000 + 90000 * i])
    want = [oracle.encode_block(d, bs)[2] for d in distinct]
    blocks = [distinct[(7 * k) % 12] for k in range(120)]
    n = len(blocks)
    try:
        assert gpu_lib.bz3_hip_set_front_end_duo(1) == 0
        for lean in (0, 1):
            assert gpu_lib.bz3_hip_set_lean_states(lean) == 0
            states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
            assert all(states)
            cap = gpu_lib.bz3_bound(bs) + 64
            for trip in range(3):
                bufs = [(C.c_uint8 * cap)() for _ in range(n)]
                for b, d in zip(bufs, blocks):
                    C.memmove(b, d, len(d))
                ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
                sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
                gpu_lib.bz3_encode_blocks(states, ptrs, sizes, n)
                assert (gpu_lib.bz3_hip_debug_front_end_ring() >> 29) & 1 == 1
                for k in range(n):
                    assert bytes(bufs[k][: sizes[k]]) == want[(7 * k) % 12], (lean, trip, k)
            bsz = (C.c_size_t * n)(*[cap] * n)
            orig = (C.c_int32 * n)(*[len(d) for d in blocks])
            gpu_lib.bz3_decode_blocks(states, ptrs, bsz, sizes, orig, n)
            for k, d in enumerate(blocks):
                assert gpu_lib.bz3_last_error(states[k]) == 0 and bytes(bufs[k][: len(d)]) == d, (lean, k)
            for s_ in states:
                gpu_lib.bz3_free(s_)
    finally:
        gpu_lib.bz3_hip_set_front_end_duo(-1)
        gpu_lib.bz3_hip_set_lean_states(0)
        gpu_lib.bz3_hip_release_cached_memory()
