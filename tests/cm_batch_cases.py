"""Inputs and expected counters for the CM batch tests (tests/test_gpu_cm_batches.py on hardware, tests/test_cm_batch_cases.py for the
preconditions, without a GPU).

A batch of `n_jobs` CM jobs (blocks of 64 bytes or more) plus one stored and one empty block, every block distinct, seeded and deterministic:

  fitting   >= 60 %: Markov text (datagen.text) mapped onto an alphabet of at most 40 byte values, kept only when the reference's coded block has
            model byte 0 (neither LZP nor mRLE applied).  The CM input is then a permutation of the block: at most 40 distinct values, so at most 40 order-1
            rows (rows are keyed by byte value).  The row caches hold 44 rows at least (cm.hip CM_ROWS3_ENC), nothing is ever evicted, the only misses are
            the first touches (<= 40 < CM_MISS_BASE = 1024): such a block can neither be routed (nothing lies outside its 40 most frequent values) nor
            given up.
  ordinary  ~ 30 %: Shakespeare slices at scattered offsets, a third with a repeated passage appended (LZP applies), a third with a run of b"q" and a few
            0xF2 bytes (mRLE applies).  They recycle row slots through the spill area; whether one is handed back is left open.
  specials  four random blocks (routed in both directions), two blocks of 128 equally likely byte values (routed on encode: 88 / 128 of the bytes lie
            outside the top 40; they shrink to ~0.875, so the decoder does not route them and its row cache hands them back), a 41-byte block (stored)
            and an empty one.

The routing counts are DERIVED here from the rules of the library (api_encode.hip: bytes outside the block's 40 most frequent values > n / 4, on the CM
input, whose histogram is that of the bytes after mRLE and LZP; api_decode.hip: payload * 10 >= size before the BWT * 9, both from the block's header) and
from the reference's coded blocks; nothing is taken from the code under test.
"""
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import datagen

BLOCK_SIZE = 128 * 1024
MIN_LEN, MAX_LEN = 4 * 1024, 96 * 1024
ROUTE_KEEP = 40          # stages.hpp BWT_ROUTE_KEEP
# A third of the tokens get random letters and digits (datagen.text's noise; the digits fold onto the punctuation): plain word-bigram text repeats phrases, LZP
# applies to most pieces of 50 KiB and more, and a fitting block needs the reference to have declined it.
NOISE = 0.35
ALPHABET = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz \n.,;:'!?-", dtype=np.uint8)  # 37 values
assert len(set(ALPHABET.tolist())) == len(ALPHABET) <= ROUTE_KEEP


def _alphabet_map(shift):
    """256 -> at most 37 byte values: letters fold to lower case, everything else spreads over the punctuation; `shift` moves the whole alphabet
    (rows are keyed by byte value: three different sets of rows across a batch, one of them above 127)."""
    m = np.empty(256, dtype=np.uint8)
    for c in range(256):
        ch = bytes([c]).lower()
        k = ALPHABET.tolist().index(ch[0]) if ch[0] in ALPHABET.tolist() else 26 + c % (len(ALPHABET) - 26)
        m[c] = (int(ALPHABET[k]) + shift) & 0xFF
    return m


_MAPS = [_alphabet_map(s) for s in (0, 77, 154)]


def restricted_text(n, seed, shift_index=0):
    """n bytes of Markov text on at most 37 byte values."""
    raw = np.frombuffer(datagen.text(n, seed=seed, chains=64, noise=NOISE), dtype=np.uint8)
    return _MAPS[shift_index % 3][raw].tobytes()


def thresholds(lib, device=0, limit=1 << 16):
    """(c1, c2): the smallest batch sizes at which the library's automatic policy takes the two- and the three-per-CU CM kernels."""
    c = {}
    for k in range(1, limit):
        v = (lib.bz3_hip_cm_variant_for(device, k, 0), lib.bz3_hip_cm_variant_for(device, k, 1))
        assert v[0] == v[1], (k, v)
        c.setdefault(v[0], k)
        if 2 in c:
            break
    assert 1 in c and 2 in c, c
    assert c[2] - 1 == 2 * (c[1] - 1), c
    return c[1], c[2]


def batch_sizes(c1, c2):
    """The three batch sizes (in CM jobs): two per CU, three per CU, more workgroups than fit at once."""
    return {"two_per_cu": c1 + 43, "three_per_cu": c2 + 39, "oversubscribed": 3 * (c1 - 1) + 40}


def parse_header(blk):
    """(model, size_before_bwt or None, payload bytes, header bytes) of a coded block; model -1: stored."""
    if struct.unpack("<i", blk[4:8])[0] == -1:
        return -1, None, len(blk) - 8, 8
    model = blk[8]
    p, lzp, rle = 0, None, None
    if model & 2:
        lzp = struct.unpack("<i", blk[9 + 4 * p : 13 + 4 * p])[0]
        p += 1
    if model & 4:
        rle = struct.unpack("<i", blk[9 + 4 * p : 13 + 4 * p])[0]
        p += 1
    head = 9 + 4 * p
    return model, (lzp if model & 2 else rle if model & 4 else None), len(blk) - head, head


def outside_top(data, keep=ROUTE_KEEP):
    """Bytes of `data` that are not among its `keep` most frequent byte values (ties: the sum does not depend on how they are broken)."""
    h = np.sort(np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256))[::-1]
    return int(h[keep:].sum())


def cm_input_like(oracle, data, model):
    """Bytes with the histogram of the block's CM input: the block after mRLE and LZP where the reference applied them (model bits 4 and 2; the encoder
    runs mRLE first), the block itself where both declined.  The BWT only permutes them."""
    cur = data
    if model & 4:
        cur = oracle.mrle_encode(cur)
    if model & 2:
        n, z = oracle.lzp_encode(cur)
        assert 0 < n < len(cur)
        cur = z
    return cur


class Batch:
    """blocks, kinds ('fit' | 'ord' | 'rand' | 'v128' | 'stored' | 'empty'), want (the reference's coded blocks), and what the counters must show."""

    def __init__(self, blocks, kinds, want, oracle):
        self.blocks, self.kinds, self.want = blocks, kinds, want
        self.n = len(blocks)
        self.jobs = [i for i, d in enumerate(blocks) if len(d) >= 64]
        self.n_jobs = len(self.jobs)
        self.fitting = [i for i in self.jobs if kinds[i] == "fit"]
        self.routed_encode, self.routed_decode = [], []
        self.cm_in_size = {}
        for i in self.jobs:
            model, before, payload, _ = parse_header(want[i])
            assert model >= 0
            cm_in = blocks[i] if model == 0 else cm_input_like(oracle, blocks[i], model)
            n_cm = len(cm_in)
            assert n_cm == (len(blocks[i]) if before is None else before), (i, model, n_cm, before)  # the header's size before the BWT
            self.cm_in_size[i] = n_cm
            if outside_top(cm_in) > n_cm // 4:      # api_encode.hip: outside > n / 4
                self.routed_encode.append(i)
            if payload * 10 >= n_cm * 9:            # api_decode.hip: cm_in_size * 10 >= size_before_bwt * 9
                self.routed_decode.append(i)

    def given_up_cap(self, routed):
        """Blocks the row-cache kernels may hand back at most: every job that is neither fitting nor routed."""
        return self.n_jobs - len(self.fitting) - routed

    def flip_target(self, c1):
        """A fitting block with an index between c1 and n_jobs, and the offset of a byte in the middle of its payload."""
        i = next(i for i in self.fitting if c1 <= i < self.n_jobs)
        _, _, payload, head = parse_header(self.want[i])
        return i, head + payload // 2

    def check_distinct(self, stride):
        """Every block differs from every other; spelled out for neighbours and for blocks `stride` (one per CU) apart, which share a CU when the dispatch is
        undisturbed."""
        assert len(set(self.blocks)) == self.n
        for i in range(self.n - 1):
            assert self.blocks[i] != self.blocks[i + 1], i
        for i in range(self.n):
            for j in range(i + stride, self.n, stride):
                assert self.blocks[i] != self.blocks[j], (i, j)


def _length(i):
    """4 KiB .. 96 KiB, scattered over the indices, more short blocks than long ones (mean ~35 KiB): workgroups end at very different times."""
    u = ((i * 40503 + 12345) % 9973) / 9972.0
    return MIN_LEN + int((MAX_LEN - MIN_LEN) * u * u)


def _kinds(n_jobs, c1):
    n = n_jobs + 2
    kinds = ["fit" if i % 10 >= 3 else "ord" for i in range(n)]
    for i in (3, n // 4 + 1, c1 + 7, n - 7):
        kinds[i] = "rand"
    for i in (n // 3, c1 + 21):
        kinds[i] = "v128"
    kinds[19], kinds[23] = "stored", "empty"
    assert len({3, n // 4 + 1, c1 + 7, n - 7, n // 3, c1 + 21, 19, 23}) == 8 and n - 2 - kinds.count("ord") - 6 >= 0.6 * n_jobs
    return kinds


def build_batch(n_jobs, c1, encode_block, oracle, seed=1, workers=16):
    """encode_block(data, block_size) -> coded bytes of the REAL reference (Bz3(ref.lib).encode_block(...)[2]); called from at most 16 threads."""
    shakespeare = datagen.shakespeare()
    kinds = _kinds(n_jobs, c1)
    n = len(kinds)
    lens = [_length(i) for i in range(n)]
    # one pool of Markov text, cut into pieces three times over: block i takes the next piece of the cursor of ITS alphabet (i % 3), so no two blocks hold
    # the same bytes (same alphabet: different pieces; different alphabets: different byte values)
    need = max(sum(L for i, (L, k) in enumerate(zip(lens, kinds)) if k == "fit" and i % 3 == m) for m in range(3))
    pool = np.frombuffer(datagen.text(need + need // 3 + 8 * MAX_LEN, seed=1000 * seed + n_jobs, chains=2048, noise=NOISE), dtype=np.uint8)
    rng = np.random.Generator(np.random.PCG64(seed * 7919 + n_jobs))
    cursor = [0, 0, 0]

    def fitting(i):
        L, m = lens[i], i % 3
        assert cursor[m] + L <= len(pool), "the pool of Markov text ran out: too many candidates were refused"
        piece = pool[cursor[m] : cursor[m] + L]
        cursor[m] += L
        return _MAPS[m][piece].tobytes()

    def ordinary(i):
        L = lens[i]
        o = (i * 37123 + seed * 101) % (len(shakespeare) - 2 * MAX_LEN)
        if i % 3 == 1:  # a repeated passage: LZP applies
            body = L * 2 // 3
            return shakespeare[o : o + body] + shakespeare[o + 100 : o + 100 + (L - body)]
        if i % 3 == 2:  # a run and a few escape bytes: mRLE applies
            run = 300 + i % 200
            return shakespeare[o : o + L - run - 4] + b"\xf2" * (1 + i % 4) + b"q" * run
        return shakespeare[o : o + L]

    blocks = []
    for i, k in enumerate(kinds):
        if k == "fit":
            blocks.append(fitting(i))
        elif k == "ord":
            blocks.append(ordinary(i))
        elif k == "rand":
            blocks.append(bytes(rng.integers(0, 256, size=max(lens[i], 8192), dtype=np.uint8)))
        elif k == "v128":
            blocks.append(bytes((rng.integers(0, 128, size=max(lens[i], 32768)) + 64 + i % 64).astype(np.uint8)))
        elif k == "stored":
            blocks.append(bytes(rng.integers(97, 123, size=41, dtype=np.uint8)))
        else:
            blocks.append(b"")
    with ThreadPoolExecutor(max_workers=min(workers, 16)) as ex:
        want = list(ex.map(lambda d: encode_block(d, BLOCK_SIZE), blocks))
        for attempt in range(8):  # a fitting candidate on which LZP or mRLE applied is replaced by the next piece of the pool
            redo = [i for i, k in enumerate(kinds) if k == "fit" and want[i][8] != 0]
            if not redo:
                break
            for i in redo:
                blocks[i] = fitting(i)
            for i, w in zip(redo, ex.map(lambda i: encode_block(blocks[i], BLOCK_SIZE), redo)):
                want[i] = w
        else:
            raise AssertionError("fitting blocks with model byte 0 could not be found")
    return Batch(blocks, kinds, want, oracle)
