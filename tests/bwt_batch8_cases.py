"""Inputs shared by tests/test_bwt_batch8_emu.py and tests/test_gpu_front_small.py: nine jobs for one bz3_hip_debug_bwt_many call (a run of eight and
a run of one) that take different paths of the suffix sorter, and forty small blocks for the encoder's front end.  Built once, never changed."""
import numpy as np

import datagen

_NINE = []
_WANT = {}


def nine_jobs():
    """[(name, bytes)]: n = 2 and 3 (no second tile, no second wave); 513 (a tile + 1), 4,097 (a radix tile + 1) and 65,537 bytes of text (done after pass 0 or
    one more window); one byte value 70,000 times and a period-7 string of 100,000 bytes (a list overflows at pass 0: the deep path, several doubling rounds);
    300 KB of text (the largest: it sets every grid's extent); 50 KB of random bytes (all 256 values, done after pass 0)."""
    if not _NINE:
        t = datagen.text(400000, seed=8)
        rng = np.random.default_rng(8)
        _NINE.extend([
            ("n2", b"ba"),
            ("n3", b"aba"),
            ("tile513", t[4242 : 4242 + 513]),
            ("n4097", t[100 : 100 + 4097]),
            ("n65537", t[1000 : 1000 + 65537]),
            ("run70000", b"q" * 70000),
            ("period7", (b"abcdefg" * 14286)[:100000]),
            ("text300k", t[50000:350000]),
            ("random50k", bytes(rng.integers(0, 256, size=50000, dtype=np.uint8))),
        ])
    return _NINE


def nine_expected(oracle):
    """name -> (index, bytes) of the job alone; the oracle alone decides it."""
    if not _WANT:
        for name, b in nine_jobs():
            _WANT[name] = oracle.bwt(b)
    return _WANT


def rotated(jobs, by):
    return jobs[by:] + jobs[:by]


def check_nine(g, oracle, jobs, what):
    want = nine_expected(oracle)
    rc, got = g.bwt_many([b for _, b in jobs])
    assert rc == 0, what
    assert len(got) == len(jobs), what
    for (name, _), r in zip(jobs, got):
        assert r == want[name], (name, what)


_FORTY = {}


def forty_blocks(oracle, text):
    """40 blocks of 64 KiB to 1 MiB (and three stored ones of fewer than 64 bytes) for ONE batch: text that LZP shortens (plain, and a passage repeated), text LZP
    declines (independently drawn words), random bytes, a run of one byte value.  (blocks, block size of the states, the oracle's coded bytes per block)."""
    if not _FORTY:
        bs = 1 << 20
        distinct = []
        for i in range(10):
            if i in (2, 7):  # LZP applies: the same 60,000 bytes five times over
                distinct.append(text[i * 50000 : i * 50000 + 60000] * 5 + text[900000:930000])
            elif i == 3:
                distinct.append(b"x" * 41)  # stored
            elif i == 5:
                distinct.append(datagen.random_bytes(100000, seed=5))
            elif i == 8:
                distinct.append(b"\x00" * (64 * 1024 + 1))
            elif i == 9:
                distinct.append(text[1000:1063])  # stored: 63 bytes
            elif i in (1, 4):  # LZP is declined: words drawn independently from a vocabulary repeat, but never for as long as a match has to be
                rng = np.random.default_rng(40 + i)
                vocab = [bytes(rng.integers(97, 123, size=rng.integers(2, 9), dtype=np.uint8)) for _ in range(3000)]
                distinct.append(b" ".join(vocab[j] for j in rng.integers(0, 3000, size=12000 * i)))
            else:  # text of 64 KiB and of 1 MiB (LZP applies)
                distinct.append(text[:64 * 1024] if i == 0 else (text[400000:460000] * 18)[:bs])  # (1 MiB that LZP cuts to a sixteenth: the CM stage sets a test's pace)
        want = [oracle.encode_block(d, bs)[2] for d in distinct]
        model = [w[8] if w[4:8] != b"\xff" * 4 else None for w in want]  # None: stored
        assert model[3] is None and model[9] is None
        assert model[2] & 2 and model[7] & 2, "LZP was meant to apply to the repeated passages"
        assert model[0] & 2 and model[6] & 2 and not model[1] & 2 and not model[4] & 2, "LZP was meant to apply to the text and to be declined for the drawn words"
        order = [(3 * k) % 10 for k in range(40)]
        _FORTY["v"] = ([distinct[j] for j in order], bs, [want[j] for j in order])
    return _FORTY["v"]
