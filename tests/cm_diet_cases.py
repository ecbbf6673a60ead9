"""Inputs for the per-byte paths of the guess-ahead CM decoder (cm.hip cm_decode_block_sync): tests/test_cm_decoder_diet_emu.py runs them through the
emulated kernels, tests/test_gpu_cm_decoder_diet.py through the hardware's.  Expected bytes are the oracle's: a block is coded by oracle.cm_encode, decoded
by the product and compared with the plaintext; a truncated stream is compared with oracle.cm_decode of the same stream.

Families (name -> bytes):
  lengths    n = 1 .. 6 and 63, 64, 65: the loops handle two bytes per trip and must end in either half; n = 1 meets no barrier 1.
  runs       runs of length 1 .. 6 of two alternating values, starting at an even and at an odd position: the run flag switches (three equal bytes behind the
             one being evaluated) in both halves of the trip, and the wrong guess at the end of a run falls right behind the switch (run 4), before it
             (run 3) and elsewhere.
  values     byte values whose tree paths lie in each model wave and in the spare lanes (node-to-lane map of round 4), as pairs (guess g, real byte c) over all
             100 ordered pairs: g's wave updates and c's does not, the reverse, both (same wave) and neither (seen from the other waves).
  checked    4 KiB of skewed random bytes: renormalisations fall on every tree level (asserted with the Python model of tests/cm_cases.py).
  rows       8 KiB of runs over 48 previous-byte values (the emulator's 40-slot cache fetches and evicts rows on the repair path without giving up), 64 KiB
             over 70 values for the 56 rows of the three-per-CU decoder, and 8 KiB of uniformly random bytes, which every row cache gives up.
"""
import numpy as np

import cm_cases as cc

VALUES = [0x00, 0x3F, 0x40, 0x7D, 0x7E, 0x7F, 0x80, 0xBF, 0xC0, 0xFF]
LENGTHS = [1, 2, 3, 4, 5, 6, 63, 64, 65]
TRUNCATIONS = [0, 1, 3, 4, 5]   # and the middle of the stream
_CACHE = {}


def skewed(seed, n):
    """Skewed random bytes over 24 values, repeats allowed (so right and wrong guesses both occur)."""
    rng = np.random.default_rng(seed)
    v = (rng.permutation(200)[:24] + 30).astype(np.uint8)
    p = 1.0 / np.arange(1, 25)
    return bytes(v[rng.choice(24, size=n, p=p / p.sum())])


def lengths():
    src = skewed(41, 80)
    return {"len%d" % n: src[:n] for n in LENGTHS}


def runs():
    out = {}
    for run in range(1, 7):
        for start in (0, 1):
            body = (bytes([0x61]) * run + bytes([0x20]) * run) * 6
            out["run%d_start%d" % (run, start)] = bytes([0x74]) * start + body + bytes([0x61])
    return out


def values():
    """Every ordered pair (g, c) of VALUES as `g g c`: byte 2 of the triple is guessed right (the update of g runs in g's wave), byte 3 is guessed g and is c."""
    seq = bytearray()
    for g in VALUES:
        for c in VALUES:
            seq += bytes([g, g, c])
    return {"values_pairs": bytes(seq), "values_pairs_twice": bytes(seq) * 2}


def checked():
    return {"checked_skewed4k": skewed(42, 4096)}


def rows_runs(nvalues, run, n):
    return bytes(1 + (i // run) % nvalues for i in range(n))


def rows(gpu=False):
    out = {"rows48_8k": rows_runs(48, 12, 8192)}
    if gpu:
        out["rows70_64k"] = rows_runs(70, 32, 65536)
    return out


def random8k():
    return bytes(np.random.default_rng(43).integers(0, 256, size=8192, dtype=np.uint8))


def plain_families(gpu=False):
    if gpu not in _CACHE:
        _CACHE[gpu] = {"lengths": lengths(), "runs": runs(), "values": values(), "checked": checked(), "rows": rows(gpu)}
    return _CACHE[gpu]


def truncated_streams(oracle):
    """[(stream, n, expected bytes)]: the coded stream of 600 skewed bytes cut after 0, 1, 3, 4, 5 bytes and in the middle; bytes past the end read as -1 and
    push `code` below `low` (the walker's `inside` test and the checked walk).  Expected: the oracle's decode of the same cut stream."""
    if "trunc" not in _CACHE:
        d = skewed(42, 600)
        coded = oracle.cm_encode(d)
        out = []
        for cut in TRUNCATIONS + [len(coded) // 2]:
            n = len(d) if cut > 5 else 160   # (behind a cut of a few bytes everything is the -1 fill: 160 bytes of it say what 600 would)
            out.append((coded[:cut], n, oracle.cm_decode(coded[:cut], n)))
        _CACHE["trunc"] = out
    return _CACHE["trunc"]


def renorm_levels(data):
    """The tree levels (bit positions 0 .. 7) at which the coder renormalised while coding `data` (the Python model of cm_cases, held against the oracle there)."""
    _, e = cc.model_encode(data)
    return {t.k for t in e.trace if t.emitted}


def check_preconditions(oracle):
    """What the families are named for, without a kernel."""
    fam = plain_families(True)
    d = fam["checked"]["checked_skewed4k"]
    coded, _ = cc.model_encode(d)
    assert coded == oracle.cm_encode(d)
    assert renorm_levels(d) == set(range(8))
    up, directory = cc.decoder_rows(fam["rows"]["rows48_8k"], 40, *cc.BUDGET[9])
    assert not up and directory.recycled > 0 and len(directory.reloaded) == 48      # fetched, evicted and fetched again; kept
    for size in (56, 96):
        assert not cc.decoder_rows(fam["rows"]["rows48_8k"], size, *cc.BUDGET[2])[0]
    up, directory = cc.decoder_rows(fam["rows"]["rows70_64k"], 56, *cc.BUDGET[2])
    assert not up and directory.recycled > 0 and len(directory.reloaded) == 70
    assert not cc.decoder_rows(fam["rows"]["rows70_64k"], 96, *cc.BUDGET[1])[0]
    for mode in (9, 1, 2):
        assert cc.expected_given_up(random8k(), "dec", mode) == 1
    # the run flag switches in either half of the loop trip: at an odd and at an even byte index
    parity = set()
    for name, r in fam["runs"].items():
        f = cc.flags_by_definition(r)
        parity |= {i & 1 for i in range(1, len(f)) if f[i] and not f[i - 1]}
    assert parity == {0, 1}


def run_plain(lib, oracle, mode, family, gpu=False):
    """Decode of every block of a family in CM mode `mode` through the single-job hook; the given-up counter must not move."""
    import bzip3_amd

    g = bzip3_amd.StageApi(lib)
    try:
        assert lib.bz3_hip_set_cm_mode(mode) == 0
        for name, d in plain_families(gpu)[family].items():
            coded = oracle.cm_encode(d)
            n0 = lib.bz3_hip_cm_blocks_given_up()
            assert g.cm_decode(coded, len(d)) == d, (name, mode)
            assert lib.bz3_hip_cm_blocks_given_up() == n0, (name, mode)
    finally:
        lib.bz3_hip_set_cm_mode(-1)


def run_truncated(lib, oracle, mode):
    import bzip3_amd

    g = bzip3_amd.StageApi(lib)
    try:
        assert lib.bz3_hip_set_cm_mode(mode) == 0
        for stream, n, want in truncated_streams(oracle):
            assert g.cm_decode(stream, n) == want, (len(stream), mode)
    finally:
        lib.bz3_hip_set_cm_mode(-1)


def run_given_up(lib, oracle, mode):
    """Uniformly random bytes: a row-cache decoder gives the block up (status word 1, counted) and the full-model kernel decodes it again: the same bytes."""
    import bzip3_amd

    g = bzip3_amd.StageApi(lib)
    d = random8k()
    coded = oracle.cm_encode(d)
    try:
        assert lib.bz3_hip_set_cm_mode(mode) == 0
        n0 = lib.bz3_hip_cm_blocks_given_up()
        assert g.cm_decode(coded, len(d)) == d, mode
        assert lib.bz3_hip_cm_blocks_given_up() - n0 == (1 if mode else 0), mode
    finally:
        lib.bz3_hip_set_cm_mode(-1)


FAMILIES = ("lengths", "runs", "values", "checked", "rows")


PARTS = ("short", "long", "ends")


def run_part(lib, oracle, mode, part):
    """A third of the above in one go (the stalled-wave subprocesses of the emulator test)."""
    if part == "short":
        for family in ("lengths", "runs", "values"):
            run_plain(lib, oracle, mode, family)
    elif part == "long":
        for family in ("checked", "rows"):
            run_plain(lib, oracle, mode, family)
    else:
        run_truncated(lib, oracle, mode)
        run_given_up(lib, oracle, mode)
