"""Inputs aimed at the geometry of the LZP encoder (bzip3_amd/csrc/lzp.hip): the serial driver's event cap and bitmap windows, the
re-flagging of next[s] behind a match, chain compression, the length tokens, the escape rule of the emission and the edges of the main
loop.  Seeded and deterministic; shared by tests/test_lzp_cases.py (oracle, emulator) and tests/test_gpu_lzp_cases.py (device).
DESIGN.md ("What the LZP cases pin") says what each case is for.

Vocabulary: a position p is VISITED unless it lies inside a match (its start excepted); the table slot of hash(in[p-4..p-1]) holds the last
visited position with that hash; the PRE-TEST compares in[p..p+3] and in[p+36..p+39] with the candidate's (src/libbz3.c:143-144)."""
import functools

import numpy as np

import datagen

LZ_MIN = 40
ESC = 0xF2
EV_CAP = 2048            # lzp.hip LZ_EV_CAP: the tests check it against the hook's report
WINDOW = 131072          # lzp.hip LZ_WIN_WORDS * 32
ROUND = 4096             # bytes one workgroup round of the measuring loop covers (4 x LZ_DRV)
LONG_LENGTHS = (30000, 20000, 9000, 40 + 8196, 40 + 8195, 40 + 8192, 40 + 8188, 40 + 4100, 40 + 4099, 40 + 4097, 40 + 4096, 40 + 4092)
LASTMATCH_D = tuple(range(-2, 5))
FARFLAG_PARAMS = ((140000, 1), (3000, 1), (3000, 300))
ENDS_SMALL = tuple(range(70, 141))
ENDS_LINKS = tuple(range(8195, 8201))  # m = n - 4 <= 2 * RS_TILE (8192) takes k_lzp_links, above it the binned link build


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _letters(rng, k):
    return bytes(rng.integers(97, 123, size=k, dtype=np.uint8))


def lz_hash(ctx):
    """Table slot of a big-endian 4-byte context (int, or a numpy array of them)."""
    return ((ctx >> 15) ^ ctx ^ (ctx >> 3)) & 0x3FFFF


def ctx_of(b):
    return int.from_bytes(b, "big")


def main_end(n):
    return n - 72


def pretest_passes(data, matches, lo, hi):
    """Positions of [lo, hi) at which the encoder's 8-byte pre-test passes, replayed over the table of an encoder that takes exactly
    `matches` ((start, length) pairs, ascending).  Pure Python: meant for a few hundred thousand positions."""
    tab = {}
    me = main_end(len(data))
    out = []
    mi, p = 0, 4
    while p < min(hi, me):
        h = lz_hash(ctx_of(data[p - 4 : p]))
        c = tab.get(h, 0)
        tab[h] = p
        if c > 0 and p >= lo and data[p : p + 4] == data[c : c + 4] and data[p + 36 : p + 40] == data[c + 36 : c + 40]:
            out.append(p)
        if mi < len(matches) and matches[mi][0] == p:
            p += matches[mi][1]
            mi += 1
        else:
            p += 1
    return out


# ---- capcut ---------------------------------------------------------------------------------------------------------------------
def _capcut_build(records, seed):
    rng = _rng(seed)
    phrase = _letters(rng, 400)
    recs = b"".join(b"HASHABCD" + _letters(rng, 32) + b"WXYZ" for _ in range(records))
    data = phrase + recs + b"#" + phrase + _letters(rng, 300)
    return data, len(phrase) + len(recs) + 1 + 4  # the phrase's second copy is matched from its fifth byte on


@functools.lru_cache(maxsize=None)
def capcut():
    """(data, match position): 2500 records that share a context and pass the pre-test but fail at 40 -- more events than one driver
    iteration resolves -- and then, in the same bitmap window, a real match."""
    return _capcut_build(2500, 31)


@functools.lru_cache(maxsize=None)
def capcut_exact(events):
    """The same with exactly `events` pre-test-passing positions in front of the match."""
    # the first record has no predecessor and a few records pass at a second position by chance: count over the longest candidate once
    # (the records are a prefix of it), then confirm the record counts that fit
    # (a record that passes twice makes the count skip a value, and a record may take the table slot of the phrase's context: then another seed)
    for seed in range(32, 48):
        data, mpos = _capcut_build(events + 1, seed)
        passes = np.array(pretest_passes(data, [], 4, mpos))
        for records in range(events + 1, events - 200, -1):
            if int((passes < 400 + 44 * records).sum()) == events:
                data, mpos = _capcut_build(records, seed)
                got = pretest_passes(data, [], 4, mpos + 1)
                if len(got) == events + 1 and got[-1] == mpos:
                    return data, mpos
    raise AssertionError("capcut_exact(%d): no record count gives that many events" % events)


# ---- farflag --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _quiet_context_bytes():
    """Byte values x whose context xxxx hashes to a slot that no context of four letters shares: the filler cannot take the slot."""
    a = np.arange(97, 123, dtype=np.uint32)
    ctx = ((a[:, None, None, None] << 24) | (a[None, :, None, None] << 16) | (a[None, None, :, None] << 8) | a[None, None, None, :]).reshape(-1)
    taken = np.zeros(1 << 18, dtype=bool)
    taken[lz_hash(ctx)] = True
    quiet = [x for x in range(1, 256) if not (97 <= x <= 122) and x != ESC and not taken[lz_hash(x * 0x01010101)]]
    assert len({lz_hash(x * 0x01010101) for x in quiet}) == len(quiet)
    return quiet


@functools.lru_cache(maxsize=None)
def farflag(distance, depth):
    """(data, [final positions]).  For 12 contexts c_k: a region R_k around c_k (visited), c_k + B1_k (visited), `depth` copies of every R_k
    (swallowed by matches: the positions behind c_k in them are never visited), `distance` letters, c_k + B1_k again.  The hash predecessor of
    the last position behind c_k is a swallowed one with another body -- the static pass does not flag it --, its candidate is the visited
    c_k + B1_k, `depth` swallowed ancestors further back, and the reference takes a match there.  Only the re-flagging of next[s] behind the
    matches of the copies brings the driver to it."""
    rng = _rng(41 + depth)
    cs = [bytes([x]) * 4 for x in _quiet_context_bytes()[:12]]
    assert len(cs) == 12
    regions = [_letters(rng, 30) + c + _letters(rng, 50) for c in cs]
    bodies = [_letters(rng, 60) for _ in cs]
    parts = list(regions)
    parts += [c + b for c, b in zip(cs, bodies)]
    parts += regions * depth
    parts.append(_letters(rng, distance))
    head = b"".join(parts)
    finals, tail = [], []
    at = len(head)
    for k in reversed(range(12)):  # the other way round than above: every final occurrence is a match of its own
        finals.append(at + 4)
        tail.append(cs[k] + bodies[k])
        at += 64
    return head + b"".join(tail) + _letters(rng, 120), finals


# ---- long -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_case():
    """A 30000-byte text and copies of its head whose matches have exactly the lengths LONG_LENGTHS (every copy is matched from its fifth
    byte against the copy before it, which is longer), each followed by a distinct byte and 20 letters; a last copy runs into the end of the
    block, where main_end cuts its match."""
    rng = _rng(51)
    src = b"\x7f\x7e\x7d\x7c" + datagen.shakespeare()[200000:230000]  # a context of its own in front: a copy's candidate is the copy before it
    parts = [src, b"\x80", _letters(rng, 19), b"a"]  # (the letter in front of a copy is its own too: no match begins before the fifth byte)
    for i, length in enumerate(LONG_LENGTHS):
        parts += [src[: length + 4], bytes([0x81 + i]), _letters(rng, 19), bytes([98 + i])]
    parts.append(src[:3000])
    return b"".join(parts)


# ---- lens -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lens():
    """One record per prefix length k of a 700-letter string behind a fixed context, closed by two breaker bytes: record k matches record
    k - 1 over k - 1 bytes, so every match length from 40 to 40 + 2 * 254 + 6 occurs -- every shape of the length token around its
    254-steps.  The contexts in front of a record's letters hold its breakers, so a breaker value may not come back while its context and
    letters are in use (the match would begin a byte or two early, with some other length): the records come in three groups of at most
    200, each with a context and letters of its own and breakers that are distinct within it; a group begins with the prefix length the
    one before it ended with, which has nothing to match yet."""
    rng = _rng(61)
    marks = [bytes([x]) for x in _quiet_context_bytes()[:3]]
    breakers = [x for x in range(1, 256) if not (97 <= x <= 122) and x not in (ESC, 254, 255) and bytes([x]) not in marks]
    out, last = [], LZ_MIN + 2 * 254 + 7
    slots = [{lz_hash(ctx_of(m * 4))} for m in marks] + [set()]  # (nor may two of these contexts of a group share a table slot)
    for g, k0 in enumerate((36, 236, 436)):
        body = _letters(rng, 700)
        ks = range(k0 - (g > 0), min(k0 + 200, last + 1))
        for i, k in enumerate(ks):
            closes = k == ks[-1]  # the breakers of a group's last record stand in front of the next group's context
            b2 = breakers[210 + g] if closes else breakers[i]
            behind = marks[g + 1] if closes and g < 2 else marks[g]
            for b1 in breakers[(i + 77) % len(breakers) :] + breakers:
                seam = body[k - 2 : k] + bytes([b1, b2]) + behind * 3
                new = {lz_hash(ctx_of(seam[j : j + 4])) for j in range(4)}
                if len(new) == 4 and not (new & slots[g + closes]):
                    break
            else:
                raise AssertionError("lens: no breaker pair left for record %d" % k)
            slots[g + closes] |= new
            out.append(marks[g] * 4 + body[:k] + bytes([b1, b2]))
    return b"".join(out) + _letters(rng, 100)  # (the last match ends in front of the main loop's end)


# ---- collide --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def collide():
    """(data, [(second body position, closing 0xF2 position)]).  20 pairs of four-letter contexts A != B with one hash and other last three
    letters.  The body behind B is matched against the body behind A: a match through a colliding context, so the contexts B[1:4] + body[0]
    ... inside it are never visited (behind A they were other contexts).  A closing 0xF2 behind that very context then finds an empty
    slot -- no 0xFF behind it -- although its hash predecessor exists: the one place where the emission must ask lz_candidate, not prev."""
    rng = _rng(71)
    a = np.arange(97, 123, dtype=np.uint32)
    ctx = ((a[:, None, None, None] << 24) | (a[None, :, None, None] << 16) | (a[None, None, :, None] << 8) | a[None, None, None, :]).reshape(-1)
    h = lz_hash(ctx)
    order = np.argsort(h, kind="stable")
    hs, cs = h[order], ctx[order]
    pairs, used = [], set()
    while len(pairs) < 20:
        i = int(rng.integers(0, len(cs) - 1))
        A, B = int(cs[i]), int(cs[i + 1])
        if hs[i] != hs[i + 1] or (A & 0xFFFFFF) == (B & 0xFFFFFF) or int(hs[i]) in used:
            continue
        used.add(int(hs[i]))
        pairs.append((A.to_bytes(4, "big"), B.to_bytes(4, "big")))
    out, marks, at = [], [], 0
    for A, B in pairs:
        body = _letters(rng, 60)
        piece = _letters(rng, 100) + A + body + _letters(rng, 50) + B
        second = at + len(piece)
        piece += body + _letters(rng, 50) + B[1:4] + body[0:1]
        marks.append((second, at + len(piece)))
        piece += b"\xf2" + _letters(rng, 30)
        out.append(piece)
        at += len(piece)
    return b"".join(out) + _letters(rng, 100), marks


# ---- ends -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ends():
    """{name: data}: blocks around the size LZP declines below (72, main_end = n - 72) with escapes in the tail loop, and blocks around
    the size at which the link build changes kernels."""
    t = datagen.shakespeare()
    c = {}
    for n in ENDS_SMALL:
        c["f2-%d" % n] = (b"abcdefghij\xf2" * 20)[:n]
        c["text-%d" % n] = (t[40:75] * 8)[: n - 3] + b"\xf2\xf2\xf2"
    for n in ENDS_LINKS:
        c["links-%d" % n] = (t[:2700] * 4)[:n]
    return c


# ---- lastmatch ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lastmatch(d):
    """(data, p): a 60-byte phrase twice, the second copy matchable from p = main_end - 37 - d.  The length loop stops below main_end, so
    p = main_end - 37 is the last position that can reach 40 bytes: a match for d >= 0, none for d < 0.  (Another phrase is matched
    early in the block, so that LZP applies either way.)"""
    rng = _rng(81)
    phrase, early = _letters(rng, 60), _letters(rng, 80)
    head = _letters(rng, 20) + early + _letters(rng, 30) + early + _letters(rng, 50) + phrase + _letters(rng, 200)
    data = head + phrase + _letters(rng, 53 + d)
    p = len(head) + 4
    assert p == main_end(len(data)) - 37 - d
    return data, p


def stage_cases():
    """{name: data} of every case but `ends`: LZP applies to all of them."""
    c = {"capcut": capcut()[0], "long": long_case(), "lens": lens(), "collide": collide()[0]}
    for e in (EV_CAP - 1, EV_CAP, EV_CAP + 1):
        c["capcut-%d" % e] = capcut_exact(e)[0]
    for dist, depth in FARFLAG_PARAMS:
        c["farflag-%d-%d" % (dist, depth)] = farflag(dist, depth)[0]
    for d in LASTMATCH_D:
        c["lastmatch%+d" % d] = lastmatch(d)[0]
    return c


STAGE_NAMES = ("capcut", "capcut-2047", "capcut-2048", "capcut-2049", "collide", "farflag-140000-1", "farflag-3000-1", "farflag-3000-300", "lens",
               "long") + tuple("lastmatch%+d" % d for d in LASTMATCH_D)


def windows_of(n):
    """Bitmap windows the driver walks when nothing is flagged: it starts at position 4 and steps to the next multiple of 4096 words."""
    return -(-main_end(n) // WINDOW)


# ---- what the tests on the emulator and on the device share -----------------------------------------------------------------------
def oracle_facts(oracle, data):
    """(size, bytes, matches, end_pos) of the oracle's encoder: end_pos is where its main loop stops."""
    n, z = oracle.lzp_encode(data)
    m = oracle.lzp_matches(data)
    end = 0
    if len(data) >= 72:
        end = max([main_end(len(data))] + [p + l for p, l in m[-1:]])
    return n, z, m, end


def check_encoder(g, oracle, name, data):
    """One stage call: the oracle's bytes, and the driver's record against the oracle's match list.  Returns the record."""
    n, z, m, end = oracle_facts(oracle, data)
    gn, gz, st = g.lzp_encode_stats(data)
    assert (st["event_cap"], st["window_positions"]) == (EV_CAP, WINDOW), name
    assert gn == n, (name, gn, n, st)
    assert gz == z, name
    if n > 0:  # (where the oracle gives up for size its loop stops early; the driver's does not)
        assert (st["n_matches"], st["end_pos"]) == (len(m), end), (name, st, len(m), end)
    elif len(data) < 72:
        assert (st["n_matches"], st["end_pos"], st["iterations"], st["evaluated"]) == (0, 0, 0, 0), (name, st)
    if name == "capcut":
        assert st["evaluated"] > EV_CAP, st
        assert st["iterations"] >= windows_of(len(data)) + st["n_matches"] + 1, st  # the window was cut at the cap and resumed
    if name == "farflag-140000-1":
        assert st["iterations"] >= 2, st
    return st


def check_decoder(g, oracle):
    """k_lzp_decode works in trips of 16 KiB with one 16-byte access per lane each way (lzp.hip): several trips, 0xF2 bytes at every
    alignment inside the 16 bytes of a lane, a ragged last lane, outputs capped at awkward places (the decoder stops AT the cap,
    :211), and streams that are not LZP output at all -- always the oracle's (count, bytes).  Then the coded `lens` and `long` cases:
    chained 254 tokens and copies longer than a trip, whole, capped one byte short and cut in half."""
    rng = np.random.default_rng(17)
    t = datagen.shakespeare()
    body = bytearray((t[20000:26000] * 4 + t[40000:52000] + t[20000:23000]) * 2)  # repeats: LZP applies
    for k in rng.integers(0, len(body), size=400):
        body[int(k)] = 0xF2  # escapes all over, at every offset modulo 16
    data = bytes(body)
    nlz, lz = oracle.lzp_encode(data)
    assert 0 < nlz == len(lz) < len(data) - 8
    for cap in (len(data) + 100, len(data), len(data) - 1, 32768 + 7, 16384 + 3, 16384, 16383, 4000, 17, 5):
        assert g.lzp_decode(lz, cap) == oracle.lzp_decode(lz, cap), cap
    for cut in (len(lz) - 1, len(lz) // 2, 16384 + 5, 4):  # truncated streams
        assert g.lzp_decode(lz[:cut], len(data) + 100) == oracle.lzp_decode(lz[:cut], len(data) + 100), cut
    for seed in range(3):  # arbitrary bytes with many escapes: matches into garbage, lengths running past the cap
        r2 = np.random.default_rng(100 + seed)
        junk = bytes(r2.choice(np.frombuffer(b"ab\xf2\xf2\xff\xfe\x00q", dtype=np.uint8), size=40000))
        for cap in (60000, 33000, 1000):
            assert g.lzp_decode(junk, cap) == oracle.lzp_decode(junk, cap), (seed, cap)
    for name, data in (("lens", lens()), ("long", long_case())):
        nlz, lz = oracle.lzp_encode(data)
        assert 0 < nlz == len(lz) < len(data) - 8, name
        assert g.lzp_decode(lz, len(data)) == (len(data), data), name
        for cap in (len(data) - 1, len(data) // 2):
            assert g.lzp_decode(lz, cap) == oracle.lzp_decode(lz, cap), (name, cap)
        assert g.lzp_decode(lz[: len(lz) // 2], len(data)) == oracle.lzp_decode(lz[: len(lz) // 2], len(data)), name
