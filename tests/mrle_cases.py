"""Inputs aimed at the geometry of the mRLE filter (bzip3_amd/csrc/mrle.hip): 16 bytes per lane, 1,024 per wave, 4,096 per tile, 1,024 tiles
per chunk of the three spine kernels, and the `r % 255` rule of the length bytes.  Seeded and deterministic; shared by tests/test_mrle_cases.py
(oracle, preconditions, emulator) and tests/test_gpu_mrle_cases.py (device).  DESIGN.md ("What the mRLE cases pin") says what each family is for.

An encoder case is (name, input bytes); a decoder case is (name, stream bytes, outlen, maxin).  What a case is built to hit stands in
INTENT[name]; `precondition_enc` / `precondition_dec` prove from a small numpy model of the emit rule (`Model`, `DecodeModel`) and from the
oracle's output that the case does hit it.  The model itself is held against the oracle on every case."""
import functools

import numpy as np

LANE = 16
WAVE = 1024
T = 4096                 # mrle.hip MR_TILE
C = 1024 * T             # bytes one chunk of a spine kernel covers
FILL = (0x61, 0x62)      # the filler: these two bytes in turn -- no runs, a head at every position, neither value ever flagged
V = 0x7A                 # the value of most runs
INTENT = {}


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def filler(n):
    return np.tile(np.array(FILL, dtype=np.uint8), n // 2 + 1)[:n]


def build(n, runs):
    """n bytes of filler with the runs [(position, length, value)] laid over them."""
    a = filler(n)
    for p, ln, v in runs:
        assert 0 <= p and p + ln <= n
        a[p : p + ln] = v
    return a


def coded_run(ln):
    """Bytes a flagged run of ln takes: the symbol, an 0xFF per full 255 in front of the last byte, the last length byte."""
    return 1 + -(-ln // 255)


# ---- the model -------------------------------------------------------------------------------------------------------------------
class Model:
    """The closed form of mrlec (mrle.hip's header) over a whole input: r, head, last, gain, flagged, emitted bytes per position."""

    def __init__(self, data):
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        n = len(a)
        idx = np.arange(n, dtype=np.int64)
        head = np.ones(n, dtype=bool)
        head[1:] = a[1:] != a[:-1]
        last = np.ones(n, dtype=bool)
        last[:-1] = head[1:]
        r = idx - np.maximum.accumulate(np.where(head, idx, 0))
        ff = (r > 0) & (r % 255 == 0)
        w = np.where(head, -1, (r % 255 != 0).astype(np.int64))
        self.a, self.n, self.head, self.last, self.r, self.ff = a, n, head, last, r, ff
        self.gain = np.bincount(a, weights=w, minlength=256).astype(np.int64)
        self.flagged = self.gain > 0
        fl = self.flagged[a]
        self.cnt = np.where(fl, head.astype(np.int64) + ff + last, 1)

    def bitmap(self):
        return bytes(np.packbits(self.flagged, bitorder="little"))

    def stream(self):
        """The encoder's whole output."""
        a, fl = self.a, self.flagged[self.a]
        off = np.cumsum(self.cnt) - self.cnt
        out = np.zeros(int(self.cnt.sum()), dtype=np.uint8)
        keep = ~fl | self.head
        out[off[keep]] = a[keep]
        m = fl & self.ff
        out[off[m] + self.head[m]] = 255
        m = fl & self.last
        out[off[m] + self.head[m] + self.ff[m]] = (self.r[m] % 255).astype(np.uint8)
        return self.bitmap() + bytes(out)

    def per(self, unit):
        """Emitted bytes per lane (unit 16) or tile (unit 4096)."""
        k = -(-self.n // unit)
        c = np.zeros(k * unit, dtype=np.int64)
        c[: self.n] = self.cnt
        return c.reshape(k, unit).sum(axis=1)

    def tile_head(self):
        """k_mrle_heads' table: 1 + the last head position inside each tile, 0 for a tile without one."""
        k = -(-self.n // T)
        h = np.zeros(k * T, dtype=np.int64)
        h[: self.n] = np.where(self.head, np.arange(self.n) + 1, 0)
        return h.reshape(k, T).max(axis=1)

    def out_offset(self, i):
        """Stream position of the first byte position i emits."""
        return 32 + int(self.cnt[:i].sum())


class DecodeModel:
    """The decoder's automaton over a stream (bitmap + body), vectorised: which body bytes are symbols, which length bytes, and the
    per-tile tables of k_mrd_tile_counts.  Positions are body offsets: stream tile t covers body[t * T : (t + 1) * T]."""

    def __init__(self, stream, maxin=None):
        s = np.frombuffer(bytes(stream), dtype=np.uint8)
        self.flagged = np.unpackbits(s[:32], bitorder="little").astype(bool)
        b = s[32 : len(s) if maxin is None else maxin]
        m = len(b)
        fl, is255 = self.flagged[b], b == 255
        # a byte maps the state (S = 0, L = 1): plain and not 0xFF -> S; flagged and 0xFF -> L; flagged -> swap; 0xFF -> keep
        const = fl == is255
        idx = np.arange(m, dtype=np.int64)
        lc = np.maximum.accumulate(np.where(const, idx, -1))
        swaps = np.cumsum(fl & ~is255)
        base = np.where(lc >= 0, (fl & is255)[np.maximum(lc, 0)], False)
        since = swaps - np.where(lc >= 0, swaps[np.maximum(lc, 0)], 0)
        after = base ^ (since & 1).astype(bool)
        before = np.zeros(m, dtype=bool)
        before[1:] = after[:-1]
        self.b, self.m, self.before, self.after = b, m, before, after
        self.is_sym = ~before
        self.cnt = np.where(before, np.where(is255, 255, b.astype(np.int64) + 1), (~fl).astype(np.int64))

    def tile_sym(self):
        """1 + the last symbol's body position per tile, 0 for a tile without a symbol."""
        k = -(-self.m // T)
        h = np.zeros(k * T, dtype=np.int64)
        h[: self.m] = np.where(self.is_sym, np.arange(self.m) + 1, 0)
        return h.reshape(k, T).max(axis=1)

    def tile_off(self):
        """Output offset at which each stream tile begins."""
        k = -(-self.m // T)
        c = np.zeros(k * T, dtype=np.int64)
        c[: self.m] = self.cnt
        c = c.reshape(k, T).sum(axis=1)
        return np.cumsum(c) - c

    def output(self):
        """What a stream that ends in state S decodes to, uncapped."""
        assert self.m == 0 or not self.after[-1]
        idx = np.arange(self.m, dtype=np.int64)
        gov = np.maximum.accumulate(np.where(self.is_sym, idx, -1))
        return bytes(np.repeat(self.b[np.maximum(gov, 0)], self.cnt))


def decode_count(stream, maxin=None):
    """Bytes mrled would produce from stream[:maxin] with room for all of them, its quirk included (src/libbz3.c:320-322): a length
    sequence that the end of the stream cuts off still adds 1 + the last length byte read anywhere before (-1 at first)."""
    s = bytes(stream)
    maxin = len(s) if maxin is None else maxin
    if maxin < 32:
        return 0
    fl = np.unpackbits(np.frombuffer(s[:32], dtype=np.uint8), bitorder="little")
    ip, op, pc = 32, 0, -1
    while ip < maxin:
        c = s[ip]
        ip += 1
        if fl[c]:
            run = 0
            while ip < maxin:
                pc = s[ip]
                ip += 1
                if pc != 255:
                    break
                run += 255
            op += run + pc + 1
        else:
            op += 1
    return op


def make_bitmap(values):
    f = np.zeros(256, dtype=bool)
    f[list(values)] = True
    return bytes(np.packbits(f, bitorder="little"))


# ---- encoder families ------------------------------------------------------------------------------------------------------------
LONGRUN_LENGTHS = (T - 1, T, T + 1, 2 * T + 1, 3 * T + 5)
LONGRUN_HEADS = (("t0", 0), ("t1", 1), ("tlast", T - 1), ("lane0", 100 * LANE), ("lane15", 100 * LANE + 15))


def headless_tiles(p, ln):
    """Tiles that lie wholly inside the run [p, p + ln) without holding its head."""
    return [t for t in range(p // T + 1, (p + ln) // T + 1) if p < t * T and (t + 1) * T <= p + ln]


@functools.lru_cache(maxsize=None)
def longrun():
    """One flagged run of every length in LONGRUN_LENGTHS with its head at tile offset 0, 1 and T - 1 and at the first and the last
    byte of a lane in mid-tile, in tile 1 of a block of filler.  A run of ln leaves a tile without a head only if it covers one behind
    its own head: always from 2T + 1 on, at T + 1 only from the last byte of a tile, never below; INTENT holds the tiles."""
    out = []
    for ln in LONGRUN_LENGTHS:
        for tag, off in LONGRUN_HEADS:
            p = T + off
            n = p + ln + T + 37
            name = "longrun-%d-%s" % (ln, tag)
            INTENT[name] = dict(p=p, ln=ln, n=n, headless=headless_tiles(p, ln))
            out.append((name, bytes(build(n, [(p, ln, V)]))))
    return out


MOD255_EDGES = (("tile-first", 2 * T), ("tile-last", 3 * T - 1), ("wave-first", 3 * T + WAVE), ("wave-last", 4 * T + 2 * WAVE - 1),
                ("lane-first", 5 * T + 7 * LANE), ("lane-last", 5 * T + 30 * LANE + 15))
MOD255_LENGTHS = tuple(255 * k + d for k in (1, 2, 17) for d in (-1, 0, 1))


@functools.lru_cache(maxsize=None)
def mod255():
    """edges: six runs of 300 whose position with r == 255 (the 0xFF in mid-run) is the first and the last byte of a tile, of a wave and
    of a lane.  ends: the same six edges under the LAST byte of runs of 256 (r == 255 there: 0xFF and then 0x00).  lengths: runs of
    255k - 1, 255k and 255k + 1.  unflagged: the edges again with so many single bytes of the value behind them that it is not flagged."""
    out = []
    edges = [(q - 255, 300, V) for _, q in MOD255_EDGES]
    n = 6 * T + 501
    out.append(("mod255-edges", bytes(build(n, edges))))
    INTENT["mod255-edges"] = dict(at=[q for _, q in MOD255_EDGES], flagged=True, last=False)
    out.append(("mod255-ends", bytes(build(n, [(q - 255, 256, V) for _, q in MOD255_EDGES]))))
    INTENT["mod255-ends"] = dict(at=[q for _, q in MOD255_EDGES], flagged=True, last=True)
    runs, p = [], 3
    for ln in MOD255_LENGTHS:
        runs.append((p, ln, V))
        p += ln + 11
    out.append(("mod255-lengths", bytes(build(p + 5, runs))))
    INTENT["mod255-lengths"] = dict(runs=runs)
    singles = 6 * (300 - 2 - 1)  # what the six runs gain
    a = build(n + 2 * singles, edges)
    a[n::2] = V
    out.append(("mod255-unflagged", bytes(a)))
    INTENT["mod255-unflagged"] = dict(at=[q for _, q in MOD255_EDGES], flagged=False, last=False)
    return out


GAIN_VALUES = (0x11, 0x22, 0x33)  # summed gain -1, 0, +1


def _settle(parts, values):
    """Append singles or one short run per value so that the summed gains are -1, 0, +1."""
    g = Model(np.concatenate(parts)).gain
    for v, want in zip(values, (-1, 0, 1)):
        d = int(g[v]) - want
        if d > 0:
            s = filler(2 * d).copy()
            s[1::2] = v
            parts.append(s)
        elif d < 0:
            assert -d + 2 < 255
            parts.append(np.concatenate([filler(2), np.full(-d + 2, v, dtype=np.uint8)]))
        parts.append(filler(2))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def gain():
    out = []
    x, y, z = GAIN_VALUES
    # tiles: for each value a run of 260 across a tile boundary (r == 255 on the far side) and single bytes spread over three later tiles
    a = build(6 * T, [(T - 130, 260, x), (2 * T - 3, 260, y), (3 * T - 100, 260, z)])
    for v, k in zip(GAIN_VALUES, (258, 257, 256)):
        pos = 3 * T + 300 + 40 * np.arange(k) + 2 * GAIN_VALUES.index(v)
        assert pos.max() < 6 * T
        a[pos] = v
    out.append(("gain-tiles", bytes(a)))
    INTENT["gain-tiles"] = dict(gains={x: -1, y: 0, z: 1}, flags={z})
    # lanes: one tile of short runs of the three values and of filler, the value changing in mid-lane; the sums are settled behind it
    rng = _rng(7)
    parts, prev = [], -1
    while sum(len(p) for p in parts) < T:
        v = int(rng.choice([x, y, z, FILL[0], FILL[1]]))
        if v == prev:
            continue
        parts.append(np.full(int(rng.integers(1, 5)) if v in GAIN_VALUES else 1, v, dtype=np.uint8))
        prev = v
    parts.append(filler(2) if prev != FILL[0] else filler(3)[1:])
    out.append(("gain-lanes", bytes(_settle(parts, GAIN_VALUES))))
    INTENT["gain-lanes"] = dict(gains={x: -1, y: 0, z: 1}, flags={z}, midlane=True)
    out.append(("gain-all", bytes(np.repeat(np.arange(256, dtype=np.uint8), 3))))
    INTENT["gain-all"] = dict(flags=set(range(256)))
    out.append(("gain-none", bytes(np.tile(np.arange(256, dtype=np.uint8), 3))))
    INTENT["gain-none"] = dict(flags=set())
    # 0xFF flagged: the symbol 0xFF next to the length marker 0xFF, its own and another value's
    a = np.concatenate([filler(5), np.full(256, V, np.uint8), np.full(256, 255, np.uint8), filler(3), np.full(3, 255, np.uint8), filler(4),
                        np.full(511, 255, np.uint8), np.full(255, V, np.uint8), np.full(1, 255, np.uint8), filler(9)])
    out.append(("gain-ff", bytes(a)))
    INTENT["gain-ff"] = dict(flags={V, 255})
    a = np.concatenate([np.zeros(5, np.uint8), filler(7), np.zeros(1, np.uint8), filler(20), np.zeros(256, np.uint8), np.full(3, 1, np.uint8), np.zeros(2, np.uint8)])
    out.append(("gain-00", bytes(a)))
    INTENT["gain-00"] = dict(flags={0, 1})
    return out


FAST_N = (T + 160, T + 161, T + 175)


@functools.lru_cache(maxsize=None)
def fastpath():
    """k_mrle_emit<1> stores a lane's 16 bytes at once when it emits 16 and none of its values is flagged.  coincide: lanes that emit 16
    although they hold flagged bytes (V V: two for two; V V V and a single V: four for four), with plain lanes on both sides.
    residue-k: a leading run of 3 to 18 bytes, coded in two, so that the plain lanes behind it are stored at every offset k modulo 16.
    tail-n: the last full lane in front of n for n % 16 of 0, 1 and 15."""
    out = []
    a = build(40 * LANE, [(3 * LANE + 40, 9, V)])
    two, four = 10 * LANE, 20 * LANE
    a[two + 5 : two + 7] = V
    a[four + 2 : four + 5] = V
    a[four + 9] = V
    out.append(("fastpath-coincide", bytes(a)))
    INTENT["fastpath-coincide"] = dict(lanes=[two // LANE, four // LANE])
    for k in range(16):
        name = "fastpath-residue-%d" % ((15 - k) % 16)  # lane 2 leaves at 32 + 2 + 32 - (k + 3)
        out.append((name, bytes(build(20 * LANE + 3, [(0, k + 3, V)]))))
        INTENT[name] = dict(residue=(15 - k) % 16, lane=2)
    for n in FAST_N:
        out.append(("fastpath-tail-%d" % n, bytes(build(n, [(7, 30, V)]))))
        INTENT["fastpath-tail-%d" % n] = dict(n=n)
    return out


ENDS_SMALL = (1, 2, 15, 16, 17, T - 1, T, T + 1)
ENDS_LARGE = (C - 1, C, C + 1)


def _ends(sizes):
    out = []
    for n in sizes:
        ln = min(n, 300)
        out.append(("ends-run-%d" % n, bytes(build(n, [(n - ln, ln, V)]))))  # a run that reaches n - 1
        a = build(n, [(max(0, n - 40), min(30, max(0, n - 2)), V)] if n > 2 else [])
        a[n - 1] = V  # a head at n - 1, of a value that is flagged wherever the block has room for a run of it
        out.append(("ends-head-%d" % n, bytes(a)))
    return out


@functools.lru_cache(maxsize=None)
def ends():
    return _ends(ENDS_SMALL)


@functools.lru_cache(maxsize=None)
def ends_large():
    return _ends(ENDS_LARGE)


@functools.lru_cache(maxsize=None)
def spine():
    """Blocks just over one chunk of k_mrle_head_spine (and one just over two).  run: from inside tile 1022 to inside tile 1025, so that
    tile 1024 -- the first of the second chunk -- takes its head from the carry.  head-C / head-C-1: a run that begins on the chunk's first
    byte, and one that begins a byte in front of it.  third-*: the same three around the second boundary, 2C, where the third chunk's
    first tile takes its carry from the second chunk's last thread; each block repeats a shape at C, so that both carries are live."""
    out = []

    def add(name, n, runs, headless):
        out.append((name, bytes(build(n, runs))))
        INTENT[name] = dict(n=n, runs=runs, headless=headless)

    add("spine-run", C + 3 * T + 11, [(1022 * T + 100, 3 * T - 50, V)], [1023, 1024])
    add("spine-head-C", C + T + 5, [(C, 600, V)], [])
    add("spine-head-C-1", C + T + 5, [(C - 1, 600, V)], [])
    add("spine-third", 2 * C + 3 * T + 7, [(C - 1, T + 300, V), (2046 * T + 9, 3 * T + 70, V)], [1024, 2047, 2048])
    add("spine-third-head-2C", 2 * C + T + 3, [(C, 600, V), (2 * C, 600, V)], [])
    add("spine-third-head-2C-1", 2 * C + T + 3, [(C - 1, 600, V), (2 * C - 1, 600, V)], [])
    return out


# ---- decoder families ------------------------------------------------------------------------------------------------------------
def _body(n, items):
    """n bytes of filler with byte strings laid over them: [(body offset, bytes)]."""
    a = filler(n)
    for p, s in items:
        s = np.frombuffer(bytes(s), dtype=np.uint8)
        assert p + len(s) <= n
        a[p : p + len(s)] = s
    return a


def _whole(name, bitmap, body):
    s = bitmap + bytes(body)
    return (name, s, decode_count(s) if len(s) < (1 << 20) else int(DecodeModel(s).cnt.sum()), len(s))


@functools.lru_cache(maxsize=None)
def lenchain():
    out = []
    bm = make_bitmap({V})
    out.append(_whole("lenchain-tiles", bm, _body(4 * T + 90, [(T - 9, bytes([V]) + b"\xff" * (2 * T + 100) + b"\x07"), (3 * T + 500, bytes([V, 3]))])))
    INTENT["lenchain-tiles"] = dict(symless=[1, 2])
    at = (T - 1, T + WAVE - 1, 2 * T + 9 * LANE + 15)
    out.append(_whole("lenchain-bounds", bm, _body(3 * T + 33, [(p, bytes([V, 5 + i])) for i, p in enumerate(at)])))
    INTENT["lenchain-bounds"] = dict(sym_at=at)
    out.append(_whole("lenchain-bounds-ff", bm, _body(3 * T + 33, [(p - 1, bytes([V, 255, 5 + i])) for i, p in enumerate(at)])))
    INTENT["lenchain-bounds-ff"] = dict(len_at=at)  # the 0xFF is the last byte, the closing length byte the first behind the boundary
    out.append(_whole("lenchain-ffsym", make_bitmap({255}), _body(3 * T + 50, [(T - 40, b"\xff" * (T + 61) + b"\x03"), (2 * T + 700, b"\xff\x00\xff\xff\x02")])))
    INTENT["lenchain-ffsym"] = dict(symless=[1])
    return out


@functools.lru_cache(maxsize=None)
def dspine():
    """Streams longer than one chunk of k_mrd_spine / k_mrd_spine2.  L: a symbol in tile 1022, 0xFF through tile 1023 and into tile
    1024, run expansions behind it.  S: an unflagged 0xFF as the chunk's last byte (the identity map) and a flagged symbol as the next
    chunk's first."""
    bm = make_bitmap({V})
    chain = bytes([V]) + b"\xff" * (C + 100 - (1022 * T + 51)) + b"\x21"
    out = [_whole("dspine-L", bm, _body(C + 2 * T + 77, [(1022 * T + 50, chain), (C + 900, bytes([V, 9])), (C + T + 5, bytes([V, 255, 0]))]))]
    INTENT["dspine-L"] = dict(state=True, symless=[1023], sym_tile=1022)
    out.append(_whole("dspine-S", bm, _body(C + T + 13, [(1000, bytes([V, 4])), (C - 1, b"\xff" + bytes([V, 255, 17])), (C + 300, bytes([V, 0]))])))
    INTENT["dspine-S"] = dict(state=False)
    return out


@functools.lru_cache(maxsize=None)
def cuts_stream():
    """The stream of `cuts` and the stream positions it is cut behind.  Tile 0: a flagged symbol with no length byte anywhere in front of
    it.  Tile 1: a chain of twelve 0xFF.  Tile 2: a flagged symbol whose last length byte lies in tile 1."""
    first, chain, late = 700, T + 2000, 2 * T + 900
    body = _body(3 * T + 50, [(first, bytes([V, 41])), (chain, bytes([V]) + b"\xff" * 12 + b"\x08"), (late, bytes([V, 2]))])
    return make_bitmap({V}) + bytes(body), dict(first=32 + first + 1, chain=range(32 + chain + 2, 32 + chain + 14), late=32 + late + 1)


@functools.lru_cache(maxsize=None)
def cuts():
    """maxin at every value named in cuts_stream and around the first two tile boundaries, and 32 and 33; outlen is what the reference
    makes of the stream cut there, so that the return value is 0 and the bytes count."""
    s, at = cuts_stream()
    where = {32: "bare", 33: "one", at["first"]: "pc-1", at["late"]: "stale"}
    for edge in (32 + T, 32 + 2 * T):
        for d in range(-3, 4):
            where[edge + d] = "tile%d%+d" % ((edge - 32) // T, d)
    for m in at["chain"]:
        where[m] = "chain%d" % (m - at["chain"][0])
    out = []
    for m in sorted(where):
        name = "cuts-%s" % where[m]
        out.append((name, s, decode_count(s, m), m))
        INTENT[name] = dict(maxin=m)
    return out


@functools.lru_cache(maxsize=None)
def caps_input():
    """Three tiles of filler with three runs in mid-tile; the oracle codes them in 10,361 bytes, two and a half stream tiles."""
    return bytes(build(3 * T + 200, [(500, 700, V), (T + 3000, 1400, V), (2 * T + 2000, 40, V)]))


def hostile():
    """One flagged symbol and enough 0xFF behind it for the count to pass 2^32 by a little over 2 MiB: (body, count)."""
    k = ((1 << 32) + (1 << 21)) // 255 + 1
    return bytes([V]) + b"\xff" * k, 255 * k


@functools.lru_cache(maxsize=None)
def caps(oracle_stream):
    """`oracle_stream` is the oracle's coding of caps_input()."""
    s = oracle_stream
    true = len(caps_input())
    d = DecodeModel(s)
    off = d.tile_off()
    inside = int(np.flatnonzero(d.cnt > 200)[1])  # the second 0xFF of the first run, in mid-tile: it stands for 255 bytes
    mid = int(d.cnt[:inside].sum()) + 100
    out = [("caps-%s" % tag, s, ol, len(s)) for tag, ol in (("true-1", true - 1), ("true+1", true + 1), ("inrun", mid), ("tilefirst", int(off[1])), ("one", 1))]
    INTENT["caps-inrun"] = dict(byte=inside)
    # three tiles of the hostile stream: the count passes outlen in the first tile and every later tile's offset is the cap
    bm = make_bitmap({V})
    small = bm + bytes([V]) + b"\xff" * (3 * T) + b"\x00" + bytes(FILL) * 30
    out.append(("caps-hostile3", small, 1000, len(small)))
    return out


HOSTILE_OUTLEN = 1 << 20


@functools.lru_cache(maxsize=None)
def caps_hostile():
    """Device only (16 MiB of stream each).  single: the symbol and the chain alone.  The count as mrled keeps it, in a signed 32 bits, has
    then wrapped once and still lies above outlen, so that the reference fills the output too: that wrap is undefined behaviour in C, so this
    case pins what the compilers of the oracle and of the reference make of it (its precondition checks that they fill the output), not the
    format; `filled` does not depend on it.  filled: a run that fills the output first --
    mrled stops there and never reads the chain --, then the chain, closed so that the count stands at 2^32 + 4100, then other bytes:
    an offset kept modulo 2^32 would put them at 4100."""
    bm = make_bitmap({V})
    chain, count = hostile()
    single = bm + chain
    INTENT["caps-hostile-single"] = dict(count=count)
    fill = bytes([V]) + b"\xff" * (HOSTILE_OUTLEN // 255) + bytes([HOSTILE_OUTLEN % 255 + 20])
    got = 255 * (HOSTILE_OUTLEN // 255) + HOSTILE_OUTLEN % 255 + 21
    rest = (1 << 32) + 4100 - got
    k, last = (rest - 1) // 255, (rest - 1) % 255
    filled = bm + fill + bytes([V]) + b"\xff" * k + bytes([last]) + bytes(FILL) * 4000
    INTENT["caps-hostile-filled"] = dict(count=got + 255 * k + last + 1, second=len(fill))
    return [("caps-hostile-single", single, HOSTILE_OUTLEN, len(single)), ("caps-hostile-filled", filled, HOSTILE_OUTLEN, len(filled))]


@functools.lru_cache(maxsize=None)
def arbitrary():
    """Three random bodies of 20,000 bytes, heavy in 0xFF and small values, under random bitmaps; outlen at the count, half of it and
    five more."""
    out = []
    for seed in range(3):
        rng = _rng(300 + seed)
        body = rng.integers(0, 256, size=20000, dtype=np.uint8)
        body[rng.random(20000) < 0.2] = 255
        small = rng.random(20000) < 0.3
        body[small] = rng.integers(0, 6, size=int(small.sum()), dtype=np.uint8)
        s = bytes(rng.integers(0, 256, size=32, dtype=np.uint8)) + bytes(body)
        n = decode_count(s)
        for tag, ol in (("count", n), ("half", n // 2), ("more", n + 5)):
            out.append(("arbitrary-%d-%s" % (seed, tag), s, ol, len(s)))
    return out


# ---- through the block API -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def threshold():
    """[(name, data, whether mRLE applies)]: a run of 34 (the coded block is as long as the input: the filter is declined) and of 35
    (a byte shorter: it applies), each followed by bytes that do not repeat and do not hold the run's value."""
    tail = bytes(np.arange(1, 151, dtype=np.uint8))
    return [("threshold-34", bytes([0xEE]) * 34 + tail, False), ("threshold-35", bytes([0xEE]) * 35 + tail, True)]


UNALIGNED_OFFSETS = (1, 7, 15)


def unaligned_input():
    return dict((n, d) for n, d in longrun())["longrun-%d-tlast" % (3 * T + 5)]


ENDS_LARGE_NAMES = tuple("ends-%s-%d" % (k, n) for n in ENDS_LARGE for k in ("run", "head"))
SPINE_NAMES = ("spine-run", "spine-head-C", "spine-head-C-1", "spine-third", "spine-third-head-2C", "spine-third-head-2C-1")
DSPINE_NAMES = ("dspine-L", "dspine-S")
SMALL_ENC = ("longrun", "mod255", "gain", "fastpath", "ends")      # families of small cases: a test walks a whole family
SMALL_DEC = ("lenchain", "cuts", "caps", "arbitrary")
ENC_FAMILIES = {"longrun": longrun, "mod255": mod255, "gain": gain, "fastpath": fastpath, "ends": ends, "ends-large": ends_large, "spine": spine}
DEC_FAMILIES = {"lenchain": lenchain, "dspine": dspine, "cuts": cuts, "arbitrary": arbitrary}  # (and caps / caps_hostile, which take the oracle's stream)


def dec_cases(oracle, family):
    """The cases of a decoder family; `caps` and `caps-hostile` are the two that need the oracle's encoder."""
    if family == "caps":
        return caps(oracle.mrle_encode(caps_input()))
    return caps_hostile() if family == "caps-hostile" else DEC_FAMILIES[family]()


def case(family, name):
    return dict((c[0], c) for c in (ENC_FAMILIES.get(family) or DEC_FAMILIES[family])())[name]


# ---- preconditions ---------------------------------------------------------------------------------------------------------------
def precondition_enc(oracle, family, name, data):
    """The model equals the oracle, and the case hits what its family names."""
    m = Model(data)
    e = oracle.mrle_encode(data)
    assert m.stream() == e, name
    assert m.bitmap() == e[:32], name
    it = INTENT.get(name, {})
    n = len(data)
    if family == "longrun":
        p, ln = it["p"], it["ln"]
        assert m.flagged[V] and list(np.flatnonzero(m.flagged)) == [V], name
        th = m.tile_head()
        assert [t for t in range(len(th)) if th[t] == 0] == it["headless"], name
        assert len(e) == 32 + n - ln + coded_run(ln), name
    elif family == "mod255":
        if "at" in it:
            at = np.array(it["at"])
            assert [q % T for q in at[:2]] == [0, T - 1] and [q % WAVE for q in at[2:4]] == [0, WAVE - 1] and [q % LANE for q in at[4:]] == [0, LANE - 1], name
            assert all(q % T not in (0, T - 1) for q in at[2:4]) and all(q % WAVE not in (0, WAVE - 1) for q in at[4:]), name
            assert (m.r[at] == 255).all() and (m.a[at] == V).all() and bool(m.flagged[V]) == it["flagged"], name
            assert (m.last[at] == it["last"]).all(), name
            if it["flagged"]:
                for q in at:
                    o = m.out_offset(q)
                    assert e[o] == 255 and (not it["last"] or e[o + 1] == 0), name  # (behind the run's last byte: 0xFF and then 0x00)
            else:
                assert len(e) == 32 + n and int(m.gain[V]) == 0, name
        else:
            assert [ln for _, ln, _ in it["runs"]] == list(MOD255_LENGTHS) and m.flagged[V], name
            assert len(e) == 32 + n - sum(ln - coded_run(ln) for _, ln, _ in it["runs"]), name
    elif family == "gain":
        assert set(int(v) for v in np.flatnonzero(m.flagged)) == it["flags"], name
        assert e[:32] == make_bitmap(it["flags"]), name
        for v, g in it.get("gains", {}).items():
            assert int(m.gain[v]) == g, (name, v)
        if it.get("midlane"):
            lanes = m.a[:T].reshape(-1, LANE)
            assert sum(len(set(l.tolist()) & set(GAIN_VALUES)) >= 2 for l in lanes) >= 50, name
        if name == "gain-tiles":
            for v in GAIN_VALUES:  # contributions of both signs, in different tiles
                w = np.where(m.head, -1, (m.r % 255 != 0).astype(np.int64)) * (m.a == v)
                per = np.add.reduceat(w, np.arange(0, n, T))
                assert (per > 0).sum() >= 2 and (per < 0).sum() >= 2, (name, v)
        if name == "gain-ff":
            assert b"\x7a\xff\x00\xff\xff\x00" in e and b"\xff\xff\xff\x00\x7a" in e, name
    elif family == "fastpath":
        lanes = m.per(LANE)
        fl = m.flagged[m.a]
        assert m.flagged[V], name
        if "lanes" in it:
            for l in it["lanes"]:
                assert lanes[l] == LANE and fl[l * LANE : (l + 1) * LANE].any(), name
                assert not fl[(l - 1) * LANE : l * LANE].any() and not fl[(l + 1) * LANE : (l + 2) * LANE].any(), name
        if "residue" in it:
            l = it["lane"]
            assert not fl[l * LANE : (l + 1) * LANE].any() and m.out_offset(l * LANE) % 16 == int(name.rsplit("-", 1)[1]), name
        if "n" in it:
            l = n // LANE - 1
            assert n % LANE in (0, 1, 15) and not fl[l * LANE : (l + 1) * LANE].any() and lanes[l] == LANE, name
    elif family in ("ends", "ends-large"):
        kind, size = name.split("-")[1], int(name.split("-")[2])
        assert n == size, name
        if kind == "run":
            assert m.r[n - 1] == min(n, 300) - 1 and m.a[n - 1] == V, name
            assert bool(m.flagged[V]) == (n > 2), name
        else:
            assert m.head[n - 1] and m.a[n - 1] == V and bool(m.flagged[V]) == (n >= 15), name
    elif family == "spine":
        th = m.tile_head()
        assert n > C and all(th[t] == 0 for t in it["headless"]) and int((th == 0).sum()) == len(it["headless"]), name
        assert len(e) == 32 + n - sum(ln - coded_run(ln) for _, ln, _ in it["runs"]), name
        assert list(np.flatnonzero(m.flagged)) == [V], name
        if name in ("spine-head-C", "spine-third-head-2C"):
            assert m.head[C] and m.a[C] == V and m.r[C + 1] == 1, name
        if name in ("spine-head-C-1", "spine-third", "spine-third-head-2C-1"):
            assert m.head[C - 1] and m.a[C - 1] == V and m.r[C] == 1, name
        if "third" in name:
            assert n > 2 * C, name
        if name == "spine-third":
            assert m.a[2 * C] == V and m.r[2 * C] == 2 * C - (2046 * T + 9), name
        if name == "spine-third-head-2C":
            assert m.head[2 * C] and m.a[2 * C] == V and m.r[2 * C + 1] == 1, name
        if name == "spine-third-head-2C-1":
            assert m.head[2 * C - 1] and m.a[2 * C - 1] == V and m.r[2 * C] == 1, name
    else:
        raise AssertionError(family)


def precondition_dec(oracle, family, name, s, outlen, maxin):
    it = INTENT.get(name, {})
    if family == "caps-hostile":
        b = np.frombuffer(s, dtype=np.uint8)[32:]
        at = it.get("second", 0)  # where the symbol of the chain stands
        k = int(np.argmax(b[at + 1 :] != 255)) or len(b) - at - 1
        assert b[at] == V and (b[at + 1 : at + 1 + k] == 255).all() and (16 << 20) < k and len(s) < (17 << 20), name
        if at:
            assert decode_count(s[: 32 + at]) == outlen + 21 and decode_count(s[: 32 + at]) + 255 * k + int(b[at + 1 + k]) + 1 == it["count"] == (1 << 32) + 4100, name
            assert len(b) == at + k + 2 + 8000 and not np.isin(b[-8000:], (V, 255)).any(), name
        else:
            assert len(b) == k + 1 and it["count"] == 255 * k and outlen < (it["count"] + 256) % (1 << 32) < (1 << 31), name
        assert oracle.mrle_decode(s, outlen) == (0, bytes([V]) * outlen), name  # the oracle is bounded on it, and fills the output
        return
    d = DecodeModel(s, maxin)
    assert d.m == maxin - 32, name
    if family in ("lenchain", "dspine"):
        out = d.output()
        assert len(out) == outlen and oracle.mrle_decode(s, outlen) == (0, out), name
        ts = d.tile_sym()
        if "symless" in it:
            assert [t for t in range(len(ts)) if ts[t] == 0] == it["symless"], name
        for p in it.get("sym_at", ()):
            assert d.is_sym[p] and d.before[p + 1] and d.is_sym[p + 2], (name, p)
        for p in it.get("len_at", ()):
            assert d.before[p] and d.b[p] == 255 and d.before[p + 1] and d.is_sym[p + 2], (name, p)
        if "sym_at" in it or "len_at" in it:
            at = it.get("sym_at") or it.get("len_at")
            assert at[0] % T == T - 1 and at[1] % WAVE == WAVE - 1 and at[1] % T != T - 1 and at[2] % LANE == LANE - 1 and at[2] % WAVE != WAVE - 1, name
        if family == "dspine":
            assert d.m > C and bool(d.before[C]) == it["state"], name
            assert (d.cnt[C:] > 1).any(), name  # a run expansion behind the boundary
            if it["state"]:
                assert ts[it["sym_tile"]] > 0 and d.before[C : C + 101].all() and d.is_sym[C + 101], name
            else:
                assert d.b[C - 1] == 255 and d.is_sym[C - 1] and not d.flagged[255] and d.is_sym[C] and d.flagged[d.b[C]], name
    elif family == "cuts":
        full, at = cuts_stream()
        assert s == full and outlen == decode_count(s, maxin), name
        rc, out = oracle.mrle_decode(s, outlen, maxin)
        assert rc == 0, name  # (the count above is the reference's)
        if maxin > 32:
            assert oracle.mrle_decode(s, outlen + 1, maxin)[0] == 1, name
        if name == "cuts-pc-1":  # behind the first flagged symbol: no length byte yet, no copy of it
            assert s[maxin - 1] == V and not d.before[: maxin - 32].any() and outlen == maxin - 33, name
        if name == "cuts-stale":  # the copies come from the length byte 0x08 of tile 1
            assert s[maxin - 1] == V and d.after[-1] and not d.before[2 * T :].any() and int(np.flatnonzero(d.before)[-1]) // T == 1, name
            assert outlen == decode_count(s, maxin - 1) + 9, name
        if name.startswith("cuts-chain"):
            assert d.after[-1] and d.before[-1], name
    elif family == "caps":
        if name == "caps-inrun":
            b = it["byte"]
            assert d.before[b] and d.cnt[b] > 200 and 0 < outlen - int(d.cnt[:b].sum()) < d.cnt[b] and 16 < b % T < T - 16, name
        if name == "caps-tilefirst":
            assert outlen == int(d.tile_off()[1]) and 0 < outlen < len(caps_input()), name
        if name == "caps-hostile3":
            assert int(d.cnt[:T].sum()) > outlen and d.m > 3 * T and oracle.mrle_decode(s, outlen) == (0, bytes([V]) * outlen), name
    elif family == "arbitrary":
        assert d.m == 20000 and outlen in (decode_count(s), decode_count(s) // 2, decode_count(s) + 5), name
        assert oracle.mrle_decode(s, decode_count(s))[0] == 0 and oracle.mrle_decode(s, decode_count(s) + 1)[0] == 1, name
    else:
        raise AssertionError(family)


# ---- what the tests on the emulator and on the device share ------------------------------------------------------------------------
def check_encoder_case(g, oracle, name, data):
    """Encode bytes, decode bytes and return value for one input and the oracle's genuine stream of it."""
    e = oracle.mrle_encode(data)
    assert g.mrle_encode(data) == e, name
    assert g.mrle_decode(e, len(data)) == (0, data), name


def check_decoder_case(g, oracle, name, s, outlen, maxin):
    """The return value, and the bytes where it is 0 (where it is not, mrled's output is cut somewhere the kernels need not agree on)."""
    a, b = g.mrle_decode(s, outlen, maxin), oracle.mrle_decode(s, outlen, maxin)
    assert a[0] == b[0], (name, a[0], b[0])
    if b[0] == 0:
        assert a[1] == b[1], name


def check_threshold(lib, oracle, state_cls):
    """Through the block API: model bit 4 follows `coded size < input size` exactly (src/libbz3.c:609-614), bytes and round trip."""
    bs = 65 * 1024
    for name, d, applies in threshold():
        assert len(d) >= 64 and len(oracle.mrle_encode(d)) == len(d) - (1 if applies else 0), name
        want = oracle.encode_block(d, bs)
        assert want[0] > 0 and bool(want[2][8] & 4) == applies, name
        with state_cls(bs, lib) as st:
            assert st.encode_block(d) == want, name
            assert st.decode_block(want[2], len(d)) == (len(d), 0, d), name


def check_unaligned(lib, oracle, base_ptr, offset, write, read):
    """bz3_hip_encode_blocks_device / bz3_hip_decode_blocks_device on a buffer that begins `offset` bytes behind a 16-byte boundary
    (base_ptr is 16-byte aligned): load16 takes its scalar path in every lane and in[base - 1] is read from another 16 bytes than it
    would be.  write(ptr, bytes) and read(ptr, n) reach the buffer, wherever it lives."""
    import ctypes as C

    d = unaligned_input()
    bs = 65 * 1024
    want = oracle.encode_block(d, bs)
    assert want[0] > 0 and want[2][8] & 4 and base_ptr % 16 == 0  # mRLE applies
    ptr = base_ptr + offset
    st = lib.bz3_new(bs)
    assert st
    try:
        states, ptrs = (C.c_void_p * 1)(st), (C.c_void_p * 1)(ptr)
        write(ptr, d)
        sizes = (C.c_int32 * 1)(len(d))
        lib.bz3_hip_encode_blocks_device(states, ptrs, sizes, 1)
        assert (sizes[0], lib.bz3_last_error(st)) == want[:2], offset
        assert read(ptr, sizes[0]) == want[2], offset
        bsz, orig = (C.c_size_t * 1)(lib.bz3_bound(bs)), (C.c_int32 * 1)(len(d))
        lib.bz3_hip_decode_blocks_device(states, ptrs, bsz, sizes, orig, 1)
        assert lib.bz3_last_error(st) == 0, offset
        assert read(ptr, len(d)) == d, offset
    finally:
        lib.bz3_free(st)
