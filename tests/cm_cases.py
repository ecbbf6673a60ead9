"""Adversarial inputs for the CM kernels (bzip3_amd/csrc/cm.hip), each family with a precondition that proves it reaches the mechanism it is named for
(tests/test_cm_cases.py asserts them without a GPU and runs every case through the emulator; tests/test_gpu_cm_cases.py runs them on hardware).

The expected bytes of every test come from the oracle (oracle/bz3_oracle.c), never from this module and never from the library.  What lives here:

  Encoder / model_decode   a plain Python model of the coder, exact integer arithmetic, written from the description in cm.hip: C0 u16[256] (shift 2),
                           C1 u16[256][256] (shift 4), C2 u16[512][17] (shift 6, row 2 * node + run flag, cells j = p >> 12 and j + 1, cell 16 starts at
                           65535), p = ((c0 + c1[prev1]) * 7 + 2 * c1[prev2]) >> 4, the 18-bit probability 3 * ssep + p, low / high, the renormalisation
                           while low and high share their top byte, the 4-byte flush.  Per coded bit it records the range (high - low) BEFORE the
                           renormalisation, the bytes emitted, the probability, the C2 cell and the output offset; per counter kind the fixed points
                           reached.  It is held against oracle.cm_encode on every case; it only DRIVES the generators and proves the preconditions.
  shortcut_encode          the encoder's fast-path scheme (8 bits without a test, then halves of 4, then bit by bit) transcribed from the comment in
                           cm.hip, with either `rmin == 0` guard removable: the two "wrong encoders" the straddle family must tell from the right one.
  RowDirectory             the documented rule of the row caches: slots in order of first use, then FIFO skipping pinned rows, give up when
                           misses > base + (position >> shift), per chunk in the encoder, per wrong guess in the decoder.
  sink_switch              the rule of the CmSink comment: the first output byte that must go to the side buffer.

Families (build() returns all of them, built once per session):

  straddle  every bit is chosen so that the coder's interval still contains a multiple of 2^24 (a seeded random bit where neither half does): the interval
            shrinks to one or two values without a renormalisation, then four bytes come out at one bit.  On ordinary data that state occurs once in
            ~2^24 bits; here a fifth of the bytes have it.
  seams     lengths and runs around the encoder's chunk (32), ring (64) and publish (16) boundaries; blocks that begin with zero bytes.
  extremes  counters at their update fixed points in both directions, then the improbable bit.  Found (asserted by the CPU test):
            C0 3 / 65532, C1 15 / 65520, C2 pairs (0, 63) in cells 0, 1 and (65472, 65535) in cells 15, 16; the 18-bit probability at those fixed
            points is P18_MIN = 9 and P18_MAX = 262127 (of 262143), and each is coded with a 0 and with a 1.
  windows   coded sizes at the edges of the decoder's 64-byte input window, truncations, a junk stream that reaches code < low.
  rows      cyclic orders over more values than a cache has rows plus a chunk, exactly R and R + 1 values, value 0 late, and the budget boundary.
  sink      in-place coding: where the sink must switch to the side buffer, and how many side bytes that takes.
"""
import ctypes as C
import os

import numpy as np

import bzip3_amd
import datagen

M32 = 0xFFFFFFFF
TOP = 1 << 24
CM_CHUNK, CM_RING, CM_PUBLISH = 32, 64, 16           # cm.hip: bytes per model chunk, bytes of ring, the coder tells the model waves every 16 bytes
CM_MISS_BASE, CM_MISS_SHIFT = 1024, 5                # stages.hpp
CM_TEST_MISS_BASE, CM_TEST_MISS_SHIFT = 64, 3        # api_hooks.hip: the emulator-only 40-row variant
ROWS_ENC = {1: 96, 2: 44, 9: 40}                     # cm.hip CM_ROWS_ENC / CM_ROWS3_ENC / CM_ROWS_TEST by cm mode
ROWS_DEC = {1: 96, 2: 56, 9: 40}
BUDGET = {1: (CM_MISS_BASE, CM_MISS_SHIFT), 2: (CM_MISS_BASE, CM_MISS_SHIFT), 9: (CM_TEST_MISS_BASE, CM_TEST_MISS_SHIFT)}
# update fixed points: x - (x >> s) == x  <=>  x < 2^s;  x + ((x ^ 65535) >> s) == x  <=>  65535 - x < 2^s.  Coming from 32768 (or a C2 cell's start)
# the updates stop at the first such value.
FIX_LOW = {"c0": 3, "c1": 15, "c2": 63}
FIX_HIGH = {"c0": 65532, "c1": 65520, "c2": 65472}
P18_MIN = 9        # c0 = 3, c1 = 15 twice: p = (18 * 7 + 30) >> 4 = 9, cells 0 / 1 = 0 / <= 455: ssep = 0
P18_MAX = 262127   # c0 = 65532, c1 = 65520 twice: p = 65525, cells 15 / 16 = 65472 / 65535: ssep = 65534
_C2_INIT = [(k << 12) - (k == 16) for k in range(17)]


class Bit:
    """One coded bit of the trace."""
    __slots__ = ("i", "k", "bit", "p18", "rng", "at", "emitted", "j", "flag")

    def __init__(self, i, k, bit, p18, rng, at, emitted, j, flag):
        self.i, self.k, self.bit, self.p18, self.rng, self.at, self.emitted, self.j, self.flag = i, k, bit, p18, rng, at, emitted, j, flag


class Encoder:
    """The model coder, one bit at a time: begin_byte(), then eight times p18() / put(bit), or encode(data); finish() flushes."""

    def __init__(self):
        self.c0 = [32768] * 256
        self.c1 = {}
        self.c2 = {}
        self.low, self.high = 0, M32
        self.prev1 = self.prev2 = self.run = 0
        self.out = bytearray()
        self.trace = []       # Bit records
        self.flags = []       # run flag per byte
        self.fixed = set()    # (kind, "low" | "high"[, run flag]) fixed points at which a further update left the counter where it was
        self.i = -1

    def _row1(self, r):
        row = self.c1.get(r)
        if row is None:
            row = self.c1[r] = [32768] * 256
        return row

    def _row2(self, r):
        row = self.c2.get(r)
        if row is None:
            row = self.c2[r] = list(_C2_INIT)
        return row

    def begin_byte(self):
        self.i += 1
        self.run = self.run + 1 if self.prev1 == self.prev2 else 0
        self.flag = 1 if self.run > 2 else 0
        self.flags.append(self.flag)
        self.node, self.k = 1, 0

    def p18(self):
        node = self.node
        self._r1, self._r2 = self._row1(self.prev1), self._row1(self.prev2)
        p = ((self.c0[node] + self._r1[node]) * 7 + 2 * self._r2[node]) >> 4
        self._j = j = p >> 12
        self._cells = cells = self._row2(2 * node + self.flag)
        x1, x2 = cells[j], cells[j + 1]
        ssep = x1 + (((x2 - x1) * (p & 4095)) >> 12)   # Python's >> is arithmetic, like the reference's on a negative product
        self._p18 = ssep * 3 + p
        return self._p18

    def split(self):
        """mid of the current interval for the current node (bit 1 keeps [low, mid], bit 0 keeps [mid + 1, high])."""
        return (self.low + (((self.high - self.low) * self.p18()) >> 18)) & M32

    def put(self, bit):
        mid = self.split()
        node, j, cells, r1 = self.node, self._j, self._cells, self._r1
        if bit:
            self.high = mid
        else:
            self.low = (mid + 1) & M32
        rng = (self.high - self.low) & M32
        at, emitted = len(self.out), 0
        while (self.low ^ self.high) < TOP:
            self.out.append(self.low >> 24)
            self.low = (self.low << 8) & M32
            self.high = ((self.high << 8) | 0xFF) & M32
            emitted += 1
        self.trace.append(Bit(self.i, self.k, bit, self._p18, rng, at, emitted, j, self.flag))
        old = (self.c0[node], r1[node], cells[j], cells[j + 1])
        if bit:
            self.c0[node] += (self.c0[node] ^ 65535) >> 2
            r1[node] += (r1[node] ^ 65535) >> 4
            cells[j] += (cells[j] ^ 65535) >> 6
            cells[j + 1] += (cells[j + 1] ^ 65535) >> 6
        else:
            self.c0[node] -= self.c0[node] >> 2
            r1[node] -= r1[node] >> 4
            cells[j] -= cells[j] >> 6
            cells[j + 1] -= cells[j + 1] >> 6
        side = "high" if bit else "low"
        fix = FIX_HIGH if bit else FIX_LOW
        if old[0] == self.c0[node] == fix["c0"]:
            self.fixed.add(("c0", side))
        if old[1] == r1[node] == fix["c1"]:
            self.fixed.add(("c1", side))
        if (old[2], old[3]) == (cells[j], cells[j + 1]) and (cells[j + 1] if not bit else cells[j]) == fix["c2"]:
            self.fixed.add(("c2", side, self.flag, j))   # both cells of the pair stay: (0, 63) below, (65472, 65535) above
        self.node = node * 2 + bit
        self.k += 1
        if self.k == 8:
            self.prev2, self.prev1 = self.prev1, self.node & 255

    def put_byte(self, c):
        self.begin_byte()
        for k in range(7, -1, -1):
            self.put((c >> k) & 1)

    def encode(self, data):
        for c in data:
            self.put_byte(c)
        return self

    def finish(self):
        """The flush: four bytes of low.  Returns the coded bytes."""
        low = self.low
        out = bytearray(self.out)
        for _ in range(4):
            out.append(low >> 24)
            low = (low << 8) & M32
        return bytes(out)


def model_encode(data):
    e = Encoder().encode(data)
    return e.finish(), e


def model_decode(coded, n, outside=None, lone=None):
    """(bytes, code_below_low): the decoder of the same model; bytes past the end of `coded` read as -1 (0xFFFFFFFF added into code), after which code can
    fall below low -- the reference then still decodes by comparing absolute values; code_below_low tells whether that state occurred at a decision.
    outside (a list) receives the bytes that begin with code outside [low, high] (cm.hip's `inside == false`); lone those among them with a range so small
    that exactly one of the root's two halves has range 0
    (bit 1: (range * P) >> 18 == 0 with range >= 2; bit 0: range == t + 1 with t >= 1).  cm.hip's fast walk tells a lane on the true path by d = code - low
    <= range; a lane whose range is 0 and that assumes a 0 next wraps to range 2^32 - 1 and looks valid again.  Here that happens in ONE of the four groups
    of lanes that share their first two bits, so one lane survives to the end: only `inside` (d <= range at the start of the byte) sends such a byte to the
    checked walk."""
    m = Encoder()
    pos = 0
    code = 0
    below = False

    def nxt():
        nonlocal pos
        if pos < len(coded):
            pos += 1
            return coded[pos - 1]
        return M32

    for _ in range(4):
        code = ((code << 8) + nxt()) & M32
    out = bytearray()
    for i in range(n):
        m.begin_byte()
        for k in range(8):
            mid = m.split()
            below = below or code < m.low
            if k == 0 and not m.low <= code <= m.high:
                r = m.high - m.low
                t = mid - m.low
                if outside is not None:
                    outside.append(i)
                if lone is not None and (t == 0 and r >= 2) != (r == t + 1 and t >= 1):
                    lone.append(i)
            bit = 1 if code <= mid else 0
            before = len(m.out)
            m.put(bit)
            for _e in range(len(m.out) - before):
                code = ((code << 8) + nxt()) & M32
        out.append(m.node & 255)
    return bytes(out), below


# ---- the encoder's fast-path scheme (cm.hip: cm_code_bits_raw, bucket_or_zero, code_byte) -------------------------------------------------------------
def shortcut_encode(trace, whole_guard=True, half_guard=True):
    """Coded bytes of the scheme from the (bit, p18) events of a trace.  Bit 1: range' = (range * P) >> 18; bit 0: range' = (range * (2^18 - P) - 1) >> 18 and
    low += range - range', all mod 2^32 and WITHOUT a test, 8 bits at a time; the byte is redone in halves when the final interval lies in one 2^24 bucket or
    (whole_guard) the range reached 0 on the way; a half is redone bit by bit under the same test (half_guard: its range-reached-0 part)."""
    out = bytearray()
    rng, low = M32, 0

    def raw(ev, r, l):
        rmin = M32
        for bit, p in ev:
            add = 0 if bit else (1 << 64) - 1
            r2 = ((r * (p if bit else (1 << 18) - p) + add) >> 18) & M32
            if not bit:
                l = (l + ((r - r2) & M32)) & M32
            r = r2
            rmin = min(rmin, r)
        return r, l, rmin

    def checked(ev, r, l):
        for e in ev:
            r, l, _ = raw([e], r, l)
            if r < TOP:
                while (l ^ ((l + r) & M32)) < TOP:
                    out.append(l >> 24)
                    l = (l << 8) & M32
                    r = ((r << 8) | 0xFF) & M32
        return r, l

    def bad(l, r, rmin, guard):
        return (l ^ ((l + r) & M32)) < TOP or (guard and rmin == 0)

    for b in range(0, len(trace), 8):
        ev = [(t.bit, t.p18) for t in trace[b:b + 8]]
        r4, l4, rmin4 = raw(ev[:4], rng, low)
        r, l, rmin = raw(ev[4:], r4, l4)
        rmin = min(rmin, rmin4)
        if not bad(l, r, rmin, whole_guard):
            rng, low = r, l
            continue
        if not bad(l4, r4, rmin4, half_guard):
            rng, low = r4, l4
        else:
            rng, low = checked(ev[:4], rng, low)
        r, l, rmin = raw(ev[4:], rng, low)
        if not bad(l, r, rmin, half_guard):
            rng, low = r, l
        else:
            rng, low = checked(ev[4:], rng, low)
    for _ in range(4):
        out.append(low >> 24)
        low = (low << 8) & M32
    return bytes(out)


# ---- straddle -----------------------------------------------------------------------------------------------------------------------------------------
def straddle(seed, n, force_one=False, prefix=b"", anti=0, mix=None):
    """n bytes (after `prefix` and `anti` bytes of the least probable bits) whose every bit keeps a multiple of 2^24 inside the interval where one half
    does.  force_one: the bit after a range-0 state, in the same byte, is a 1 (the greedy rule only ever follows it with a 0: after the four bytes the
    interval is [0, 2^32 - 1] and only a probability above 255 / 256 puts 0xFF000000 into the half of the 1)."""
    rng = np.random.default_rng(seed)
    coins = rng.integers(0, 2, size=8 * (n + anti) + 8).tolist()
    e = Encoder().encode(prefix)
    for _ in range(anti):
        e.begin_byte()
        for _k in range(8):
            e.put(0 if e.p18() >= (1 << 17) else 1)
    t = 0
    for x in range(n):
        e.begin_byte()
        zero = False
        for _k in range(8):
            mid = e.split()
            if mix and x % (mix[0] + mix[1]) >= mix[0]:   # mix = (s, a): after every s bytes of the rule, a bytes of the least probable bits
                e.put(0 if e.p18() >= (1 << 17) else 1)
                continue
            b = e.high & ~(TOP - 1) & M32          # the multiple of 2^24 in (low, high]: after a renormalisation low and high differ in the top byte
            if zero and force_one:
                bit = 1
            elif mid >= b > e.low:
                bit = 1                            # [low, mid] contains b - 1 and b
            elif mid + 2 <= b:
                bit = 0                            # [mid + 1, high] does
            else:
                bit = coins[t]
                t += 1
            e.put(bit)
            zero = e.trace[-1].rng == 0
    return bytes(_bytes_of(e.trace)), e


def _bytes_of(trace):
    out = bytearray()
    for b in range(0, len(trace), 8):
        c = 0
        for t in trace[b:b + 8]:
            c = c * 2 + t.bit
        out.append(c)
    return out


def bursts(trace, least=3):
    """(output offset, length, input byte) of every renormalisation that emitted `least` bytes or more at one bit."""
    return [(t.at, t.emitted, t.i) for t in trace if t.emitted >= least]


def zero_states(trace):
    """{(k, following bit in the same byte or None)} over the bits after which the range was 0 before the renormalisation."""
    got = set()
    for x, t in enumerate(trace):
        if t.rng == 0:
            got.add((t.k, trace[x + 1].bit if t.k < 7 and x + 1 < len(trace) else None))
    return got


STRADDLE_NAMES = ["straddle_s%d" % s for s in range(1, 7)] + ["straddle_one_s11", "straddle_one_s12", "straddle_ends_in_zero"]


def build_straddle():
    cases = {}
    for seed in range(1, 7):
        cases["straddle_s%d" % seed] = straddle(seed, 600)[0]
    for seed in (11, 12):
        cases["straddle_one_s%d" % seed] = straddle(seed, 600, force_one=True)[0]
    # the block's last byte ends in range 0 (the flush follows a four-byte burst directly)
    d, e = straddle(3, 600)
    last = max(t.i for t in e.trace if t.k == 7 and t.rng == 0)
    cases["straddle_ends_in_zero"] = d[:last + 1]
    assert list(cases) == STRADDLE_NAMES
    return cases


# ---- seams --------------------------------------------------------------------------------------------------------------------------------------------
SEAM_LENGTHS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129]
SEAM_LEN = 76    # chunks of 32, 32 and a ragged 12: the runs around 64 lie in the last, partial chunk; those around 32 cross two full ones


def _background(seed, n):
    """A skewed source over 24 values in which no byte repeats its predecessor (no run of its own)."""
    rng = np.random.default_rng(seed)
    v = (rng.permutation(200)[:24] + 30).astype(np.uint8)
    p = 1.0 / np.arange(1, 25)
    x = v[rng.choice(24, size=n, p=p / p.sum())].tolist()
    for i in range(1, n):
        if x[i] == x[i - 1]:
            x[i] = int(v[(int(np.where(v == x[i])[0][0]) + 1) % 24])
    return x


def build_seams():
    """name -> (bytes, pre-seam position or None).  Where a position is given, the CPU test asserts that changing the byte there changes the run flag of a byte
    at or behind the seam: the flag depends on a byte of the previous chunk (hist, hrow1 / hrow2).  The other run cases are the negative ones: a run
    that ends before the seam, begins behind it or is too short must not set a flag across it (the model's flags are checked against their definition)."""
    cases = {}
    for n in SEAM_LENGTHS:
        cases["seam_len%d" % n] = (bytes(_background(100 + n, n)), None)
    placed = set()
    for run in range(2, 7):
        for off in range(-4, 5):
            placed.add((off - run, run))   # ends at seam + off (its last byte at seam + off - 1)
            placed.add((off, run))         # begins at seam + off
    for start, run in sorted(placed):
        x = _background(7 * run + start + 50, SEAM_LEN)
        for seam, val in ((32, 0xA5), (64, 0x3C)):
            for q in range(seam + start, seam + start + run):
                x[q] = val
            for q in (seam + start - 1, seam + start + run):   # the neighbours differ from the run: its length is exact
                if x[q] == val:
                    x[q] = val ^ 1
        # a flag at seam + k (k = 0 .. 3) needs the four equal bytes seam + k - 4 .. seam + k - 1, of which seam - 1 lies in front of the seam: a run of four or
        # more that holds byte seam - 1 and ends at the seam or behind it
        crosses = run >= 4 and start <= -1 and start + run >= 0
        cases["seam_run%d_at%+d" % (run, start)] = (bytes(x), (31, 63) if crosses else None)
    for z in range(0, 6):   # the history before the block is zeros: with two leading zeros the flag is set at byte 2
        cases["seam_zeros%d" % z] = (bytes([0] * z + _background(300 + z, 40 - z)), None)
    return cases


def flags_by_definition(data):
    """Run flag of byte i: i >= 2 and bytes i-1 .. i-4 equal, the bytes before the block being zeros (cm.hip, the model wave)."""
    h = [0, 0, 0, 0] + list(data)
    return [1 if i >= 2 and h[i + 3] == h[i + 2] == h[i + 1] == h[i] else 0 for i in range(len(data))]


# ---- extremes -----------------------------------------------------------------------------------------------------------------------------------------
def build_extremes():
    a = 0x61   # 0110 0001: the root always sees a 0, the level-1 node (node 2) always a 1
    flip_root = a ^ 0x80       # a 1 at the root where a 0 is all but certain: P18_MIN coded with a 1
    flip_l1 = a ^ 0x40         # a 0 at node 2 where a 1 is all but certain: P18_MAX coded with a 0
    run = bytes([a]) * 700     # run flag 1: C0, C1[a] and the flag-1 C2 rows at their fixed points in both directions (0 bits: down, 1 bits: up)
    alt = bytes([a, a ^ 1]) * 400   # never a run: the flag-0 C2 rows, the rows C1[a] and C1[a ^ 1]
    cases = {
        "extremes_run": run + bytes([flip_root]) + bytes([a]) * 40 + bytes([flip_l1]) + bytes([a]) * 40,
        "extremes_alternating": alt + bytes([flip_root, a, a ^ 1, a, flip_l1, a, a ^ 1]) * 3,
        "extremes_ff_00": b"\xff" * 500 + b"\x00" * 500 + b"\xff" * 8 + b"\x00\xff" * 20,
    }
    return cases


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------------------
class RowDirectory:
    """The cache directory by the documented rule (cm.hip "Row cache"): byte value -> slot; slot 0 belongs to value 0 from the start; slots are handed out in
    order of first use, then recycled FIFO, skipping pinned rows."""

    def __init__(self, rows):
        self.rows = rows
        self.slot_of = {0: 0}
        self.sym_of = {0: 0}
        self.spilled = set()
        self.nused, self.hand = 1, 0
        self.misses = self.recycled = 0
        self.reloaded = set()

    def fetch(self, sym, pinned):
        if self.nused < self.rows:
            slot = self.nused
            self.nused += 1
        else:
            while True:
                slot = self.hand
                self.hand = (self.hand + 1) % self.rows
                if slot not in pinned:
                    break
            victim = self.sym_of[slot]
            del self.slot_of[victim]
            self.spilled.add(victim)
            self.recycled += 1
        if sym in self.spilled:
            self.spilled.discard(sym)
            self.reloaded.add(sym)
        self.slot_of[sym] = slot
        self.sym_of[slot] = sym
        self.misses += 1
        return slot


def encoder_rows(data, rows, base, shift):
    """(given_up, directory): the encoder's model wave, chunk by chunk.  A chunk pins the resident rows of its bytes and of the two bytes before it, then
    fetches the missing ones in the order of their first lane; the budget is tested once per chunk, after its fetches, against the chunk's first position."""
    d = RowDirectory(rows)
    h1 = h2 = 0   # slots of bytes -1 and -2 (only moved on after a full chunk, like the kernel's)
    for b in range(0, len(data), CM_CHUNK):
        chunk = data[b:b + CM_CHUNK]
        if any(c not in d.slot_of for c in chunk):
            pinned = {d.slot_of[c] for c in chunk if c in d.slot_of} | {h1, h2}
            for c in chunk:
                if c not in d.slot_of:
                    pinned.add(d.fetch(c, pinned))
            if d.misses > base + (b >> shift):
                return True, d
        if len(chunk) == CM_CHUNK:
            h1, h2 = d.slot_of[chunk[-1]], d.slot_of[chunk[-2]]
    return False, d


def decoder_rows(data, rows, base, shift):
    """(given_up, directory): the decoder's model waves.  Step i (1 <= i < n) learns byte i - 1; when it differs from byte i - 2 (0 before the block) its row
    is looked up, fetched with only the row of byte i - 2 pinned, and the budget is tested against i.  The last byte is never looked up."""
    d = RowDirectory(rows)
    g = 0
    for i in range(1, len(data)):
        c = data[i - 1]
        if c != g:
            if c not in d.slot_of:
                d.fetch(c, {d.slot_of[g]})
                if d.misses > base + (i >> shift):
                    return True, d
            g = c
    return False, d


def cyclic(values, n):
    return bytes(values[i % len(values)] for i in range(n))


def budget_boundary(side, mode, values):
    """The shortest cyclic block over `values` that the rule gives up on `side` ("enc" / "dec") in cm mode `mode`; the block one byte shorter is kept."""
    rows = (ROWS_ENC if side == "enc" else ROWS_DEC)[mode]
    sim = encoder_rows if side == "enc" else decoder_rows
    base, shift = BUDGET[mode]
    for n in range(1, 4096):
        if sim(cyclic(values, n), rows, base, shift)[0]:
            assert not sim(cyclic(values, n - 1), rows, base, shift)[0]
            return n
    raise AssertionError("never given up")


THRASH = list(range(1, 130))   # 129 values, none of them 0: more than the largest cache (96) plus a chunk


def build_rows():
    """name -> (bytes, {(side, mode): expected change of the given-up counter} for the modes the case speaks about)."""
    cases = {}
    # (a) cyclic over V = R + 33 values: every chunk brings 32 new rows, every row comes back from the spill area; kept (all-miss, but short)
    for r, modes, n in ((96, (1,), 3 * 129), (56, (2,), 3 * 89)):
        v = list(range(1, r + 34))
        cases["rows_cyclic_R%d" % r] = (cyclic(v, n), {(s, m): 0 for m in modes for s in ("enc", "dec")})
    # the 40-row test cache gives up beyond 64 + position / 8 misses: the cycle is over runs of 12 (one miss in 12 bytes), two rounds over 73 values
    cases["rows_cyclic_R40"] = (bytes(v for _ in range(2) for v in range(1, 74) for _ in range(12)), {("enc", 9): 0, ("dec", 9): 0})
    # (b) the budget boundary of each side and mode
    for side in ("enc", "dec"):
        for mode in (1, 2, 9):
            n = budget_boundary(side, mode, THRASH)
            other = "dec" if side == "enc" else "enc"
            for length, moved in ((n - 1, 0), (n, 1)):
                name = "rows_budget_%s_m%d_%s" % (side, mode, "kept" if moved == 0 else "given_up")
                d = cyclic(THRASH, length)
                base, shift = BUDGET[mode]
                o_rows = (ROWS_ENC if other == "enc" else ROWS_DEC)[mode]
                o_up = (encoder_rows if other == "enc" else decoder_rows)(d, o_rows, base, shift)[0]
                cases[name] = (d, {(side, mode): moved, (other, mode): int(o_up)})
    # (c) value 0 late: slot 0 (pre-assigned to value 0, never touched) is recycled, then 0 arrives and its virgin row comes back from the spill area
    cases["rows_zero_late"] = (cyclic(list(range(1, 130)), 200) + bytes([0, 7, 0, 0, 9]) + cyclic(list(range(1, 130)), 60) + b"\0" * 6, {})
    # (d) exactly R and R + 1 distinct values (value 0 among them: its slot is one of the R)
    for r in (40, 44, 56, 96):
        cases["rows_exactly_R%d" % r] = (cyclic(list(range(0, r)), 3 * r + 5), {})
        cases["rows_R%d_plus_1" % r] = (cyclic(list(range(0, r + 1)), 3 * r + 5), {})
    return cases


# ---- sink ---------------------------------------------------------------------------------------------------------------------------------------------
def sink_switch(trace, n, gap, chunk=CM_CHUNK):
    """(sw, side bytes needed): CmSink by its comment.  An output byte emitted while input byte i is coded may be stored in place only below the input
    that is in registers by then, the chunks up to and including the one that holds i: the first byte at an offset >= gap + min(n, (i | 31) + 1) and
    everything after it goes to the side buffer.  sw None: never switches.  (chunk = 1: the rule of a sink that counts only the bytes up to i as loaded.)"""
    emitted = [t.i for t in trace for _ in range(t.emitted)] + [n - 1] * 4   # the flush counts as the last byte's
    for op, i in enumerate(emitted):
        if op >= gap + min(n, (i | (chunk - 1)) + 1):
            return op, len(emitted) - op
    return None, 0


def build_sink():
    """name -> (bytes, gap).  The side bytes needed follow from sink_switch; the CPU test asserts them against the switch the family is named for."""
    cases = {}
    # noise, then a run: every byte of noise costs a little more than eight bits, so the output creeps up on the input and the sink switches late in the noise;
    # the run that follows goes to the side buffer although it shrinks.  The gap is the largest, at most four below the largest lead the output ever has,
    # at which a sink that counted only the bytes up to i as loaded (not the whole chunk) would switch at another byte.
    d = bytes(np.random.default_rng(8).integers(0, 256, size=1200, dtype=np.uint8)) + b"\x55" * 700
    e = Encoder().encode(d)
    emitted = [t.i for t in e.trace for _ in range(t.emitted)] + [len(d) - 1] * 4
    lead = max(op - min(len(d), (i | (CM_CHUNK - 1)) + 1) for op, i in enumerate(emitted))
    gap = next(g for g in range(lead - 4, 0, -1) if sink_switch(e.trace, len(d), g, 1)[0] != sink_switch(e.trace, len(d), g)[0])
    cases["sink_expands_then_run"] = (d, gap)
    # a straddle block behind an expanding prefix, the gap chosen so that the switch falls INSIDE a four-byte burst
    # (a straddle block alone shrinks, its output never catches up with its input: after every six bytes of the rule come three of the least probable bits)
    pick = None
    for seed in range(5, 40):
        d, e = straddle(seed, 500, anti=32, mix=(6, 3))
        n = len(d)
        for at, length, i in bursts(e.trace, 4):
            for inside in (1, 2, 3):
                gap = at + inside - min(n, (i | (CM_CHUNK - 1)) + 1)
                if gap >= 0 and sink_switch(e.trace, n, gap)[0] == at + inside:
                    pick = gap
        if pick is not None:
            break
    assert pick is not None, "no burst of four bytes can carry the switch"
    cases["sink_burst_crosses_switch"] = (d, pick)
    cases["sink_gap0_compressible"] = (b"abcabcabd" * 100, 0)
    return cases


# ---- windows ------------------------------------------------------------------------------------------------------------------------------------------
WINDOW_SIZES = [4, 5, 63, 64, 65, 127, 128, 129]   # (a coded block is never shorter than its 4-byte flush: 0 .. 3 are reached by the truncations)


def build_windows(oracle):
    """name -> plain bytes whose coded size is exactly the size in the name."""
    cases = {}
    for want in WINDOW_SIZES:
        found = None
        for seed in range(40):
            src = bytes(_background(900 + seed, 400))
            for n in range(0, 400):
                got = len(oracle.cm_encode(src[:n]))
                if got == want:
                    found = src[:n]
                    break
                if got > want:
                    break
            if found is not None:
                break
        assert found is not None, want
        cases["window_coded%d" % want] = found
    return cases


def truncations(coded, n_plain):
    """[(cut, bytes to decode)]: a coded stream cut to each of its last 8 lengths and to 0 .. 4 bytes.  Behind a cut of 0 .. 4 bytes everything the decoder
    reads is the -1 fill: 160 bytes of that say what 600 would."""
    n = len(coded)
    return sorted({(k, n_plain) for k in range(max(0, n - 8), n)} | {(k, min(n_plain, 160)) for k in range(0, 5) if k <= n})


def below_low_stream():
    """A stream on which the decoder reaches code < low: a straddle block's coded bytes cut where the decoder sits at code == low == high (range 0) and the
    next byte it reads is the -1 past the end.  (Random junk does not get there: 240 seeded streams of 2 .. 150 bytes never did.)  Returns (stream, n)."""
    _, e = straddle(1, 600)
    c = e.finish()
    for k in range(60, 200):
        if model_decode(c[:k], 300)[1]:
            return c[:k], 300
    raise AssertionError("no cut reaches code < low")


# ---- generic inputs in the style of the older tests ------------------------------------------------------------------------------------------------------
def generic_inputs():
    rng = np.random.default_rng(2)
    vals = rng.integers(0, 256, size=120, dtype=np.uint8)
    lens = rng.integers(1, 71, size=120)
    return {
        "random2600": bytes(rng.integers(0, 256, size=2600, dtype=np.uint8)),
        "a3000": b"a" * 3000,
        "runs_1_70": bytes(np.repeat(vals, lens)[:3000]),
        "skewed4_20000": bytes(np.array([3, 200, 17, 90], dtype=np.uint8)[rng.choice(4, size=20000, p=[0.7, 0.2, 0.07, 0.03])]),
    }


_TABLE = {}


def build(oracle):
    """Every family, built once per process: {family: {name: ...}}."""
    if not _TABLE:
        _TABLE["straddle"] = build_straddle()
        _TABLE["seams"] = build_seams()
        _TABLE["extremes"] = build_extremes()
        _TABLE["rows"] = build_rows()
        _TABLE["sink"] = build_sink()
        _TABLE["windows"] = build_windows(oracle)
        _TABLE["below_low"] = below_low_stream()
    return _TABLE


def plain_cases(oracle):
    """name -> bytes of every case of every family (what goes through encode and decode in every mode)."""
    t = build(oracle)
    out = dict(t["straddle"])
    out.update({k: v[0] for k, v in t["seams"].items()})
    out.update(t["extremes"])
    out.update({k: v[0] for k, v in t["rows"].items()})
    out.update({k: v[0] for k, v in t["sink"].items()})
    out.update(t["windows"])
    return out


# ---- the checks, shared by the emulator tests and the -m gpu tests ------------------------------------------------------------------------------------------
def family_cases(oracle, family):
    t = build(oracle)[family]
    return {k: (v[0] if isinstance(v, tuple) else v) for k, v in t.items()}


def text_case(oracle):
    return oracle.bwt(datagen.shakespeare()[100000:100700])[1]


def expected_given_up(d, side, mode):
    if mode == 0:
        return 0
    rows = (ROWS_ENC if side == "enc" else ROWS_DEC)[mode]
    return int((encoder_rows if side == "enc" else decoder_rows)(d, rows, *BUDGET[mode])[0])


def run_family(lib, oracle, family, mode):
    """Encode equals the oracle, decode returns the plain bytes, and the given-up counter moves as the documented rule of the directory says."""
    g = bzip3_amd.StageApi(lib)
    try:
        assert lib.bz3_hip_set_cm_mode(mode) == 0
        for name, d in family_cases(oracle, family).items():
            coded = oracle.cm_encode(d)
            n0 = lib.bz3_hip_cm_blocks_given_up()
            assert g.cm_encode(d) == coded, (name, mode)
            n1 = lib.bz3_hip_cm_blocks_given_up()
            if d:
                assert g.cm_decode(coded, len(d)) == d, (name, mode)
            n2 = lib.bz3_hip_cm_blocks_given_up()
            want = (expected_given_up(d, "enc", mode), expected_given_up(d, "dec", mode) if d else 0)
            assert (n1 - n0, n2 - n1) == want, (name, mode, (n1 - n0, n2 - n1), want)
            if family == "rows":
                for (side, m), moved in build(oracle)["rows"][name][1].items():
                    assert m != mode or want[0 if side == "enc" else 1] == moved, (name, side, m)
    finally:
        lib.bz3_hip_set_cm_mode(-1)


TRUNCATED = STRADDLE_NAMES + ["text", "below_low"]


def run_truncations(lib, oracle, mode, name):
    """The decoder on a stream that ends early equals the oracle's: the -1 fill, code < low, `inside == false`."""
    g = bzip3_amd.StageApi(lib)
    try:
        assert lib.bz3_hip_set_cm_mode(mode) == 0
        if name == "below_low":
            stream, n = build(oracle)["below_low"]
            assert g.cm_decode(stream, n) == oracle.cm_decode(stream, n), mode
            return
        d = text_case(oracle) if name == "text" else build(oracle)["straddle"][name]
        coded = oracle.cm_encode(d)
        for cut, n in truncations(coded, len(d)):
            assert g.cm_decode(coded[:cut], n) == oracle.cm_decode(coded[:cut], n), (name, cut, mode)
    finally:
        lib.bz3_hip_set_cm_mode(-1)


def sink_encode(lib, d, gap, side):
    os.environ["BZ3_CM_TEST_GAP"], os.environ["BZ3_CM_TEST_SIDE"] = str(gap), str(side)
    try:
        out = (C.c_uint8 * (len(d) + len(d) // 50 + 200))()
        n = lib.bz3_hip_stage_cm_encode(bzip3_amd._cbuf(d, len(d)), len(d), out)
        return n, (C.string_at(out, n) if n > 0 else b"")
    finally:
        os.environ.pop("BZ3_CM_TEST_GAP", None)
        os.environ.pop("BZ3_CM_TEST_SIDE", None)


def run_sink(lib, oracle, mode):
    """In place: the oracle's bytes with exactly the side bytes the rule asks for, -1 with one fewer."""
    try:
        assert lib.bz3_hip_set_cm_mode(mode) == 0
        for name, (d, gap) in build(oracle)["sink"].items():
            coded = oracle.cm_encode(d)
            sw, need = sink_switch(model_encode(d)[1].trace, len(d), gap)
            assert sink_encode(lib, d, gap, need) == (len(coded), coded), (name, mode, need)
            if need:
                assert sink_encode(lib, d, gap, need - 1)[0] == -1, (name, mode, need)
    finally:
        lib.bz3_hip_set_cm_mode(-1)


def run_sink_thrash(lib, oracle, mode):
    """A thrashing block in place: with a gap of 4096 or less the coded bytes may already lie on input the full-model kernel would need again, so the row
    cache must see the block through (abort_limit 0); with a large gap it gives it up, once."""
    d = cyclic(THRASH, 1400)
    assert expected_given_up(d, "enc", mode) == 1
    coded = oracle.cm_encode(d)
    try:
        assert lib.bz3_hip_set_cm_mode(mode) == 0
        for gap, moved in ((4096, 0), (3000, 0), (16384, 1)):
            n0 = lib.bz3_hip_cm_blocks_given_up()
            assert sink_encode(lib, d, gap, 65536) == (len(coded), coded), (mode, gap)
            assert lib.bz3_hip_cm_blocks_given_up() - n0 == moved, (mode, gap)
    finally:
        lib.bz3_hip_set_cm_mode(-1)
