"""CPU: the preconditions of tests/cm_cases.py (every family reaches the mechanism it is named for, proved with the Python model of the coder, which is itself
held against the oracle), and every case through the emulated kernels of cm.hip in modes 0 (whole model), 9 (the emulator's 40-row cache), 1 and 2 (the
shipped caches).  Expected bytes: the oracle's.  tests/test_gpu_cm_cases.py runs the same table on hardware."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import bzip3_amd
import cm_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = (0, 9, 1, 2)
FAMILIES = ("straddle", "seams", "extremes", "rows", "sink", "windows")


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


@pytest.fixture(scope="module")
def table(oracle):
    return cc.build(oracle)


@pytest.fixture(scope="module")
def traces(oracle, table):
    """name -> Encoder after the case; the model's bytes equal the oracle's on every one of them (asserted here, once)."""
    out = {}
    for name, d in cc.plain_cases(oracle).items():
        coded, e = cc.model_encode(d)
        assert coded == oracle.cm_encode(d), name
        out[name] = e
    return out


# ---- the model and the preconditions ---------------------------------------------------------------------------------------------------------------------
def test_model_equals_oracle_and_generic_inputs_never_reach_a_zero_range(oracle, traces):
    """The model reproduces the oracle on the four inputs in the style of the older CM tests as well -- and on none of them does the range before a
    renormalisation come anywhere near 0: the states the straddle family is built for are not in them."""
    for name, d in cc.generic_inputs().items():
        coded, e = cc.model_encode(d)
        assert coded == oracle.cm_encode(d), name
        assert cc.model_decode(coded, len(d)) == (d, False), name
        smallest = min(t.rng for t in e.trace)
        print(name, "smallest range before a renormalisation", smallest)
        assert smallest > 256, name


def test_straddle_preconditions(oracle, table, traces):
    zero, residues, spans, ones = set(), set(), set(), False
    for name, d in table["straddle"].items():
        tr = traces[name].trace
        assert len(d) < cc.CM_MISS_BASE, name   # no row cache can give it up: fewer bytes than the budget has misses
        z = cc.zero_states(tr)
        assert z, name
        zero |= z
        ones = ones or any(t.rng == 1 for t in tr)
        for at, length, _ in cc.bursts(tr):
            residues.add(at % 64)
            spans.add((at, at + length - 1))
        assert cc.shortcut_encode(tr) == oracle.cm_encode(d), name   # the scheme with both guards is right
    for k in range(8):   # range 0 after every bit position; up to bit 6 followed, in the same byte, by a 0 and by a 1
        assert (k, None) in zero if k == 7 else {(k, 0), (k, 1)} <= zero, (k, sorted(zero, key=str))
    assert ones, "range 1 never reached"
    assert residues == set(range(64)), sorted(set(range(64)) - residues)   # 61, 62, 63 among them; 57 .. 59 are 61 .. 63 of the decoder, four bytes ahead
    for edge in (64, 128):
        assert any(a < edge <= b for a, b in spans), edge
    # the last byte of the block ends in range 0: the flush follows the burst
    last = traces["straddle_ends_in_zero"].trace[-1]
    assert (last.k, last.rng, last.emitted) == (7, 0, 4)
    # the two wrong encoders are told apart from the right one
    for kw in ({"whole_guard": False}, {"half_guard": False}):
        differ = [name for name, d in table["straddle"].items() if cc.shortcut_encode(traces[name].trace, **kw) != oracle.cm_encode(d)]
        print(kw, "differs on", len(differ), "of", len(table["straddle"]))
        assert differ, kw
    # and nothing else in the table would have: without the straddle family both guards are dead code
    for fam in ("seams", "extremes", "windows"):
        for name, d in cc.family_cases(oracle, fam).items():
            assert cc.shortcut_encode(traces[name].trace, whole_guard=False, half_guard=False) == oracle.cm_encode(d), name


def test_seams_preconditions(oracle, table, traces):
    assert [len(table["seams"]["seam_len%d" % n][0]) for n in cc.SEAM_LENGTHS] == cc.SEAM_LENGTHS
    crossing = 0
    for name, (d, pre) in table["seams"].items():
        assert traces[name].flags == cc.flags_by_definition(d), name
        if pre is None:
            continue
        crossing += 1
        for p in pre:   # the flag of a byte at or behind the seam depends on the byte in front of it
            seam = p + 1
            other = bytearray(d)
            other[p] ^= 0x10
            f0, f1 = cc.flags_by_definition(d), cc.flags_by_definition(bytes(other))
            assert any(f0[i] != f1[i] for i in range(seam, min(seam + 4, len(d)))), (name, p)
            assert cc.Encoder().encode(bytes(other)).flags == f1
    assert crossing >= 10
    # runs of 2 .. 6 ending and beginning at every offset -4 .. +4
    names = set(table["seams"])
    for run in range(2, 7):
        for off in range(-4, 5):
            assert "seam_run%d_at%+d" % (run, off) in names and "seam_run%d_at%+d" % (run, off - run) in names
    for z in range(6):   # leading zeros: the flag at byte 2 needs bytes 0 and 1 to be zero (the history before the block is)
        d = table["seams"]["seam_zeros%d" % z][0]
        assert d[:z] == bytes(z) and (len(d) <= z or d[z] != 0)
        assert traces["seam_zeros%d" % z].flags[2] == (1 if z >= 2 else 0)


def test_extremes_preconditions(table, traces):
    for name in table["extremes"]:
        e = traces[name]
        flag = 0 if name == "extremes_alternating" else 1
        want = {("c0", "low"), ("c0", "high"), ("c1", "low"), ("c1", "high"), ("c2", "low", flag, 0), ("c2", "high", flag, 15)}
        assert want <= e.fixed, (name, sorted(want - e.fixed, key=str))
        met = {(t.p18, t.bit) for t in e.trace if t.p18 in (cc.P18_MIN, cc.P18_MAX)}
        assert met == {(cc.P18_MIN, 0), (cc.P18_MIN, 1), (cc.P18_MAX, 0), (cc.P18_MAX, 1)}, (name, met)
        assert min(t.p18 for t in e.trace) == cc.P18_MIN and max(t.p18 for t in e.trace) == cc.P18_MAX, name
        assert 15 in {t.j for t in e.trace}, name   # cells 15 and 16: the cell that starts at 65535 is read
    assert {"extremes_run", "extremes_alternating"} <= set(table["extremes"])


def test_rows_preconditions(table):
    rows = table["rows"]
    for r, mode in ((96, 1), (56, 2)):
        d = rows["rows_cyclic_R%d" % r][0]
        values = set(d)
        assert len(values) > r + 32 and len(values) > cc.ROWS_ENC[mode] + 32
        for sim, size in ((cc.encoder_rows, cc.ROWS_ENC[mode]), (cc.decoder_rows, cc.ROWS_DEC[mode])):
            up, dr = sim(d, size, *cc.BUDGET[mode])
            assert not up and dr.reloaded == values, (r, sim.__name__, len(dr.reloaded))   # every row came back from the spill area
    up, dr = cc.encoder_rows(rows["rows_cyclic_R40"][0], 40, *cc.BUDGET[9])
    assert not up and len(set(rows["rows_cyclic_R40"][0])) == 73 and len(dr.reloaded) == 73
    up, dr = cc.decoder_rows(rows["rows_cyclic_R40"][0], 40, *cc.BUDGET[9])
    assert not up and len(dr.reloaded) == 73
    # the budget boundary: one byte apart, and the hand count for the encoder at 1024 / 5
    for side in ("enc", "dec"):
        for mode in (1, 2, 9):
            kept, lost = (rows["rows_budget_%s_m%d_%s" % (side, mode, w)] for w in ("kept", "given_up"))
            assert len(lost[0]) == len(kept[0]) + 1 and kept[1][(side, mode)] == 0 and lost[1][(side, mode)] == 1
            print("budget boundary", side, "mode", mode, "kept", len(kept[0]), "given up", len(lost[0]))
    assert (len(rows["rows_budget_enc_m1_kept"][0]), len(rows["rows_budget_enc_m1_given_up"][0])) == (1057, 1058)
    # value 0 late: its untouched row was spilled (slot 0 recycled) and came back
    for sim, size in ((cc.encoder_rows, 96), (cc.encoder_rows, 44), (cc.decoder_rows, 56), (cc.decoder_rows, 96), (cc.encoder_rows, 40)):
        assert 0 in sim(rows["rows_zero_late"][0], size, 1 << 30, 0)[1].reloaded, (sim.__name__, size)
    # exactly R values: first touches only; R + 1: slots are recycled
    for r in (40, 44, 56, 96):
        for sim in (cc.encoder_rows, cc.decoder_rows):
            fit = sim(rows["rows_exactly_R%d" % r][0], r, 1 << 30, 0)[1]
            over = sim(rows["rows_R%d_plus_1" % r][0], r, 1 << 30, 0)[1]
            assert (fit.recycled, fit.misses) == (0, r - 1) and over.recycled > 0 and over.reloaded, (r, sim.__name__)


def test_sink_preconditions(oracle, table, traces):
    def switch(name):
        d, gap = table["sink"][name]
        return cc.sink_switch(traces[name].trace, len(d), gap)

    d, gap = table["sink"]["sink_expands_then_run"]
    sw, side = switch("sink_expands_then_run")
    assert sw is not None and sw < 1200 + 40 and side > 8 and len(oracle.cm_encode(d)) < len(d)   # switches in the noise although the block shrinks
    early = cc.sink_switch(traces["sink_expands_then_run"].trace, len(d), gap, chunk=1)
    assert early[0] < sw and early[1] > side   # the bytes of the chunk that are loaded but not coded yet count: without them the switch comes earlier
    d, gap = table["sink"]["sink_burst_crosses_switch"]
    sw, side = switch("sink_burst_crosses_switch")
    assert any(at < sw < at + 4 for at, length, _ in cc.bursts(traces["sink_burst_crosses_switch"].trace, 4)), sw   # inside a four-byte burst
    assert switch("sink_gap0_compressible") == (None, 0)
    for name in table["sink"]:
        print(name, "gap", table["sink"][name][1], "sw, side bytes", switch(name))


def test_windows_preconditions(oracle, table):
    for want in cc.WINDOW_SIZES:
        assert len(oracle.cm_encode(table["windows"]["window_coded%d" % want])) == want
    stream, n = table["below_low"]
    outside, lone = [], []
    got, below = cc.model_decode(stream, n, outside, lone)
    assert below and got == oracle.cm_decode(stream, n)
    # bytes that BEGIN with code outside the interval: the walker's `inside == false`.  None of them is of the kind on which `inside` alone decides (see
    # model_decode and DESIGN.md, mutant D2): no stream of this table is, and the test says so instead of leaving it to be assumed.
    print("bytes that begin with code outside [low, high]:", len(outside), "lone survivors:", len(lone))
    assert outside and not lone   # (low only shifts while code < low: after four renormalisations it is 0 and the state is over)
    d = table["straddle"]["straddle_s2"]
    coded = oracle.cm_encode(d)
    for cut, n in cc.truncations(coded, len(d)):   # the model decoder follows the oracle through the -1 fill as well
        assert cc.model_decode(coded[:cut], n)[0] == oracle.cm_decode(coded[:cut], n), cut


# ---- every case through the emulated kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_kernels_on_every_case(emu, oracle, mode, family):
    cc.run_family(emu, oracle, family, mode)


@pytest.mark.parametrize("name", cc.TRUNCATED)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_decoder_on_truncated_streams(emu, oracle, mode, name):
    cc.run_truncations(emu, oracle, mode, name)


@pytest.mark.parametrize("mode", MODES)
def test_emulated_sink(emu, oracle, mode):
    cc.run_sink(emu, oracle, mode)
    if mode:
        cc.run_sink_thrash(emu, oracle, mode)


def test_straddle_and_rows_survive_stalled_waves(oracle):
    """One straddle and one rows case under the stalled-wave scheduler (cf. test_cm_protocols_survive_stalled_waves): bursts of four bytes and row fetches while
    whole waves sleep.  In a subprocess: the scheduler mode is fixed when the library is loaded."""
    code = r'''
import sys, ctypes as C
sys.path[:0] = [%r, %r, %r]
import bzip3_amd, cm_cases as cc
from build_emu import build
from oracle_lib import Oracle
lib = bzip3_amd._declare(C.CDLL(build()))
o, g = Oracle(), bzip3_amd.StageApi(lib)
for d in (cc.build_straddle()["straddle_one_s11"][:300], cc.build_rows()["rows_cyclic_R56"][0]):
    c = o.cm_encode(d)
    for mode in (0, 9, 1, 2):
        assert lib.bz3_hip_set_cm_mode(mode) == 0
        assert g.cm_encode(d) == c and g.cm_decode(c, len(d)) == d, mode
        assert g.cm_decode(c[: len(c) - 3], len(d)) == o.cm_decode(c[: len(c) - 3], len(d)), mode
print("ok")
''' % (os.path.dirname(HERE), HERE, os.path.join(HERE, "emu"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BZ3_EMU_SCHED="-3"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-300:], r.stderr[-800:])
