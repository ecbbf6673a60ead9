"""CPU tests of the LZP encoder cases (tests/lzp_cases.py): the oracle against the real reference, the preconditions that make every
case hit what it aims at (from the oracle's own match list, so that a case cannot go stale silently), and the kernel sources under the
emulator -- bytes and the driver's record (bz3_hip_debug_lzp_encode).  tests/test_gpu_lzp_cases.py runs the same cases on the device."""
import ctypes as C
import os
import sys

import pytest

import bzip3_amd
import lzp_cases as L

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


@pytest.fixture(scope="module")
def cases():
    return L.stage_cases()


def _matches(oracle, data):
    return oracle.lzp_matches(data)


def test_oracle_equals_the_reference_on_every_case(oracle, ref_stages, cases):
    for name, d in list(cases.items()) + list(L.ends().items()):
        assert oracle.lzp_encode(d) == ref_stages.lzp_encode(d), name


def test_match_list_is_the_encoders(oracle, cases):
    """orc_lzp_matches shares its loop with orc_lzp_encode: replaying the list over the input gives the encoder's bytes."""
    for name in ("collide", "lens", "long", "farflag-3000-1"):
        d = cases[name]
        n, z = oracle.lzp_encode(d)
        m = dict(oracle.lzp_matches(d))
        out, p = bytearray(d[:4]), 4
        tab = {}
        while p < len(d):
            h = L.lz_hash(L.ctx_of(d[p - 4 : p]))
            c, tab[h] = tab.get(h, 0), p
            if p in m:
                rest = m[p] - L.LZ_MIN
                out += bytes([L.ESC]) + b"\xfe" * (rest // 254) + bytes([rest % 254])
                p += m[p]
            else:
                out.append(d[p])
                if d[p] == L.ESC and c > 0:
                    out.append(255)
                p += 1
        assert (len(out), bytes(out)) == (n, z), name


def test_lzp_applies_to_every_stage_case(oracle, cases):
    assert tuple(sorted(cases)) == tuple(sorted(L.STAGE_NAMES))
    for name, d in cases.items():
        n, z = oracle.lzp_encode(d)
        assert 0 < n == len(z) < len(d) - 8, name


def test_capcut_preconditions(oracle):
    d, mpos = L.capcut()
    m = _matches(oracle, d)
    assert mpos < L.WINDOW and L.windows_of(len(d)) == 1  # the match lies in the first bitmap window
    assert any(p == mpos and ln >= 390 for p, ln in m), m
    before = [x for x in m if x[0] < mpos]
    assert len(L.pretest_passes(d, before, 4, mpos)) > L.EV_CAP
    for events in (L.EV_CAP - 1, L.EV_CAP, L.EV_CAP + 1):
        d, mpos = L.capcut_exact(events)
        m = _matches(oracle, d)
        assert m and m[0][0] == mpos and m[0][1] >= 390 and mpos < L.WINDOW, (events, m)
        assert len(L.pretest_passes(d, [], 4, mpos)) == events


@pytest.mark.parametrize("distance,depth", L.FARFLAG_PARAMS)
def test_farflag_preconditions(oracle, distance, depth):
    d, finals = L.farflag(distance, depth)
    m = _matches(oracle, d)
    starts = {p for p, _ in m}
    hits = sum(f in starts for f in finals)
    assert len(finals) == 12 and hits >= 10, (hits, m[-14:])  # (a filler context in one of the slots would cost that occurrence)
    # the static pass cannot flag them: with every position visited, the hash predecessor is a copy's position with another body
    static = set(L.pretest_passes(d, [], finals[0], len(d)))
    assert not (static & set(finals))
    # ... and the flag comes from a match at least `distance` positions in front: from another bitmap window where that is the point
    last_copy_end = max(p + ln for p, ln in m if p < finals[0] - distance)
    assert finals[0] - last_copy_end >= distance
    if distance > L.WINDOW:
        assert finals[0] // L.WINDOW > last_copy_end // L.WINDOW
    else:  # ... or from the same one: the window the driver opens behind that match reaches them all
        assert finals[-1] - last_copy_end < L.WINDOW
    if depth > 1:  # `depth` swallowed occurrences of every context between the final one and its candidate
        inside = lambda q: any(p < q < p + ln for p, ln in m)
        c = d[finals[0] - 4 : finals[0]]
        occ = [i + 4 for i in range(len(d) - 4) if d[i : i + 4] == c]
        assert occ[-1] == finals[0] and sum(inside(q) for q in occ) == depth and not inside(occ[1])


def test_lens_preconditions(oracle):
    m = _matches(oracle, L.lens())
    assert set(range(0, 2 * 254 + 2 + 1)) <= {ln - L.LZ_MIN for _, ln in m}


def test_long_preconditions(oracle):
    d = L.long_case()
    m = _matches(oracle, d)
    lens = {ln for _, ln in m}
    assert set(L.LONG_LENGTHS) <= lens  # every length around the rounds of the measuring loop, exactly
    for edge in (L.LZ_MIN + L.ROUND, L.LZ_MIN + 2 * L.ROUND):
        assert any(edge - 8 <= x < edge for x in lens) and edge in lens and any(edge < x <= edge + 8 for x in lens), edge
    assert max(lens) > 16384  # (a copy longer than a trip of the decoder)
    end = m[-1][0] + m[-1][1]
    assert abs(end - L.main_end(len(d))) <= 6


def test_collide_preconditions(oracle):
    d, marks = L.collide()
    n, z = oracle.lzp_encode(d)
    m = _matches(oracle, d)
    starts = dict(m)
    assert len(marks) == 20 and all(s in starts for s, _ in marks)
    # walk input and output side by side: the only 0xF2 bytes of the input are the closing ones, each followed by a letter
    assert d.count(b"\xf2") == 20
    bare, ip, op = 0, 4, 4
    closing = {f for _, f in marks}
    while ip < len(d):
        if ip in starts:
            op += 2 + (starts[ip] - L.LZ_MIN) // 254
            ip += starts[ip]
            continue
        assert z[op] == d[ip]
        if ip in closing:
            assert d[ip] == L.ESC and d[ip + 1] != 255
            if z[op + 1] == 255:
                op += 1
            else:
                bare += 1
        ip += 1
        op += 1
    assert op == n
    assert bare >= 15, bare
    # the hash predecessor of every closing 0xF2 exists all the same (inside the match): prev > 0 is not the rule
    for _, f in marks:
        c = d[f - 4 : f]
        assert any(d[i : i + 4] == c for i in range(f - 5)), f


@pytest.mark.parametrize("delta", L.LASTMATCH_D)
def test_lastmatch_preconditions(oracle, delta):
    d, p = L.lastmatch(delta)
    assert p == L.main_end(len(d)) - 37 - delta
    m = _matches(oracle, d)
    assert [x for x in m if x[0] >= p - 60] == ([(p, m[-1][1])] if delta >= 0 else []), m


def test_ends_cover_both_sides_of_their_edges(oracle):
    e = L.ends()
    assert len(e) == 2 * len(L.ENDS_SMALL) + len(L.ENDS_LINKS)
    assert min(L.ENDS_SMALL) < 72 < max(L.ENDS_SMALL) and min(L.ENDS_LINKS) - 4 <= 8192 < max(L.ENDS_LINKS) - 4
    for name, d in e.items():
        assert len(d) == int(name.split("-")[1]), name
        assert (oracle.lzp_encode(d)[0] > 0) or not name.startswith("links"), name


# ---- the kernel sources under the emulator ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", L.STAGE_NAMES)
def test_emulated_encoder_bytes_and_driver_record(emu, oracle, cases, name):
    L.check_encoder(bzip3_amd.StageApi(emu), oracle, name, cases[name])


def test_emulated_encoder_on_the_ends(emu, oracle):
    g = bzip3_amd.StageApi(emu)
    for name, d in L.ends().items():
        L.check_encoder(g, oracle, name, d)
