"""CPU: tools/cm_isa_count.py on the tree's cm.hip (skipped without hipcc): it finds every per-byte path in the three guess-ahead decoders, no kernel uses
scratch or loses occupancy, and no path costs more instructions than recorded here from this tree.  The counts belong to one compiler: with another version
string they are printed and not asserted; the resource checks stay."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc is missing")

COMPILER = "HIP version: 7.2.26015-fc0010cf6a"
OCCUPANCY = {"sync": 8, "sync2": 8, "sync3": 8}   # waves per SIMD, as the commit before the instruction diet had them
# instructions per byte, this tree with COMPILER (the commit before: 42 / 59 / 78 / 111 / 108.5 for sync, 44 / 61 / 89.5 / 122.5 / 111 for sync2 and sync3)
TOTALS = {
    "sync": {"model right guess": 37.0, "model right guess + update": 56.0, "model repair": 78.0, "model repair + updates": 113.0,
             "walker fast path": 104.5, "walker checked walk (excess)": 144.0},
    "sync2": {"model right guess": 37.5, "model right guess + update": 56.5, "model repair": 85.5, "model repair + updates": 120.5,
              "walker fast path": 107.0, "walker checked walk (excess)": 144.0},
    "sync3": {"model right guess": 37.0, "model right guess + update": 56.0, "model repair": 85.0, "model repair + updates": 120.0,
              "walker fast path": 107.0, "walker checked walk (excess)": 144.0},
}


@pytest.fixture(scope="module")
def counted():
    import cm_isa_count

    return cm_isa_count.run(sorted(cm_isa_count.KERNELS))


def test_every_path_is_found_in_every_kernel(counted):
    assert [k["variant"] for k in counted["kernels"]] == ["sync", "sync2", "sync3"]
    for k in counted["kernels"]:
        assert set(k["paths"]) == set(TOTALS[k["variant"]])
        for name, row in k["paths"].items():
            assert row is not None, (k["kernel"], name)
            assert row["total"] > 0 and abs(sum(row[c] for c in ("valu", "lds", "gmem", "wait", "salu")) - row["total"]) < 1e-9, (k["kernel"], name)
        p = k["paths"]
        assert p["model right guess"]["total"] < p["model right guess + update"]["total"] < p["model repair + updates"]["total"]
        assert p["model right guess"]["total"] < p["model repair"]["total"] <= p["model repair + updates"]["total"]
        assert p["model right guess"]["lds"] >= 4 and p["walker fast path"]["lds"] >= 9   # two cells, the table entry, the byte; nine table reads and the hand-over


def test_no_scratch_and_no_occupancy_lost(counted):
    for k in counted["kernels"]:
        r = k["resources"]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k["kernel"], r)
        assert r["occupancy"] >= OCCUPANCY[k["variant"]], (k["kernel"], r)


def test_no_path_costs_more_than_recorded(counted):
    for k in counted["kernels"]:
        for name, row in k["paths"].items():
            print(k["kernel"], name, row["total"], "recorded", TOTALS[k["variant"]][name])
    if counted["compiler"] != COMPILER:
        pytest.skip("another compiler (%r): the recorded counts are %r's" % (counted["compiler"], COMPILER))
    for k in counted["kernels"]:
        for name, row in k["paths"].items():
            assert row["total"] <= TOTALS[k["variant"]][name], (k["kernel"], name, row["total"])
