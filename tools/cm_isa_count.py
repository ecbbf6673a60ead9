"""Instructions per decoded byte of the guess-ahead CM decoders, counted in the compiler's own assembly.  (No GPU needed.)
    python tools/cm_isa_count.py [--variant sync|sync2|sync3] [--json] [--asm FILE.s --remarks FILE.txt]
Compiles bzip3_amd/csrc/cm.hip for gfx950 with bzip3_amd/build.py's flags to assembly (`-S --cuda-device-only
-Rpass-analysis=kernel-resource-usage`) and, for k_cm_decode_sync / _sync2 / _sync3, walks the control-flow graph of the two
depth-1 loops that contain workgroup barriers: the model waves' loop and the walker's loop (the one with more child loops:
every level of the checked walk has a renormalisation loop).  Both loops handle TWO bytes per trip, and every wave takes one
barrier per byte after a right guess and two after a wrong one, so a per-byte path is a cycle header -> header with a given
number of barriers, and among those the one with the fewest instructions:

  model waves   right guess, no lane on the path   barrier 1 of either byte; the lane-masked regions (s_and_saveexec .. s_cbranch_exec*) skipped
                right guess + update block         the same; every lane-masked region entered
                repair, row resident               both barriers of either byte; lane-masked regions skipped / entered
  walker        fast path                          barrier 1 of either byte
                checked walk                       the same through the first child loop of the loop (the first byte of the trip is
                                                   decoded again with one renormalisation step at its first level); reported as the
                                                   excess over the fast path

Counts are per trip / 2.  Instructions are classified by mnemonic prefix only: v_ = VALU, ds_ = LDS, global_ / flat_ / buffer_ /
scratch_ / s_load / s_buffer_load = global memory, s_waitcnt / s_nop = waits, every other s_ = other scalar.  The kernel's
registers, scratch, LDS and occupancy are the compiler's kernel-resource-usage remarks."""
import argparse
import heapq
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from bzip3_amd import build as B  # noqa: E402

KERNELS = {"sync": "k_cm_decode_sync", "sync2": "k_cm_decode_sync2", "sync3": "k_cm_decode_sync3"}
CLASSES = ("valu", "lds", "gmem", "wait", "salu")


def compiler_version():
    r = subprocess.run([B._hipcc(), "--version"], capture_output=True, text=True)
    return r.stdout.strip().splitlines()[0] if r.returncode == 0 and r.stdout.strip() else ""


def compile_asm(out_s):
    """cm.hip -> assembly with the build's flags; returns the compiler's remarks (stderr)."""
    flags = [f for f in B.FLAGS if f != "-fPIC"]
    cmd = [B._hipcc(), *flags, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", os.path.join(B.CSRC, "cm.hip"), "-o", out_s]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stderr)
    return r.stderr


def resources(remarks):
    """{mangled kernel name: {sgprs, vgprs, agprs, scratch, occupancy, lds}} from the kernel-resource-usage remarks."""
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
            "LDS Size [bytes/block]": "lds", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill"}
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return out


def classify(mnemonic):
    if mnemonic.startswith("v_"):
        return "valu"
    if mnemonic.startswith("ds_"):
        return "lds"
    if mnemonic.startswith(("global_", "flat_", "buffer_", "scratch_", "s_load", "s_buffer_load")):
        return "gmem"
    if mnemonic.startswith(("s_waitcnt", "s_nop")):
        return "wait"
    return "salu"


class Block:
    def __init__(self, name):
        self.name = name
        self.loops = set()     # headers of the loops the block lies in
        self.header_depth = 0  # > 0: the block is a loop header of that depth
        self.counts = dict.fromkeys(CLASSES, 0)
        self.barriers = 0
        self.exec_branch = None  # target of a branch on EXEC that ends the block (skips a lane-masked region)
        self.exec_enters = False
        self.succ = []           # names of the blocks that can follow
        self.ends = False        # ends in an unconditional branch or the end of the program

    @property
    def total(self):
        return sum(self.counts.values())


def parse_function(asm_lines, mangled):
    """Basic blocks of one function, in layout order."""
    start = next(i for i, l in enumerate(asm_lines) if l.startswith(mangled + ":"))
    blocks = [Block("entry")]
    for line in asm_lines[start + 1:]:
        if line.startswith(".Lfunc_end"):
            break
        s = line.strip()
        m = re.match(r"(\.LBB\d+_\d+):", s) or re.match(r"; (%bb\.\d+):", s)
        if m:
            blocks.append(Block(m.group(1)))
        cur = blocks[-1]
        if ";" in s:  # loop membership travels in the compiler's comments
            c = s[s.index(";"):]
            for h in re.findall(r"(?:Header=|Parent Loop )(BB\d+_\d+)", c):
                cur.loops.add(".L" + h)
            m2 = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", c)
            if m2:
                cur.header_depth = int(m2.group(1))
                cur.loops.add(cur.name)
        if m or not line.startswith("\t") or s.startswith((";", ".")) or not s:
            continue
        mnem = s.split()[0]
        cur.counts[classify(mnem)] += 1
        if mnem.startswith("s_barrier"):
            cur.barriers += 1
        elif mnem.startswith("s_cbranch_exec"):
            cur.exec_branch = s.split()[1]
            cur.exec_enters = mnem.startswith("s_cbranch_execnz")  # taken when some lane is active: the branch LEADS to the masked region
            cur.succ.append(s.split()[1])
            blocks.append(Block(cur.name + "+"))  # what follows a conditional branch is a block of its own
            blocks[-1].loops = set(cur.loops)
        elif mnem.startswith("s_cbranch"):
            cur.succ.append(s.split()[1])
            blocks.append(Block(cur.name + "+"))
            blocks[-1].loops = set(cur.loops)
        elif mnem.startswith(("s_branch", "s_endpgm")):
            if mnem.startswith("s_branch"):
                cur.succ.append(s.split()[1])
            cur.ends = True
    return blocks


def _rename_continuations(blocks):
    """Continuation blocks get unique names and the fall-through edges are rebuilt by position."""
    for i, b in enumerate(blocks):
        if b.name.endswith("+"):
            b.name = f"{b.name}{i}"
    for i, b in enumerate(blocks):
        b.succ = [t for t in b.succ if t.startswith(".LBB")]
        if not b.ends and i + 1 < len(blocks):
            b.succ.append(blocks[i + 1].name)


def shortest_cycle(blocks, header, sites, enter_masked, via=None):
    """The cycle header -> header inside the loop that passes exactly the barriers `sites` (indices in layout order within the
    loop: 0 / 1 = barriers 1 / 2 of the trip's first byte, 2 / 3 = of its second), each once, with the fewest instructions.
    enter_masked: some lane is active at every branch on EXEC (every lane-masked region is entered).  via: a block the cycle must pass."""
    by = {b.name: b for b in blocks}
    inside = [b for b in blocks if header in b.loops]
    names = {b.name for b in inside}
    mask_of, k = {}, 0
    for b in inside:
        mask_of[b.name] = ((1 << b.barriers) - 1) << k
        k += b.barriers
    want = sum(1 << i for i in sites)

    def search(src, dst, have, need):
        # Dijkstra over (block about to be entered, barriers passed so far); the cost counts the blocks already left
        done = set()
        heap = [(0, 0, src, have, dict.fromkeys(CLASSES, 0), [])]
        tie = 0
        while heap:
            cost, _, name, seen, acc, trail = heapq.heappop(heap)
            if name == dst and trail and seen == need:
                return cost, acc, trail
            if trail:
                if (name, seen) in done:
                    continue
                done.add((name, seen))
            b = by[name]
            m = mask_of[name]
            if (m & seen) or (m & ~want):
                continue
            acc2 = {c: acc[c] + b.counts[c] for c in CLASSES}
            for t in b.succ:
                if t not in names:
                    continue
                if enter_masked and b.exec_branch is not None and len(b.succ) > 1 and b.exec_branch in names:
                    if (b.exec_branch == t) != b.exec_enters:  # some lane is active at every branch on EXEC
                        continue
                tie += 1
                heapq.heappush(heap, (cost + b.total, tie, t, seen | m, acc2, trail + [name]))
        return None

    if via is None:
        return search(header, header, 0, want)
    res = None
    for mid in range(want + 1):  # the barriers passed before the forced block
        if mid & ~want:
            continue
        a = search(header, via, 0, mid)
        z = search(via, header, mid, want) if a else None
        if a and z and (res is None or a[0] + z[0] < res[0]):
            res = (a[0] + z[0], {c: a[1][c] + z[1][c] for c in CLASSES}, a[2] + z[2])
    return res


def _row(res, per=2.0, minus=None):
    if res is None:
        return None
    acc = dict(res[1])
    if minus is not None:  # the excess of a trip over another one: the cost of the ONE byte that differs
        acc = {k: acc[k] - minus[1][k] for k in CLASSES}
        per = 1.0
    row = {k: acc[k] / per for k in CLASSES}
    row["total"] = sum(row.values())
    return row


def analyse(variant, asm_lines, res_all):
    kernel = KERNELS[variant]
    mangled = next(n for n in res_all if re.fullmatch(r"_ZN3bz3\d+" + kernel + r"E.*", n))
    blocks = parse_function(asm_lines, mangled)
    _rename_continuations(blocks)
    by = {b.name: b for b in blocks}
    for b in blocks:  # a block inside a child loop names that loop only: it lies in the loops of the child's header too
        for h in list(b.loops):
            b.loops |= by[h].loops if h in by else set()
    # the depth-1 loops with barriers in them
    loops = []
    for h in (b for b in blocks if b.header_depth == 1):
        members = [b for b in blocks if h.name in b.loops]
        if sum(b.barriers for b in members):
            children = [b for b in members if b.header_depth == 2]
            loops.append((len(children), h.name, children))
    if len(loops) != 2:
        raise RuntimeError(f"{kernel}: expected two depth-1 loops with barriers, found {len(loops)}")
    for _, h, _ in loops:
        nb = sum(b.barriers for b in blocks if h in b.loops)
        if nb != 4:
            raise RuntimeError(f"{kernel}: loop {h} has {nb} barriers, expected two per byte of a two-byte trip")
    loops.sort(key=lambda t: t[0])
    (_, model, _), (_, walker, wchildren) = loops
    paths = {}
    paths["model right guess"] = _row(shortest_cycle(blocks, model, (0, 2), False))
    paths["model right guess + update"] = _row(shortest_cycle(blocks, model, (0, 2), True))
    paths["model repair"] = _row(shortest_cycle(blocks, model, (0, 1, 2, 3), False))
    paths["model repair + updates"] = _row(shortest_cycle(blocks, model, (0, 1, 2, 3), True))
    fast = shortest_cycle(blocks, walker, (0, 2), False)
    paths["walker fast path"] = _row(fast)
    checked = shortest_cycle(blocks, walker, (0, 2), False, via=wchildren[0].name) if wchildren else None
    paths["walker checked walk (excess)"] = _row(checked, minus=fast) if checked and fast else None
    return {"kernel": kernel, "variant": variant, "resources": res_all[mangled], "paths": paths,
            "loops": {"model": model, "walker": walker}}


def run(variants, asm_file=None, remarks_file=None):
    if asm_file:
        remarks = open(remarks_file).read()
        asm_lines = open(asm_file).read().splitlines()
    else:
        with tempfile.TemporaryDirectory() as d:
            s = os.path.join(d, "cm.s")
            remarks = compile_asm(s)
            asm_lines = open(s).read().splitlines()
    res_all = resources(remarks)
    return {"compiler": compiler_version(), "kernels": [analyse(v, asm_lines, res_all) for v in variants]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--variant", choices=sorted(KERNELS), action="append", help="default: all three")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--asm", help="an assembly file made earlier instead of compiling")
    ap.add_argument("--remarks", help="the compiler's remarks (stderr) that belong to --asm")
    a = ap.parse_args()
    out = run(a.variant or sorted(KERNELS), a.asm, a.remarks)
    if a.json:
        print(json.dumps(out))
        return
    print("compiler:", out["compiler"])
    for k in out["kernels"]:
        r = k["resources"]
        print(f"\n{k['kernel']}: VGPRs {r.get('vgprs')}  SGPRs {r.get('sgprs')}  scratch {r.get('scratch')} B/lane  LDS {r.get('lds')} B static  "
              f"occupancy {r.get('occupancy')} waves/SIMD   (loops: model {k['loops']['model']}, walker {k['loops']['walker']})")
        print(f"  {'path (instructions per byte)':<36}{'total':>7}{'VALU':>7}{'LDS':>6}{'gmem':>6}{'wait':>6}{'scalar':>8}")
        for name, row in k["paths"].items():
            if row is None:
                print(f"  {name:<36}  not found")
                continue
            print(f"  {name:<36}{row['total']:>7.1f}{row['valu']:>7.1f}{row['lds']:>6.1f}{row['gmem']:>6.1f}{row['wait']:>6.1f}{row['salu']:>8.1f}")


if __name__ == "__main__":
    main()
