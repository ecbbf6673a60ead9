// TEST INFRASTRUCTURE ONLY.  A stand-alone host program for the sanitizers: the kernel sources and the API compiled against the CPU emulation
// of the HIP execution model (tests/emu) with -fsanitize=address,undefined, and the sweep of the comparison of a sync call (planes.hpp,
// "diff segments") through bz3_hip_debug_diff.
//
//   FLAGS="-O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -DBZ3_EMU -DBZ3_EMU_API_UNITS -I tests/emu -I bzip3_amd/csrc \
//          -Wno-unknown-pragmas -Wno-attributes"
//   for f in bzip3_amd/csrc/*.hip; do g++ $FLAGS -x c++ -c $f -o $OUT/$(basename $f).o; done
//   g++ $FLAGS tests/emu/hip_emu.cpp tests/emu/diff_main.cpp $OUT/*.o -lpthread -o $OUT/diff_sweep && $OUT/diff_sweep
//
// The lengths of tests/test_frame_sync_emu.py (0 .. 33, around one tile of 16 KiB, two tiles + 5) with `a` and `b` at independent alignments out
// of {0, 7, 9}; per (length, alignment pair) equal runs, and one flipped byte at the first and the last byte and on each side of every 16-byte
// seam of either side's granules (the tile seams are among a's).  Every run is a heap allocation of its own that holds exactly the aligned
// 16-byte granules with a byte of the run: the kernel may load those granules and nothing else, so one load beyond them is a report.  The
// bytes of a run's first and last granule that lie outside the run differ between the two sides in every case, so a wrong end mask shows as a
// wrong flag.  One launch holds up to 256 runs of `b` against one run of `a`.  Every run is compared with itself afterwards.  Prints
// "diff sweep ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../../include/bz3_hip.h"
#include "../../include/libbz3.h"

namespace {
uint32_t seed = 2463534242u;
uint32_t rnd() { return (seed = seed * 1664525u + 1013904223u) >> 8; }

// n bytes inside an allocation that holds exactly the aligned 16-byte granules with a byte of them (patch_main.cpp's); one byte where n == 0.
struct Tight {
    uint8_t * mem = nullptr;
    uint8_t * p = nullptr;
    size_t lead, n, size;
    Tight(size_t n_, size_t lead_) : lead(n_ ? lead_ : 0), n(n_), size(n_ ? (lead_ + n_ + 15) & ~(size_t)15 : 0) {
        if (posix_memalign((void **)&mem, 16, size ? size : 1) != 0) abort();
        p = mem + lead;
        for (size_t i = 0; i < size; i++) mem[i] = (uint8_t)rnd();
    }
    Tight(const Tight &) = delete;
    Tight & operator=(const Tight &) = delete;
    ~Tight() { free(mem); }
};

int fail(const char * what, size_t n, unsigned al_a, unsigned al_b, long flip) {
    fprintf(stderr, "diff sweep: %s (%zu bytes, a at %u, b at %u mod 16, flipped byte %ld)\n", what, n, al_a, al_b, flip);
    return 1;
}
}  // namespace

int main() {
    const size_t TILE = 16384, BATCH = 256;
    const size_t lengths[] = {0, 1, 15, 16, 17, 31, 33, TILE - 17, TILE - 1, TILE, TILE + 1, TILE + 17, 2 * TILE + 5};
    const unsigned aligns[] = {0, 7, 9};
    size_t launches = 0, segments = 0;
    for (size_t n : lengths)
        for (unsigned al_a : aligns)
            for (unsigned al_b : aligns) {
                std::vector<long> flips = {-1};  // -1: equal runs
                std::set<long> pts;
                if (n) pts.insert(0), pts.insert((long)n - 1);
                for (unsigned al : {al_a, al_b})
                    for (size_t o = (16 - al) % 16; o < n; o += 16)
                        if (o > 0) pts.insert((long)o - 1), pts.insert((long)o);
                flips.insert(flips.end(), pts.begin(), pts.end());
                Tight a(n, al_a);
                const std::vector<uint8_t> a0(a.mem, a.mem + a.size);
                for (size_t first = 0; first < flips.size(); first += BATCH) {
                    const size_t cnt = flips.size() - first < BATCH ? flips.size() - first : BATCH;
                    std::vector<Tight *> bs;
                    std::vector<std::vector<uint8_t>> b0;
                    const uint8_t * lowest = nullptr;
                    for (size_t i = 0; i < cnt; i++) {
                        Tight * b = new Tight(n, al_b);  // (random granules: the bytes outside the run differ from a's)
                        if (n) memcpy(b->p, a.p, n);
                        for (size_t g = 0; g < b->lead && g < a.lead; g++) b->p[-(long)g - 1] = (uint8_t)~a.p[-(long)g - 1];
                        for (size_t g = n; b->lead + g < b->size && a.lead + g < a.size; g++) b->p[g] = (uint8_t)~a.p[g];
                        if (flips[first + i] >= 0) b->p[flips[first + i]] ^= (uint8_t)(1u << (rnd() % 8));
                        b0.emplace_back(b->mem, b->mem + b->size);
                        if (!lowest || b->p < lowest) lowest = b->p;
                        bs.push_back(b);
                    }
                    std::vector<uint64_t> table;
                    for (const Tight * b : bs) table.insert(table.end(), {(uint64_t)0, (uint64_t)(b->p - lowest), (uint64_t)n});
                    std::vector<uint32_t> flags(cnt, 7);
                    if (bz3_hip_debug_diff(a.p, lowest, table.data(), (int32_t)cnt, flags.data()) != BZ3_OK) return fail("the hook failed", n, al_a, al_b, 0);
                    launches++;
                    for (size_t i = 0; i < cnt; i++) {
                        segments++;
                        if (flags[i] != (flips[first + i] >= 0 ? 1u : 0u)) return fail("a flag is wrong", n, al_a, al_b, flips[first + i]);
                        if (bs[i]->size && memcmp(bs[i]->mem, b0[i].data(), bs[i]->size) != 0) return fail("b was written", n, al_a, al_b, flips[first + i]);
                        delete bs[i];
                    }
                    if (a.size && memcmp(a.mem, a0.data(), a.size) != 0) return fail("a was written", n, al_a, al_b, 0);
                }
            }
    printf("diff sweep ok: %zu launches, %zu segments\n", launches, segments);
    return 0;
}
