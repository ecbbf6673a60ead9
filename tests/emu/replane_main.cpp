// TEST INFRASTRUCTURE ONLY.  A stand-alone host program for the sanitizers: the kernel sources and the API compiled against the CPU emulation
// of the HIP execution model (tests/emu) with -fsanitize=address,undefined, and the sweep of the replane segment (planes.hpp, "Replane")
// through bz3_hip_debug_replane.
//
//   FLAGS="-O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -DBZ3_EMU -DBZ3_EMU_API_UNITS -I tests/emu -I bzip3_amd/csrc \
//          -Wno-unknown-pragmas -Wno-attributes"
//   for f in bzip3_amd/csrc/*.hip; do g++ $FLAGS -x c++ -c $f -o $OUT/$(basename $f).o; done
//   g++ $FLAGS tests/emu/hip_emu.cpp tests/emu/replane_main.cpp $OUT/*.o -lpthread -o $OUT/replane_sweep && $OUT/replane_sweep
//
// Element sizes 1, 2, 4, 8, the old element counts around one and two tiles of 4080 and around 4096 and a count of more than one copy tile per
// plane, every tail length 0 .. k - 1, every kept size a of the clip points of tests/test_frame_range_emu.py, and for each new lengths below,
// equal to and above the old one.  Every source and destination slot is a heap allocation of its own that holds exactly the aligned 16-byte
// granules with a byte of the slot (the alignment mod 16 of the first byte is drawn per buffer): the kernel may load those granules and nothing
// else, so one load or store beyond them is a report.  One launch per (count, tail, k) holds all its segments.  Every destination's whole
// allocation is compared with the model (the bytes around the slot and the slot's bytes that hold no kept byte keep their fill), and the sources
// with themselves.  Prints "replane sweep ok" and returns 0.
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

// n bytes inside an allocation that holds exactly the aligned 16-byte granules with a byte of them (tests/emu/patch_main.cpp).
struct Tight {
    uint8_t * mem = nullptr;
    uint8_t * p = nullptr;
    size_t lead, n, size;
    Tight(size_t n_, size_t lead_) : lead(lead_), n(n_), size((lead_ + n_ + 15) & ~(size_t)15) {
        if (size == 0) size = 16;
        if (posix_memalign((void **)&mem, 16, size) != 0) abort();
        p = mem + lead;
        for (size_t i = 0; i < size; i++) mem[i] = (uint8_t)rnd();
    }
    Tight(const Tight &) = delete;
    Tight & operator=(const Tight &) = delete;
    ~Tight() { free(mem); }
};

size_t pos(size_t c, size_t len, size_t k) {
    const size_t m = len / k;
    return c < m * k ? (c % k) * m + c / k : c;
}

int fail(const char * what, unsigned k, size_t len_old, size_t len_new, uint64_t a) {
    fprintf(stderr, "replane sweep: %s (k %u, %zu -> %zu bytes, %llu kept)\n", what, k, len_old, len_new, (unsigned long long)a);
    return 1;
}
}  // namespace

int main() {
    const size_t TILE = 4080;
    const size_t counts[] = {0, 1, 15, 16, 17, 31, 4079, 4080, 4081, 4095, 4096, 4097, 8159, 8160, 8161, 16385, 33000};
    size_t launches = 0, segments = 0;
    for (unsigned k : {1u, 2u, 4u, 8u})
        for (size_t elems : counts)
            for (size_t tail = 0; tail < k; tail++) {
                const size_t s = elems * k + tail, mk = elems * k;
                std::set<uint64_t> pts;
                for (uint64_t v : {(uint64_t)0, (uint64_t)1, (uint64_t)k - 1, (uint64_t)k, (uint64_t)k + 1, (uint64_t)15, (uint64_t)16, (uint64_t)17, (uint64_t)mk - 1, (uint64_t)mk,
                                   (uint64_t)s - 1, (uint64_t)s, TILE * k - 1, TILE * k, TILE * k + 1, 2 * TILE * k - 1, 2 * TILE * k, 2 * TILE * k + 1})
                    if (v <= s) pts.insert(v);  // (0 - 1 wraps to 2^64 - 1 and is dropped here)
                struct Seg {
                    Tight *src, *dst;
                    std::vector<uint8_t> src0, want;
                    size_t len_new;
                    uint64_t a;
                };
                std::vector<Seg> segs;
                for (uint64_t a : pts) {
                    std::vector<size_t> lens = {s, s + 1 + rnd() % 40, s + k * (16 + rnd() % 5000) + rnd() % k};
                    if (a < s) {
                        lens.push_back((size_t)a + rnd() % (s - (size_t)a));
                        lens.push_back((size_t)a);
                    }
                    for (size_t len_new : lens) {
                        Seg g;
                        g.a = a, g.len_new = len_new;
                        g.src = new Tight(s, rnd() % 16);
                        g.dst = new Tight(len_new, rnd() % 16);
                        g.src0.assign(g.src->p, g.src->p + s);
                        g.want.assign(g.dst->mem, g.dst->mem + g.dst->size);
                        for (uint64_t c = 0; c < a; c++) g.want[g.dst->lead + pos(c, len_new, k)] = g.src0[pos(c, s, k)];
                        segs.push_back(std::move(g));
                    }
                }
                if (segs.empty()) continue;
                // offsets relative to the lowest address of each kind (the hook takes unsigned offsets)
                uint8_t *s0 = segs[0].src->p, *d0 = segs[0].dst->p;
                for (const Seg & g : segs) {
                    if (g.src->p < s0) s0 = g.src->p;
                    if (g.dst->p < d0) d0 = g.dst->p;
                }
                std::vector<uint64_t> table;
                for (const Seg & g : segs) table.insert(table.end(), {(uint64_t)(g.src->p - s0), (uint64_t)(g.dst->p - d0), (uint64_t)s, (uint64_t)g.len_new, (uint64_t)k, g.a});
                if (bz3_hip_debug_replane(s0, d0, table.data(), (int32_t)segs.size()) != BZ3_OK) return fail("the hook failed", k, s, 0, 0);
                launches++;
                for (const Seg & g : segs) {
                    segments++;
                    if (memcmp(g.dst->mem, g.want.data(), g.want.size()) != 0) return fail("the slot differs from the model", k, s, g.len_new, g.a);
                    if (!g.src0.empty() && memcmp(g.src->p, g.src0.data(), g.src0.size()) != 0) return fail("the source was written", k, s, g.len_new, g.a);
                    delete g.src;
                    delete g.dst;
                }
            }
    printf("replane sweep ok: %zu launches, %zu segments\n", launches, segments);
    return 0;
}
