// TEST INFRASTRUCTURE ONLY.  A stand-alone host program for the sanitizers: the kernel sources and the API compiled against the CPU emulation
// of the HIP execution model (tests/emu) with -fsanitize=address,undefined, and the sweep of the clipped split (planes.hpp, "Clipped split")
// through bz3_hip_debug_patch.
//
//   FLAGS="-O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -DBZ3_EMU -DBZ3_EMU_API_UNITS -I tests/emu -I bzip3_amd/csrc \
//          -Wno-unknown-pragmas -Wno-attributes"
//   for f in bzip3_amd/csrc/*.hip; do g++ $FLAGS -x c++ -c $f -o $OUT/$(basename $f).o; done
//   g++ $FLAGS tests/emu/hip_emu.cpp tests/emu/patch_main.cpp $OUT/*.o -lpthread -o $OUT/patch_sweep && $OUT/patch_sweep
//
// Element sizes 1, 2, 4, 8, with and without a base, the element counts around one and two tiles of 4080 and around 4096, every tail length
// 0 .. k - 1, every pair a < b of the clip points of tests/test_frame_range_emu.py.  Every source, base and slot is a heap allocation of its own
// that holds exactly the aligned 16-byte granules with a byte of the buffer (the alignment mod 16 of the first byte is drawn per buffer): the
// kernel may load those granules and nothing else, so one load or store beyond them is a report.  One launch per (count, tail, k, base) holds
// all its pairs.  Every slot's whole allocation is compared with the model (the bytes around the slot keep their fill), and the inputs with
// themselves.  Prints "patch sweep ok" and returns 0.
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

// n bytes inside an allocation that holds exactly the aligned 16-byte granules with a byte of them: the buffer starts `lead` < 16 bytes behind the
// allocation's 16-byte aligned start, and the allocation ends at the first 16-byte boundary at or behind the buffer's end.
struct Tight {
    uint8_t * mem = nullptr;
    uint8_t * p = nullptr;
    size_t lead, n, size;
    Tight(size_t n_, size_t lead_) : lead(lead_), n(n_), size((lead_ + n_ + 15) & ~(size_t)15) {
        if (posix_memalign((void **)&mem, 16, size) != 0) abort();
        p = mem + lead;
        for (size_t i = 0; i < size; i++) mem[i] = (uint8_t)rnd();
    }
    Tight(const Tight &) = delete;
    Tight & operator=(const Tight &) = delete;
    ~Tight() { free(mem); }
};

int fail(const char * what, unsigned k, size_t elems, size_t tail, uint64_t a, uint64_t b) {
    fprintf(stderr, "patch sweep: %s (k %u, %zu elements, tail %zu, clip [%llu, %llu))\n", what, k, elems, tail, (unsigned long long)a, (unsigned long long)b);
    return 1;
}
}  // namespace

int main() {
    const size_t TILE = 4080;
    const size_t counts[] = {0, 1, 15, 16, 17, 31, 4079, 4080, 4081, 4095, 4096, 4097, 8159, 8160, 8161};
    size_t launches = 0, segments = 0;
    for (unsigned k : {1u, 2u, 4u, 8u})
        for (int has_base = 0; has_base < 2; has_base++)
            for (size_t elems : counts)
                for (size_t tail = 0; tail < k; tail++) {
                    const size_t s = elems * k + tail, mk = elems * k, m = elems;
                    std::set<uint64_t> pts;
                    for (uint64_t v : {(uint64_t)0, (uint64_t)1, (uint64_t)k - 1, (uint64_t)k, (uint64_t)k + 1, (uint64_t)15, (uint64_t)16, (uint64_t)17, (uint64_t)mk - 1, (uint64_t)mk,
                                       (uint64_t)s - 1, (uint64_t)s, TILE * k - 1, TILE * k, TILE * k + 1, 2 * TILE * k - 1, 2 * TILE * k, 2 * TILE * k + 1})
                        if (v <= s) pts.insert(v);  // (0 - 1 wraps to 2^64 - 1 and is dropped here)
                    struct Seg {
                        Tight *src, *base, *slot;
                        std::vector<uint8_t> src0, base0, want;
                        uint64_t a, b;
                    };
                    std::vector<Seg> segs;
                    for (uint64_t a : pts)
                        for (uint64_t b : pts) {
                            if (a >= b) continue;
                            Seg g;
                            g.a = a, g.b = b;
                            g.src = new Tight(b - a, rnd() % 16);
                            g.base = new Tight(b - a, rnd() % 16);
                            g.slot = new Tight(s, rnd() % 16);
                            g.src0.assign(g.src->p, g.src->p + (b - a));
                            g.base0.assign(g.base->p, g.base->p + (b - a));
                            g.want.assign(g.slot->mem, g.slot->mem + g.slot->size);
                            for (uint64_t c = a; c < b; c++) {
                                const uint8_t v = has_base ? (uint8_t)(g.src0[c - a] - g.base0[c - a]) : g.src0[c - a];
                                g.want[g.slot->lead + (c < mk ? (c % k) * m + c / k : c)] = v;
                            }
                            segs.push_back(std::move(g));
                        }
                    if (segs.empty()) continue;
                    // offsets relative to the lowest address of each kind (the hook takes unsigned offsets)
                    uint8_t *s0 = segs[0].src->p, *b0 = segs[0].base->p, *d0 = segs[0].slot->p;
                    for (const Seg & g : segs) {
                        if (g.src->p < s0) s0 = g.src->p;
                        if (g.base->p < b0) b0 = g.base->p;
                        if (g.slot->p < d0) d0 = g.slot->p;
                    }
                    std::vector<uint64_t> table;
                    for (const Seg & g : segs)
                        table.insert(table.end(), {(uint64_t)(g.src->p - s0), has_base ? (uint64_t)(g.base->p - b0) : UINT64_MAX, (uint64_t)(g.slot->p - d0), (uint64_t)s, (uint64_t)k, g.a, g.b});
                    if (bz3_hip_debug_patch(s0, b0, d0, table.data(), (int32_t)segs.size()) != BZ3_OK) return fail("the hook failed", k, elems, tail, 0, 0);
                    launches++;
                    for (const Seg & g : segs) {
                        segments++;
                        if (memcmp(g.slot->mem, g.want.data(), g.want.size()) != 0) return fail("the slot differs from the model", k, elems, tail, g.a, g.b);
                        if (memcmp(g.src->p, g.src0.data(), g.src0.size()) != 0 || memcmp(g.base->p, g.base0.data(), g.base0.size()) != 0)
                            return fail("an input was written", k, elems, tail, g.a, g.b);
                        delete g.src;
                        delete g.base;
                        delete g.slot;
                    }
                }
    printf("patch sweep ok: %zu launches, %zu segments\n", launches, segments);
    return 0;
}
