// TEST INFRASTRUCTURE ONLY.  A stand-alone host program for the sanitizers: the kernel sources and the API compiled against the CPU emulation
// of the HIP execution model (tests/emu) with -fsanitize=address,undefined, and the sweep of the select split (planes.hpp, "Select split")
// through bz3_hip_debug_patch_select.
//
//   FLAGS="-O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -DBZ3_EMU -DBZ3_EMU_API_UNITS -I tests/emu -I bzip3_amd/csrc \
//          -Wno-unknown-pragmas -Wno-attributes"
//   for f in bzip3_amd/csrc/*.hip; do g++ $FLAGS -x c++ -c $f -o $OUT/$(basename $f).o; done
//   g++ $FLAGS tests/emu/hip_emu.cpp tests/emu/patch_select_main.cpp $OUT/*.o -lpthread -o $OUT/patch_select_sweep && $OUT/patch_select_sweep
//
// Element sizes 1, 2, 4, 8, with and without a base, source counts around the tile edges of 4080 elements (plus 0 .. k - 1 bytes), piece counts 2,
// 3, 64, 65 and 1000 with piece lengths below, at and above 16 elements mixed within a list (every eighth piece some hundred elements long, now and
// then an empty one and two neighbours that touch), a first byte inside a piece (r0 > 0) of a later period (q0 > 0), as many periods as the source
// spans, and the three ends: the last byte written is the chunk's last and the chunk has no tail, it is the one before the chunk's last, it lies
// inside the chunk's tail of len % k bytes.  Every source, base and slot is a heap allocation of its own that holds exactly the aligned 16-byte
// granules with a byte of the buffer (the alignment mod 16 of the first byte is drawn per buffer), and every piece table an allocation of exactly
// its 16 m bytes: the kernel may load those granules and nothing else, so one load or store beyond them is a report.  One launch per (count, k,
// base) holds all its segments.  Every slot's whole allocation is compared with the model (the bytes around the slot keep their fill), and the
// inputs with themselves.  Prints "patch select sweep ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

int fail(const char * what, unsigned k, size_t elems, size_t m, int end_mode) {
    fprintf(stderr, "patch select sweep: %s (k %u, %zu source elements, %zu pieces, end %d)\n", what, k, elems, m, end_mode);
    return 1;
}

struct Seg {
    Tight *src = nullptr, *base = nullptr, *slot = nullptr;
    uint64_t * pieces = nullptr;  // an allocation of exactly 16 m bytes
    std::vector<uint8_t> src0, base0, want;
    uint64_t m, len, rel, stride, q0, r0, nbytes;
};
}  // namespace

int main() {
    const size_t counts[] = {1, 17, 4079, 4080, 4081, 8160, 8161};
    const size_t piece_counts[] = {2, 3, 64, 65, 1000};
    size_t launches = 0, segments = 0;
    for (unsigned k : {1u, 2u, 4u, 8u})
        for (int has_base = 0; has_base < 2; has_base++)
            for (size_t elems : counts) {
                std::vector<Seg> segs;
                for (size_t m : piece_counts)
                    for (int end_mode = 0; end_mode < 3; end_mode++) {
                        Seg g;
                        g.m = m;
                        g.nbytes = elems * k + rnd() % k;
                        g.pieces = (uint64_t *)malloc(16 * m);
                        const uint64_t lens[] = {1, k > 1 ? k - 1 : 1, k, k + 1, 15, 16, 17, 16 * k - 1, 16 * k, 16 * k + 1};
                        uint64_t at = rnd() % 40, L = 0;
                        for (size_t j = 0; j < m; j++) {
                            uint64_t l = lens[rnd() % 10];
                            if (j % 8 == 3) l = 16 * k * 20 + rnd() % (2 * k);
                            if (m > 3 && j % 11 == 5) l = 0;
                            g.pieces[2 * j] = at, g.pieces[2 * j + 1] = l;
                            const uint64_t gaps[] = {1, k, 16};
                            at += l + (m > 3 && j % 13 == 7 ? 0 : gaps[rnd() % 3]);
                            L += l;
                        }
                        const uint64_t E = g.pieces[2 * m - 2] + g.pieces[2 * m - 1], pads[] = {0, 1, k, 16};
                        g.stride = E + pads[rnd() % 4];
                        g.q0 = rnd() % 5;
                        g.r0 = L > 1 ? 1 + rnd() % (L - 1) : 0;
                        // f[u]: the byte of the period sequence that source byte u goes to, before rel moves it into the chunk
                        std::vector<int64_t> f;
                        for (uint64_t q = g.q0, x = 0; f.size() < g.nbytes; q++)
                            for (size_t j = 0; j < m && f.size() < g.nbytes; j++)
                                for (uint64_t i = 0; i < g.pieces[2 * j + 1] && f.size() < g.nbytes; i++, x++)
                                    if (q > g.q0 || x >= g.r0) f.push_back((int64_t)(q * g.stride + g.pieces[2 * j] + i));
                        int64_t rel = (int64_t)(rnd() % 40) - f.front();
                        int64_t end = rel + f.back() + 1;
                        if (k > 1 && end_mode == 0) rel += (k - end % k) % k;
                        if (k > 1 && end_mode == 2) rel += ((int64_t)(k / 2) - end % k + k) % k;
                        end = rel + f.back() + 1;
                        g.len = (uint64_t)end + (end_mode == 1 ? 1 : 0);
                        g.rel = (uint64_t)rel;
                        g.src = new Tight(g.nbytes, rnd() % 16);
                        g.base = new Tight(g.nbytes, rnd() % 16);
                        g.slot = new Tight(g.len, rnd() % 16);
                        g.src0.assign(g.src->p, g.src->p + g.nbytes);
                        g.base0.assign(g.base->p, g.base->p + g.nbytes);
                        g.want.assign(g.slot->mem, g.slot->mem + g.slot->size);
                        const uint64_t mm = g.len / k, mk = mm * k;
                        for (uint64_t u = 0; u < g.nbytes; u++) {
                            const uint64_t c = (uint64_t)(rel + f[u]);
                            if (c >= g.len) return fail("the model left the chunk", k, elems, m, end_mode);
                            g.want[g.slot->lead + (c < mk ? (c % k) * mm + c / k : c)] = has_base ? (uint8_t)(g.src0[u] - g.base0[u]) : g.src0[u];
                        }
                        segs.push_back(std::move(g));
                    }
                // offsets relative to the lowest address of each kind (the hook takes unsigned offsets); the piece lists one after the other
                uint8_t *s0 = segs[0].src->p, *b0 = segs[0].base->p, *d0 = segs[0].slot->p;
                for (const Seg & g : segs) {
                    if (g.src->p < s0) s0 = g.src->p;
                    if (g.base->p < b0) b0 = g.base->p;
                    if (g.slot->p < d0) d0 = g.slot->p;
                }
                std::vector<uint64_t> table, all;
                for (const Seg & g : segs) {
                    table.insert(table.end(), {(uint64_t)(g.src->p - s0), has_base ? (uint64_t)(g.base->p - b0) : UINT64_MAX, (uint64_t)(g.slot->p - d0), g.len, (uint64_t)k, g.rel, g.stride,
                                               g.q0, g.r0, g.nbytes, (uint64_t)(all.size() / 2), g.m});
                    all.insert(all.end(), g.pieces, g.pieces + 2 * g.m);
                }
                uint64_t * flat = (uint64_t *)malloc(all.size() * sizeof(uint64_t));  // exactly the pieces
                memcpy(flat, all.data(), all.size() * sizeof(uint64_t));
                const int32_t rc = bz3_hip_debug_patch_select(s0, b0, d0, table.data(), (int32_t)segs.size(), flat, all.size() / 2);
                free(flat);
                if (rc != BZ3_OK) return fail("the hook failed", k, elems, 0, 0);
                launches++;
                for (const Seg & g : segs) {
                    segments++;
                    if (memcmp(g.slot->mem, g.want.data(), g.want.size()) != 0) return fail("the slot differs from the model", k, elems, g.m, -1);
                    if (memcmp(g.src->p, g.src0.data(), g.src0.size()) != 0 || memcmp(g.base->p, g.base0.data(), g.base0.size()) != 0)
                        return fail("an input was written", k, elems, g.m, -1);
                    delete g.src;
                    delete g.base;
                    delete g.slot;
                    free(g.pieces);
                }
            }
    printf("patch select sweep ok: %zu launches, %zu segments\n", launches, segments);
    return 0;
}
