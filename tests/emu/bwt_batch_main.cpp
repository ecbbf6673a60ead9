// TEST INFRASTRUCTURE ONLY.  A stand-alone host program for the sanitizers: the kernel sources and the API compiled against the CPU emulation
// of the HIP execution model (tests/emu) with -fsanitize=address,undefined, and one mixed call of the batched forward BWT made once.
//
//   FLAGS="-O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -DBZ3_EMU -DBZ3_EMU_API_UNITS -I tests/emu -I bzip3_amd/csrc \
//          -Wno-unknown-pragmas -Wno-attributes"
//   for f in bzip3_amd/csrc/*.hip; do g++ $FLAGS -x c++ -c $f -o $OUT/$(basename $f).o; done
//   g++ $FLAGS tests/emu/hip_emu.cpp tests/emu/bwt_batch_main.cpp $OUT/*.o -lpthread -o $OUT/bwt_batch && ASAN_OPTIONS=detect_leaks=0 $OUT/bwt_batch
// (detect_leaks=0: the per-device context of api_context.hip lives as long as the process and is never freed; every other check stays on.)
//
// Six jobs in one bz3_hip_debug_bwt_many call -- a run of four that all take different paths of the sorter and a run of two: a periodic string of
// 60,000 bytes (a list overflows at pass 0: rank doubling), a run of one byte (the same, deeper), 150,000 random letters with a phrase repeated 900
// times (groups too large for a wave: one more window), 3 bytes, then 2 bytes and the periodic string again.  Every job must come back as
// bz3_hip_stage_bwt returns it alone, index and bytes; and nothing may be written beyond a job's n bytes.  Prints "bwt batch ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/bz3_hip.h"
#include "../../include/libbz3.h"

namespace {
typedef std::vector<uint8_t> Bytes;

int fail(const char * what, int i) {
    fprintf(stderr, "bwt batch: %s (job %d)\n", what, i);
    return 1;
}
}  // namespace

int main() {
    constexpr int N = 6;
    uint32_t seed = 2463534242u;
    auto next = [&]() { return seed = seed * 1664525u + 1013904223u; };
    std::vector<Bytes> text(N), out(N), alone(N);
    text[0].resize(60000);
    for (size_t i = 0; i < text[0].size(); i++) text[0][i] = (uint8_t)("abracadabra-"[i % 12]);
    text[1].assign(7000, (uint8_t)'z');
    for (int rep = 0; rep < 900; rep++) {
        for (const char * p = "thesamewordsoverandover"; *p; p++) text[2].push_back((uint8_t)*p);
        for (int k = 0; k < 144; k++) text[2].push_back((uint8_t)('a' + (next() >> 24) % 26));
    }
    text[3] = Bytes{'a', 'b', 'a'};
    text[4] = Bytes{'b', 'a'};
    text[5] = text[0];
    int32_t sizes[N], idx_alone[N], idx[N];
    const uint8_t * ins[N];
    uint8_t * outs[N];
    for (int k = 0; k < N; k++) {
        sizes[k] = (int32_t)text[k].size();
        alone[k].assign(text[k].size(), 0);
        idx_alone[k] = bz3_hip_stage_bwt(text[k].data(), alone[k].data(), sizes[k]);
        if (idx_alone[k] <= 0 || idx_alone[k] > sizes[k]) return fail("stage hook", k);
        out[k].assign(text[k].size() + 32, 0xA5);
        ins[k] = text[k].data();
        outs[k] = out[k].data();
        idx[k] = -7;
    }
    if (bz3_hip_debug_bwt_many(ins, outs, sizes, idx, N) != 0) return fail("the call failed", -1);
    for (int k = 0; k < N; k++) {
        if (idx[k] != idx_alone[k]) return fail("index differs from the job alone", k);
        if (memcmp(out[k].data(), alone[k].data(), (size_t)sizes[k]) != 0) return fail("bytes differ from the job alone", k);
        for (size_t t = (size_t)sizes[k]; t < out[k].size(); t++)
            if (out[k][t] != 0xA5) return fail("wrote beyond the job", k);
    }
    puts("bwt batch ok");
    return 0;
}
