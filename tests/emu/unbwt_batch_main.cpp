// TEST INFRASTRUCTURE ONLY.  A stand-alone host program for the sanitizers: the kernel sources and the API compiled against the CPU emulation
// of the HIP execution model (tests/emu) with -fsanitize=address,undefined, and the mixed call of tests/test_unbwt_batch_emu.py made once.
//
//   FLAGS="-O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -DBZ3_EMU -DBZ3_EMU_API_UNITS -I tests/emu -I bzip3_amd/csrc \
//          -Wno-unknown-pragmas -Wno-attributes"
//   for f in bzip3_amd/csrc/*.hip; do g++ $FLAGS -x c++ -c $f -o $OUT/$(basename $f).o; done
//   g++ $FLAGS tests/emu/hip_emu.cpp tests/emu/unbwt_batch_main.cpp $OUT/*.o -lpthread -o $OUT/unbwt_batch && $OUT/unbwt_batch
//
// Six jobs in one bz3_hip_debug_unbwt_many call -- a run of four of unequal extent and a run of two: a text of 600,000 bytes (hashed splitters,
// segments that outgrow their slabs), 3 bytes, 140,000 bytes over two symbols that are no BWT of anything, 70,000 bytes of text with a WRONG
// index (every row a splitter), 2 bytes, and the same 70,000 bytes with their own index.  The genuine transforms come from bz3_hip_stage_bwt and must come back as their texts; every job must come back as
// bz3_hip_stage_unbwt returns it alone; and nothing may be written beyond a job's n bytes.  Prints "unbwt batch ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/bz3_hip.h"
#include "../../include/libbz3.h"

namespace {
typedef std::vector<uint8_t> Bytes;

int fail(const char * what, int i) {
    fprintf(stderr, "unbwt batch: %s (job %d)\n", what, i);
    return 1;
}
}  // namespace

int main() {
    constexpr int N = 6;
    const int32_t sizes[N] = {600000, 3, 140000, 70000, 2, 70000};
    const bool genuine[N] = {true, true, false, true, true, true};
    const int wrong_index = 3;  // this job's transform is genuine, its index is not: the walk ends early and the reference's rules fill the rest
    uint32_t seed = 2463534242u;
    auto next = [&]() { return seed = seed * 1664525u + 1013904223u; };
    Bytes unit(1499);
    for (uint8_t & b : unit) b = (uint8_t)("etaoin shrdlu"[(next() >> 24) % 13]);
    std::vector<Bytes> text(N), in(N), out(N), alone(N);
    int32_t idx[N];
    for (int k = 0; k < N; k++) {
        const size_t n = (size_t)sizes[k];
        text[k].resize(n);
        in[k].resize(n);
        for (size_t i = 0; i < n; i++) text[k][i] = genuine[k] ? (uint8_t)(unit[(i * (size_t)(k + 1)) % unit.size()] + (i % 8191 == 0)) : (uint8_t)((next() >> 30) & 1u);
        if (genuine[k]) {
            idx[k] = bz3_hip_stage_bwt(text[k].data(), in[k].data(), sizes[k]);
            if (idx[k] <= 0 || idx[k] > sizes[k]) return fail("forward transform", k);
            if (k == wrong_index) idx[k] = idx[k] / 2 + 1 != idx[k] ? idx[k] / 2 + 1 : idx[k] / 2 + 2;
        } else {
            in[k] = text[k];
            idx[k] = 1 + (int32_t)(next() % (uint32_t)sizes[k]);
        }
        out[k].assign(n + 32, 0xA5);
        alone[k].assign(n, 0);
        if (bz3_hip_stage_unbwt(in[k].data(), alone[k].data(), sizes[k], idx[k]) != 0) return fail("stage hook", k);
        if (genuine[k] && k != wrong_index && alone[k] != text[k]) return fail("stage hook: not the text", k);
    }
    const uint8_t * ins[N];
    uint8_t * outs[N];
    for (int k = 0; k < N; k++) {
        ins[k] = in[k].data();
        outs[k] = out[k].data();
    }
    if (bz3_hip_debug_unbwt_many(ins, outs, sizes, idx, N) != 0) return fail("the call failed", -1);
    for (int k = 0; k < N; k++) {
        if (memcmp(out[k].data(), alone[k].data(), (size_t)sizes[k]) != 0) return fail("bytes differ from the job alone", k);
        for (size_t t = (size_t)sizes[k]; t < out[k].size(); t++)
            if (out[k][t] != 0xA5) return fail("wrote beyond the job", k);
    }
    puts("unbwt batch ok");
    return 0;
}
