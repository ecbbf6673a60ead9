// TEST INFRASTRUCTURE ONLY.  A stand-alone host program for the sanitizers: the kernel sources and the API compiled against the CPU emulation
// of the HIP execution model (tests/emu) with -fsanitize=address,undefined, and ONE bz3_hip_debug_bwt_many call with runs of up to eight jobs.
// tests/test_bwt_batch8_emu.py builds it (the build line is there), writes the jobs, runs it as a child process and compares what it wrote with the
// oracle; nothing is preloaded.
// (ASAN_OPTIONS=detect_leaks=0: the per-device context of api_context.hip lives as long as the process and is never freed; every other check stays on.)
//
//   bwt_batch8 <jobs> <results>
//   jobs:    u32 count, then per job u32 n and n bytes            (little endian)
//   results: per job s32 primary index and the n transformed bytes
// Nothing may be written beyond a job's n bytes.  Prints "bwt batch8 ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/bz3_hip.h"
#include "../../include/libbz3.h"

namespace {
typedef std::vector<uint8_t> Bytes;

int fail(const char * what, int i) {
    fprintf(stderr, "bwt batch8: %s (job %d)\n", what, i);
    return 1;
}
}  // namespace

int main(int argc, char ** argv) {
    if (argc != 3) return fail("usage: bwt_batch8 <jobs> <results>", -1);
    FILE * f = fopen(argv[1], "rb");
    uint32_t count = 0;
    if (!f || fread(&count, 4, 1, f) != 1 || count == 0 || count > 64) return fail("jobs file", -1);
    std::vector<Bytes> text(count), out(count);
    std::vector<int32_t> sizes(count), idx(count, -7);
    std::vector<const uint8_t *> ins(count);
    std::vector<uint8_t *> outs(count);
    for (uint32_t k = 0; k < count; k++) {
        uint32_t n = 0;
        if (fread(&n, 4, 1, f) != 1 || n > (1u << 24)) return fail("jobs file", (int)k);
        text[k].resize(n);
        if (n && fread(text[k].data(), 1, n, f) != n) return fail("jobs file", (int)k);
        sizes[k] = (int32_t)n;
        out[k].assign((size_t)n + 32, 0xA5);
        ins[k] = text[k].data();
        outs[k] = out[k].data();
    }
    fclose(f);
    if (bz3_hip_debug_bwt_many(ins.data(), outs.data(), sizes.data(), idx.data(), (int32_t)count) != 0) return fail("the call failed", -1);
    f = fopen(argv[2], "wb");
    if (!f) return fail("results file", -1);
    for (uint32_t k = 0; k < count; k++) {
        for (size_t t = (size_t)sizes[k]; t < out[k].size(); t++)
            if (out[k][t] != 0xA5) return fail("wrote beyond the job", (int)k);
        if (fwrite(&idx[k], 4, 1, f) != 1 || (sizes[k] && fwrite(out[k].data(), 1, (size_t)sizes[k], f) != (size_t)sizes[k])) return fail("results file", (int)k);
    }
    if (fclose(f) != 0) return fail("results file", -1);
    puts("bwt batch8 ok");
    return 0;
}
