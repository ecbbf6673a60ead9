// TEST INFRASTRUCTURE ONLY.  A stand-alone host program for the sanitizers: the kernel sources and the API compiled against the CPU emulation
// of the HIP execution model (tests/emu) with -fsanitize=address,undefined, and one partial decode call that holds every request form.
//
//   FLAGS="-O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -DBZ3_EMU -DBZ3_EMU_API_UNITS -I tests/emu -I bzip3_amd/csrc \
//          -Wno-unknown-pragmas -Wno-attributes"
//   for f in bzip3_amd/csrc/*.hip; do g++ $FLAGS -x c++ -c $f -o $OUT/$(basename $f).o; done
//   g++ $FLAGS tests/emu/hip_emu.cpp tests/emu/mixed_call_main.cpp $OUT/*.o -lpthread -o $OUT/mixed_call && $OUT/mixed_call
//
// Two tensors of a block of 65 KiB + 3 and a short one, element size 4, one of them packed against a base.  Five frames in one
// bz3_hip_decompress_device_select_many call: a one-run range, the whole tensor, a two-run strided request, a two-piece select request and a
// select request with w <= l_0; once with windows of two chunks and once with all six chunks in one window, so that one launch holds whole,
// clipped, strided and select segments.  Every output byte is compared with tensor[phi(t)].  Prints "mixed call ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/bz3_hip.h"
#include "../../include/libbz3.h"

namespace {
typedef std::vector<uint8_t> Bytes;
typedef std::vector<uint64_t> Pieces;  // pairs (s_j, l_j)

struct Plan {
    int tensor;
    uint64_t offset, stride, count;
    Pieces pieces;
    size_t cap;
};

int fail(const char * what, int i) {
    fprintf(stderr, "mixed call: %s (frame %d)\n", what, i);
    return 1;
}
}  // namespace

int main() {
    const uint32_t bs = 65 * 1024 + 3, k = 4;
    const size_t T = (size_t)bs + 6001;
    Bytes x[2] = {Bytes(T), Bytes(T)}, base(T), frame[2];
    uint32_t seed = 12345;
    Bytes unit(997);
    for (uint8_t & b : unit) b = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
    for (size_t i = 0; i < T; i++) {
        x[0][i] = unit[i % 997];
        base[i] = unit[(i + 31) % 997];
        x[1][i] = (uint8_t)(base[i] + (i % 97 == 0));  // (few bytes differ from the base)
    }
    for (int t = 0; t < 2; t++) {
        frame[t].resize(bz3_bound(T) + 64);
        size_t n = frame[t].size();
        if (bz3_hip_compress_device_delta(bs, k, x[t].data(), t ? base.data() : nullptr, frame[t].data(), T, &n) != BZ3_OK) return fail("compress", t);
        frame[t].resize(n);
    }
    const std::vector<Plan> plan = {{1, bs + 10, 0, 1, {0, 777}, 1000000},
                                    {0, 0, 0, 1, {0, T}, 1000000},
                                    {0, bs + 5, 1000, 2, {3, 401}, 1000000},
                                    {1, bs + 100, 2000, 2, {0, 300, 650, 130}, 1000000},
                                    {0, bs + 9, 900, 3, {4, 500, 600, 100}, 333}};
    const int32_t n = (int32_t)plan.size();
    for (const char * window : {"2", "8"}) {
        setenv("BZ3_HIP_FRAME_WINDOW", window, 1);
        std::vector<Bytes> outs, bases;
        std::vector<std::vector<uint64_t>> index;  // phi(t) for t < w
        for (const Plan & p : plan) {
            uint64_t L = 0;
            for (size_t j = 1; j < p.pieces.size(); j += 2) L += p.pieces[j];
            const size_t w = p.cap < p.count * L ? p.cap : (size_t)(p.count * L);
            std::vector<uint64_t> phi;
            for (uint64_t q = 0; q < p.count; q++)
                for (size_t j = 0; j < p.pieces.size(); j += 2)
                    for (uint64_t b = 0; b < p.pieces[j + 1] && phi.size() < w; b++) phi.push_back(p.offset + q * p.stride + p.pieces[j] + b);
            Bytes bb;
            if (p.tensor == 1)
                for (uint64_t at : phi) bb.push_back(base[at]);
            index.push_back(phi);
            bases.push_back(bb);
            outs.push_back(Bytes(w + 24, 0xA5));
        }
        std::vector<uint32_t> ks((size_t)n, k);
        std::vector<const void *> ins, bps;
        std::vector<void *> ops;
        std::vector<size_t> in_sizes, base_sizes, out_sizes;
        std::vector<uint64_t> params;
        std::vector<const uint64_t *> lists;
        for (int32_t i = 0; i < n; i++) {
            const Plan & p = plan[(size_t)i];
            ins.push_back(frame[p.tensor].data());
            in_sizes.push_back(frame[p.tensor].size());
            bps.push_back(p.tensor == 1 ? bases[(size_t)i].data() : nullptr);
            base_sizes.push_back(bases[(size_t)i].size());
            ops.push_back(outs[(size_t)i].data());
            out_sizes.push_back(p.cap);
            params.insert(params.end(), {p.offset, p.stride, p.count, p.pieces.size() / 2});
            lists.push_back(p.pieces.data());
        }
        std::vector<int> rcs((size_t)n, 77);
        if (bz3_hip_decompress_device_select_many(n, ks.data(), ins.data(), in_sizes.data(), params.data(), lists.data(), bps.data(), base_sizes.data(), ops.data(),
                                                  out_sizes.data(), rcs.data()) != BZ3_OK)
            return fail("the call failed", -1);
        for (int32_t i = 0; i < n; i++) {
            const std::vector<uint64_t> & phi = index[(size_t)i];
            if (rcs[(size_t)i] != BZ3_OK || out_sizes[(size_t)i] != phi.size()) return fail("code or size", i);
            for (size_t t = 0; t < phi.size(); t++)
                if (outs[(size_t)i][t] != x[plan[(size_t)i].tensor][phi[t]]) return fail("bytes differ", i);
            for (size_t t = phi.size(); t < outs[(size_t)i].size(); t++)
                if (outs[(size_t)i][t] != 0xA5) return fail("wrote beyond the request", i);
        }
    }
    puts("mixed call ok");
    return 0;
}
