// api_hooks.hip -- the stage hooks of include/bz3_hip.h: one stage (or one primitive) on host buffers, for tests and profiling.
#include "api_internal.hpp"

using namespace bz3;
using namespace bz3::api;

// =====================================================================================================
// stage hooks on host buffers (tests / profiling)
// =====================================================================================================
namespace {

struct StageEnv {
    DeviceCtx * ctx = nullptr;
    hipStream_t s = nullptr;
    std::vector<void *> allocs;
    std::unique_lock<std::mutex> lock;
    StageEnv() {
        int dev = pick_device();
        if (dev < 0) {
            fprintf(stderr, "bzip3_amd: no HIP device available -- this library has no CPU code path\n");
            abort();
        }
        ctx = get_ctx(dev);
        HIP_CHECK(hipSetDevice(dev));
        HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        lock = std::unique_lock<std::mutex>(ctx->mu);
    }
    ~StageEnv() {
        (void)hipStreamSynchronize(s);
        for (void * p : allocs) (void)hipFree(p);
        (void)hipStreamDestroy(s);
    }
    u8 * dev(size_t bytes, const void * init = nullptr, size_t init_bytes = 0) {
        void * p = nullptr;
        HIP_CHECK(hipMalloc(&p, bytes + 4096));
        allocs.push_back(p);
        if (init && init_bytes) HIP_CHECK(hipMemcpy(p, init, init_bytes, hipMemcpyHostToDevice));
        return (u8 *)p;
    }
    void down(void * host, const void * d, size_t bytes) {
        HIP_CHECK(hipStreamSynchronize(s));
        if (bytes) HIP_CHECK(hipMemcpy(host, d, bytes, hipMemcpyDeviceToHost));
    }
    u32 word(const u32 * d) {
        u32 v = 0;
        down(&v, d, 4);
        return v;
    }
};

template <typename F>
auto stage_guard(F && f) -> decltype(f()) {
    try {
        return f();
    } catch (const HipError & e) {
        fprintf(stderr, "bzip3_amd: HIP failure '%s' at %s:%d\n", e.what, e.file, e.line);
        abort();
    }
}

}  // namespace

extern "C" {

BZIP3_API uint32_t bz3_hip_stage_crc32c(const uint8_t * data, size_t n, uint32_t init) {
    return stage_guard([&]() -> u32 {
        StageEnv e;
        u8 * d = e.dev(n + 16, data, n);
        u32 * w = (u32 *)e.dev(64);
        crc32c_device(d, n, init, e.ctx->d_crc, w, e.s);
        return e.word(w + 1);
    });
}

BZIP3_API int32_t bz3_hip_stage_mrle_encode(const uint8_t * in, int32_t n, uint8_t * out) {
    return stage_guard([&]() -> s32 {
        StageEnv e;
        u8 * d = e.dev((size_t)n + 16, in, (size_t)n);
        u8 * o = e.dev((size_t)n + 64);
        Arena a = e.ctx->arena_for(workspace_bytes_for((u64)n + 64));
        MrleEncScratch sc;
        mrle_encode_size(d, (u32)n, sc, a, e.s);
        const s32 size = (s32)(32u + e.word(sc.total));
        mrle_encode_write(d, (u32)n, sc, o, e.s);
        e.down(out, o, (size_t)size);
        return size;
    });
}

BZIP3_API int bz3_hip_stage_mrle_decode(const uint8_t * in, uint8_t * out, int32_t outlen, int32_t maxin) {
    return stage_guard([&]() -> int {
        if (maxin < 32) return 1;
        StageEnv e;
        u8 * d = e.dev((size_t)maxin + 16, in, (size_t)maxin);
        u8 * o = e.dev((size_t)outlen + 64);
        u32 * w = (u32 *)e.dev(64);
        Arena a = e.ctx->arena_for(workspace_bytes_for((u64)maxin + 64));
        mrle_decode(d, (u32)maxin, o, (u32)outlen, w, a, e.s);
        const u32 got = e.word(w);
        e.down(out, o, (size_t)(got < (u32)outlen ? got : (u32)outlen));
        return got != (u32)outlen;
    });
}

BZIP3_API int32_t bz3_hip_stage_lzp_encode(const uint8_t * in, int32_t n, uint8_t * out) {
    return stage_guard([&]() -> s32 {
        StageEnv e;
        u8 * d = e.dev((size_t)n + 64, in, (size_t)n);
        u8 * o = e.dev((size_t)n + 64);
        Arena a = e.ctx->arena_for(workspace_bytes_for((u64)n + 64));
        const s32 r = lzp_encode(d, (u32)n, o, a, e.s);
        if (r > 0) e.down(out, o, (size_t)r);
        return r;
    });
}

// Tests only: bz3_hip_stage_lzp_encode plus what the serial driver did (lzp.hip k_lzp_driver, LzDriverOut) and its two constants.
BZIP3_API int32_t bz3_hip_debug_lzp_encode(const uint8_t * in, int32_t n, uint8_t * out, uint32_t stats[6]) {
    return stage_guard([&]() -> s32 {
        StageEnv e;
        u8 * d = e.dev((size_t)n + 64, in, (size_t)n);
        u8 * o = e.dev((size_t)n + 64);
        Arena a = e.ctx->arena_for(workspace_bytes_for((u64)n + 64));
        LzDriverOut drv;
        const s32 r = lzp_encode(d, (u32)n, o, a, e.s, &drv);
        if (r > 0) e.down(out, o, (size_t)r);
        if (stats) {
            stats[0] = drv.end_pos;
            stats[1] = drv.n_matches;
            stats[2] = drv.iterations;
            stats[3] = drv.evaluated;
            lzp_driver_geometry(stats[4], stats[5]);
        }
        return r;
    });
}

BZIP3_API int32_t bz3_hip_stage_lzp_decode(const uint8_t * in, int32_t n, uint8_t * out, int32_t max) {
    return stage_guard([&]() -> s32 {
        StageEnv e;
        u8 * d = e.dev((size_t)n + 64, in, (size_t)n);
        u8 * o = e.dev((size_t)max + 64);
        Arena a = e.ctx->arena_for(workspace_bytes_for((u64)n + 64));
        if (n < 4) return -1;  // :252
        u32 * d_result = a.take<u32>(4);
        LzpDecodeJob job{dev_addr(d), dev_addr(o), dev_addr(a.take<u32>(LZP_LUT_WORDS)), dev_addr(d_result), (u32)n, (u32)max};
        LzpDecodeJob * d_job = a.take<LzpDecodeJob>(1);
        lzp_decode_batch(&job, d_job, 1, e.s);
        const s32 r = (s32)e.word(d_result);
        if (r > 0) e.down(out, o, (size_t)r);
        return r;
    });
}

// Wall time of the last bz3_hip_stage_bwt / bz3_hip_stage_unbwt call's transform alone (both are synchronous: from the first launch to
// the last result on the host; the hook's own allocations and PCIe copies are outside).  Profiling only.
static std::atomic<float> g_stage_ms{0.f};
BZIP3_API float bz3_hip_stage_last_ms(void) { return g_stage_ms.load(); }

BZIP3_API int32_t bz3_hip_stage_bwt(const uint8_t * in, uint8_t * out, int32_t n) {
    return stage_guard([&]() -> s32 {
        StageEnv e;
        u8 * d = e.dev((size_t)n + 64, in, (size_t)n);
        u8 * o = e.dev((size_t)n + 64);
        Arena a = e.ctx->arena_for(workspace_bytes_for((u64)n + 64));
        HIP_CHECK(hipStreamSynchronize(e.s));
        const auto t0 = std::chrono::steady_clock::now();
        const s32 idx = bwt_forward(d, (u32)n, o, a, e.s, nullptr);
        g_stage_ms.store(std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count());
        e.down(out, o, (size_t)n);
        return idx;
    });
}

// Tests and sweeps only: the forward BWT of `count` blocks on host buffers, through bwt_forward_batch in runs of at most BWT_MAX_BATCH in the
// order given (blocks of fewer than 2 bytes apart) -- the forward twin of bz3_hip_debug_unbwt_many.  Synchronous.  The arena is sized for a
// full run of the largest block; how long a run is, is bwt_batch_size's decision (bz3_hip_debug_set_bwt_batch forces it).  idx_out[k] receives
// block k's primary index (0 for an empty block, 1 for one byte).  Returns 0, or -1 on bad arguments.
// rec (may be NULL): BWT_RECORD_WORDS words per block, what the sorter did with it (bwt_record_flatten; a block of fewer than 2 bytes: the geometry alone).
static s32 debug_bwt_many(const uint8_t * const * in, uint8_t * const * out, const int32_t * n, int32_t * idx_out, int32_t count, uint32_t * rec) {
    return stage_guard([&]() -> s32 {
        if (count < 0 || (count > 0 && (!in || !out || !n || !idx_out))) return -1;
        std::vector<BwtRecord> recs(rec ? (size_t)count : 0);
        u64 largest = 0;
        for (s32 k = 0; k < count; k++) {
            if (n[k] < 0) return -1;
            if ((u64)n[k] > largest) largest = (u64)n[k];
        }
        std::vector<BwtBatchItem> items;
        std::vector<u32> sizes;
        std::vector<s32> owner;
        StageEnv e;
        for (s32 k = 0; k < count; k++) {
            idx_out[k] = n[k];  // (n < 2: the block is its own transform)
            if (n[k] == 1) out[k][0] = in[k][0];
            if (n[k] < 2) continue;
            const u8 * d = e.dev((size_t)n[k] + 64, in[k], (size_t)n[k]);
            items.push_back(BwtBatchItem{d, (u32)n[k], e.dev((size_t)n[k] + 64), nullptr, nullptr, nullptr, 0, rec ? &recs[(size_t)k] : nullptr});
            sizes.push_back((u32)n[k]);
            owner.push_back(k);
        }
        for (s32 k = 0; rec && k < count; k++) bwt_record_flatten(recs[(size_t)k], (u32)n[k], rec + (size_t)k * BWT_RECORD_WORDS);  // (blocks that never enter a run)
        if (items.empty()) return 0;
        const size_t plain = workspace_bytes_for(largest + 64), full = (size_t)BWT_MAX_BATCH * bwt_workspace_bytes(largest + 64);
        Arena a = e.ctx->arena_for(plain > full ? plain : full);
        HIP_CHECK(hipStreamSynchronize(e.s));
        const auto t0 = std::chrono::steady_clock::now();
        for (size_t at = 0; at < items.size();) {
            const u32 b = bwt_batch_size(sizes.data() + at, (u32)(items.size() - at), a.cap - a.used);
            bwt_forward_batch(items.data() + at, b, a, e.s);
            at += b;
        }
        g_stage_ms.store(std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count());
        for (size_t j = 0; j < items.size(); j++) {
            e.down(out[owner[j]], items[j].out, (size_t)items[j].n);
            idx_out[owner[j]] = items[j].idx;
            if (rec) bwt_record_flatten(recs[(size_t)owner[j]], items[j].n, rec + (size_t)owner[j] * BWT_RECORD_WORDS);
        }
        return 0;
    });
}
BZIP3_API int32_t bz3_hip_debug_bwt_many(const uint8_t * const * in, uint8_t * const * out, const int32_t * n, int32_t * idx_out, int32_t count) {
    return debug_bwt_many(in, out, n, idx_out, count, nullptr);
}
// Tests only: bz3_hip_debug_bwt_many plus a record per block of what the sorter did with it -- its code table, the counter words of every pass of the resolve
// loop, whether and from which depth it went to rank doubling, the rounds of that, the statistics -- and the geometry constants a test needs (the layout:
// bwt.hip bwt_record_flatten).  rec holds rec_words words per block; rec_words must be at least the record's size, which the call leaves in rec[0].
// bz3_hip_debug_bwt_record is the same for one block alone.  -1 on bad arguments, -2 when rec_words is too small (nothing is run).
BZIP3_API int32_t bz3_hip_debug_bwt_record_many(const uint8_t * const * in, uint8_t * const * out, const int32_t * n, int32_t * idx_out, int32_t count, uint32_t * rec, uint32_t rec_words) {
    if (!rec) return -1;
    if (rec_words < BWT_RECORD_WORDS) {
        if (rec_words) rec[0] = BWT_RECORD_WORDS;
        return -2;
    }
    if (rec_words == BWT_RECORD_WORDS) return debug_bwt_many(in, out, n, idx_out, count, rec);
    std::vector<uint32_t> flat((size_t)(count > 0 ? count : 0) * BWT_RECORD_WORDS);
    const s32 rc = debug_bwt_many(in, out, n, idx_out, count, flat.data());
    for (s32 k = 0; rc == 0 && k < count; k++) memcpy(rec + (size_t)k * rec_words, flat.data() + (size_t)k * BWT_RECORD_WORDS, (size_t)BWT_RECORD_WORDS * 4);
    return rc;
}
BZIP3_API int32_t bz3_hip_debug_bwt_record(const uint8_t * in, int32_t n, uint8_t * out, int32_t * idx_out, uint32_t * rec, uint32_t rec_words) {
    return bz3_hip_debug_bwt_record_many(&in, &out, &n, idx_out, 1, rec, rec_words);
}
BZIP3_API void bz3_hip_debug_set_bwt_batch(int b) { bwt_set_batch(b); }

BZIP3_API int32_t bz3_hip_stage_unbwt(const uint8_t * in, uint8_t * out, int32_t n, int32_t idx) {
    return stage_guard([&]() -> s32 {
        if (n < 0) return -1;
        if (n <= 1) {
            if (idx != n) return -1;
            if (n == 1) out[0] = in[0];
            return 0;
        }
        if (idx <= 0 || idx > n) return -1;
        StageEnv e;
        u8 * d = e.dev((size_t)n + 64, in, (size_t)n);
        u8 * o = e.dev((size_t)n + 64);
        Arena a = e.ctx->arena_for(workspace_bytes_for((u64)n + 64));
        HIP_CHECK(hipStreamSynchronize(e.s));
        const auto t0 = std::chrono::steady_clock::now();
        bwt_inverse(d, (u32)n, (u32)idx, o, a, e.s);
        HIP_CHECK(hipStreamSynchronize(e.s));
        g_stage_ms.store(std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count());
        e.down(out, o, (size_t)n);
        return 0;
    });
}

// Tests and sweeps only: the inverse BWT of `count` blocks on host buffers, through bwt_inverse_batch in runs of at most UB_MAX_BATCH in the order
// given (blocks of fewer than 2 bytes apart) -- the way to put chosen sizes into one batch.  Synchronous.  The arena is sized for a full run of the
// largest block.  Returns 0, or -1 when a block's arguments are ones libsais_unbwt refuses (nothing is written then).
BZIP3_API int32_t bz3_hip_debug_unbwt_many(const uint8_t * const * in, uint8_t * const * out, const int32_t * n, const int32_t * idx, int32_t count) {
    return stage_guard([&]() -> s32 {
        if (count < 0 || (count > 0 && (!in || !out || !n || !idx))) return -1;
        u64 largest = 0;
        for (s32 k = 0; k < count; k++) {
            if (n[k] < 0 || (n[k] <= 1 ? idx[k] != n[k] : (idx[k] <= 0 || idx[k] > n[k]))) return -1;
            if ((u64)n[k] > largest) largest = (u64)n[k];
        }
        std::vector<UbBatchItem> items;
        std::vector<u32> sizes;
        std::vector<s32> owner;
        StageEnv e;
        for (s32 k = 0; k < count; k++) {
            if (n[k] == 1) out[k][0] = in[k][0];
            if (n[k] < 2) continue;
            const u8 * d = e.dev((size_t)n[k] + 64, in[k], (size_t)n[k]);
            items.push_back(UbBatchItem{d, e.dev((size_t)n[k] + 64), (u32)n[k], (u32)idx[k]});
            sizes.push_back((u32)n[k]);
            owner.push_back(k);
        }
        if (items.empty()) return 0;
        const size_t plain = workspace_bytes_for(largest + 64), full = unbwt_batch_workspace_bytes(largest + 64, UB_MAX_BATCH);
        Arena a = e.ctx->arena_for(plain > full ? plain : full);
        HIP_CHECK(hipStreamSynchronize(e.s));
        const auto t0 = std::chrono::steady_clock::now();
        for (size_t at = 0; at < items.size();) {
            const u32 b = unbwt_batch_size(sizes.data() + at, (u32)(items.size() - at), a.cap - a.used, 0u);
            bwt_inverse_batch(items.data() + at, b, a, e.s);
            HIP_CHECK(hipStreamSynchronize(e.s));
            at += b;
        }
        g_stage_ms.store(std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count());
        for (size_t j = 0; j < items.size(); j++) e.down(out[owner[j]], items[j].out, (size_t)items[j].n);
        return 0;
    });
}

// Tests only: the CU masks of the partition (DeviceCtx::cu_masks) for a device of `cus` CUs and `reserve` reserved ones: words = (cus + 31) / 32 each.
BZIP3_API int32_t bz3_hip_debug_cu_masks(int cus, int reserve, uint32_t * side, uint32_t * rest) {
    if (cus < 32 || cus > 1024 || reserve < 8 || !side || !rest) return -1;
    std::vector<uint32_t> a, b;
    DeviceCtx::cu_masks(cus, reserve, a, b);
    for (size_t k = 0; k < a.size(); k++) {
        side[k] = a[k];
        rest[k] = b[k];
    }
    return (int32_t)a.size();
}

// Tests only: sort.hip's device-wide exclusive scan on a host buffer (in place); returns the grand total through *total.
BZIP3_API int32_t bz3_hip_debug_scan_u32(uint32_t * data, uint32_t n, uint32_t * total) {
    return stage_guard([&]() -> s32 {
        if (n == 0) return -1;
        StageEnv e;
        u32 * d = (u32 *)e.dev((size_t)n * 4 + 64, data, (size_t)n * 4);
        u32 * t = (u32 *)e.dev(64);
        Arena a = e.ctx->arena_for(scan_temp_words(n) * 4 + (1u << 20));
        exclusive_scan_u32(d, n, t, a, e.s);
        e.down(data, d, (size_t)n * 4);
        if (total) *total = e.word(t);
        return 0;
    });
}

// Tests only: the stable LSD radix sort of sort.hip on host buffers -- (keys[i], i) sorted over key bits [0, key_bits) with digits of
// digit_bits (8 or 9) bits; passes of up to RS_RAW_TILES tiles take the scatter that reads the raw count table (round 5), larger ones
// the scanned table.  Returns the number of passes, -1 on bad arguments.
BZIP3_API int32_t bz3_hip_debug_sort_u32(const uint32_t * keys, uint32_t n, int key_bits, int digit_bits, uint32_t * sorted_keys, uint32_t * sorted_index) {
    return stage_guard([&]() -> s32 {
        if ((digit_bits != 8 && digit_bits != 9) || key_bits < 1 || key_bits > 32 || n == 0) return -1;
        StageEnv e;
        u32 * k[2] = {(u32 *)e.dev((size_t)n * 4 + 64, keys, (size_t)n * 4), (u32 *)e.dev((size_t)n * 4 + 64)};
        u32 * v[2] = {(u32 *)e.dev((size_t)n * 4 + 64), (u32 *)e.dev((size_t)n * 4 + 64)};
        Arena a = e.ctx->arena_for(radix_temp_bytes(n, digit_bits) + (1u << 20));
        int cur = 0, passes = 0;
        for (int shift = 0; shift < key_bits; shift += digit_bits, passes++) {
            const u32 * vin = passes ? v[cur] : nullptr;  // the first pass generates the indices
            if (digit_bits == 9) radix_pass_bits<u32, 9>(k[cur], k[cur ^ 1], vin, v[cur ^ 1], n, shift, 0xFFFFFFFFu, 0u, a, e.s);
            else radix_pass<u32>(k[cur], k[cur ^ 1], vin, v[cur ^ 1], n, shift, 0xFFFFFFFFu, 0u, a, e.s);
            cur ^= 1;
        }
        e.down(sorted_keys, k[cur], (size_t)n * 4);
        e.down(sorted_index, v[cur], (size_t)n * 4);
        return passes;
    });
}

// One CM job through the variant the current mode selects (auto = full model for a single block); a block the
// row-cache kernel gives up is coded again by the full-model kernel, as in run_cm_jobs.
extern "C++" template <class Job, class Launch>
void stage_cm_job(StageEnv & e, Job job, Launch && go) {
    const int variant = cm_variant_for(e.ctx, 1, std::is_same<Job, CmEncodeJob>::value);
    u32 * status = nullptr;
    if (cm_variant_has_rows(variant)) {
        job.spill = dev_addr(e.dev(CM_SPILL_BYTES));
        status = (u32 *)e.dev(64);
        HIP_CHECK(hipMemsetAsync(status, 0, 64, e.s));  // on the launching stream: a non-blocking stream does not order with the null stream
        job.status = dev_addr(status);
        job.miss_base = cm_variant_is_test(variant) ? 64u : CM_MISS_BASE;
        job.miss_shift = cm_variant_is_test(variant) ? 3u : CM_MISS_SHIFT;
    }
    Job * d_job = (Job *)e.dev(sizeof job, &job, sizeof job);
    go(d_job, 1u, e.s, variant);
    if (cm_variant_has_rows(variant) && e.word(status) != 0u) {
        g_cm_given_up.fetch_add(1u);
        go(d_job, 1u, e.s, (int)CM_VARIANT_FULL);
    }
}

BZIP3_API int32_t bz3_hip_stage_cm_encode(const uint8_t * in, int32_t n, uint8_t * out) {
    return stage_guard([&]() -> s32 {
        StageEnv e;
        u8 * d = e.dev((size_t)n + 64, in, (size_t)n);
        u8 * o = e.dev(bz3_bound((size_t)n) + 64);
        u32 * w = (u32 *)e.dev(64);
        const char * dbg = getenv("BZ3_CM_DEBUG");  // profiling only: 1 = coder alone, 2 = model alone (output invalid)
        CmEncodeJob job{dev_addr(d), dev_addr(o), dev_addr(w), (u32)n, dbg ? (u32)atoi(dbg) : 0u};
        // tests: BZ3_CM_TEST_GAP=<g> codes IN PLACE, the input g bytes above the output in one buffer (cm.hip CmSink), with a
        // side buffer of BZ3_CM_TEST_SIDE bytes (default 64 KiB); returns -1 when the side buffer overflowed
        const char * tg = getenv("BZ3_CM_TEST_GAP");
        u8 * side = nullptr;
        if (tg) {
            const size_t g = (size_t)atol(tg);
            const char * ts = getenv("BZ3_CM_TEST_SIDE");
            const size_t side_cap = ts ? (size_t)atol(ts) : CM_SIDE_BYTES;
            u8 * both = e.dev(g + (size_t)n + 64);
            HIP_CHECK(hipMemcpy(both + g, d, (size_t)n, hipMemcpyDeviceToDevice));
            side = e.dev(side_cap + 64);
            o = both;
            job.in = dev_addr(both + g);
            job.out = dev_addr(both);
            job.gap = (u32)g;
            job.side = dev_addr(side);
            job.side_cap = (u32)side_cap;
        }
        stage_cm_job(e, job, [](const CmEncodeJob * j, u32 nj, hipStream_t st, int variant) { cm_encode_batch(j, nj, st, variant); });
        const u32 coded = e.word(w), sw = e.word(w + 1);
        if (coded == 0xFFFFFFFFu) return -1;
        const u32 head = (tg && sw < coded) ? sw : coded;
        e.down(out, o, (size_t)head);
        if (head < coded) e.down(out + head, side, (size_t)(coded - head));
        return (s32)coded;
    });
}

BZIP3_API void bz3_hip_stage_cm_decode(const uint8_t * in, int32_t in_size, uint8_t * out, int32_t n) {
    stage_guard([&]() -> int {
        StageEnv e;
        u8 * d = e.dev((size_t)in_size + 64, in, (size_t)in_size);
        u8 * o = e.dev((size_t)n + 64);
        const char * dbg = getenv("BZ3_CM_DEBUG");  // profiling only (output invalid)
        CmDecodeJob job{dev_addr(d), dev_addr(o), (u32)in_size, (u32)n, dbg ? (u32)atoi(dbg) : 0u, 0u};
        stage_cm_job(e, job, [](const CmDecodeJob * j, u32 nj, hipStream_t st, int variant) { cm_decode_batch(j, nj, st, variant); });
        e.down(out, o, (size_t)n);
        return 0;
    });
}

// Profiling: `copies` identical CM decode jobs in ONE launch (same coded input, one output buffer each), through the kernel
// variant the current mode selects (no hand-back of given-up blocks: this measures the variant itself).  Returns the launch
// time in ms (HIP events).  out receives the n decoded bytes of copy 0.  With BZ3_CM_DEBUG=3 the guess-ahead decoder leaves
// cycle counters instead of the first output bytes (walker: wait, walk, slow-path bytes, wrong guesses at u64[0..3]; model
// wave 1: speculate, wait, redo at u64[8..10]; the walker's wait behind wrong guesses and its right guesses at u64[4..5]); `counters`, if not
// NULL, receives u64[16] per copy.  The counters need a block of 256 bytes or more.
BZIP3_API float bz3_hip_stage_cm_decode_many(const uint8_t * in, int32_t in_size, uint8_t * out, int32_t n, int32_t copies, uint64_t * counters) {
    return stage_guard([&]() -> float {
        StageEnv e;
        const char * dbg = getenv("BZ3_CM_DEBUG");
        const u32 debug = dbg ? (u32)atoi(dbg) : 0u;
        if (copies < 1 || n < 1 || ((debug || counters) && n < 256)) return -1.f;
        u8 * d = e.dev((size_t)in_size + 64, in, (size_t)in_size);
        const size_t stride = ((size_t)n + 64 + 255) & ~(size_t)255;
        u8 * o = e.dev(stride * (size_t)copies);
        const int variant = cm_variant_for(e.ctx, (size_t)copies, false);
        u8 * spill = cm_variant_has_rows(variant) ? e.dev(CM_SPILL_BYTES * (size_t)copies) : nullptr;
        u32 * status = (u32 *)e.dev(4 * (size_t)copies + 64);
        HIP_CHECK(hipMemsetAsync(status, 0, 4 * (size_t)copies, e.s));
        std::vector<CmDecodeJob> jobs;
        for (int32_t k = 0; k < copies; k++) {
            CmDecodeJob j{dev_addr(d), dev_addr(o + stride * (size_t)k), (u32)in_size, (u32)n, debug, 0u};
            if (spill) {
                j.spill = dev_addr(spill + CM_SPILL_BYTES * (size_t)k);
                j.status = dev_addr(status + k);
                j.miss_base = CM_MISS_BASE;
                j.miss_shift = CM_MISS_SHIFT;
            }
            jobs.push_back(j);
        }
        CmDecodeJob * d_jobs = (CmDecodeJob *)e.dev(sizeof(CmDecodeJob) * jobs.size(), jobs.data(), sizeof(CmDecodeJob) * jobs.size());
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        HIP_CHECK(hipEventRecord(e0, e.s));
        cm_decode_batch(d_jobs, (u32)copies, e.s, variant, (debug & 15u) == 3u);
        HIP_CHECK(hipEventRecord(e1, e.s));
        HIP_CHECK(hipStreamSynchronize(e.s));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        e.down(out, o, (size_t)n);
        if (counters)
            for (int32_t k = 0; k < copies; k++) e.down(counters + 16 * (size_t)k, o + stride * (size_t)k, 128);
        if (getenv("BZ3_CM_MANY_CHECK")) {  // every copy must have decoded the same bytes (-2 otherwise)
            std::vector<u8> other((size_t)n);
            for (int32_t k = 1; k < copies; k++) {
                e.down(other.data(), o + stride * (size_t)k, (size_t)n);
                if (memcmp(other.data(), out, (size_t)n) != 0) return -2.f;
            }
        }
        return ms;
    });
}

// Profiling: `copies` identical CM encode jobs in ONE launch through the encoder of the current CM kernel variant; returns the launch
// time in ms (HIP events) and the coded size of copy 0 in *coded (its bytes in `out`, capacity bz3_bound(n)).  BZ3_CM_DEBUG=1 / 2 runs
// the coder wave / the model waves alone (output invalid): which side of the LDS ring limits the kernel at a given co-residency.
// BZ3_CM_MANY_CHECK=1: every copy's coded bytes are compared with copy 0's (-2 when they differ).
BZIP3_API float bz3_hip_stage_cm_encode_many(const uint8_t * in, int32_t n, uint8_t * out, int32_t * coded, int32_t copies) {
    return stage_guard([&]() -> float {
        StageEnv e;
        if (copies < 1 || n < 1) return -1.f;
        u8 * d = e.dev((size_t)n + 64, in, (size_t)n);
        const size_t stride = (bz3_bound((size_t)n) + 64 + 255) & ~(size_t)255;
        u8 * o = e.dev(stride * (size_t)copies);
        u32 * w = (u32 *)e.dev(16 * (size_t)copies + 64);
        const char * dbg = getenv("BZ3_CM_DEBUG");
        const u32 debug = dbg ? (u32)atoi(dbg) : 0u;
        const int variant = cm_variant_for(e.ctx, (size_t)copies, true);
        u8 * spill = cm_variant_has_rows(variant) ? e.dev(CM_SPILL_BYTES * (size_t)copies) : nullptr;
        u32 * status = (u32 *)e.dev(4 * (size_t)copies + 64);
        HIP_CHECK(hipMemsetAsync(status, 0, 4 * (size_t)copies, e.s));
        u32 * claim = getenv("BZ3_CM_NO_CLAIM") ? nullptr : (u32 *)e.dev(CM_CLAIM_WORDS * 4);  // (BZ3_CM_NO_CLAIM: the block index decides which wave codes, as up to round 4)
        if (claim) HIP_CHECK(hipMemsetAsync(claim, 0, CM_CLAIM_WORDS * 4, e.s));
        std::vector<CmEncodeJob> jobs;
        for (int32_t k = 0; k < copies; k++) {
            CmEncodeJob j{dev_addr(d), dev_addr(o + stride * (size_t)k), dev_addr(w + 4 * (size_t)k), (u32)n, debug};
            j.claim = claim ? dev_addr(claim) : 0;
            if (spill) {
                j.spill = dev_addr(spill + CM_SPILL_BYTES * (size_t)k);
                j.status = dev_addr(status + k);
                j.miss_base = CM_MISS_BASE;
                j.miss_shift = CM_MISS_SHIFT;
            }
            jobs.push_back(j);
        }
        CmEncodeJob * d_jobs = (CmEncodeJob *)e.dev(sizeof(CmEncodeJob) * jobs.size(), jobs.data(), sizeof(CmEncodeJob) * jobs.size());
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        HIP_CHECK(hipEventRecord(e0, e.s));
        cm_encode_batch(d_jobs, (u32)copies, e.s, variant);
        HIP_CHECK(hipEventRecord(e1, e.s));
        HIP_CHECK(hipStreamSynchronize(e.s));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        const u32 got = e.word(w);
        if (coded) *coded = (int32_t)got;
        if (got != 0xFFFFFFFFu && got <= bz3_bound((size_t)n) && !(debug & 15u)) {
            e.down(out, o, (size_t)got);
            if (getenv("BZ3_CM_MANY_CHECK")) {  // every copy must have coded the same bytes (-2 otherwise)
                std::vector<u8> other((size_t)got);
                for (int32_t k = 1; k < copies; k++) {
                    if (e.word(w + 4 * (size_t)k) != got) return -2.f;
                    e.down(other.data(), o + stride * (size_t)k, (size_t)got);
                    if (memcmp(other.data(), out, (size_t)got) != 0) return -2.f;
                }
            }
        }
        return ms;
    });
}

}  // extern "C"
