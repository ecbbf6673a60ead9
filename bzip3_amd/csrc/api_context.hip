// api_context.hip -- the per-device context (CU masks, side streams, swap-buffer pool, workspace arena), the states, the second half of the
// headroom rule, and the control, timing and debug-counter entry points of include/bz3_hip.h.
//
// Every mutable global of the API layer is defined HERE, in one translation unit, so that no initialisation order between the units
// exists; api_internal.hpp declares the ones the other units use.
#include "api_internal.hpp"

using namespace bz3;
using namespace bz3::api;

namespace {

std::mutex g_mu;
std::vector<DeviceCtx *> g_ctx;
int g_device_count = -1;
std::atomic<int> g_bound_device{-2};  // -2 = not initialised from the environment yet, -1 = round robin
std::atomic<unsigned> g_rr{0};
std::atomic<unsigned> g_headroom_trims{0}, g_headroom_releases{0};  // statistics (bz3_hip_debug_headroom_events)

#ifndef BZ3_EMU
// The rings run a group's whole-GPU kernels on one stream and the serial one-workgroup-per-block kernels (LZP drivers / decoders) of up to four windows on
// side streams.  The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and streams that share a queue do not
// overlap: with five streams on four queues the tail of 256 x 64 MiB blocks measured 3.23 s, with more queues 3.08 s (profiles/r05_tail_hw_queues.txt).
// The library asks for 8 ONCE, when it is loaded (before any thread of the host program can be reading the environment through it), never overrides the
// user's setting, and BZ3_HIP_SET_HW_QUEUES=0 turns even that off.  It only has an effect if the runtime is not up yet: a host program that initialises HIP
// first (bench.py through torch) sets the variable itself -- INTEGRATION.md lists it as a requirement on the host.
__attribute__((constructor)) static void bz3_hip_on_load() {
    const char * e = getenv("BZ3_HIP_SET_HW_QUEUES");
    if (!e || atoi(e) != 0) (void)setenv("GPU_MAX_HW_QUEUES", "8", 0);
}
#endif

}  // namespace

namespace bz3 {
namespace api {

// ---- the globals the other units see (api_internal.hpp) ----------------------------------------------------------------------------
std::atomic<int> g_lean{-1};  // -1 = not read from the environment yet; see bz3_hip_set_lean_states
std::atomic<int> g_front_end_ring{0};  // window | slots << 16 of the last encode_group (bz3_hip_debug_front_end_ring)
std::atomic<int> g_arena_swaps{0};  // swap buffers served from the arena (bz3_hip_debug_arena_swap_buffers)
std::atomic<unsigned> g_cm_given_up{0};  // blocks the row-cache CM kernels handed back to the full-model kernels (statistics)
std::atomic<unsigned> g_crc_launches{0};  // kernels launched by bz3_hip_crc32c_device_many (statistics, bz3_hip_debug_crc_launches)
std::atomic<unsigned> g_cm_launches{0};  // CM kernel launches (statistics, bz3_hip_debug_cm_launches)
std::atomic<unsigned> g_cm_routed_full{0};  // blocks sent straight to the full-model kernels by their histogram / payload size (statistics)
std::atomic<int> g_cm_mode{-2};  // -2 = not read from the environment yet, -1 = auto, else CM_VARIANT_*
std::atomic<long long> g_ws_headroom{-1};  // bytes; -1 = the environment decides
std::atomic<int> g_keep_ws{-1};  // bz3_hip_set_keep_workspace: -1 = the environment decides
std::atomic<int> g_front_duo{-1};  // bz3_hip_set_front_end_duo: -1 = the environment decides (BZ3_HIP_FRONT_DUO, read once)
std::atomic<int> g_groups_running{0}, g_groups_peak{0};  // statistics (bz3_hip_debug_peak_concurrent_groups)
Collector g_collect;
std::atomic<int> g_collect_window_us{200};
std::atomic<unsigned> g_collect_batches{0}, g_collect_largest{0};

void DeviceCtx::cu_masks(int cus, int reserve, std::vector<uint32_t> & side, std::vector<uint32_t> & main) {
    const int words = (cus + 31) / 32;
    side.assign((size_t)words, 0u);
    main.assign((size_t)words, 0u);
    for (int i = 0; i < cus; i++) main[(size_t)(i >> 5)] |= 1u << (i & 31);
    const int per = reserve / 8 > 0 ? reserve / 8 : 1;
    for (int a = 0; a < 8 && a * 32 < cus; a++)
        for (int t = 0; t < per && t < 8; t++) {
            const int j = t & 3;
            const int i = 32 * a + 8 * j + ((a + 2 * j + (t >> 2)) & 7);
            if (i < cus) {
                side[(size_t)(i >> 5)] |= 1u << (i & 31);
                main[(size_t)(i >> 5)] &= ~(1u << (i & 31));
            }
        }
}

void DeviceCtx::ensure_aux() {  // caller holds mu
    if (aux_ready) return;
    // built into locals and committed only when everything exists: a failure half way must not leave a context whose first
    // stream is there and whose events are not (every later call would record on null events)
    hipStream_t st[AUX] = {}, sm[AUX] = {}, rs = nullptr, du = nullptr;
    hipEvent_t e0[AUX] = {}, e1[AUX] = {}, ep = nullptr;
    int reserved = 0, device_cus = 0;
    try {
        HIP_CHECK(hipEventCreate(&ep));
#ifndef BZ3_EMU
        const int want = cu_reserve_setting();
        int real_cus = 0;  // (the device's own count: `cus` may be a test's pretence, BZ3_HIP_CUS)
        if (hipDeviceGetAttribute(&real_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) real_cus = 0;
        if (want >= 8 && real_cus >= 64 && real_cus % 32 == 0) {
            std::vector<uint32_t> side, mainm;
            cu_masks(real_cus, want, side, mainm);
            bool ok = hipExtStreamCreateWithCUMask(&rs, (uint32_t)mainm.size(), mainm.data()) == hipSuccess;
            // (RING_SLOTS of them: every masked stream is a hardware queue of its own, and call 8 -- eight of them, a tail ring of 8 x 8 -- ran every
            // phase of the tail slower than call 6's four; a ring with more slots than that runs unpartitioned on the plain streams)
            for (int k = 0; ok && k < RING_SLOTS; k++) ok = hipExtStreamCreateWithCUMask(&sm[k], (uint32_t)side.size(), side.data()) == hipSuccess;
            if (!ok) {  // the runtime refuses: plain streams only
                (void)hipGetLastError();
                if (rs) (void)hipStreamDestroy(rs);
                rs = nullptr;
                for (int k = 0; k < AUX; k++) {
                    if (sm[k]) (void)hipStreamDestroy(sm[k]);
                    sm[k] = nullptr;
                }
            } else {
                for (uint32_t wd : side) reserved += __builtin_popcount(wd);
                device_cus = real_cus;
            }
        }
#endif
        for (int k = 0; k < AUX; k++) {
            HIP_CHECK(hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking));
            HIP_CHECK(hipEventCreate(&e0[k]));
            HIP_CHECK(hipEventCreate(&e1[k]));
        }
        HIP_CHECK(hipStreamCreateWithFlags(&du, hipStreamNonBlocking));
    } catch (...) {
        if (du) (void)hipStreamDestroy(du);
        if (ep) (void)hipEventDestroy(ep);
        if (rs) (void)hipStreamDestroy(rs);
        for (int k = 0; k < AUX; k++)
            if (sm[k]) (void)hipStreamDestroy(sm[k]);
        for (int k = 0; k < AUX; k++) {
            if (st[k]) (void)hipStreamDestroy(st[k]);
            if (e0[k]) (void)hipEventDestroy(e0[k]);
            if (e1[k]) (void)hipEventDestroy(e1[k]);
        }
        throw;
    }
    ev_prep = ep;
    duo = du;
    rest = rs;
    for (int k = 0; k < AUX; k++) aux_m[k] = sm[k];
    reserved_cus = reserved;
    real_cus = device_cus;
    for (int k = 0; k < AUX; k++) {
        aux[k] = st[k];
        ev_d0[k] = e0[k];
        ev_d1[k] = e1[k];
    }
    aux_ready = true;
}

u8 * DeviceCtx::temp_get(size_t cap) {
    std::lock_guard<std::mutex> lk(temp_mu);
    for (size_t k = 0; k < temps_free.size(); k++)
        if (temps_free[k].second >= cap) {
            auto t = temps_free[k];
            temps_free.erase(temps_free.begin() + (long)k);
            temps_out.push_back(t);
            return t.first;
        }
    u8 * p = nullptr;
    if (hipMalloc((void **)&p, cap) != hipSuccess) {
        // (the ring's budget is an estimate: before the block fails, give back what the pool holds idle -- buffers of other sizes -- and ask again)
        (void)hipGetLastError();
        // A buffer goes back to the pool by STREAM ORDER (encode_front_b): kernels already queued on the group's stream may still read it.
        // Every borrower launches on that one stream, which is what protects a re-borrowed buffer; a FREE is not a stream operation, so wait.
        (void)hipDeviceSynchronize();
        for (auto & t : temps_free) (void)hipFree(t.first);
        temps_free.clear();
        HIP_CHECK(hipMalloc((void **)&p, cap));
    }
    temps_out.push_back({p, cap});
    return p;
}

void DeviceCtx::temp_put(u8 * p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(temp_mu);
    for (size_t k = 0; k < temps_out.size(); k++)
        if (temps_out[k].first == p) {
            temps_free.push_back(temps_out[k]);
            temps_out.erase(temps_out.begin() + (long)k);
            return;
        }
}

void DeviceCtx::temp_trim() {  // hand the idle swap buffers back to the driver
    std::lock_guard<std::mutex> lk(temp_mu);
    if (temps_free.empty()) return;
    (void)hipDeviceSynchronize();  // (see temp_get: a pooled buffer may still be read by kernels in flight; hipFree's own synchronisation is not documented)
    for (auto & t : temps_free) (void)hipFree(t.first);
    temps_free.clear();
}

size_t DeviceCtx::temp_idle_bytes() {
    std::lock_guard<std::mutex> lk(temp_mu);
    size_t b = 0;
    for (auto & t : temps_free) b += t.second;
    return b;
}

Arena DeviceCtx::arena_for(size_t bytes) {  // caller holds mu
    if (bytes > ws_cap) {
        if (ws) HIP_CHECK(hipFree(ws));
        ws = nullptr;
        ws_cap = 0;
        size_t want = bytes + arena_slack(bytes);
        HIP_CHECK(hipMalloc((void **)&ws, want));
        ws_cap = want;
    }
    Arena a;
    a.base = ws;
    a.cap = ws_cap;
    a.used = 0;
    return a;
}

int device_count() {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_device_count < 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        g_device_count = n;
        g_ctx.assign((size_t)(n > 0 ? n : 0), nullptr);
    }
    return g_device_count;
}

DeviceCtx * get_ctx(int dev) {
    const int n = device_count();
    if (dev < 0 || dev >= n) return nullptr;
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_ctx[dev]) {
        HIP_CHECK(hipSetDevice(dev));
        DeviceCtx * c = new DeviceCtx;
        c->device = dev;
        CrcTables t;
        memset(&t, 0, sizeof t);
        crc_build_tables(t);
        HIP_CHECK(hipMalloc((void **)&c->d_crc, sizeof(CrcTables)));
        HIP_CHECK(hipMemcpy(c->d_crc, &t, sizeof t, hipMemcpyHostToDevice));
#ifndef BZ3_EMU
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) c->cus = cus;
#endif
        if (const char * e = getenv("BZ3_HIP_CUS"))  // tests / experiments: pretend the GPU has this many CUs (batch-size policies)
            if (atoi(e) > 0) c->cus = atoi(e);
        g_ctx[dev] = c;
    }
    return g_ctx[dev];
}

int pick_device() {
    const int n = device_count();
    if (n <= 0) return -1;
    int b = g_bound_device.load();
    if (b == -2) {
        const char * e = getenv("BZ3_HIP_DEVICE");
        b = (e && *e) ? atoi(e) : -1;
        if (b >= n) b = -1;
        g_bound_device.store(b);
    }
    if (b >= 0) return b;
    return (int)(g_rr.fetch_add(1) % (unsigned)n);
}

// Second half of the headroom rule (see ws_headroom): called with the context's mutex held when a group's call ends.
void enforce_headroom(DeviceCtx * ctx, hipStream_t s) {
    const size_t h = ws_headroom();
    size_t free_b = 0, total_b = 0;
    if (!h || hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b >= h) return;
    if (ctx->temp_idle_bytes() > 0) {
        ctx->temp_trim();
        g_headroom_trims.fetch_add(1);
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b >= h) return;
    }
    if (ctx->ws) {
        (void)hipStreamSynchronize(s);
        (void)hipDeviceSynchronize();  // side streams included
        (void)hipFree(ctx->ws);
        ctx->ws = nullptr;
        ctx->ws_cap = 0;
        g_headroom_releases.fetch_add(1);
    }
}

void state_release(bz3_state * st) {
    if (!st) return;
    (void)hipSetDevice(st->device);
    if (st->stream) (void)hipStreamSynchronize(st->stream);
    if (st->ev0) (void)hipEventDestroy(st->ev0);
    if (st->ev1) (void)hipEventDestroy(st->ev1);
    if (st->d_swap && st->lean && st->ctx) st->ctx->temp_put(st->d_swap);
    else if (st->d_swap) (void)hipFree(st->d_swap);
    if (st->d_io) (void)hipFree(st->d_io);
    if (st->d_words) (void)hipFree(st->d_words);
    if (st->stream) (void)hipStreamDestroy(st->stream);
    delete st;
}

// A new state on device `dev` (bz3_new: the device pick_device chose; the device frame API: the device that owns the caller's buffers).
bz3_state * new_state_on(int32_t block_size, int dev) {
    if (block_size < KiB65 || block_size > MiB511) return nullptr;
    bz3_state * st = nullptr;
    try {
        DeviceCtx * ctx = get_ctx(dev);
        if (!ctx) return nullptr;
        st = new bz3_state;
        st->block_size = block_size;
        st->device = dev;
        st->ctx = ctx;
        HIP_CHECK(hipSetDevice(dev));
        HIP_CHECK(hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking));
        st->xs = st->stream;
        HIP_CHECK(hipEventCreate(&st->ev0));
        HIP_CHECK(hipEventCreate(&st->ev1));
        st->cap = (bz3_bound((size_t)block_size) + 4096 + 255) & ~(size_t)255;
        st->lean = lean_states();
        if (!st->lean) HIP_CHECK(hipMalloc((void **)&st->d_swap, st->cap));
        HIP_CHECK(hipMalloc((void **)&st->d_words, 64 * sizeof(u32)));
        st->last_error = BZ3_OK;
        return st;
    } catch (const HipError & e) {
        fprintf(stderr, "bzip3_amd: bz3_new failed: %s (%s:%d)\n", e.what, e.file, e.line);
        state_release(st);
        return nullptr;
    } catch (const std::bad_alloc &) {
        state_release(st);
        return nullptr;
    }
}

}  // namespace api
}  // namespace bz3

extern "C" {

// ---- bz3_hip.h: settings and debug counters ------------------------------------------------------------
BZIP3_API unsigned bz3_hip_cm_blocks_routed_full(void) { return g_cm_routed_full.load(); }
BZIP3_API void bz3_hip_set_workspace_headroom(long long bytes) { g_ws_headroom.store(bytes < 0 ? -1 : bytes); }
BZIP3_API size_t bz3_hip_workspace_headroom(void) { return ws_headroom(); }
BZIP3_API unsigned bz3_hip_debug_headroom_events(int reset, unsigned * releases) {
    const unsigned t = reset ? g_headroom_trims.exchange(0) : g_headroom_trims.load();
    const unsigned r = reset ? g_headroom_releases.exchange(0) : g_headroom_releases.load();
    if (releases) *releases = r;
    return t;
}
BZIP3_API size_t bz3_hip_debug_ring_contexts(size_t free_b, size_t have, size_t need, size_t fixed, size_t ctx_bytes, size_t cap, int lean, size_t headroom) {
    return ring_contexts_for(free_b, have, need, fixed, ctx_bytes, cap, lean != 0, headroom);
}
BZIP3_API size_t bz3_hip_debug_workspace_bytes(size_t block_bytes, int which) {  // 0: per-block scratch of the stages, 1: one LZP context of the encoder's ring
    return which == 0 ? workspace_bytes_for((u64)block_bytes + 64) : lzp_encode_ctx_bytes((u64)block_bytes + 64) + 65536;
}
BZIP3_API unsigned bz3_hip_debug_cm_launches(int reset) { return reset ? g_cm_launches.exchange(0) : g_cm_launches.load(); }
BZIP3_API size_t bz3_hip_debug_arena_slack(size_t bytes) { return DeviceCtx::arena_slack(bytes); }
BZIP3_API size_t bz3_hip_debug_cached_bytes(int device) {  // workspace + idle pooled swap buffers the library holds on `device` right now
    DeviceCtx * c = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (device >= 0 && (size_t)device < g_ctx.size()) c = g_ctx[(size_t)device];
    }
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->ws_cap + c->temp_idle_bytes();
}
BZIP3_API int bz3_hip_set_front_end_duo(int on) {
    g_front_duo.store(on < 0 ? -1 : (on ? 1 : 0));
    return 0;
}
BZIP3_API int bz3_hip_set_keep_workspace(int on) {
    g_keep_ws.store(on < 0 ? -1 : (on ? 1 : 0));
    return 0;
}
BZIP3_API void bz3_hip_set_collect_window_us(int us) { g_collect_window_us.store(us < 0 ? 200 : us); }
BZIP3_API unsigned bz3_hip_debug_collected_batches(int reset, unsigned * largest) {  // batches run for single-block callers; *largest = blocks in the largest
    if (largest) *largest = g_collect_largest.load();
    const unsigned b = g_collect_batches.load();
    if (reset) {
        g_collect_batches.store(0);
        g_collect_largest.store(0);
    }
    return b;
}

// ---- bz3_hip.h: device control, timings ----------------------------------------------------------------
BZIP3_API int bz3_hip_device_count(void) { return device_count(); }

BZIP3_API int bz3_hip_bind_device(int device) {
    if (device < -1 || device >= device_count()) return -1;
    g_bound_device.store(device);
    return 0;
}

BZIP3_API int bz3_hip_state_device(struct bz3_state * st) { return st->device; }

BZIP3_API int bz3_hip_set_cm_mode(int mode) {
    bool ok = mode >= -1 && mode <= CM_VARIANT_ROWS3;
#ifdef BZ3_EMU
    ok = ok || mode == CM_VARIANT_ROWS_TEST;
#endif
    if (!ok) return -1;
    g_cm_mode.store(mode);
    return 0;
}

BZIP3_API unsigned bz3_hip_cm_blocks_given_up(void) { return g_cm_given_up.load(); }

BZIP3_API void bz3_hip_debug_bwt_big_rounds(int k) { bwt_set_big_rounds(k); }
BZIP3_API void bz3_hip_debug_set_unbwt_log_stride(int log_stride) { unbwt_set_log_stride(log_stride); }

BZIP3_API int bz3_hip_cm_variant_for(int device, int blocks, int encode) {
    DeviceCtx * c = get_ctx(device);
    return (c && blocks > 0) ? cm_variant_for(c, (size_t)blocks, encode != 0) : -1;
}

BZIP3_API int bz3_hip_debug_front_end_ring(void) { return g_front_end_ring.load(); }
BZIP3_API int bz3_hip_debug_arena_swap_buffers(int reset) { return reset ? g_arena_swaps.exchange(0) : g_arena_swaps.load(); }

BZIP3_API int bz3_hip_debug_peak_concurrent_groups(int reset) {
    const int v = g_groups_peak.load();
    if (reset) g_groups_peak.store(0);
    return v;
}

BZIP3_API int bz3_hip_set_lean_states(int on) {
    g_lean.store(on ? 1 : 0);
    return 0;
}

BZIP3_API void bz3_hip_release_cached_memory(void) {
    const int n = device_count();
    for (int d = 0; d < n; d++) {
        DeviceCtx * c = nullptr;
        {
            std::lock_guard<std::mutex> lk(g_mu);
            c = g_ctx[(size_t)d];
        }
        if (!c) continue;
        (void)hipSetDevice(d);
        std::lock_guard<std::mutex> lk(c->mu);
        c->temp_trim();
        if (c->ws) (void)hipFree(c->ws);
        c->ws = nullptr;
        c->ws_cap = 0;
    }
}

BZIP3_API void bz3_hip_last_timings(struct bz3_state * st, float ms[BZ3_HIP_T_COUNT]) {
    for (int i = 0; i < BZ3_HIP_T_COUNT; i++) ms[i] = st->t[i];
}

BZIP3_API void bz3_hip_last_bwt_stats(struct bz3_state * st, int32_t * rounds, int32_t * radix_passes, uint64_t * sorted_elements) {
    if (rounds) *rounds = st->bwt.rounds;
    if (radix_passes) *radix_passes = st->bwt.radix_passes;
    if (sorted_elements) *sorted_elements = st->bwt.sorted_elements;
}

}  // extern "C"
