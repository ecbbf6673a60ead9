// api_internal.hpp -- what the translation units of the API layer share (api_context.hip, api_encode.hip, api_decode.hip, api.hip,
// api_frames.hip, api_hooks.hip): the per-device context, struct bz3_state, the small helpers, the settings readers, the scratch-size rules
// and the CM routing policy, in namespace bz3::api.  The library is built with -fvisibility=hidden, so none of it is exported.
//
// Every mutable global of the layer is DEFINED in api_context.hip and only declared here: no initialisation order between the units exists.
// No kernel lives here: the orchestration's small kernels sit in the unit that launches them.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <new>
#include <stdexcept>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/bz3_hip.h"
#include "prims.hpp"
#include "sort.hpp"
#include "stages.hpp"

namespace bz3 {
namespace api {

constexpr s32 KiB65 = 65 * 1024;
constexpr s32 MiB511 = 511 * 1024 * 1024;

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline u32 rd_le32(const u8 * p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }
inline void wr_le32(u8 * p, u32 v) {
    p[0] = (u8)v; p[1] = (u8)(v >> 8); p[2] = (u8)(v >> 16); p[3] = (u8)(v >> 24);
}

// ---- per-device context -----------------------------------------------------------------------
struct DeviceCtx {
    int device = 0;
    std::mutex mu;          // serialises users of the shared workspace
    CrcTables * d_crc = nullptr;
    char * ws = nullptr;
    size_t ws_cap = 0;
    int cus = 256;          // compute units: one full-model CM workgroup fits per CU
    // side streams of the device: the serial LZP drivers of a window of blocks run there while the calling thread drives the
    // whole-GPU stages of the neighbouring windows on the group's stream (encode_group and decode_group: one side stream per slot
    // of their rings, so that the serial kernels of consecutive windows overlap)
    static constexpr int AUX = 8;           // side streams / ring slots available; the rings use four unless a test or an experiment asks for more
    static constexpr int RING_SLOTS = 4;
    hipStream_t aux[AUX] = {};
    hipStream_t duo = nullptr;  // round 6: phase A of the encoder's front end when it runs on a thread of its own (encode_group)
    hipEvent_t ev_prep = nullptr, ev_d0[AUX] = {}, ev_d1[AUX] = {};
    bool aux_ready = false;
    // CU partition (round 5).  The serial kernels on the side streams hold a CU each for the better part of a second (an LZP decoder: 1024 lanes, ~0.5 s per
    // 256 MiB block), and a whole-GPU kernel that finds half of such a CU's wave slots taken runs its workgroups there at a fraction of the pace -- the
    // inverse BWT's walk kernels, whose launch lasts as long as their slowest workgroup, measured 2.5x their stand-alone time beside the decoders of three
    // windows (profiles/r05_rings_256x64MiB.txt: the tail's host thread spent 82 % of its time in the inverse-BWT loop, 0.6 % waiting for LZP decoders).
    // So the side streams are created on `reserve` CUs of their own and the tail's whole-GPU kernels run on a stream masked to the OTHER CUs
    // (hipExtStreamCreateWithCUMask); the CM launches keep the group's unmasked stream (they need every CU).  BZ3_HIP_CU_RESERVE=<CUs> (read once;
    // default 64 since round 6 -- the most cu_masks hands out --, round 5: 48; 0 = no partition).  Falls back to plain streams when the runtime refuses.
    hipStream_t rest = nullptr;   // whole-GPU kernels beside the side streams' serial kernels: every CU but the reserved ones (null: no partition)
    hipStream_t aux_m[AUX] = {};  // the decoder's side streams, on the reserved CUs (the encoder's rings keep the plain ones: call 4 measured its
                                         // front end 6 % SLOWER with its LZP drivers confined to 32 CUs, profiles/r05_cu_partition_256x64MiB.txt)
    int reserved_cus = 0;
    int real_cus = 0;             // the device's own CU count where the partition exists (0: none)
    static int reserved_cus_wanted() { return cu_reserve_setting(); }
    static int cu_reserve_setting() {
        static const int v = [] {
            const char * e = getenv("BZ3_HIP_CU_RESERVE");
            return e ? atoi(e) : 64;  // the most cu_masks hands out (8 per block of 32 CUs); round 5: 48 = three windows of 16 LZP decoders, a CU each
        }();
        return v;
    }
    // Mask bit i of the reserved set: 32 a + 8 j + ((a + 2 j + t / 4) mod 8), j = t mod 4, for a < 8 and t < reserve / 8 (at most 8) -- the same number
    // of CUs from every block of 32 bits AND from every residue class mod 8, so that each XCD gives up equally many whether the driver deals the mask
    // bits to the XCDs in blocks or round robin.
    static void cu_masks(int cus, int reserve, std::vector<uint32_t> & side, std::vector<uint32_t> & main);
    void ensure_aux();  // caller holds mu

    // Swap buffers lent to "lean" states for the duration of a stage sequence (see bz3_hip_set_lean_states).
    std::mutex temp_mu;
    std::vector<std::pair<u8 *, size_t>> temps_free;
    std::vector<std::pair<u8 *, size_t>> temps_out;
    u8 * temp_get(size_t cap);
    void temp_put(u8 * p);
    void temp_trim();  // hand the idle swap buffers back to the driver
    size_t temp_idle_bytes();

    // What arena_for allocates beyond the request (alignment losses of the takes, a somewhat larger next call): a sixteenth, but never more than
    // 512 MiB -- round 5's unbounded sixteenth was 5 GB of an 80 GB ring that nobody used and the host program could not have.
    static size_t arena_slack(size_t bytes) {
        const size_t s16 = bytes >> 4, cap = (size_t)512 << 20;
        return (s16 < cap ? s16 : cap) + ((size_t)1 << 20);
    }
    Arena arena_for(size_t bytes);  // caller holds mu
};

// ---- the layer's mutable globals, all defined in api_context.hip (see there for what each one counts) -----------------------------
extern std::atomic<int> g_lean, g_cm_mode, g_keep_ws, g_front_duo;  // settings: bz3_hip_set_lean_states / _cm_mode / _keep_workspace / _front_end_duo
extern std::atomic<long long> g_ws_headroom;                         // bz3_hip_set_workspace_headroom
extern std::atomic<int> g_front_end_ring, g_arena_swaps, g_groups_running, g_groups_peak;
extern std::atomic<unsigned> g_cm_given_up, g_crc_launches, g_cm_launches, g_cm_routed_full;

// The two halves of the encoder's front end have scratch needs of their own (round 6: they may run on two host threads and two streams, see encode_group):
// phase A = CRC, mRLE, LZP preparation (hash sort, binned links); phase B = LZP emission and the suffix sort.
inline size_t front_a_scratch_bytes(u64 n) { return (size_t)n * 30 + radix_temp_bytes(n, 9) + scan_temp_words(n / 8 + 4096) * 4 + (4u << 20); }
inline size_t front_b_scratch_bytes(u64 n) { return bwt_workspace_bytes(n) + (size_t)(n / 1024 + 4096) * 4; }
inline size_t workspace_bytes_for(u64 n) {
    size_t a = bwt_workspace_bytes(n), b = unbwt_workspace_bytes(n);
    size_t c = (size_t)n * 30 + radix_temp_bytes(n, 9) + scan_temp_words(n / 8 + 4096) * 4 + (4u << 20);  // LZP: links, mlen, bitmaps, the hash sort's buffers + the binned link records (lzp.hip)
    size_t m = a > b ? a : b;
    return m > c ? m : c;
}

// ---- CM kernel variant -------------------------------------------------------------------------------
// The full-model CM kernels need a whole CU's LDS per block; the row-cache kernels (cm.hip) need half or a third of it, so two or
// three blocks share a CU, but they give up blocks whose order-1 working set does not fit (binary data), which are then coded again
// by the full-model kernel.  Policy (BZ3_HIP_CM_MODE=auto|full|rows|rows3, bz3_hip_set_cm_mode): `auto` picks by batch size.
inline int cm_mode() {
    int m = g_cm_mode.load();
    if (m == -2) {
        const char * e = getenv("BZ3_HIP_CM_MODE");
        m = -1;
        if (e && !strcmp(e, "full")) m = CM_VARIANT_FULL;
        else if (e && !strcmp(e, "rows")) m = CM_VARIANT_ROWS;
        else if (e && !strcmp(e, "rows3")) m = CM_VARIANT_ROWS3;
#ifdef BZ3_EMU
        else if (e && !strcmp(e, "rows-test")) m = CM_VARIANT_ROWS_TEST;
#endif
        g_cm_mode.store(m);
    }
    return m;
}

inline bool lean_states() {
    int v = g_lean.load();
    if (v < 0) {
        const char * e = getenv("BZ3_HIP_LEAN");
        v = (e && *e && strcmp(e, "0")) ? 1 : 0;
        g_lean.store(v);
    }
    return v != 0;
}

inline int cm_variant_for(const DeviceCtx * ctx, size_t njobs, bool encode) {
    (void)encode;
    const int m = cm_mode();
    const size_t c = (size_t)ctx->cus;
    if (m >= 0) return m;
    // auto, by batch size.  Up to one block per CU the whole model sits in LDS; beyond that the CM launch would need a second round of
    // workgroups, and the row-cache kernels put two / three blocks on a CU instead: ns per byte and block of a 2 MiB text block on
    // MI355X, decoder 551 / ~650 / 737 with one / two / three blocks per CU (profiles/r03_cm_decoder_steps.txt), the encoder's
    // model waves interleave even better (x1.5 / x2.0 throughput, profiles/r01_cm_rows_probe.txt).
    if (njobs > 2 * c) return CM_VARIANT_ROWS3;
    if (njobs > c) return CM_VARIANT_ROWS;
    return CM_VARIANT_FULL;
}

inline size_t cm_scratch_bytes(size_t njobs) { return njobs * (CM_SPILL_BYTES + 256) + 4096 + CM_CLAIM_WORDS * 4 + 256; }

// Runs the CM kernel over `jobs` (host copies; d_jobs has room for all of them) and returns the kernel time in ms.
// Row-cache variants: blocks the kernel gave up are coded again by the full-model kernel in a second launch.
// to_full (optional, one flag per job): blocks known not to fit the row cache -- many live byte values (encode: from the BWT's histogram), or a
// payload that hardly shrank (decode) -- skip the row-cache kernels and go straight into the whole-model launch (round 5; g_cm_given_up counts only
// blocks the row-cache kernels really handed back).
template <class Job, class Launch>
float run_cm_jobs(const DeviceCtx * ctx, Arena & arena, std::vector<Job> & jobs, Job * d_jobs, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, Launch && go,
                  const std::vector<char> * to_full = nullptr) {
    if (jobs.empty()) return 0.f;
    std::vector<Job> direct;  // straight to the whole-model kernel
    // Routing only pays when the WHOLE batch would take a row-cache variant: a batch that fits one block per CU is whole-model work anyway, and splitting it
    // would run two serial launches, each as long as its slowest block, where one does.
    if (to_full && cm_mode() < 0 && cm_variant_has_rows(cm_variant_for(ctx, jobs.size(), std::is_same<Job, CmEncodeJob>::value))) {
        std::vector<Job> keep;
        for (size_t i = 0; i < jobs.size(); i++) ((*to_full)[i] ? direct : keep).push_back(jobs[i]);
        if (!direct.empty()) {
            g_cm_routed_full.fetch_add((unsigned)direct.size());
            jobs.swap(keep);
        }
    }
    if (jobs.empty()) {  // everything is whole-model work: one launch
        float ms0 = 0.f;
        HIP_CHECK(hipMemcpyAsync(d_jobs, direct.data(), sizeof(Job) * direct.size(), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipEventRecord(ev0, s));
        g_cm_launches.fetch_add(1);
        go(d_jobs, (u32)direct.size(), s, (int)CM_VARIANT_FULL);
        HIP_CHECK(hipEventRecord(ev1, s));
        HIP_CHECK(hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&ms0, ev0, ev1);
        jobs.swap(direct);
        return ms0;
    }
    const int variant = cm_variant_for(ctx, jobs.size(), std::is_same<Job, CmEncodeJob>::value);
    const size_t mk = arena.mark();
    if constexpr (std::is_same<Job, CmEncodeJob>::value) {  // a word per CU for the coder waves' SIMD claims (cm.hip)
        static const bool no_claim = getenv("BZ3_CM_NO_CLAIM") != nullptr;  // (experiments, read once: the block index decides, as up to round 4)
        if (!no_claim) {
            u32 * claim = arena.take<u32>(CM_CLAIM_WORDS);
            HIP_CHECK(hipMemsetAsync(claim, 0, CM_CLAIM_WORDS * sizeof(u32), s));
            for (auto & j : jobs) j.claim = dev_addr(claim);
            for (auto & j : direct) j.claim = dev_addr(claim);
        }
    }
    u32 * d_status = nullptr;
    if (cm_variant_has_rows(variant)) {
        u8 * spill = arena.take<u8>(jobs.size() * CM_SPILL_BYTES);
        d_status = arena.take<u32>(jobs.size());
        HIP_CHECK(hipMemsetAsync(d_status, 0, jobs.size() * 4, s));
        for (size_t i = 0; i < jobs.size(); i++) {
            jobs[i].spill = dev_addr(spill + i * CM_SPILL_BYTES);
            jobs[i].status = dev_addr(d_status + i);
            jobs[i].miss_base = cm_variant_is_test(variant) ? 64u : CM_MISS_BASE;
            jobs[i].miss_shift = cm_variant_is_test(variant) ? 3u : CM_MISS_SHIFT;  // give up beyond 3 % misses (test variants: 12.5 %)
        }
    }
    float ms = 0.f, ms2 = 0.f;
    HIP_CHECK(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(Job) * jobs.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(ev0, s));
    g_cm_launches.fetch_add(1);
    go(d_jobs, (u32)jobs.size(), s, variant);
    HIP_CHECK(hipEventRecord(ev1, s));
    HIP_CHECK(hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&ms, ev0, ev1);
    if (cm_variant_has_rows(variant)) {
        std::vector<u32> status(jobs.size());
        HIP_CHECK(hipMemcpyAsync(status.data(), d_status, jobs.size() * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        std::vector<Job> again;
        for (size_t i = 0; i < jobs.size(); i++)
            if (status[i]) again.push_back(jobs[i]);
        g_cm_given_up.fetch_add((unsigned)again.size());
        again.insert(again.end(), direct.begin(), direct.end());
        direct.clear();
        if (!again.empty()) {
            HIP_CHECK(hipMemcpyAsync(d_jobs, again.data(), sizeof(Job) * again.size(), hipMemcpyHostToDevice, s));
            HIP_CHECK(hipEventRecord(ev0, s));
            g_cm_launches.fetch_add(1);
            go(d_jobs, (u32)again.size(), s, (int)CM_VARIANT_FULL);  // whole model in LDS: nothing to give up
            HIP_CHECK(hipEventRecord(ev1, s));
            HIP_CHECK(hipStreamSynchronize(s));
            (void)hipEventElapsedTime(&ms2, ev0, ev1);
        }
    }
    if (!direct.empty()) {  // (the variant had no row cache: nothing was handed back, the routed blocks still wait)
        HIP_CHECK(hipMemcpyAsync(d_jobs, direct.data(), sizeof(Job) * direct.size(), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipEventRecord(ev0, s));
        g_cm_launches.fetch_add(1);
        go(d_jobs, (u32)direct.size(), s, (int)CM_VARIANT_FULL);
        HIP_CHECK(hipEventRecord(ev1, s));
        HIP_CHECK(hipStreamSynchronize(s));
        float ms3 = 0.f;
        (void)hipEventElapsedTime(&ms3, ev0, ev1);
        ms2 += ms3;
    }
    arena.release(mk);
    return ms + ms2;
}

}  // namespace api
}  // namespace bz3

// ---- the state ------------------------------------------------------------------------------------
struct bz3_state {
    s32 block_size = 0;
    s8 last_error = BZ3_OK;
    int device = 0;
    bz3::api::DeviceCtx * ctx = nullptr;
    hipStream_t stream = nullptr;  // owned
    hipStream_t xs = nullptr;      // execution stream of the current call: the lead state's stream of its device group
    u8 * d_swap = nullptr;  // the reference's swap_buffer, in HBM (lean states: borrowed from the device's pool while a call needs it)
    bool lean = false;      // see bz3_hip_set_lean_states
    bool timed = true;      // this block's stages are timed with host clocks (a stream synchronisation per stage): the first block of a group only
    u8 * d_io = nullptr;    // staging for the host-buffer API (lazy)
    size_t cap = 0;         // bz3_bound(block_size) rounded up
    u32 * d_words = nullptr;  // [0..1] crc scratch/result, [2] cm coded size, [4] rle total, [5] lzp result
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float t[BZ3_HIP_T_COUNT] = {0};
    bz3::BwtStats bwt;

    // block in flight inside one API call
    enum Pending { NONE, ENC_STORED, ENC_CODED, DEC_STORED, DEC_CODED, FAILED } pending = NONE;
    u8 * user = nullptr;  // caller's device buffer
    u8 * b1 = nullptr, * b2 = nullptr;
    s32 size = 0, overhead = 0, result = -1;
    u32 n_cm = 0;         // bytes entering / leaving the CM stage
    const u8 * cm_in = nullptr;
    u32 cm_in_size = 0;
    u8 * side = nullptr;  // lean encode: this block's slice of the in-place coder's side buffer
    bool hold_swap = false;  // lean encode, two-thread front end: encode_front_b leaves the swap buffer with the state; the window's thread returns it behind an event
    bool skip = false;    // host-buffer API: staging this block failed (on_failure has set the error); the group leaves it alone
    // decode
    size_t buffer_size = 0;
    u32 crc = 0;
    s32 bwt_idx = 0, model = 0, lzp_size = -1, rle_size = -1, orig_size = 0, size_before_bwt = 0, size_src = 0;
};

namespace bz3 {
namespace api {

struct DeviceGuard {
    explicit DeviceGuard(int d) { HIP_CHECK(hipSetDevice(d)); }
};

// A group call that is left by an exception must not leave kernels in flight on either stream of the device: the caller is about to
// hand borrowed swap buffers back to the pool and to reuse the arena (the serial LZP kernels run on the side streams).
struct DrainOnUnwind {
    hipStream_t main;
    hipStream_t * side;  // n_side side streams
    int n_side;
    int live = std::uncaught_exceptions();
    ~DrainOnUnwind() {
        if (std::uncaught_exceptions() > live) {
            if (main) (void)hipStreamSynchronize(main);
            for (int k = 0; k < n_side; k++)
                if (side[k]) (void)hipStreamSynchronize(side[k]);
        }
    }
};

inline u32 read_word(hipStream_t s, const u32 * d) {
    u32 v = 0;
    HIP_CHECK(hipMemcpyAsync(&v, d, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return v;
}

inline bool sizes_fit(size_t buffer_size, s32 lzp_size, s32 rle_size, s32 orig_size) {  // bz3_check_buffer_size, :114-122
    const size_t a = lzp_size < 0 ? 0 : (size_t)lzp_size, b = rle_size < 0 ? 0 : (size_t)rle_size, c = orig_size < 0 ? 0 : (size_t)orig_size;
    return a <= buffer_size && b <= buffer_size && c <= buffer_size;
}

// ---- headroom: the device memory the library leaves to the host program -------------------------------------------------------------------------
// The library keeps memory between calls (the workspace arena, idle pooled swap buffers; with keep-workspace a GPU-filling batch's whole ring).  The caller
// owns its memory, so there is a rule about how much the library may sit on: when a batch call returns, at least `headroom` bytes of the
// device are free (hipMemGetInfo), or the library holds nothing cached at all.  Two halves: (1) the rings are SIZED for it -- the encoder's ring of LZP
// contexts takes the free memory minus headroom minus what the arena adds on top (ring_contexts_for); (2) it is ENFORCED when a group returns
// (enforce_headroom): idle pooled swap buffers go back to the driver first, the workspace second.  bz3_hip_set_workspace_headroom / environment
// BZ3_HIP_WS_HEADROOM_MB; default 4 GiB.  Round 5 had a fixed 6 GiB margin that the arena's own slack consumed: bench.py's next 48 MiB allocation failed.
inline size_t ws_headroom() {
    static const long long env = [] {
        const char * e = getenv("BZ3_HIP_WS_HEADROOM_MB");
        return e && *e ? (long long)strtoull(e, nullptr, 10) << 20 : (long long)4 << 30;
    }();
    const long long v = g_ws_headroom.load();
    return (size_t)(v < 0 ? env : v);
}
// LZP contexts the encoder's ring may hold.  free_b: free device memory now; have: the arena the context already owns (reused); need: per-block scratch of the
// stages; fixed: the batch's job arrays, side buffers and CM scratch in the arena; ctx_bytes: one LZP context; cap: one borrowed swap buffer (lean states: a block
// in the ring holds exactly one context and one swap buffer; others own their swap buffers, and 7/10 of what is free is the estimate of rounds 1-4).
inline size_t ring_contexts_for(size_t free_b, size_t have, size_t need, size_t fixed, size_t ctx_bytes, size_t cap, bool lean, size_t headroom) {
    const size_t total = free_b + have;
    const size_t base = need + fixed;
    if (total <= base || !ctx_bytes) return 0;
    size_t by_share = (total - base) / 10 * 7 / ctx_bytes;
    // what is left once the headroom, the arena's slack and the takes' alignment are set aside
    const size_t aside = headroom + ((size_t)513 << 20) + ((size_t)64 << 20);
    const size_t room = total > base + aside ? total - base - aside : 0;
    if (!lean) {
        const size_t by_room = room / ctx_bytes;
        return by_share < by_room ? by_share : by_room;
    }
    return room / (ctx_bytes + cap);
}
// Second half of the rule: called with the context's mutex held when a group's call ends (api_context.hip).
void enforce_headroom(DeviceCtx * ctx, hipStream_t s);

// Lean states own no swap buffer: they borrow one from the device's pool while a stage sequence needs it.
// BZ3_HIP_KEEP_WS=1 (experiment, round 5's first measurement): a lean batch's workspace survives the call -- the decode call that follows reuses the
// encode call's arena and carves the swap buffers of its tail windows from it -- instead of one hipFree and two multi-GB hipMallocs per round trip
// (30-45 ms per GiB: profiles/r04_first_touch.txt).  Read once.
#ifndef BZ3_FRONT_DUO_DEFAULT
#define BZ3_FRONT_DUO_DEFAULT 0
#endif
inline bool keep_workspace() {
    static const bool env_on = [] {
        const char * e = getenv("BZ3_HIP_KEEP_WS");
        return e && atoi(e) != 0;
    }();
    const int v = g_keep_ws.load();
    return v < 0 ? env_on : v != 0;
}
inline bool front_end_duo() {
    static const int env_on = [] {
        const char * e = getenv("BZ3_HIP_FRONT_DUO");
        return e ? (atoi(e) != 0 ? 1 : 0) : BZ3_FRONT_DUO_DEFAULT;
    }();
    const int v = g_front_duo.load();
    return v < 0 ? env_on != 0 : v != 0;
}
inline void lean_borrow(bz3_state * st) {
    if (st->lean && !st->d_swap) st->d_swap = st->ctx->temp_get(st->cap);
}
inline void lean_return(bz3_state * st) {
    if (st->lean && st->d_swap) {
        st->ctx->temp_put(st->d_swap);
        st->d_swap = nullptr;
    }
}
constexpr u32 CM_SIDE_BYTES = 64 * 1024;  // per block: where in-place CM output goes should it ever catch up with its input

// ---- single-block calls from several host threads are collected into batches (api.hip collect) ---------------------------------------
struct SingleReq {
    bz3_state * st;
    u8 * buffer;
    size_t buffer_size;
    s32 size, orig_size;
    bool done = false;
};
struct Collector {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<SingleReq *> pending[2];  // [0] encode, [1] decode
    bool leader[2] = {false, false};
    size_t last_size[2] = {0, 0};  // callers in the previous batch: the leader stops waiting as soon as that many have arrived
    int lonely[2] = {0, 0};        // batches of ONE caller in a row with nobody queued behind them
};
extern Collector g_collect;
extern std::atomic<int> g_collect_window_us;
extern std::atomic<unsigned> g_collect_batches, g_collect_largest;

// ---- what the units call of one another ---------------------------------------------------------------------------------------------
// api_context.hip
int device_count();
DeviceCtx * get_ctx(int dev);
int pick_device();
bz3_state * new_state_on(int32_t block_size, int dev);
void state_release(bz3_state * st);
// api_encode.hip / api_decode.hip: `n` blocks whose states live on ONE device; bufs are device pointers
void encode_group(bz3_state ** sts, u8 ** bufs, const s32 * sizes, s32 n);
void decode_group(bz3_state ** sts, u8 ** bufs, const size_t * buffer_sizes, const s32 * sizes, const s32 * orig_sizes, const u8 * hdrs, s32 n);
// api.hip: a batch split by device, one host thread per GPU; host = the buffers are host memory, staged through the states
void run_encode(bz3_state ** states, void ** buffers, s32 * sizes, s32 n, bool host);
void run_decode(bz3_state ** states, void ** buffers, const size_t * buffer_sizes, const s32 * sizes, const s32 * orig_sizes, const u8 * hdrs, s32 n, bool host);

}  // namespace api
}  // namespace bz3
