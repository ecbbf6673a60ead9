// api_decode.hip -- the decoder of a device group: header checks, the CM launches, and the tail (inverse BWT, LZP decoders, mRLE, CRC) in
// windows over a ring of side streams.
#include "api_internal.hpp"

using namespace bz3;
using namespace bz3::api;

namespace {

__global__ void __launch_bounds__(128) k_unstore_small(u8 * __restrict__ b, u32 n) {  // memmove(buffer, buffer + 8, n), :684
    const u32 t = threadIdx.x;
    const u8 v = t < n ? b[8 + t] : (u8)0;
    __syncthreads();
    if (t < n) b[t] = v;
}

// ======================================================================================================
// decode.  Phases per GPU: validate headers -> ONE CM launch (one CU per block) -> per block inverse BWT
// (whole GPU) -> ONE LZP-decode launch (one workgroup per block) -> per block mRLE decode + CRC check.
// ======================================================================================================
// hdr: host copy of the first min(17, buffer_size) bytes of the block.
void decode_front(bz3_state * st, u8 * buf, size_t buffer_size, s32 compressed_size, s32 orig_size, const u8 * hdr) {
    st->pending = bz3_state::FAILED;
    st->result = -1;
    if (st->skip) return;  // last_error as on_failure left it
    if (buffer_size < 9 || buffer_size < (size_t)compressed_size) {  // :658-661 (s32 -> size_t as in the reference)
        st->last_error = BZ3_ERR_DATA_SIZE_TOO_SMALL;
        return;
    }
    const u32 crc = rd_le32(hdr);
    const s32 bwt_idx = (s32)rd_le32(hdr + 4);
    const size_t bound = bz3_bound((size_t)st->block_size);
    if (compressed_size < 0 || (size_t)compressed_size > bound) {  // :667-670
        st->last_error = BZ3_ERR_MALFORMED_HEADER;
        return;
    }
    hipStream_t s = st->xs;
    for (float & x : st->t) x = 0.f;
    st->user = buf;
    st->buffer_size = buffer_size;
    st->crc = crc;
    if (bwt_idx == -1) {  // stored block, :672-692
        if (compressed_size - 8 > 64 || compressed_size < 8) {
            st->last_error = BZ3_ERR_MALFORMED_HEADER;
            return;
        }
        if ((size_t)(compressed_size - 8) > buffer_size) {
            st->last_error = BZ3_ERR_DATA_SIZE_TOO_SMALL;
            return;
        }
        st->size = compressed_size - 8;
        launch(k_unstore_small, dim3(1), dim3(128), 0, s, buf, (u32)st->size);
        crc32c_device(buf, (u64)st->size, 1u, st->ctx->d_crc, st->d_words, s);
        st->pending = bz3_state::DEC_STORED;
        return;
    }
    const s32 model = (s8)hdr[8];
    const size_t need = 9 + (size_t)((model & 2) * 4) + (size_t)((model & 4) * 4);  // :697 (9 / 17 / 25 / 33)
    if (buffer_size < need) {
        st->last_error = BZ3_ERR_DATA_SIZE_TOO_SMALL;
        return;
    }
    s32 lzp_size = -1, rle_size = -1, p = 0;
    if (model & 2) lzp_size = (s32)rd_le32(hdr + 9 + 4 * p++);
    if (model & 4) rle_size = (s32)rd_le32(hdr + 9 + 4 * p++);
    p += 2;
    compressed_size -= p * 4 + 1;
    if (((model & 2) && (lzp_size < 0 || (size_t)lzp_size > bound)) || ((model & 4) && (rle_size < 0 || (size_t)rle_size > bound))) {  // :710-714
        st->last_error = BZ3_ERR_MALFORMED_HEADER;
        return;
    }
    if (orig_size < 0 || (size_t)orig_size > bound) {  // :716-719
        st->last_error = BZ3_ERR_MALFORMED_HEADER;
        return;
    }
    const s32 size_before_bwt = (model & 2) ? lzp_size : (model & 4) ? rle_size : orig_size;  // :724-729
    if (!sizes_fit(buffer_size, lzp_size, rle_size, orig_size)) {  // :734-737
        st->last_error = BZ3_ERR_DATA_SIZE_TOO_SMALL;
        return;
    }
    st->bwt_idx = bwt_idx;
    st->model = model;
    st->lzp_size = lzp_size;
    st->rle_size = rle_size;
    st->orig_size = orig_size;
    st->size_before_bwt = size_before_bwt;
    st->cm_in = buf + p * 4 + 1;  // :742-747
    st->cm_in_size = (u32)(compressed_size < 0 ? 0 : compressed_size);
    st->pending = bz3_state::DEC_CODED;
}

// After the CM kernel: the index checks in front of the inverse BWT, and the choice of buffers.  Leaves the data-to-be in st->b1 and the free buffer
// in st->b2, as the inverse BWT will have left them.  Returns -1 when the block failed, 0 when it needed no transform (n <= 1), 1 when `item`
// is to go through bwt_inverse_batch.
// The inverse BWTs themselves run in decode_group, collected per window and in runs of up to UB_MAX_BATCH blocks per launch sequence
// (unbwt_batch_size), and the host waits for the stream once per RUN.  bwt_inverse_batch waits for nothing, and nothing depends on that wait
// for correctness -- every later user of the arena launches on st->xs -- it is there for speed: with no wait at all the host runs a whole window
// ahead, some 900 launches deep, and the tail of 768 x 8 MiB blocks measured 0.87 s against 0.75 s with a wait after every block (0.73 s after
// every third, 0.74 s after every tenth: profiles/unbwt_tail_after.txt; with runs: profiles/unbwt_batch.txt).
int decode_unbwt_check(bz3_state * st, float cm_ms, UbBatchItem & item) {
    hipStream_t s = st->xs;
    st->t[BZ3_HIP_T_CM] = cm_ms;
    const s32 n = st->size_before_bwt;
    if (st->bwt_idx > n) {  // :750-753
        st->last_error = BZ3_ERR_MALFORMED_HEADER;
        return -1;
    }
    u8 *b1 = st->d_swap, *b2 = st->user;  // after the swap of :748
    if (st->lean) {  // lean state: the coder wrote into the caller's buffer; the borrowed swap buffer receives the text
        b1 = st->user;
        b2 = st->d_swap;
    }
    const double t0 = now_ms();
    // libsais_unbwt's own argument checks (include/libsais.h:5210-5232)
    int queued = 0;
    if (n <= 1) {
        if (st->bwt_idx != n) { st->last_error = BZ3_ERR_BWT; return -1; }
        if (n == 1) HIP_CHECK(hipMemcpyAsync(b2, b1, 1, hipMemcpyDeviceToDevice, s));
    } else {
        if (st->bwt_idx <= 0) { st->last_error = BZ3_ERR_BWT; return -1; }
        item = UbBatchItem{b1, b2, (u32)n, (u32)st->bwt_idx};  // :758
        queued = 1;
    }
    st->b1 = b2;
    st->b2 = b1;
    st->size_src = n;
    st->t[BZ3_HIP_T_BWT] = (float)(now_ms() - t0);  // (a queued block: its run's wall time / the run's blocks, set by decode_group)
    return queued;
}

// After the LZP kernel (if any): mRLE decode, size checks, copy back, CRC.
void decode_finish(bz3_state * st, Arena & arena) {
    hipStream_t s = st->xs;
    const size_t bound = bz3_bound((size_t)st->block_size);
    (void)bound;
    u8 *b1 = st->b1, *b2 = st->b2;
    s32 size_src = st->size_src;
    if (st->model & 2) {  // :767-781 (the kernel already ran; its result is in d_words[5])
        size_src = (s32)read_word(s, st->d_words + 5);
        if (size_src == -1) { st->last_error = BZ3_ERR_CRC; return; }
        if ((size_t)size_src > st->buffer_size) { st->last_error = BZ3_ERR_DATA_SIZE_TOO_SMALL; return; }
        u8 * tmp = b1; b1 = b2; b2 = tmp;
    }
    if (st->model & 4) {  // :783-792
        const double t0 = now_ms();
        bool bad = size_src < 32;  // mrled: `if (maxin < 32) return 1`
        if (!bad) {
            mrle_decode(b1, (u32)size_src, b2, (u32)st->orig_size, st->d_words + 4, arena, s);
            bad = read_word(s, st->d_words + 4) != (u32)st->orig_size;
        }
        st->t[BZ3_HIP_T_RLE] = (float)(now_ms() - t0);
        if (bad) { st->last_error = BZ3_ERR_CRC; return; }
        size_src = st->orig_size;
        u8 * tmp = b1; b1 = b2; b2 = tmp;
    }
    st->last_error = BZ3_OK;  // :794
    if (size_src > st->block_size || size_src < 0) {  // :796-799
        st->last_error = BZ3_ERR_MALFORMED_HEADER;
        return;
    }
    if (b1 != st->user) {  // :801
        const double t0 = now_ms();
        HIP_CHECK(hipMemcpyAsync(st->user, b1, (size_t)size_src, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
        st->t[BZ3_HIP_T_COPY] += (float)(now_ms() - t0);
    }
    const double t0 = now_ms();
    crc32c_device(st->user, (u64)size_src, 1u, st->ctx->d_crc, st->d_words, s);  // :803
    const u32 got = read_word(s, st->d_words + 1);
    st->t[BZ3_HIP_T_CRC] = (float)(now_ms() - t0);
    if (got != st->crc) {
        st->last_error = BZ3_ERR_CRC;
        return;
    }
    st->result = size_src;
}

}  // namespace

namespace bz3 {
namespace api {

// hdrs: n x 17 bytes (host copies of the block headers).
void decode_group(bz3_state ** sts, u8 ** bufs, const size_t * buffer_sizes, const s32 * sizes, const s32 * orig_sizes, const u8 * hdrs, s32 n) {
    if (n <= 0) return;
    bz3_state * lead = sts[0];
    DeviceGuard g(lead->device);
    std::lock_guard<std::mutex> lk(lead->ctx->mu);
    hipStream_t s = lead->stream;
    for (s32 i = 0; i < n; i++) sts[i]->xs = s;  // see encode_group
    size_t need = 0;
    bool any_lean = false;
    for (s32 i = 0; i < n; i++) {
        const size_t w = workspace_bytes_for(bz3_bound((size_t)sts[i]->block_size) + 64);
        if (w > need) need = w;
        any_lean = any_lean || sts[i]->lean;
    }
    // ---- phase 1: headers ----------------------------------------------------------------------------------
    std::vector<s32> coded;
    for (s32 i = 0; i < n; i++) {
        decode_front(sts[i], bufs[i], buffer_sizes[i], sizes[i], orig_sizes[i], hdrs + 17 * (size_t)i);
        if (sts[i]->pending == bz3_state::DEC_CODED) coded.push_back(i);
    }
    // A lean state's CM output goes straight into the caller's buffer, which also holds the coded payload: that
    // payload (a fraction of the block) is staged in the workspace first.  Rounds: as many blocks per CM launch as
    // the staging budget holds (normally all of them).
    auto stage_bytes = [&](s32 i) { return sts[i]->lean ? (((size_t)sts[i]->cm_in_size + 64 + 255) & ~(size_t)255) : (size_t)0; };
    size_t stage_budget = (size_t)48 << 30;
    {
        size_t free_b = 0, total_b = 0;
        if (any_lean && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const size_t have = lead->ctx->ws_cap;
            const size_t aside = need + ws_headroom() + ((size_t)577 << 20);  // (+ the arena's slack: see ring_contexts_for)
            const size_t room = free_b + have > aside ? free_b + have - aside : 0;
            stage_budget = room - room / 4;  // leave a quarter for the swap buffers of the tail windows
        }
    }
    std::vector<size_t> round_end;  // indices into `coded`
    size_t max_round = 0;
    for (size_t k = 0; k < coded.size();) {
        size_t bytes = 0, e = k;
        while (e < coded.size() && (e == k || bytes + stage_bytes(coded[e]) <= stage_budget)) bytes += stage_bytes(coded[e++]);
        round_end.push_back(e);
        if (bytes > max_round) max_round = bytes;
        k = e;
    }
    // tail windows, software-pipelined like the encoder's front end: the serial LZP decoders of a window (one workgroup per
    // block, ~1 s for a 256 MiB text block beside other blocks' kernels) run on a side stream while this thread drives the inverse
    // BWTs of the next windows and the mRLE / CRC stages of the previous ones on the group's stream.  Lean states hold a borrowed
    // swap buffer while their window is in flight: 64 buffers at most either way -- two slots of 32 blocks for small batches, four
    // slots of 16 for large ones (a window's decoders then hide behind three other windows' whole-GPU work: 1 s / 48 blocks
    // instead of 1 s / 32, which starts to matter once the inverse BWT of a block takes less than ~30 ms).  Round 3 tried eight slots
    // of 8 on a 128-block batch (profiles/r03_gaps_128x256MiB.txt): no gain there, where the pool's first allocations set the pace.
    s32 tail_slots = n >= 128 ? 4 : 2;
    s32 tail_window = tail_slots == 4 ? 16 : 32;
    // Round 6: 64 reserved CUs and wider windows, where the swap buffers can be had.  What the ring can hide is the whole-GPU work of the blocks whose decoders are in flight,
    // and the tail's whole-GPU kernels do not miss the CUs (they are bound by HBM line fetches).  At 768 x 256 MiB, one step each ("inverse BWTs + LZP launches" + "waiting for a
    // window's decoders" + "mRLE / CRC"; BZ3_HIP_CU_RESERVE above 64 still reserves 64: cu_masks hands out at most 8 CUs per block of 32):
    //   16 x 4 on 48 CUs: 12.7 + 3.9 + 3.0 = 19.6 s    20 x 4 on 64: 13.0 + 2.3 + 3.0 = 18.3 s    25 x 4: 12.4 + 1.5 + 3.0 = 16.9 s    30 x 4: 12.7 + 0.9 + 3.0 = 16.6 s    32 x 4: 13.2 + 0.7 + 3.0 = 16.9 s
    // (profiles/r06_call4_full_*.progress.txt, r06_call6_stdout_tail.txt, r06_tail_ring_full_size.txt): with windows of 30 up to 90 decoders share the 64 CUs, and a CU with two
    // of them still beats a window that waits.  The buffers come out of the kept arena (below) or, without keep-workspace, out of the pool -- only when the device has the room
    // beside the headroom (lean states; classic states own their swap buffers).
    if (tail_slots == 4) {
        size_t cap_max = 0;
        for (s32 i = 0; i < n; i++)
            if (sts[i]->lean && sts[i]->cap > cap_max) cap_max = sts[i]->cap;
        const size_t cap_al = (cap_max + 255) & ~(size_t)255;
        size_t free_b = 0, total_b = 0;
        const bool have_info = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
        for (s32 w : {30, 25, 20}) {
            if (n < 4 * w || lead->ctx->reserved_cus_wanted() < 64) continue;
            const size_t bufs = (size_t)4 * (size_t)w;
            const bool from_arena = keep_workspace() && any_lean && lead->ctx->ws_cap >= need + need / 16 + bufs * cap_al + ((size_t)64 << 20);
            if (!any_lean || from_arena || (have_info && free_b >= bufs * cap_max + ws_headroom() + ((size_t)2 << 30) + max_round)) {
                tail_window = w;
                break;
            }
        }
    }
    lead->ctx->ensure_aux();
    // With the CU partition the whole-GPU kernels run at their stand-alone pace and the LZP decoders become what the ring has to hide: ~1.0 s per launch
    // at 256 MiB beside the streaming kernels (0.55 s alone: their 1 MiB tables do not stay in L2), whatever the window.  Measured at full size on 48
    // reserved CUs (profiles/r05_call{6,7,8}_*): 16 x 4 waits 3.7 s of a 21.9 s tail for them, 12 x 4 7.1 s of 22.8, 8 x 8 (eight masked streams) 7.0 s of
    // 29.5 with every other phase slower too.  Four slots of 16 stay.
    if (const char * e = getenv("BZ3_HIP_TAIL_PIPE")) {  // "window,slots": tests / experiments
        int w = 0, q = 0;
        if (sscanf(e, "%d,%d", &w, &q) == 2 && w >= 1 && q >= 2 && q <= DeviceCtx::AUX) {
            tail_window = w;
            tail_slots = q;
        }
    }
    if (tail_window > n) tail_window = n;
    size_t lzp_in_window = 0;
    for (s32 w0 = 0; w0 < n; w0 += tail_window) {
        size_t c = 0;
        for (s32 i = w0; i < n && i < w0 + tail_window; i++)
            if (sts[i]->pending == bz3_state::DEC_CODED && (sts[i]->model & 2)) c++;
        if (c > lzp_in_window) lzp_in_window = c;
    }
    Arena arena = lead->ctx->arena_for(need + (size_t)tail_slots * lzp_in_window * (LZP_LUT_WORDS * 4 + sizeof(LzpDecodeJob) + 256) + (size_t)n * 256 + cm_scratch_bytes(coded.size()) + max_round + 65536);
    // ---- phase 2: the CM launches (one workgroup per block) ------------------------------------------------------
    float cm_ms = 0.f;
    for (size_t r = 0, k0 = 0; r < round_end.size(); k0 = round_end[r++]) {
        const size_t mk = arena.mark();
        std::vector<CmDecodeJob> cm_jobs;
        std::vector<char> to_full;  // a payload that hardly shrank has (nearly) every byte value live: no row cache holds that
        for (size_t k = k0; k < round_end[r]; k++) {
            bz3_state * st = sts[coded[k]];
            to_full.push_back((u64)st->cm_in_size * 10u >= (u64)(u32)st->size_before_bwt * 9u ? 1 : 0);
            const u8 * in = st->cm_in;
            if (st->lean) {
                u8 * stage = arena.take<u8>(stage_bytes(coded[k]));
                if (st->cm_in_size) HIP_CHECK(hipMemcpyAsync(stage, st->cm_in, st->cm_in_size, hipMemcpyDeviceToDevice, s));
                in = stage;
            }
            cm_jobs.push_back(CmDecodeJob{dev_addr(in), dev_addr(st->lean ? st->user : st->d_swap), st->cm_in_size, (u32)st->size_before_bwt, 0u, 0u});
        }
        CmDecodeJob * d_jobs = arena.take<CmDecodeJob>(cm_jobs.size());
        cm_ms += run_cm_jobs(lead->ctx, arena, cm_jobs, d_jobs, s, lead->ev0, lead->ev1,
                             [](const CmDecodeJob * j, u32 nj, hipStream_t st, int variant) { cm_decode_batch(j, nj, st, variant); }, &to_full);
        arena.release(mk);
    }
    // ---- phases 3-5 per tail window: inverse BWT per block, ONE LZP-decode launch (one workgroup per block), mRLE + CRC ----
    struct TailWindow {
        s32 w0 = 0, w1 = 0;
        std::vector<LzpDecodeJob> lz_jobs;  // host copies: alive until the window is finished
        std::vector<s32> lz_owner;
        std::vector<char> alive;
        LzpDecodeJob * d_lz = nullptr;
        u32 * luts = nullptr;
    } tw[DeviceCtx::AUX];
    for (int k = 0; k < tail_slots; k++) {
        tw[k].d_lz = lzp_in_window ? arena.take<LzpDecodeJob>(lzp_in_window) : nullptr;
        tw[k].luts = lzp_in_window ? arena.take<u32>(lzp_in_window * LZP_LUT_WORDS) : nullptr;
    }
    // keep-workspace mode: the swap buffers the lean states of the windows in flight borrow come out of the arena -- the staging area of the CM
    // rounds is free again by now -- as long as the per-block scratch of the stages (`need`) still fits behind them; the pool serves the rest
    std::vector<u8 *> arena_swaps;
    size_t swap_cap = 0;
    if (keep_workspace() && any_lean) {
        for (s32 i = 0; i < n; i++)
            if (sts[i]->lean && sts[i]->cap > swap_cap) swap_cap = sts[i]->cap;
        const size_t want = (size_t)tail_slots * (size_t)tail_window;
        const size_t step = (swap_cap + 255) & ~(size_t)255;
        const size_t keep_free = need + need / 32 + 65536;  // the per-block scratch of the stages and half of the slack arena_for adds
        while (swap_cap && arena_swaps.size() < want && arena.cap - arena.used >= keep_free + step) arena_swaps.push_back(arena.take<u8>(swap_cap));
    }
    std::vector<char> from_arena((size_t)n, 0);
    auto borrow = [&](s32 i) {
        bz3_state * st = sts[i];
        if (st->lean && !st->d_swap && !arena_swaps.empty() && st->cap <= swap_cap) {
            st->d_swap = arena_swaps.back();
            arena_swaps.pop_back();
            from_arena[(size_t)i] = 1;
            g_arena_swaps.fetch_add(1);
        } else {
            lean_borrow(st);
        }
    };
    auto give_back = [&](s32 i) {
        bz3_state * st = sts[i];
        if (from_arena[(size_t)i]) {
            if (st->d_swap) arena_swaps.push_back(st->d_swap);  // (a failure path may have dropped it already: lean_return of a buffer the pool does not know is a no-op)
            st->d_swap = nullptr;
            from_arena[(size_t)i] = 0;
        } else {
            lean_return(st);
        }
    };
    lead->ctx->ensure_aux();
    DrainOnUnwind drain{s, lead->ctx->aux, DeviceCtx::AUX};
    // The tail's whole-GPU kernels keep off the CUs the side streams' LZP decoders sit on (DeviceCtx::rest), when the device is partitioned
    hipStream_t s_cm = s;
    hipStream_t * side_streams = lead->ctx->aux;
    // Only in the regime it was measured in (profiles/r05_call{6,7,8}_*: 256-768 blocks): a small batch has at most 32 short LZP decoders, and its inverse
    // BWT, mRLE and CRC kernels would give up 19 % of the device and gain a synchronisation for them.  BZ3_HIP_CU_PARTITION_MIN_BLOCKS (read once; tests: 2).
    static const s32 part_min = [] { const char * e = getenv("BZ3_HIP_CU_PARTITION_MIN_BLOCKS"); return e && atoi(e) > 0 ? (s32)atoi(e) : (s32)128; }();
    if (lead->ctx->rest && n >= part_min && tail_slots <= DeviceCtx::RING_SLOTS) {
        side_streams = lead->ctx->aux_m;
        HIP_CHECK(hipStreamSynchronize(s));  // headers, stored blocks' CRCs and the CM launches ran on the group's stream
        s = lead->ctx->rest;
        for (s32 i = 0; i < n; i++) sts[i]->xs = s;
    }
    // the walk of the inverse BWT is sized to the lanes its stream's CUs keep resident: on the masked stream, the CUs that are not reserved
    const u32 unbwt_lanes = s != s_cm && lead->ctx->real_cus > lead->ctx->reserved_cus ? (u32)(lead->ctx->real_cus - lead->ctx->reserved_cus) * UNBWT_LANES_PER_CU : 0u;
    DrainOnUnwind drain_rest{s == s_cm ? nullptr : s, side_streams == lead->ctx->aux ? nullptr : side_streams, side_streams == lead->ctx->aux ? 0 : DeviceCtx::AUX};
    std::vector<UbBatchItem> ub_items;
    std::vector<u32> ub_sizes;
    std::vector<s32> ub_owner;
    const s32 nwin = (n + tail_window - 1) / tail_window;
    const s32 lag = tail_slots - 1;  // window k is finished in iteration k + lag
    // BZ3_HIP_TRACE_RINGS=1 (diagnosis, read once): where this thread's wall time goes in the ring -- a line on stderr when the call ends
    static const bool trace_rings = getenv("BZ3_HIP_TRACE_RINGS") != nullptr;
    double tr_unbwt = 0, tr_wait = 0, tr_finish = 0, tr_t0 = now_ms();
    for (s32 k = 0; k < nwin + lag; k++) {
        const double tr_a = now_ms();
        if (k < nwin) {  // window k: inverse BWTs on the group's stream, then its LZP decoders on the slot's side stream
            const int q = (int)(k % tail_slots);
            hipStream_t s2 = side_streams[q];
            TailWindow & w = tw[q];
            w.w0 = k * tail_window;
            w.w1 = (w.w0 + tail_window < n) ? w.w0 + tail_window : n;
            w.lz_jobs.clear();
            w.lz_owner.clear();
            w.alive.assign((size_t)(w.w1 - w.w0), 0);
            // the window's blocks first through their checks: the ones that fail keep their error and drop out, the rest are collected ...
            ub_items.clear();
            ub_sizes.clear();
            ub_owner.clear();
            for (s32 i = w.w0; i < w.w1; i++) {
                bz3_state * st = sts[i];
                if (st->pending == bz3_state::DEC_STORED) {  // :686-691
                    HIP_CHECK(hipStreamSynchronize(st->xs));
                    if (read_word(st->xs, st->d_words + 1) != st->crc) st->last_error = BZ3_ERR_CRC;
                    else st->result = st->size;  // last_error untouched (:691)
                    continue;
                }
                if (st->pending != bz3_state::DEC_CODED) continue;
                borrow(i);
                UbBatchItem item{};
                const int r = decode_unbwt_check(st, cm_ms, item);
                if (r < 0) continue;
                w.alive[(size_t)(i - w.w0)] = 1;
                if (r > 0) {
                    ub_items.push_back(item);
                    ub_sizes.push_back(item.n);
                    ub_owner.push_back(i);
                }
            }
            // ... and go through the inverse BWT in runs: one launch sequence and one wait per run (decode_unbwt_check: why there is a wait)
            for (size_t at = 0; at < ub_items.size();) {
                const u32 b = unbwt_batch_size(ub_sizes.data() + at, (u32)(ub_items.size() - at), arena.cap - arena.used, unbwt_lanes);
                const double t0 = now_ms();
                // every block's stride is picked for ALL of the stream's lanes, as for a block alone: a stride picked for lanes / b measured slower
                // (tail 0.650 against 0.633 s at 768 x 8 MiB: profiles/unbwt_batch.txt)
                bwt_inverse_batch(ub_items.data() + at, b, arena, s, unbwt_lanes);
                HIP_CHECK(hipStreamSynchronize(s));
                const float each = (float)(now_ms() - t0) / (float)b;
                for (u32 j = 0; j < b; j++) sts[ub_owner[at + j]]->t[BZ3_HIP_T_BWT] = each;
                at += b;
            }
            for (s32 i = w.w0; i < w.w1; i++) {
                bz3_state * st = sts[i];
                if (!w.alive[(size_t)(i - w.w0)]) continue;
                if (st->model & 2) {
                    if (st->lzp_size < 4) {  // lzp_decompress: `if (n < 4) return -1` (:252) -> BZ3_ERR_CRC (:769-771)
                        st->last_error = BZ3_ERR_CRC;
                        w.alive[(size_t)(i - w.w0)] = 0;
                        continue;
                    }
                    // The reference decodes into its swap buffer (bz3_bound(block_size) bytes) and compares with buffer_size
                    // afterwards (:767-781).  A lean state decodes into the caller's buffer, so the cap is the smaller of the two;
                    // decode_finish tells the two failures apart.
                    const size_t bound = bz3_bound((size_t)st->block_size);
                    const size_t room = st->lean && st->buffer_size < bound ? st->buffer_size : bound;
                    w.lz_jobs.push_back(LzpDecodeJob{dev_addr(st->b1), dev_addr(st->b2), dev_addr(w.luts + w.lz_jobs.size() * LZP_LUT_WORDS), dev_addr(st->d_words + 5),
                                                     (u32)st->lzp_size, (u32)room});
                    w.lz_owner.push_back(i);
                }
            }
            if (!w.lz_jobs.empty()) {
                HIP_CHECK(hipEventRecord(lead->ctx->ev_prep, s));  // the inverse BWTs above are in flight on the group's stream
                HIP_CHECK(hipStreamWaitEvent(s2, lead->ctx->ev_prep, 0));
                HIP_CHECK(hipEventRecord(lead->ctx->ev_d0[q], s2));
                lzp_decode_batch(w.lz_jobs.data(), w.d_lz, (u32)w.lz_jobs.size(), s2);
                HIP_CHECK(hipEventRecord(lead->ctx->ev_d1[q], s2));
            }
        }
        const double tr_b = now_ms();
        tr_unbwt += tr_b - tr_a;
        if (k >= lag) {  // finish window k-lag: its LZP decoders have had the inverse BWTs of `lag` other windows to hide behind
            const int q = (int)((k - lag) % tail_slots);
            TailWindow & w = tw[q];
            if (!w.lz_jobs.empty()) {
                HIP_CHECK(hipEventSynchronize(lead->ctx->ev_d1[q]));
                tr_wait += now_ms() - tr_b;
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, lead->ctx->ev_d0[q], lead->ctx->ev_d1[q]);
                for (s32 i : w.lz_owner) sts[i]->t[BZ3_HIP_T_LZP] = ms;
                // lean state whose buffer is smaller than the reference's swap buffer: the decoder stops at the cap (:211) and
                // returns it, where the reference would have gone on to bz3_bound(block_size) and then either reported a larger
                // size (-> BZ3_ERR_DATA_SIZE_TOO_SMALL, :776) or run into malformed input (-> BZ3_ERR_CRC): when the cap was
                // reached, decode once more into a borrowed buffer of the reference's size and keep that verdict
                for (size_t j = 0; j < w.lz_jobs.size(); j++) {
                    bz3_state * st = sts[w.lz_owner[j]];
                    const size_t bound = bz3_bound((size_t)st->block_size);
                    if (!st->lean || st->buffer_size >= bound || read_word(s, st->d_words + 5) != w.lz_jobs[j].max_out) continue;
                    u8 * big = st->ctx->temp_get(st->cap);
                    LzpDecodeJob again = w.lz_jobs[j];
                    again.out = dev_addr(big);
                    again.max_out = (u32)bound;
                    again.lut = dev_addr(w.luts);
                    lzp_decode_batch(&again, w.d_lz, 1u, s);
                    HIP_CHECK(hipStreamSynchronize(s));
                    st->ctx->temp_put(big);
                }
            }
            for (s32 i = w.w0; i < w.w1; i++) {
                if (w.alive[(size_t)(i - w.w0)]) decode_finish(sts[i], arena);
                give_back(i);
            }
        }
        tr_finish += now_ms() - tr_b;
    }
    if (trace_rings)
        fprintf(stderr, "[bz3 rings] decode tail: %d blocks, %d windows of %d x %d slots: %.1f ms = inverse BWTs + LZP launches %.1f + waiting for a window's LZP decoders %.1f + mRLE / CRC / hand-back %.1f\n",
                (int)n, (int)nwin, (int)tail_window, (int)tail_slots, now_ms() - tr_t0, tr_unbwt, tr_wait, tr_finish - tr_wait);
    for (s32 i = 0; i < n; i++) sts[i]->pending = bz3_state::NONE;
    if (s != s_cm) (void)hipStreamSynchronize(s);  // (the tail ran on the masked stream; decode_finish has waited for every block already)
    enforce_headroom(lead->ctx, s_cm);
}

}  // namespace api
}  // namespace bz3
