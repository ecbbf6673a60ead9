// api_encode.hip -- the encoder of a device group: the per-block front end (CRC, mRLE, LZP, BWT, header) in windows over a ring of LZP
// contexts, on one host thread or two, ONE CM launch for the group's blocks, and the per-block finish.
#include "api_internal.hpp"

using namespace bz3;
using namespace bz3::api;

namespace {

// ---- small kernels of the orchestration layer ---------------------------------------------------
__global__ void k_write_header(u8 * __restrict__ b, const u32 * __restrict__ crc, const u32 * __restrict__ idx_word, u32 model, u32 lzp_size, u32 rle_size) {
    if (threadIdx.x != 0) return;
    const u32 c = *crc, idx = *idx_word;  // (the primary index stays on the device: bwt_forward's d_idx)
    b[0] = (u8)c; b[1] = (u8)(c >> 8); b[2] = (u8)(c >> 16); b[3] = (u8)(c >> 24);
    b[4] = (u8)idx; b[5] = (u8)(idx >> 8); b[6] = (u8)(idx >> 16); b[7] = (u8)(idx >> 24);
    b[8] = (u8)model;
    u32 o = 9;
    if (model & 2u) { b[o] = (u8)lzp_size; b[o + 1] = (u8)(lzp_size >> 8); b[o + 2] = (u8)(lzp_size >> 16); b[o + 3] = (u8)(lzp_size >> 24); o += 4; }
    if (model & 4u) { b[o] = (u8)rle_size; b[o + 1] = (u8)(rle_size >> 8); b[o + 2] = (u8)(rle_size >> 16); b[o + 3] = (u8)(rle_size >> 24); }
}

// Blocks shorter than 64 bytes are stored: [crc][0xFFFFFFFF][bytes] (src/libbz3.c:596-601).
__global__ void __launch_bounds__(64) k_store_small(u8 * __restrict__ b, u32 n, const u32 * __restrict__ crc) {
    const u32 t = threadIdx.x;
    const u8 v = t < n ? b[t] : (u8)0;
    __syncthreads();
    if (t < n) b[8 + t] = v;
    if (t == 0) {
        const u32 c = *crc;
        b[0] = (u8)c; b[1] = (u8)(c >> 8); b[2] = (u8)(c >> 16); b[3] = (u8)(c >> 24);
        b[4] = b[5] = b[6] = b[7] = 0xFF;
    }
}

// ======================================================================================================
// encode.  A call (one block or a batch) runs in three phases per GPU:
//   1. per block, whole-GPU kernels, one block after the other: CRC, mRLE, LZP, BWT        (encode_front)
//   2. ONE launch of the CM kernel, one workgroup (= one CU) per block                      (cm_encode_batch)
//   3. per block: header, copy back into the caller's buffer if the ping-pong ended there   (encode_finish)
// ======================================================================================================
// Phase 1a: CRC, mRLE, LZP preparation (hash links + static events).  c receives the LZP context.
void encode_front_a(bz3_state * st, u8 * buf, s32 data_size, Arena & arena, Arena & ctx_arena, LzpEncodeCtx & c) {
    st->pending = bz3_state::FAILED;
    st->result = -1;
    c.active = false;
    if (st->skip) return;  // last_error as on_failure left it
    if (data_size > st->block_size || data_size < 0) {  // :588-591 (a negative size would walk off the buffer)
        st->last_error = BZ3_ERR_DATA_TOO_BIG;
        return;
    }
    hipStream_t s = st->xs;
    for (float & x : st->t) x = 0.f;
    double t0 = now_ms();
    crc32c_device(buf, (u64)data_size, 1u, st->ctx->d_crc, st->d_words, s);  // :593
    st->user = buf;
    st->size = data_size;
    if (data_size < 64) {  // :596-601 (last_error is left untouched on this path)
        launch(k_store_small, dim3(1), dim3(64), 0, s, buf, (u32)data_size, (const u32 *)(st->d_words + 1));
        st->pending = bz3_state::ENC_STORED;
        return;
    }
    if (st->timed) {
        HIP_CHECK(hipStreamSynchronize(s));
        st->t[BZ3_HIP_T_CRC] = (float)(now_ms() - t0);
    }

    u32 n = (u32)data_size;
    lean_borrow(st);
    u8 *b1 = buf, *b2 = st->d_swap;
    st->model = 0;
    st->rle_size = 0;
    t0 = now_ms();
    {  // :609-614
        MrleEncScratch sc;
        const size_t mk = arena.mark();
        mrle_encode_size(b1, n, sc, arena, s);
        st->rle_size = (s32)(32u + read_word(s, sc.total));
        if (st->rle_size < (s32)n) {
            mrle_encode_write(b1, n, sc, b2, s);
            if (st->timed) HIP_CHECK(hipStreamSynchronize(s));
            u8 * tmp = b1; b1 = b2; b2 = tmp;
            n = (u32)st->rle_size;
            st->model |= 4;
        }
        arena.release(mk);
    }
    st->t[BZ3_HIP_T_RLE] = (float)(now_ms() - t0);
    st->b1 = b1;
    st->b2 = b2;
    st->n_cm = n;
    t0 = now_ms();
    lzp_encode_prepare(b1, n, c, ctx_arena, arena, s);  // :616 (first third)
    st->t[BZ3_HIP_T_LZP] = (float)(now_ms() - t0);
    st->pending = bz3_state::ENC_CODED;
}

// Phase 1b (after the LZP drivers of the window have run) comes in two halves around the transform, so that the blocks of a window can go
// through the suffix sorter in runs (bwt_forward_batch).  First half: LZP emission and the choice of the transform's buffers.  Returns false
// for a block that is not in the pipeline (stored, failed, skipped); otherwise `item` describes its transform and `copy_to` is where the
// output has to be copied afterwards (lean state whose input sits in the caller's buffer; nullptr otherwise).
bool encode_front_b_collect(bz3_state * st, Arena & arena, const LzpEncodeCtx & c, float driver_ms, BwtBatchItem & item, u8 *& copy_to) {
    if (st->pending != bz3_state::ENC_CODED) return false;
    st->pending = bz3_state::FAILED;
    hipStream_t s = st->xs;
    u8 *b1 = st->b1, *b2 = st->b2;
    u32 n = st->n_cm;
    double t0 = now_ms();
    const s32 lzp_size = lzp_encode_finish(c, b2, arena, s);  // :616-621
    if (lzp_size > 0 && lzp_size < (s32)n) {
        u8 * tmp = b1; b1 = b2; b2 = tmp;
        n = (u32)lzp_size;
        st->model |= 2;
    }
    st->lzp_size = lzp_size;
    st->t[BZ3_HIP_T_LZP] += driver_ms + (float)(now_ms() - t0);

    u32 * const d_idx = st->d_words + 6;  // the primary index never visits the host
    u32 * const d_out8 = st->d_words + 8;  // bytes outside the block's 40 most frequent values: decides the CM kernel variant (run_cm_jobs)
    copy_to = nullptr;
    if (!st->lean) {
        item = BwtBatchItem{b1, n, b2, d_idx, d_out8, &st->bwt, 0};  // :623-627
    } else {
        // Lean state: the coder will work IN PLACE in the caller's buffer (capacity bz3_bound(size), libbz3.h:172-174):
        // the BWT output goes to the END of that buffer, the coded bytes grow from its start (cm.hip CmSink).
        u8 * tail = st->user + bz3_bound((size_t)st->size) - n;
        if (b1 != st->user) {
            item = BwtBatchItem{b1, n, tail, d_idx, d_out8, &st->bwt, 0};
        } else {
            item = BwtBatchItem{b1, n, b2, d_idx, d_out8, &st->bwt, 0};
            copy_to = tail;
        }
    }
    st->b1 = b1;
    st->b2 = b2;
    st->n_cm = n;
    return true;
}

// The transforms of the collected blocks, in runs of bwt_batch_size's choosing.  A timed block's BWT figure is its run's wall time divided by the
// run's blocks (as the inverse transform's figure on the decode side); timing a run means waiting for the stream.
void encode_front_b_transform(bz3_state * const * owners, BwtBatchItem * items, size_t count, Arena & arena, hipStream_t s) {
    std::vector<u32> sizes(count);
    for (size_t k = 0; k < count; k++) sizes[k] = items[k].n;
    for (size_t at = 0; at < count;) {
        const double t0 = now_ms();
        u32 b = 1;
        if (items[at].n < 2) {  // (never part of a batch)
            (void)bwt_forward(items[at].in, items[at].n, items[at].out, arena, s, items[at].stats, items[at].d_idx, items[at].d_outside);
        } else {
            u32 avail = 0;
            while (at + avail < count && avail < BWT_MAX_BATCH && items[at + avail].n >= 2) avail++;
            b = bwt_batch_size(sizes.data() + at, avail, arena.cap - arena.used);
            bwt_forward_batch(items + at, b, arena, s);
        }
        bool timed = false;
        for (u32 k = 0; k < b; k++) timed = timed || owners[at + k]->timed;
        if (timed) {
            HIP_CHECK(hipStreamSynchronize(s));
            const float each = (float)(now_ms() - t0) / (float)b;
            for (u32 k = 0; k < b; k++)
                if (owners[at + k]->timed) owners[at + k]->t[BZ3_HIP_T_BWT] = each;
        }
        at += b;
    }
}

// Second half, per block in block order: the copy a lean state may need, the header, the swap buffer's way back.
void encode_front_b_header(bz3_state * st, const BwtBatchItem & item, u8 * copy_to) {
    hipStream_t s = st->xs;
    u8 *b1 = st->b1, *b2 = st->b2;
    const u32 n = st->n_cm;
    if (st->lean) {
        if (copy_to) HIP_CHECK(hipMemcpyAsync(copy_to, b2, n, hipMemcpyDeviceToDevice, s));
        b2 = copy_to ? copy_to : item.out;  // CM input: the end of the caller's buffer
        b1 = st->user;                      // receives header + coded bytes
    }
    s32 overhead = 2;  // :630-632
    if (st->model & 2) overhead++;
    if (st->model & 4) overhead++;
    launch(k_write_header, dim3(1), dim3(64), 0, s, b1, (const u32 *)(st->d_words + 1), (const u32 *)item.d_idx, (u32)st->model, (u32)st->lzp_size, (u32)st->rle_size);  // :641-647
    // The swap buffer goes back to the pool.  Whoever borrows it next is a later block of this group -- the group holds the device's
    // mutex for the whole call and every kernel that touches the buffer, this block's and the next borrower's, is launched on the group's
    // ONE stream (the side streams only run LZP drivers, behind events recorded on it) --, so stream order is what protects it; rounds 1-3
    // waited for the stream here, once per block.
    if (st->lean && !st->hold_swap) lean_return(st);
    st->b1 = b1;
    st->b2 = b2;
    st->overhead = overhead;
    st->pending = bz3_state::ENC_CODED;
}

void encode_finish(bz3_state * st, float cm_ms) {
    const bz3_state::Pending p = st->pending;
    st->pending = bz3_state::NONE;
    if (p == bz3_state::FAILED || p == bz3_state::NONE) return;
    HIP_CHECK(hipStreamSynchronize(st->xs));
    if (p == bz3_state::ENC_STORED) {
        st->result = st->size + 8;
        return;
    }
    st->t[BZ3_HIP_T_CM] = cm_ms;
    const u32 coded = read_word(st->xs, st->d_words + 2);
    if (coded == 0xFFFFFFFFu) {  // in-place coding ran out of side buffer (the output outgrew bz3_bound's slack by > 64 KiB mid-block)
        st->last_error = BZ3_ERR_BWT;
        return;
    }
    const s32 total = (s32)coded + st->overhead * 4 + 1;
    if (st->lean) {
        const u32 sw = read_word(st->xs, st->d_words + 3);
        if (sw != 0xFFFFFFFFu && coded > sw)  // part of the coded bytes waited in the side buffer until the input was dead
            HIP_CHECK(hipMemcpyAsync(st->user + st->overhead * 4 + 1 + sw, st->side, coded - sw, hipMemcpyDeviceToDevice, st->xs));
        HIP_CHECK(hipStreamSynchronize(st->xs));
    }
    st->last_error = BZ3_OK;  // :649
    if (st->b1 != st->user) {  // :651
        double t0 = now_ms();
        HIP_CHECK(hipMemcpyAsync(st->user, st->b1, (size_t)total, hipMemcpyDeviceToDevice, st->xs));
        HIP_CHECK(hipStreamSynchronize(st->xs));
        st->t[BZ3_HIP_T_COPY] += (float)(now_ms() - t0);
    }
    st->result = total;
}

// Shape of the encoder's front-end pipeline: `contexts` LZP contexts fit into the memory budget, the batch has n blocks.
// ns context slots (2..DeviceCtx::RING_SLOTS; up to DeviceCtx::AUX when forced) of `window` blocks each.  A window's drivers hide behind the whole-GPU work of ns-1 other
// windows, so the drivers' share of the pace is T_driver / ((ns-1) * window) per block: more slots of fewer blocks get more out
// of the same memory (4 x 4 hides as much as 2 x 12).  Small batches keep the two-slot form (nothing to overlap with anyway).
// BZ3_HIP_LZP_PIPE="window,slots" overrides (tests / experiments).
void pipeline_shape(s32 contexts, s32 n, s32 & window, s32 & ns) {
    if (contexts < 2) contexts = 2;
    ns = 2;
    for (s32 cand = DeviceCtx::RING_SLOTS; cand > 2; cand--)
        if (contexts / cand >= 3 && n >= cand * 3) {
            ns = cand;
            break;
        }
    window = contexts / ns;
    if (window > 8) window = 8;
    if (const char * e = getenv("BZ3_HIP_LZP_PIPE")) {
        int w = 0, q = 0;
        if (sscanf(e, "%d,%d", &w, &q) == 2 && w >= 1 && q >= 2 && q <= DeviceCtx::AUX) {
            window = w;
            ns = q;
        }
    }
    if (window > n) window = n;
    if (window < 1) window = 1;
}

}  // namespace

namespace bz3 {
namespace api {

// Runs `n` blocks whose states live on ONE device.  bufs are device pointers.
void encode_group(bz3_state ** sts, u8 ** bufs, const s32 * sizes, s32 n) {
    if (n <= 0) return;
    bz3_state * lead = sts[0];
    DeviceGuard g(lead->device);
    std::lock_guard<std::mutex> lk(lead->ctx->mu);
    // One execution stream per call: the whole-GPU phases of the blocks run one after the other anyway, and stream
    // order is what protects the arena's scratch regions, which consecutive blocks reuse while earlier kernels are
    // still in flight.
    for (s32 i = 0; i < n; i++) {
        sts[i]->xs = lead->stream;
        sts[i]->timed = i == 0;  // stage timings (bz3_hip_last_timings) are sampled on the group's first block: timing a stage means waiting for the stream
    }
    size_t need = 0, need_a = 0, need_b = 0;
    for (s32 i = 0; i < n; i++) {
        const u64 nb = (u64)(sizes[i] > 0 ? sizes[i] : 0) + 64;
        const size_t w = workspace_bytes_for(nb), wa = front_a_scratch_bytes(nb), wb = front_b_scratch_bytes(nb);
        if (w > need) need = w;
        if (wa > need_a) need_a = wa;
        if (wb > need_b) need_b = wb;
    }
    // Two-thread front end (round 6, bz3_hip_set_front_end_duo / BZ3_HIP_FRONT_DUO; see below): phase A and phase B have a scratch region each
    const bool duo_wanted = front_end_duo() && n >= 16;
    if (duo_wanted) need = need_a + need_b + 65536;
    // LZP drivers are serial single-workgroup kernels (0.75 s for a 256 MiB text block alone, ~1.2 s beside the whole-GPU
    // kernels of other blocks, however many run side by side).  The blocks go through the front end in WINDOWS, software-pipelined
    // over a ring of `ns` context slots with one side stream each: while the drivers of windows k-ns+2 .. k run on their side
    // streams, this thread prepares window k+1 and finishes window k-ns+2 (LZP emission, BWT, header) on the group's stream, so a
    // window's drivers hide behind ns-1 windows' worth of whole-GPU work.  Round 2 ran two slots of 6 blocks at 768 x 256 MiB:
    // 128 windows x 1.23 s of drivers = 158 s against 146 s of whole-GPU work -- the driver chain, not the kernels, set the pace
    // of the front end (profiles/r02_kernel_stats_bench_768x256MiB.txt: k_lzp_driver 137 calls, 1.23 s each).
    u64 n_max = 64;
    for (s32 i = 0; i < n; i++)
        if (sizes[i] > 0 && (u64)sizes[i] > n_max) n_max = (u64)sizes[i];
    const size_t ctx_bytes = lzp_encode_ctx_bytes(n_max + 64) + 65536;
    // contexts = what fits into 7/10 of the memory that is free right now beside the sorter's workspace (the rest: the blocks' borrowed
    // swap buffers, allocator slack).  A workspace that grew far beyond the sorter's needs for this is handed back when the call
    // ends (below): the decode call that follows needs the room for staged payloads and the swap buffers of its tail windows.
    const size_t headroom = ws_headroom();
    const size_t fixed = (size_t)n * (sizeof(CmEncodeJob) + CM_SIDE_BYTES + 256) + cm_scratch_bytes((size_t)n) + 65536 + (size_t)DeviceCtx::AUX * 8 * (sizeof(LzpDriverJob) + 256);
    // The suffix sorter takes the blocks of a window in runs (bwt_forward_batch): the workspaces of a run's other blocks come on top of `need`,
    // only for block sizes at which bwt_batch_size grants a run at all, and only beside the ring: where memory is short enough for them to cost
    // an LZP context or the headroom, they are not taken, and bwt_batch_size finds room for one block at a time.
    // Two candidates: the run the rule grants with memory to spare, and the run of BWT_BATCH_SHORT (four) where the longer one does not fit.
    size_t bwt_extra = 0, bwt_extra_short = 0;
    if (n > 1) {
        u32 sz[BWT_MAX_BATCH];
        for (u32 & x : sz) x = (u32)n_max;
        const u32 b = bwt_batch_size(sz, (u32)(n < (s32)BWT_MAX_BATCH ? n : (s32)BWT_MAX_BATCH), ~(size_t)0);
        bwt_extra = (size_t)(b - 1) * bwt_workspace_bytes(n_max + 64);
        bwt_extra_short = (size_t)((b < BWT_BATCH_SHORT ? b : BWT_BATCH_SHORT) - 1) * bwt_workspace_bytes(n_max + 64);
    }
    size_t contexts = ((size_t)32 << 30) / ctx_bytes, contexts_beside_runs = contexts, contexts_beside_short_runs = contexts;
    {
        // Swap buffers the previous call left idle in the pool (a decode call's tail ring holds up to 4 x 16 of them, 17 GB at 256 MiB)
        // are memory this call's ring of LZP contexts cannot use: round 4's full-size run had a ring of 4 x 4 contexts and an encode
        // front end 14 s longer in its SECOND step than in its first for this.  What the front end borrows again is a few dozen buffers.
        // Round 5: only when that memory is MISSING -- an ordinary lean batch whose ring gets its full shape beside the pool keeps the
        // buffers it is about to borrow again (a free + malloc cycle per buffer and call otherwise, 30-45 ms per GiB).
        size_t free_b = 0, total_b = 0;
        const s32 full = DeviceCtx::RING_SLOTS * 8;  // 4 slots x 8 blocks: what pipeline_shape grants at most
        if (lead->lean && lead->ctx->temp_idle_bytes() > 0 && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            if (ring_contexts_for(free_b, lead->ctx->ws_cap, need, fixed, ctx_bytes, lead->cap, true, headroom) < (size_t)(n < full ? n : full)) lead->ctx->temp_trim();
        }
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            contexts = ring_contexts_for(free_b, lead->ctx->ws_cap, need, fixed, ctx_bytes, lead->cap, lead->lean, headroom);
            contexts_beside_runs = ring_contexts_for(free_b, lead->ctx->ws_cap, need + bwt_extra, fixed, ctx_bytes, lead->cap, lead->lean, headroom);
            contexts_beside_short_runs = ring_contexts_for(free_b, lead->ctx->ws_cap, need + bwt_extra_short, fixed, ctx_bytes, lead->cap, lead->lean, headroom);
        }
    }
    s32 window = 1, ns = 2;
    pipeline_shape((s32)(contexts < 1024 ? contexts : 1024), n, window, ns);
    // granted only where the ring as shaped above still fits beside them: then ring, runs and headroom all lie inside what ring_contexts_for counted
    if (contexts_beside_runs < (size_t)ns * (size_t)window) bwt_extra = contexts_beside_short_runs < (size_t)ns * (size_t)window ? 0 : bwt_extra_short;
    lead->ctx->ensure_aux();
    hipStream_t s = lead->stream;
    DrainOnUnwind drain{s, lead->ctx->aux, DeviceCtx::AUX};
    // BZ3_HIP_FRONT_REST=1 (experiment, read once): the front end's whole-GPU kernels also keep off the CUs reserved for the side streams' LZP drivers
    static const bool front_rest = [] { const char * e = getenv("BZ3_HIP_FRONT_REST"); return e && atoi(e) != 0; }();
    if (front_rest && lead->ctx->rest && n > 1) {
        s = lead->ctx->rest;
        for (s32 i = 0; i < n; i++) sts[i]->xs = s;
    }
    DrainOnUnwind drain_rest{s == lead->stream ? nullptr : s, nullptr, 0};
    Arena arena;
    for (;;) {  // hipMemGetInfo's figure is not a promise (fragmentation, another process on the device): shrink the ring before giving up
        try {
            arena = lead->ctx->arena_for(need + bwt_extra + (size_t)ns * (size_t)window * (ctx_bytes + sizeof(LzpDriverJob) + 256) +
                                         (size_t)n * (sizeof(CmEncodeJob) + CM_SIDE_BYTES + 256) + cm_scratch_bytes((size_t)n) + 65536);
            break;
        } catch (const HipError &) {  // out of memory, or whatever else the runtime answers to a size it does not like
            if (ns == 2 && window == 1 && bwt_extra == 0) throw;
            (void)hipGetLastError();
            if (bwt_extra > bwt_extra_short) bwt_extra = bwt_extra_short;  // the sorter's long runs go first, then its runs altogether
            else if (bwt_extra) bwt_extra = 0;  // the sorter's runs go first (bwt_batch_size then finds room for one block at a time): never an LZP context
            else if (ns > 2) ns = 2;
            else window = (window + 1) / 2;
        }
    }
    g_front_end_ring.store(window | (ns << 16));
    CmEncodeJob * d_jobs = arena.take<CmEncodeJob>((size_t)n);
    u8 * sides = arena.take<u8>((size_t)n * CM_SIDE_BYTES);  // lean states only
    struct Window {
        s32 w0 = 0, w1 = 0;
        Arena slot;                        // the LZP contexts of the window's blocks
        LzpDriverJob * d_lz = nullptr;
        std::vector<LzpEncodeCtx> ctxs;
        std::vector<LzpDriverJob> lz;      // host copy: stays alive until the window is finished
    } win[DeviceCtx::AUX];
    for (int k = 0; k < ns; k++) {
        win[k].slot.base = arena.take<char>((size_t)window * ctx_bytes);
        win[k].slot.cap = (size_t)window * ctx_bytes;
        win[k].d_lz = arena.take<LzpDriverJob>((size_t)window);
    }
    std::vector<CmEncodeJob> jobs;
    std::vector<s32> job_owner;
    std::vector<BwtBatchItem> fb_items;  // phase B of one window: the blocks that reach the transform ...
    std::vector<bz3_state *> fb_owner;   // ... their states ...
    std::vector<u8 *> fb_copy;           // ... where a lean state's output goes afterwards ...
    std::vector<s32> fb_slot;            // ... and a block's place among them (-1: it left the pipeline before)
    const s32 nwin = (n + window - 1) / window;
    const s32 lag = ns - 1;  // window k is finished in iteration k + lag
    static const bool trace_rings = getenv("BZ3_HIP_TRACE_RINGS") != nullptr;  // (diagnosis, read once: see decode_group)
    double tr_prep = 0, tr_wait = 0, tr_fin = 0, tr_t0 = now_ms();
    // Phase A of window k on stream sp with scratch `scr`: CRC, mRLE, LZP preparation of its blocks, then its drivers on the slot's side stream behind `ev`.
    auto prepare = [&](s32 k, hipStream_t sp, Arena & scr, hipEvent_t ev) {
        const int q = (int)(k % ns);
        Window & w = win[q];
        w.w0 = k * window;
        w.w1 = (w.w0 + window < n) ? w.w0 + window : n;
        w.slot.used = 0;  // its previous tenant (window k-ns) has been finished
        w.ctxs.assign((size_t)(w.w1 - w.w0), LzpEncodeCtx());
        w.lz.clear();
        for (s32 i = w.w0; i < w.w1; i++) {
            sts[i]->xs = sp;
            sts[i]->hold_swap = false;  // (a call that was left by an exception may have left it set)
            encode_front_a(sts[i], bufs[i], sizes[i], scr, w.slot, w.ctxs[(size_t)(i - w.w0)]);
            if (sts[i]->pending == bz3_state::ENC_CODED && w.ctxs[(size_t)(i - w.w0)].active) w.lz.push_back(lzp_driver_job(w.ctxs[(size_t)(i - w.w0)]));
        }
        HIP_CHECK(hipEventRecord(ev, sp));  // the prepares above are in flight on sp
        if (!w.lz.empty()) {
            hipStream_t sq = lead->ctx->aux[q];
            HIP_CHECK(hipStreamWaitEvent(sq, ev, 0));
            HIP_CHECK(hipEventRecord(lead->ctx->ev_d0[q], sq));
            lzp_driver_batch(w.lz.data(), w.d_lz, (u32)w.lz.size(), sq);
            HIP_CHECK(hipEventRecord(lead->ctx->ev_d1[q], sq));
        }
    };
    // Phase B of window j on stream sf with scratch `scr`: waits for its drivers, then LZP emission, BWT, header per block; the CM jobs in block order.
    // held != nullptr: lean states keep their swap buffers (the caller hands them back behind an event: two-thread form).
    auto finish = [&](s32 j, hipStream_t sf, Arena & scr, std::vector<bz3_state *> * held) {
        const int q = (int)(j % ns);
        Window & w = win[q];
        float driver_ms = 0.f;
        if (!w.lz.empty()) {
            const double t0 = now_ms();
            HIP_CHECK(hipEventSynchronize(lead->ctx->ev_d1[q]));
            (void)hipEventElapsedTime(&driver_ms, lead->ctx->ev_d0[q], lead->ctx->ev_d1[q]);
            tr_wait += now_ms() - t0;
        }
        // the window's blocks first all go through the LZP emission and the buffer choice, then through the suffix sorter in runs of up to
        // BWT_MAX_BATCH; header, swap buffer and CM job follow per block, in block order
        fb_items.clear();
        fb_owner.clear();
        fb_copy.clear();
        fb_slot.assign((size_t)(w.w1 - w.w0), -1);
        for (s32 i = w.w0; i < w.w1; i++) {
            sts[i]->xs = sf;
            BwtBatchItem item{};
            u8 * copy_to = nullptr;
            if (encode_front_b_collect(sts[i], scr, w.ctxs[(size_t)(i - w.w0)], driver_ms, item, copy_to)) {
                fb_slot[(size_t)(i - w.w0)] = (s32)fb_items.size();
                fb_items.push_back(item);
                fb_owner.push_back(sts[i]);
                fb_copy.push_back(copy_to);
            }
        }
        encode_front_b_transform(fb_owner.data(), fb_items.data(), fb_items.size(), scr, sf);
        for (s32 i = w.w0; i < w.w1; i++) {
            const s32 slot = fb_slot[(size_t)(i - w.w0)];
            if (slot >= 0) {
                sts[i]->hold_swap = held != nullptr;
                encode_front_b_header(sts[i], fb_items[(size_t)slot], fb_copy[(size_t)slot]);
                sts[i]->hold_swap = false;
            }
            if (sts[i]->pending == bz3_state::ENC_CODED) {
                CmEncodeJob j2{dev_addr(sts[i]->b2), dev_addr(sts[i]->b1 + sts[i]->overhead * 4 + 1), dev_addr(sts[i]->d_words + 2), sts[i]->n_cm, 0u};  // :634-638
                if (sts[i]->lean) {  // in place: input at the end of the caller's buffer, output behind the header
                    sts[i]->side = sides + (size_t)i * CM_SIDE_BYTES;
                    j2.gap = (u32)(sts[i]->b2 - (sts[i]->b1 + sts[i]->overhead * 4 + 1));
                    j2.side = dev_addr(sts[i]->side);
                    j2.side_cap = CM_SIDE_BYTES;
                }
                jobs.push_back(j2);
                job_owner.push_back(i);
            }
            if (held) {
                if (sts[i]->lean && sts[i]->d_swap) held->push_back(sts[i]);
            } else {
                lean_return(sts[i]);  // blocks that left the pipeline early (stored, failed) still hold their swap buffer
            }
        }
    };
    const bool duo = duo_wanted && nwin >= 3 && lead->ctx->aux_ready && s == lead->stream;  // (aux_ready: ctx->duo exists -- a null handle under the emulator)
    if (!duo) {
        for (s32 k = 0; k < nwin + lag; k++) {
            const double tr_a = now_ms();
            if (k < nwin) prepare(k, s, arena, lead->ctx->ev_prep);
            const double tr_b = now_ms();
            tr_prep += tr_b - tr_a;
            if (k >= lag) finish(k - lag, s, arena, nullptr);
            tr_fin += now_ms() - tr_b;
        }
    } else {
        // ---- two-thread front end (round 6).  Phase A (14 ms of whole-GPU kernels per 256 MiB block) and phase B (56 ms) both stop for read-backs the host
        // needs (mRLE size; LZP size, one per sorter pass), and while one waits nothing of THIS stream runs.  A second host thread takes phase A on a stream of its
        // own (ctx->duo) with its own scratch region and runs up to ns - 1 windows ahead of this thread's phase B: the kernels of one fill the other's bubbles.
        //   slot reuse      A prepares window k once B has FINISHED window k - ns (host: `finished`) and behind B's kernels of that window (stream: evB[k - ns]);
        //   hand-over       B starts window j once A has prepared it (host: `prepared`), behind A's kernels (stream: evA[j]); the drivers' events as before;
        //   swap buffers    lean states' buffers go back to the pool when B has recorded evB[j] (`held`), and A's stream waits for the latest such event before the
        //                   kernels of blocks that may have borrowed them: with two streams stream order alone no longer protects a re-borrowed buffer.
        // Output bytes cannot depend on any of this: every block still runs A then B, each on one stream, B behind A's event.
        g_front_end_ring.fetch_or(1 << 29);
        hipStream_t sA = lead->ctx->duo;
        DrainOnUnwind drain_duo{sA, nullptr, 0};
        Arena scr_a;
        scr_a.base = arena.take<char>(need_a);
        scr_a.cap = need_a;
        struct Events {
            std::vector<hipEvent_t> e;
            ~Events() {
                for (hipEvent_t x : e)
                    if (x) (void)hipEventDestroy(x);
            }
        } evs;
        evs.e.assign((size_t)2 * (size_t)nwin, nullptr);
        for (auto & x : evs.e) HIP_CHECK(hipEventCreateWithFlags(&x, hipEventDisableTiming));
        hipEvent_t * evA = evs.e.data(), * evB = evs.e.data() + nwin;
        struct Shared {
            std::mutex m;
            std::condition_variable cv;
            s32 prepared = 0, finished = 0;
            bool abort = false;
            std::exception_ptr err;
            std::mutex pool;              // borrowing a window's buffers / returning a window's buffers + publishing the event that covers them
            hipEvent_t last_return = nullptr;
            double prep_ms = 0;
        } sh;
        const int device = lead->device;
        std::thread ta([&] {
            try {
                DeviceGuard gd(device);
                for (s32 k = 0; k < nwin; k++) {
                    {
                        std::unique_lock<std::mutex> ul(sh.m);
                        sh.cv.wait(ul, [&] { return sh.abort || sh.finished >= k - ns + 1; });
                        if (sh.abort) return;
                    }
                    const double t0 = now_ms();
                    if (k >= ns) HIP_CHECK(hipStreamWaitEvent(sA, evB[k - ns], 0));
                    {
                        hipEvent_t ev = nullptr;
                        const s32 w0 = k * window, w1 = (w0 + window < n) ? w0 + window : n;
                        {
                            std::lock_guard<std::mutex> pl(sh.pool);
                            for (s32 i = w0; i < w1; i++) lean_borrow(sts[i]);
                            ev = sh.last_return;
                        }
                        if (ev) HIP_CHECK(hipStreamWaitEvent(sA, ev, 0));
                    }
                    prepare(k, sA, scr_a, evA[k]);
                    {
                        std::lock_guard<std::mutex> ul(sh.m);
                        sh.prepared = k + 1;
                        sh.prep_ms += now_ms() - t0;
                    }
                    sh.cv.notify_all();
                }
            } catch (...) {
                {
                    std::lock_guard<std::mutex> ul(sh.m);
                    sh.err = std::current_exception();
                    sh.abort = true;
                }
                sh.cv.notify_all();
            }
        });
        struct Joiner {  // whatever happens on this thread, phase A's thread is joined before its std::thread object dies
            std::thread & t;
            Shared & sh;
            int live = std::uncaught_exceptions();
            ~Joiner() {
                if (std::uncaught_exceptions() > live) {  // this thread is unwinding: phase A stops at its next window
                    std::lock_guard<std::mutex> ul(sh.m);
                    sh.abort = true;
                }
                sh.cv.notify_all();
                if (t.joinable()) t.join();
            }
        } joiner{ta, sh};
        std::vector<bz3_state *> held;
        for (s32 j = 0; j < nwin; j++) {
            const double tr_b = now_ms();
            {
                std::unique_lock<std::mutex> ul(sh.m);
                sh.cv.wait(ul, [&] { return sh.abort || sh.prepared >= j + 1; });
                if (sh.abort) break;
            }
            HIP_CHECK(hipStreamWaitEvent(s, evA[j], 0));
            held.clear();
            finish(j, s, arena, &held);
            HIP_CHECK(hipEventRecord(evB[j], s));
            {
                std::lock_guard<std::mutex> pl(sh.pool);
                for (bz3_state * st : held) lean_return(st);
                sh.last_return = evB[j];
            }
            {
                std::lock_guard<std::mutex> ul(sh.m);
                sh.finished = j + 1;
            }
            sh.cv.notify_all();
            tr_fin += now_ms() - tr_b;
        }
        ta.join();
        if (sh.err) std::rethrow_exception(sh.err);
        HIP_CHECK(hipStreamSynchronize(sA));
        tr_prep = sh.prep_ms;
        for (s32 i = 0; i < n; i++) sts[i]->xs = s;
    }
    if (trace_rings)
        fprintf(stderr, "[bz3 rings] encode front end: %d blocks, %d windows of %d x %d slots: %.1f ms = CRC / mRLE / LZP prepare %.1f + waiting for a window's LZP drivers %.1f + LZP emit / BWT / header %.1f\n",
                (int)n, (int)nwin, (int)window, (int)ns, now_ms() - tr_t0, tr_prep, tr_wait, tr_fin - tr_wait);
    if (s != lead->stream) {  // the CM launch needs every CU: back to the group's unmasked stream, behind the front end
        HIP_CHECK(hipStreamSynchronize(s));
        s = lead->stream;
        for (s32 i = 0; i < n; i++) sts[i]->xs = s;
    }
    // which blocks do not fit a row cache: the bytes outside the block's 40 most frequent values (bwt.hip k_bwt_outside) -- one small read-back per
    // block, all behind the one synchronisation the CM launch needs anyway
    std::vector<char> to_full(jobs.size(), 0);
    if (jobs.size() > (size_t)lead->ctx->cus) {  // (only batches that would take a row-cache variant)
        std::vector<u32> outside(jobs.size(), 0u);
        for (size_t k = 0; k < jobs.size(); k++) HIP_CHECK(hipMemcpyAsync(&outside[k], sts[job_owner[k]]->d_words + 8, 4, hipMemcpyDeviceToHost, lead->stream));
        HIP_CHECK(hipStreamSynchronize(lead->stream));
        // Only the hopeless: more than a QUARTER of the block outside its 40 most frequent values (random data: 84 %).  The histogram is global, a row
        // cache lives on what the BWT output uses LOCALLY: the bench's calibrated text has 3 % of its bytes outside the top 40 and misses 0.3 % of its
        // rows -- round 5's first form of this test (outside > 512 + n / 64) sent all 768 text blocks to the whole-model kernel, one per CU, 183 s instead
        // of 65 (profiles/r05_full_size_call5_misrouted.txt).  What lies between is left to the kernels' own give-up test.
        for (size_t k = 0; k < jobs.size(); k++) to_full[k] = outside[k] > jobs[k].n / 4u ? 1 : 0;
    }
    const float cm_ms = run_cm_jobs(lead->ctx, arena, jobs, d_jobs, lead->stream, lead->ev0, lead->ev1,
                                    [](const CmEncodeJob * j, u32 nj, hipStream_t st, int variant) { cm_encode_batch(j, nj, st, variant); }, &to_full);
    for (s32 i = 0; i < n; i++) encode_finish(sts[i], cm_ms);
    // Hand-back only where it matters: a workspace that a GPU-filling batch grew to tens of GB (the decode call that follows needs the
    // room).  A stream of ordinary batches (the CLI, bz3_hip_encode_stream) keeps its workspace: a multi-GB hipMalloc plus a
    // device-synchronising hipFree per call would cost more than the memory is worth.
    size_t slack = (size_t)16 << 30;
    if (const char * e = getenv("BZ3_HIP_WS_KEEP_MB")) slack = (size_t)strtoull(e, nullptr, 10) << 20;  // tests only
    if (lead->ctx->ws_cap > 2 * need + slack && !(keep_workspace() && lead->lean)) {  // mostly LZP contexts of a large batch: hand the memory back (see above)
        HIP_CHECK(hipStreamSynchronize(s));  // the side streams are idle: every driver launch has been waited for
        (void)hipFree(lead->ctx->ws);
        lead->ctx->ws = nullptr;
        lead->ctx->ws_cap = 0;
        g_front_end_ring.fetch_or(1 << 30);
    }
    enforce_headroom(lead->ctx, lead->stream);
}

}  // namespace api
}  // namespace bz3
