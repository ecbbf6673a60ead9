// api.hip -- the C ABI (include/libbz3.h + include/bz3_hip.h) on top of the HIP stage pipelines.
//
// Mirrors the reference's orchestration exactly: bz3_encode_block (src/libbz3.c:585-654) and
// bz3_decode_block (:656-809) are ping-pong pipelines over the caller's buffer and the state's swap
// buffer; every size/flag decision and every error code is reproduced.  What changes is WHERE things
// live: both buffers are in HBM, the stages are the kernels of crc32c/mrle/lzp/bwt/unbwt/cm.hip, the
// suffix-sort workspace is one arena per GPU shared by all states, and a batch call
// (bz3_encode_blocks / bz3_decode_blocks, :845-870, without pthreads) runs in phases on ONE stream per GPU:
// the whole-GPU stages block after block, the serial stages (LZP driver, LZP decoder, CM coder) as ONE
// launch with one workgroup per block, so up to 256 blocks share the GPU's 256 CUs.
//
// There is no CPU implementation of any stage in this library: without a usable HIP device
// bz3_new() returns NULL and the stage hooks abort loudly.
//
// The layer is one translation unit per part, over api_internal.hpp: api_context.hip (device context, states, every global, control entry
// points), api_encode.hip / api_decode.hip (encode_group / decode_group), api_frames.hip (device-resident frames), api_hooks.hip (stage
// hooks), and this file: the split of a batch by device, the libbz3.h block entry points, the collector of single-block callers and the
// host frame API.
#include "api_internal.hpp"
#include "frame_check.hpp"

using namespace bz3;
using namespace bz3::api;

namespace {

void ensure_io(bz3_state * st) {
    if (!st->d_io) HIP_CHECK(hipMalloc((void **)&st->d_io, st->cap));
}

void on_failure(bz3_state * st) {
    if (st) {
        lean_return(st);
        st->last_error = BZ3_ERR_BWT;
        st->pending = bz3_state::NONE;
        st->result = -1;
    }
}

// Splits a batch by device (states may live on different GPUs) and runs the groups CONCURRENTLY, one host thread per
// GPU (the reference forks a thread per block, src/libbz3.c:845-856): every group has its own device context, stream,
// arena and mutex, and hipSetDevice is per host thread, so the GPUs of a node work on their blocks at the same time.
template <typename F>
void for_each_device_group(bz3_state ** states, s32 n, F && f) {
    std::vector<std::vector<s32>> groups;
    std::vector<char> done((size_t)n, 0);
    for (s32 i = 0; i < n; i++) {
        if (done[(size_t)i]) continue;
        groups.emplace_back();
        for (s32 j = i; j < n; j++)
            if (!done[(size_t)j] && states[j]->device == states[i]->device) { groups.back().push_back(j); done[(size_t)j] = 1; }
    }
    auto run = [&](const std::vector<s32> & idx) {
        const int now = g_groups_running.fetch_add(1) + 1;
        int peak = g_groups_peak.load();
        while (now > peak && !g_groups_peak.compare_exchange_weak(peak, now)) {}
        try {
            f(idx);
        } catch (const HipError & e) {
            fprintf(stderr, "bzip3_amd: HIP failure '%s' at %s:%d\n", e.what, e.file, e.line);
            for (s32 j : idx) on_failure(states[j]);
        } catch (...) {  // bad_alloc, system_error, length_error ...: nothing may leave a worker thread (std::terminate)
            for (s32 j : idx) on_failure(states[j]);
        }
        g_groups_running.fetch_sub(1);
    };
    std::vector<std::thread> workers;
    struct Joiner {  // whatever happens on the calling thread, the workers are joined before their std::thread objects die
        std::vector<std::thread> & w;
        ~Joiner() {
            for (std::thread & t : w)
                if (t.joinable()) t.join();
        }
    } joiner{workers};
    size_t spawned = 1;  // groups [1, spawned) run on a worker thread each, group 0 and the rest on this thread
    for (size_t g = 1; g < groups.size(); g++) {
        try {
            workers.emplace_back(run, std::cref(groups[g]));
        } catch (const std::system_error &) {  // no thread to be had
            break;
        }
        spawned = g + 1;
    }
    if (!groups.empty()) run(groups[0]);
    for (size_t g = spawned; g < groups.size(); g++) run(groups[g]);
}

// Host-buffer API: the blocks of a group are staged through the states' d_io buffers inside the group's own thread, all
// copies of a direction enqueued back to back on the group's stream with ONE synchronisation, so the GPUs of a batch copy
// and code at the same time.  A block whose staging fails is marked (skip) and left alone by the group; the others go on.
void stage_in(bz3_state * st, const void * host, size_t bytes, hipStream_t s) {
    try {
        ensure_io(st);
        if (bytes) HIP_CHECK(hipMemcpyAsync(st->d_io, host, bytes, hipMemcpyHostToDevice, s));
    } catch (...) {  // HIP failure or bad_alloc from ensure_io: this block fails, the others of the group go on
        on_failure(st);
        st->skip = true;
    }
}

// Host copies of the first 17 bytes of n device-resident blocks.
void fetch_headers(bz3_state ** states, void ** buffers, const size_t * buffer_sizes, s32 n, std::vector<u8> & hdrs) {
    hdrs.assign(17 * (size_t)n, 0);
    for (s32 i = 0; i < n; i++) {
        const size_t take = buffer_sizes[i] < 17 ? buffer_sizes[i] : 17;
        if (take < 9) continue;
        try {
            HIP_CHECK(hipSetDevice(states[i]->device));
            HIP_CHECK(hipMemcpyAsync(hdrs.data() + 17 * (size_t)i, buffers[i], take, hipMemcpyDeviceToHost, states[i]->stream));
            HIP_CHECK(hipStreamSynchronize(states[i]->stream));
        } catch (const HipError &) {
        }
    }
}

}  // namespace

namespace bz3 {
namespace api {

void run_encode(bz3_state ** states, void ** buffers, s32 * sizes, s32 n, bool host) {
    for_each_device_group(states, n, [&](const std::vector<s32> & idx) {
        std::vector<bz3_state *> sts;
        std::vector<u8 *> bufs;
        std::vector<s32> szs;
        DeviceGuard g(states[idx[0]]->device);
        hipStream_t s = states[idx[0]]->stream;
        const double t0 = now_ms();
        for (s32 j : idx) {
            bz3_state * st = states[j];
            st->skip = false;
            if (host) stage_in(st, buffers[j], (sizes[j] >= 0 && sizes[j] <= st->block_size) ? (size_t)sizes[j] : 0, s);
            sts.push_back(st);
            bufs.push_back(host ? st->d_io : (u8 *)buffers[j]);
            szs.push_back(sizes[j]);
        }
        if (host) HIP_CHECK(hipStreamSynchronize(s));
        const float in_ms = (float)(now_ms() - t0);
        encode_group(sts.data(), bufs.data(), szs.data(), (s32)idx.size());
        if (!host) return;
        const double t1 = now_ms();
        for (s32 j : idx) {
            bz3_state * st = states[j];
            if (st->result > 0 && !st->skip) HIP_CHECK(hipMemcpyAsync(buffers[j], st->d_io, (size_t)st->result, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
        const float out_ms = (float)(now_ms() - t1);
        for (s32 j : idx) states[j]->t[BZ3_HIP_T_COPY] += (in_ms + out_ms) / (float)idx.size();
    });
    for (s32 i = 0; i < n; i++) {
        sizes[i] = states[i]->result;
        states[i]->skip = false;
    }
}

void run_decode(bz3_state ** states, void ** buffers, const size_t * buffer_sizes, const s32 * sizes, const s32 * orig_sizes, const u8 * hdrs, s32 n, bool host) {
    for_each_device_group(states, n, [&](const std::vector<s32> & idx) {
        std::vector<bz3_state *> sts;
        std::vector<u8 *> bufs;
        std::vector<size_t> bsz;
        std::vector<s32> csz, osz;
        std::vector<u8> hd;
        DeviceGuard g(states[idx[0]]->device);
        hipStream_t s = states[idx[0]]->stream;
        const double t0 = now_ms();
        for (s32 j : idx) {
            bz3_state * st = states[j];
            st->skip = false;
            if (host) {
                // the two checks that protect the H2D copy are the reference's first two (:658, :667); decode_front repeats them
                const bool copy_ok = buffer_sizes[j] >= 9 && buffer_sizes[j] >= (size_t)sizes[j] && sizes[j] >= 0 &&
                                     (size_t)sizes[j] <= bz3_bound((size_t)st->block_size);
                stage_in(st, buffers[j], copy_ok ? (size_t)sizes[j] : 0, s);
            }
            sts.push_back(st); bufs.push_back(host ? st->d_io : (u8 *)buffers[j]); bsz.push_back(buffer_sizes[j]); csz.push_back(sizes[j]); osz.push_back(orig_sizes[j]);
            hd.insert(hd.end(), hdrs + 17 * (size_t)j, hdrs + 17 * (size_t)j + 17);
        }
        if (host) HIP_CHECK(hipStreamSynchronize(s));
        const float in_ms = (float)(now_ms() - t0);
        decode_group(sts.data(), bufs.data(), bsz.data(), csz.data(), osz.data(), hd.data(), (s32)idx.size());
        if (!host) return;
        const double t1 = now_ms();
        for (s32 j : idx) {
            bz3_state * st = states[j];
            if (st->result > 0 && !st->skip) HIP_CHECK(hipMemcpyAsync(buffers[j], st->d_io, (size_t)st->result, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
        const float out_ms = (float)(now_ms() - t1);
        for (s32 j : idx) states[j]->t[BZ3_HIP_T_COPY] += (in_ms + out_ms) / (float)idx.size();
    });
    for (s32 i = 0; i < n; i++) states[i]->skip = false;
}

}  // namespace api
}  // namespace bz3

// =====================================================================================================
// libbz3.h
// =====================================================================================================
extern "C" {

BZIP3_API const char * bz3_version(void) { return "1.5.2-mi355x"; }

BZIP3_API int8_t bz3_last_error(struct bz3_state * state) { return state->last_error; }

BZIP3_API size_t bz3_bound(size_t input_size) { return input_size + input_size / 50 + 32; }

BZIP3_API const char * bz3_strerror(struct bz3_state * state) {  // messages: src/libbz3.c:512-533
    switch (state->last_error) {
        case BZ3_OK: return "No error";
        case BZ3_ERR_OUT_OF_BOUNDS: return "Data index out of bounds";
        case BZ3_ERR_BWT: return "Burrows-Wheeler transform failed";
        case BZ3_ERR_CRC: return "CRC32 check failed";
        case BZ3_ERR_MALFORMED_HEADER: return "Malformed header";
        case BZ3_ERR_TRUNCATED_DATA: return "Truncated data";
        case BZ3_ERR_DATA_TOO_BIG: return "Too much data";
        case BZ3_ERR_DATA_SIZE_TOO_SMALL:
            return "Size of buffer `buffer_size` passed to the block decoder (bz3_decode_block) is too small. See function docs for details.";
        default: return "Unknown error";
    }
}

BZIP3_API struct bz3_state * bz3_new(int32_t block_size) {
    if (block_size < KiB65 || block_size > MiB511) return nullptr;  // :536
    const int dev = pick_device();
    if (dev < 0) {
        fprintf(stderr, "bzip3_amd: no HIP device available -- this library has no CPU code path\n");
        return nullptr;
    }
    return new_state_on(block_size, dev);
}

BZIP3_API void bz3_free(struct bz3_state * state) { state_release(state); }

BZIP3_API size_t bz3_min_memory_needed(int32_t block_size) {
    if (block_size < KiB65 || block_size > MiB511) return 0;
    const size_t cap = (bz3_bound((size_t)block_size) + 4096 + 255) & ~(size_t)255;
    return sizeof(bz3_state) + cap + 64 * sizeof(u32);
}

// ---- device-resident entry points (bz3_hip.h) -----------------------------------------------------
BZIP3_API void bz3_hip_encode_blocks_device(struct bz3_state * states[], void * buffers[], int32_t sizes[], int32_t n) {
    run_encode(states, buffers, sizes, n, false);
}

BZIP3_API void bz3_hip_decode_blocks_device(struct bz3_state * states[], void * buffers[], size_t buffer_sizes[], int32_t sizes[],
                                            int32_t orig_sizes[], int32_t n) {
    std::vector<u8> hdrs;
    fetch_headers(states, buffers, buffer_sizes, n, hdrs);
    run_decode(states, buffers, buffer_sizes, sizes, orig_sizes, hdrs.data(), n, false);
}

BZIP3_API int32_t bz3_hip_encode_block_device(struct bz3_state * st, void * buffer, int32_t size) {
    s32 sz = size;
    run_encode(&st, &buffer, &sz, 1, false);
    return sz;
}

BZIP3_API int32_t bz3_hip_decode_block_device(struct bz3_state * st, void * buffer, size_t buffer_size, int32_t compressed_size,
                                              int32_t orig_size) {
    bz3_hip_decode_blocks_device(&st, &buffer, &buffer_size, &compressed_size, &orig_size, 1);
    return st->result;
}

// ---- host-buffer entry points (libbz3.h): staged through the states' d_io buffers by the device groups (run_encode / run_decode) ------
BZIP3_API void bz3_encode_blocks(struct bz3_state * states[], uint8_t * buffers[], int32_t sizes[], int32_t n) {
    run_encode(states, (void **)buffers, sizes, n, true);
}

BZIP3_API void bz3_decode_blocks(struct bz3_state * states[], uint8_t * buffers[], size_t buffer_sizes[], int32_t sizes[], int32_t orig_sizes[],
                                 int32_t n) {
    std::vector<u8> hdrs(17 * (size_t)n, 0);
    for (s32 i = 0; i < n; i++) memcpy(hdrs.data() + 17 * (size_t)i, buffers[i], buffer_sizes[i] < 17 ? buffer_sizes[i] : 17);
    run_decode(states, (void **)buffers, buffer_sizes, sizes, orig_sizes, hdrs.data(), n, true);
}

// ---- single-block calls from several host threads ----------------------------------------------------------------------------
// The reference's batch API IS "N threads, one bz3_encode_block each" (src/libbz3.c:831-856), and a binding that does its own
// threading calls the single-block functions the same way.  Here a block's CM stage is a serial ~300 ns-per-byte recurrence that only
// pays off with many blocks in ONE launch, and a group call holds its device for its whole duration: N concurrent single-block calls
// would run as N launches one after the other.  So concurrent callers are COLLECTED: the first one in becomes the leader, waits a
// short window (bz3_hip_set_collect_window_us, default 200 us -- nothing beside a block's milliseconds) for the others, and takes
// everything that has arrived through bz3_encode_blocks / bz3_decode_blocks as one batch; callers that arrive while a batch runs form
// the next one.  Same bytes, return values and error codes: a batch call treats its blocks independently.
namespace {
void run_collected(int kind, std::vector<SingleReq *> & batch) {
    const s32 n = (s32)batch.size();
    g_collect_batches.fetch_add(1u);
    unsigned big = g_collect_largest.load();
    while ((unsigned)n > big && !g_collect_largest.compare_exchange_weak(big, (unsigned)n)) {}
    std::vector<bz3_state *> sts((size_t)n);
    std::vector<u8 *> bufs((size_t)n);
    std::vector<s32> sizes((size_t)n), orig((size_t)n);
    std::vector<size_t> bsz((size_t)n);
    for (s32 i = 0; i < n; i++) {
        sts[(size_t)i] = batch[(size_t)i]->st;
        bufs[(size_t)i] = batch[(size_t)i]->buffer;
        sizes[(size_t)i] = batch[(size_t)i]->size;
        orig[(size_t)i] = batch[(size_t)i]->orig_size;
        bsz[(size_t)i] = batch[(size_t)i]->buffer_size;
    }
    if (kind == 0) {
        bz3_encode_blocks(sts.data(), bufs.data(), sizes.data(), n);
        for (s32 i = 0; i < n; i++) batch[(size_t)i]->size = sizes[(size_t)i];
    } else {
        bz3_decode_blocks(sts.data(), bufs.data(), bsz.data(), sizes.data(), orig.data(), n);
    }
}

// The window is there for the FIRST batch of a group of threads; after it the callers that arrive while a batch runs form the next one
// by themselves.  So (round 4): a caller that has been alone twice in a row -- a single-threaded program -- no longer
// waits at all (it paid the window on every call, in both directions), and a leader stops waiting as soon as as many callers as
// the previous batch had have arrived instead of sleeping the whole window.  What remains by design: the callers of one batch share
// its latency -- a 64 KiB block that is collected with a 511 MiB block returns when that block does (bz3_hip_set_collect_window_us(0)
// gives every call a batch of its own).
void collect(int kind, SingleReq & r) {
    Collector & c = g_collect;
    std::unique_lock<std::mutex> lk(c.mu);
    c.pending[kind].push_back(&r);
    c.cv.notify_all();  // a leader inside its window counts the arrivals
    while (!r.done) {
        if (c.leader[kind]) {
            c.cv.wait(lk);
            continue;
        }
        c.leader[kind] = true;
        const int win = g_collect_window_us.load();
        if (win > 0 && c.lonely[kind] < 2) {
            const size_t want = c.last_size[kind] > 1 ? c.last_size[kind] : ~(size_t)0;
            c.cv.wait_for(lk, std::chrono::microseconds(win), [&] { return c.pending[kind].size() >= want; });  // the others arrive meanwhile (the lock is released)
        }
        std::vector<SingleReq *> batch;
        batch.swap(c.pending[kind]);
        lk.unlock();
        try {
            run_collected(kind, batch);
        } catch (...) {  // (the batch calls do not throw; belt and braces: nobody may wait for ever)
            for (SingleReq * q : batch) {
                on_failure(q->st);
                if (kind == 0) q->size = -1;  // bz3_encode_block returns this: the request's input size must not pass for a coded size
            }
        }
        lk.lock();
        for (SingleReq * q : batch) q->done = true;
        c.last_size[kind] = batch.size();
        c.lonely[kind] = (batch.size() == 1 && c.pending[kind].empty()) ? c.lonely[kind] + 1 : 0;
        c.leader[kind] = false;
        c.cv.notify_all();
    }
}
}  // namespace

BZIP3_API int32_t bz3_encode_block(struct bz3_state * st, uint8_t * buffer, int32_t size) {
    SingleReq r{st, buffer, 0, size, 0};
    try {
        collect(0, r);
    } catch (...) {  // (queueing the request could not allocate: nothing may cross the C boundary)
        on_failure(st);
        return -1;
    }
    return r.size;
}

BZIP3_API int32_t bz3_decode_block(struct bz3_state * st, uint8_t * buffer, size_t buffer_size, int32_t compressed_size, int32_t orig_size) {
    SingleReq r{st, buffer, buffer_size, compressed_size, orig_size};
    try {
        collect(1, r);
    } catch (...) {
        on_failure(st);
        return -1;
    }
    return st->result;
}

// ---- frame API (src/libbz3.c:876-997): same header, chunk layout and error codes.  The reference walks the
// blocks of a frame one after the other on one state; here a WINDOW of blocks goes through bz3_encode_blocks /
// bz3_decode_blocks at once (one state per block, blocks spread over the visible GPUs, one CM launch per GPU), because
// the serial CM stage only pays off with many blocks in flight.  Blocks are still committed in order, so the first
// failing block decides the return value exactly as in the sequential loop.
namespace {

struct FrameWindow {
    std::vector<bz3_state *> states;
    std::vector<u8 *> bufs;
    size_t cap = 0;
    ~FrameWindow() {
        for (bz3_state * s : states) bz3_free(s);
        for (u8 * b : bufs) free(b);
    }
    // Up to `want` states + host buffers of bz3_bound(block_size) bytes; at least one or false.
    bool init(u32 block_size, size_t want) {
        cap = bz3_bound(block_size);
        const int ndev = device_count();
        size_t limit = (size_t)(ndev > 0 ? ndev : 1) * 256;             // one CU per block during the CM stage
        const size_t by_mem = ((size_t)16 << 30) / (cap ? cap : 1);      // host staging budget of the window
        if (limit > by_mem) limit = by_mem;
        if (limit < 1) limit = 1;
        if (want > limit) want = limit;
        if (want < 1) want = 1;
        for (size_t i = 0; i < want; i++) {
            bz3_state * st = bz3_new((int32_t)block_size);
            u8 * b = st ? (u8 *)malloc(cap) : nullptr;
            if (!st || !b) {
                if (st) bz3_free(st);
                free(b);
                break;
            }
            states.push_back(st);
            bufs.push_back(b);
        }
        return !states.empty();
    }
};

}  // namespace

BZIP3_API int bz3_compress(uint32_t block_size, const uint8_t * in, uint8_t * out, size_t in_size, size_t * out_size) {
    if (block_size > in_size) block_size = (uint32_t)bz3_bound(in_size);  // :877
    block_size = block_size <= (uint32_t)KiB65 ? (uint32_t)KiB65 : block_size;
    u32 n_blocks = (u32)(in_size / block_size);
    if (in_size % block_size) n_blocks++;
    FrameWindow w;
    if (!w.init(block_size, n_blocks)) return BZ3_ERR_INIT;  // :879-886 (allocation precedes the size check)
    const size_t buf_max = *out_size;
    *out_size = 0;
    if (buf_max < 13 || buf_max < bz3_bound(in_size)) return BZ3_ERR_DATA_TOO_BIG;
    memcpy(out, "BZ3v1", 5);
    wr_le32(out + 5, block_size);
    wr_le32(out + 9, n_blocks);
    *out_size += 13;
    size_t in_off = 0;
    const u32 W = (u32)w.states.size();
    std::vector<s32> sizes(W), orig(W);
    for (u32 i0 = 0; i0 < n_blocks; i0 += W) {
        const u32 cnt = n_blocks - i0 < W ? n_blocks - i0 : W;
        for (u32 k = 0; k < cnt; k++) {
            s32 size = (s32)block_size;
            if (i0 + k == n_blocks - 1) size = (s32)(in_size % block_size);  // (sic) :914 -- 0 when in_size is a multiple
            memcpy(w.bufs[k], in + in_off, (size_t)size);
            sizes[k] = orig[k] = size;
            in_off += (size_t)size;
        }
        bz3_encode_blocks(w.states.data(), w.bufs.data(), sizes.data(), (int32_t)cnt);
        for (u32 k = 0; k < cnt; k++) {
            if (bz3_last_error(w.states[k]) != BZ3_OK) return w.states[k]->last_error;  // :917-922
            const s32 osz = sizes[k];
            memcpy(out + *out_size + 8, w.bufs[k], (size_t)osz);
            wr_le32(out + *out_size, (u32)osz);
            wr_le32(out + *out_size + 4, (u32)orig[k]);
            *out_size += (size_t)osz + 8;
        }
    }
    return BZ3_OK;
}

BZIP3_API int bz3_decompress(const uint8_t * in, uint8_t * out, size_t in_size, size_t * out_size) {
    if (in_size < 13) return BZ3_ERR_MALFORMED_HEADER;
    if (memcmp(in, "BZ3v1", 5) != 0) return BZ3_ERR_MALFORMED_HEADER;
    const u32 block_size = rd_le32(in + 5);
    const u32 n_blocks = rd_le32(in + 9);
    in_size -= 13;
    in += 13;
    FrameWindow w;
    {
        // The header fields are untrusted: size the window from the chunks that are actually PRESENT -- walk the chunk
        // headers with the checks of the loop below and count the chunks that lie inside the input -- never from
        // n_blocks alone (a few hundred bytes claiming thousands of 511 MiB blocks must not allocate a window of states).
        size_t present = 0, off = 0;
        while (present < n_blocks && in_size - off >= 8) {
            const s32 size = (s32)rd_le32(in + off);
            if (size < 0 || (u32)size > block_size || in_size - off < (size_t)size + 8) break;
            off += (size_t)size + 8;
            present++;
        }
        if (!w.init(block_size, present ? present : 1)) return BZ3_ERR_INIT;  // :953-960
    }
    const size_t buf_max = *out_size;
    *out_size = 0;
    const u32 W = (u32)w.states.size();
    std::vector<s32> sizes(W), orig(W);
    std::vector<size_t> caps(W, w.cap);
    u32 i = 0;
    while (i < n_blocks) {
        // Collect chunks until the window is full or a chunk header is bad.  The reference would have decoded the
        // chunks before the bad one first, so they run (and may fail) before the header error is reported.
        u32 cnt = 0;
        int header_error = BZ3_OK;
        size_t planned = *out_size;
        while (cnt < W && i + cnt < n_blocks) {
            s32 size = 0, orig_size = 0;
            header_error = frame_chunk_check(in, in_size, block_size, buf_max, planned, &size, &orig_size);  // :963-985
            if (header_error != BZ3_OK) break;
            memcpy(w.bufs[cnt], in + 8, (size_t)size);
            sizes[cnt] = size;
            orig[cnt] = orig_size;
            planned += (size_t)orig_size;
            in += size + 8;
            in_size -= (size_t)size + 8;
            cnt++;
        }
        if (cnt) bz3_decode_blocks(w.states.data(), w.bufs.data(), caps.data(), sizes.data(), orig.data(), (int32_t)cnt);
        for (u32 k = 0; k < cnt; k++) {
            if (bz3_last_error(w.states[k]) != BZ3_OK) return w.states[k]->last_error;  // :989-993
            memcpy(out + *out_size, w.bufs[k], (size_t)orig[k]);
            *out_size += (size_t)orig[k];
        }
        if (header_error != BZ3_OK) return header_error;
        i += cnt;
    }
    return BZ3_OK;
}

BZIP3_API int bz3_orig_size_sufficient_for_decode(const uint8_t * block, size_t block_size, int32_t orig_size) {  // :1025-1055
    if (block_size < 9) return -1;
    const s32 bwt_idx = (s32)rd_le32(block + 4);
    if (bwt_idx == -1) return 1;
    const s32 model = (s8)block[8];
    const size_t need = 9 + (size_t)((model & 2) * 4) + (size_t)((model & 4) * 4);
    if (block_size < need) return -1;
    s32 lzp_size = -1, rle_size = -1;
    size_t off = 9;
    if (model & 2) { lzp_size = (s32)rd_le32(block + off); off += 4; }
    if (model & 4) rle_size = (s32)rd_le32(block + off);
    return sizes_fit((size_t)orig_size, lzp_size, rle_size, orig_size) ? 1 : 0;
}

}  // extern "C"

// An emulator build that lists api.hip as the layer's one source (test trees from before the split, tests/sanitize_emu.sh) gets the
// other units through it; tests/emu/build_emu.py compiles every unit on its own, as the product build does, and says so.
#if defined(BZ3_EMU) && !defined(BZ3_EMU_API_UNITS)
#include "api_context.hip"
#include "api_encode.hip"
#include "api_decode.hip"
#include "api_frames.hip"
#include "api_hooks.hip"
#endif
