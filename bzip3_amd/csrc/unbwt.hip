// unbwt.hip -- inverse Burrows-Wheeler transform on gfx950: one block, or up to UB_MAX_BATCH blocks through one launch sequence (bwt_inverse_batch).
// Replaces libsais_unbwt (reference include/libsais.h:5260-5262; init :4593-4617, decode :4618-4636),
// which builds a bigram psi table and then follows ONE dependent pointer chain of n/2 steps.
//
// Here:
//   1. psi is built by ONE stable radix pass (sort.hip) over the BWT bytes: the row of the k-th byte
//      (rows are 1-based around a virtual sentinel row inserted at `idx`; row 0 is the empty suffix)
//      is scattered to slot 1 + (stable rank by symbol); psi[0] = idx closes the cycle.
//      T[i] = F[psi^i(idx)], where F[row] is recovered from the 257-entry cumulative symbol table.
//   2. The single chain is cut at pseudo-random splitter rows (a multiplicative hash of the row
//      number, plus rows idx and 0).  One lane per splitter walks to the next splitter ONCE: it records
//      the segment length and parks the segment's text bytes in its slab (latency-bound, ~n/256-way
//      parallel random 4-byte reads, each of which fetches a 128-byte line).
//   3. The splitter list is ranked by pointer jumping (log2 rounds, tiny).
//   4. The parked bytes are copied to their now-known positions (16 lanes per segment); the few segments
//      longer than their slab are walked on from where the first walk left them.
//   5. Input that is NOT a genuine BWT (a corrupted block) must still decode to what the reference produces, because
//      the CRC / LZP / size checks that follow decide the error code.  psi(0) = idx puts rows 0 and idx on one
//      cycle, so the chain from idx always ends at row 0, after D <= n bytes (D = n for a genuine BWT); the text is
//      laid out from position 0 and k_ub_tail reproduces what the reference's bigram chase emits once it is stuck
//      on its zero-filled table entries (oracle/bz3_oracle.c orc_unbwt spells the rules out; pinned against the
//      reference on random inputs).
// HBM layout: psi u32[n+1], splitter-id u32[n+1], seven arrays of one word per splitter, slabs of 4 bytes per row.
// The host never learns the exact number of splitters: it sizes arrays and grids from ub_split_bound(), the kernels read the count
// from a device word, and nothing inside bwt_inverse waits for the stream.
// Algorithmic traffic: 11 B per byte; the walks are random 4-byte reads.
#include "prims.hpp"
#include "sort.hpp"
#include "stages.hpp"

#include <atomic>

namespace bz3 {

constexpr int UB_BLOCK = 256;
constexpr u32 UB_EVERY_ROW = 1u << 17;     // blocks of fewer rows: every row is a splitter
constexpr int UB_MIN_LOG_STRIDE = 3, UB_MAX_LOG_STRIDE = 8;

__device__ __forceinline__ bool ub_is_splitter(u32 row, u32 idx, int log_stride) {
    if (row == 0 || row == idx || log_stride == 0) return true;
    return ((row * 0x9E3779B1u) >> (32 - log_stride)) == 0u;
}

// How many splitters `rows` rows can have, known on the host without asking the device.  The hash is the golden-ratio multiplier:
// row * 0x9E3779B1 mod 2^32 is the low-discrepancy sequence {row * phi}, and the splitters are the rows that land in [0, 2^-log_stride).
// Such an interval holds rows * 2^-log_stride points to within a few (the discrepancy of the golden-ratio sequence grows with the
// logarithm of the number of points; counted exactly for rows from 2^17 + 1 to 2^27 + 1 and every stride from 3 to 8 it is within 3
// of rows >> log_stride: tests/test_unbwt_strides_emu.py).  Rows 0 and idx add at most two.  UB_BOUND_MARGIN entries on top.
// Every kernel clamps the device's count, and every splitter id it reads, to this bound: were it ever too small the transform would
// write wrong bytes (which the CRC check of the block catches), never outside its arrays.
constexpr u32 UB_BOUND_MARGIN = 64;
static inline u32 ub_split_bound(u32 rows, int log_stride) {
    if (log_stride == 0) return rows;
    const u64 b = ((u64)rows >> log_stride) + 2 + UB_BOUND_MARGIN;
    return b < rows ? (u32)b : rows;
}
// The splitter count as the kernels see it, and a splitter id as they may use it
__device__ __forceinline__ u32 ub_count(const u32 * __restrict__ d_total, u32 bound) {
    const u32 t = *d_total;
    return t < bound ? t : bound;
}
__device__ __forceinline__ u32 ub_sid(const u32 * __restrict__ sid, u32 row, u32 bound) {
    const u32 v = sid[row];
    return v < bound ? v : bound - 1;
}

// Every kernel takes a job table, BY VALUE as a kernel argument (a few hundred bytes: nothing of it has to outlive the call), and runs on a grid of
// (x = extent of the largest job, y = job): it picks its job by blockIdx.y and leaves where its index lies beyond its own job's extent.  Each job
// keeps its own stride, bound and slab size, because the rows differ.  One block is a batch of one, through the same kernels.  No kernel waits
// for another workgroup: batching adds a grid dimension and nothing else.
struct UbJob {
    const u8 * in;
    u8 * out;
    u32 n, idx, rows;
    int log_stride;
    u32 bound, cap;
    u32 *psi, *sid, *hist, *cum, *d_total, *split_row, *seg_len, *resume;
    u32 * succ[2];
    u32 * dist[2];
    u8 * slab;
};
struct UbBatch {
    u32 count;
    UbJob job[UB_MAX_BATCH];
};

// 64 bytes per thread, 16 at a time, every load of a group in flight before the first is counted (a grid-stride loop of single-byte
// loads is one exposed HBM round trip per byte: 1.2 ms for 256 MiB in round 2's profile; same pattern as bwt.hip k_bwt_sym_hist).
__global__ void __launch_bounds__(UB_BLOCK) k_ub_hist(UbBatch b) {
    const UbJob & J = b.job[blockIdx.y];
    const u8 * __restrict__ in = J.in;
    const u32 n = J.n;
    u32 * __restrict__ hist = J.hist;
    if ((u64)blockIdx.x * (UB_BLOCK * 64) >= n) return;
    __shared__ u32 bins[256];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * (UB_BLOCK * 64);
    const u64 last = (u64)n - 1;  // n >= 2 here
    for (u32 g = 0; g < 4; g++) {
        u8 c[16];
#pragma unroll
        for (u32 k = 0; k < 16; k++) {
            const u64 i = base + (u64)(g * 16 + k) * UB_BLOCK + threadIdx.x;
            c[k] = in[i < n ? i : last];
        }
#pragma unroll
        for (u32 k = 0; k < 16; k++) {
            const u64 i = base + (u64)(g * 16 + k) * UB_BLOCK + threadIdx.x;
            if (i < n) atomicAdd(&bins[c[k]], 1u);
        }
    }
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(&hist[threadIdx.x], bins[threadIdx.x]);
}

// cum[c] = 1 + number of bytes smaller than c; cum[256] = n + 1.  Also closes the cycle psi[0] = idx.
__global__ void __launch_bounds__(256) k_ub_cum(UbBatch b) {
    const UbJob & J = b.job[blockIdx.y];
    const u32 * __restrict__ hist = J.hist;
    u32 * __restrict__ cum = J.cum;
    u32 * __restrict__ psi = J.psi;
    const u32 idx = J.idx;
    __shared__ u32 lds[256 / WAVE + 1];
    u32 tot;
    u32 pre = block_excl_add<256>(hist[threadIdx.x], lds, tot);
    cum[threadIdx.x] = pre + 1;
    if (threadIdx.x == 0) {
        cum[256] = tot + 1;
        psi[0] = idx;
    }
}

__global__ void __launch_bounds__(UB_BLOCK) k_ub_flags(UbBatch b) {
    const UbJob & J = b.job[blockIdx.y];
    const u32 r = blockIdx.x * UB_BLOCK + threadIdx.x;
    if (r < J.rows) J.sid[r] = ub_is_splitter(r, J.idx, J.log_stride) ? 1u : 0u;
}

__global__ void __launch_bounds__(UB_BLOCK) k_ub_collect(UbBatch b) {
    const UbJob & J = b.job[blockIdx.y];
    const u32 r = blockIdx.x * UB_BLOCK + threadIdx.x;
    if (r < J.rows && ub_is_splitter(r, J.idx, J.log_stride)) {
        const u32 j = J.sid[r];
        if (j < J.bound) J.split_row[j] = r;
    }
}

// F[r], the first symbol of row r >= 1: largest symbol s with c[s] <= r (c = the 257 cumulative counts, in LDS).
__device__ __forceinline__ u32 ub_symbol_lds(const u32 * c, u32 r) {
    u32 lo = 0, hi = 256;
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const u32 mid = (lo + hi) >> 1;
        if (c[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// THE walk (round 3: it used to be two -- one for the lengths, one for the bytes -- and every step of either fetches a whole 128-byte
// line for one 4-byte word, 33 GB per walk of a 256 MiB block by the FETCH_SIZE counter: profiles/r03_pmc_fetch_stages_256MiB.txt).
// Every splitter walks to the next one ONCE: segment length, successor, and the text bytes of the segment, which cannot go to their
// place yet (the position is known after the list ranking) and are parked in the splitter's slab of `cap` bytes (cap = 4 x the mean
// segment length; the few longer segments leave the row they reached in `resume` and k_ub_walk_long finishes them).  Bytes are
// collected four at a time: one store per four steps.  The segment length goes to seg_len as well as to dist: the jumping rounds turn
// dist into the distance to the terminal, and k_ub_place needs both.
__global__ void __launch_bounds__(UB_BLOCK) k_ub_walk(UbBatch b) {
    const UbJob & J = b.job[blockIdx.y];
    const u32 bound = J.bound;
    if (blockIdx.x * UB_BLOCK >= bound) return;  // (the whole workgroup: before the barrier)
    const u32 * __restrict__ psi = J.psi;
    const u32 * __restrict__ sid = J.sid;
    const u32 * __restrict__ split_row = J.split_row;
    const u32 * __restrict__ d_total = J.d_total;
    const u32 * __restrict__ cum = J.cum;
    const u32 idx = J.idx, rows = J.rows, cap = J.cap;
    const int log_stride = J.log_stride;
    u32 * __restrict__ succ = J.succ[0];
    u32 * __restrict__ dist = J.dist[0];
    u32 * __restrict__ seg_len = J.seg_len;
    u8 * __restrict__ slab = J.slab;
    u32 * __restrict__ resume = J.resume;
    __shared__ u32 c[257];
    for (int k = threadIdx.x; k < 257; k += UB_BLOCK) c[k] = cum[k];
    __syncthreads();
    const u32 j = blockIdx.x * UB_BLOCK + threadIdx.x;
    if (j >= ub_count(d_total, bound)) return;
    u32 r = split_row[j];
    if (r == 0) {  // terminal of the list: row 0 is the empty suffix, nothing is emitted for it
        succ[j] = j;
        dist[j] = 0;
        seg_len[j] = 0;
        return;
    }
    u32 * __restrict__ mine = reinterpret_cast<u32 *>(slab + (size_t)j * cap);  // (cap is a multiple of 4)
    u32 len = 0, word = 0;
    do {
        const u32 nr = psi[r];  // issue the dependent load first; the symbol search overlaps it
        if (len < cap) {
            word |= ub_symbol_lds(c, r) << (8u * (len & 3u));
            if ((len & 3u) == 3u) {
                mine[len >> 2] = word;
                word = 0;
            }
        } else if (len == cap) {
            resume[j] = r;
        }
        r = nr;
        len++;
    } while (!ub_is_splitter(r, idx, log_stride) && len <= rows);
    if (len < cap && (len & 3u)) mine[len >> 2] = word;  // the last, partial word
    succ[j] = ub_sid(sid, r, bound);
    dist[j] = len;
    seg_len[j] = len;
}

// One pointer-jumping round: dist = distance to the terminal, succ = 2^k-th successor.  cur: which of the two buffers holds the list (the same
// for every job: all of them run every round of the longest list, and a round past a list's own need leaves it as it is).
__global__ void __launch_bounds__(UB_BLOCK) k_ub_jump(UbBatch b, int cur) {
    const UbJob & J = b.job[blockIdx.y];
    const u32 * __restrict__ succ_in = J.succ[cur];
    const u32 * __restrict__ dist_in = J.dist[cur];
    u32 * __restrict__ succ_out = J.succ[cur ^ 1];
    u32 * __restrict__ dist_out = J.dist[cur ^ 1];
    const u32 j = blockIdx.x * UB_BLOCK + threadIdx.x;
    if (j >= ub_count(J.d_total, J.bound)) return;
    const u32 sj = succ_in[j];
    u64 d = (u64)dist_in[j] + dist_in[sj];
    dist_out[j] = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)d;
    succ_out[j] = succ_in[sj];
}

// After the list ranking: the parked bytes of every segment go to their place.  16 lanes per segment, 16 bytes per lane and trip
// (the slab is aligned, the destination is not: 128-bit stores at any byte address).  seg_len: the walk's segment lengths.
__global__ void __launch_bounds__(UB_BLOCK) k_ub_place(UbBatch b, int cur) {
    const UbJob & J = b.job[blockIdx.y];
    const u8 * __restrict__ slab = J.slab;
    const u32 * __restrict__ seg_len = J.seg_len;
    const u32 * __restrict__ dist = J.dist[cur];
    const u32 * __restrict__ succ = J.succ[cur];
    const u32 * __restrict__ sid = J.sid;
    const u32 * __restrict__ d_total = J.d_total;
    const u32 idx = J.idx, cap = J.cap, bound = J.bound, n = J.n;
    u8 * __restrict__ out = J.out;
    const u32 t = blockIdx.x * UB_BLOCK + threadIdx.x;
    const u32 j = t >> 4, part = t & 15u;
    if (j >= ub_count(d_total, bound)) return;
    // On the chain idx -> ... -> row 0?  After the jumping rounds every chain element points at the terminal; splitters
    // of other cycles (corrupt input only) never do.  D = bytes on the chain (n for a genuine BWT).
    if (succ[j] != sid[0]) return;
    const u32 D = dist[ub_sid(sid, idx, bound)];
    const u32 d = dist[j];
    if (d > D) return;
    const u32 len = seg_len[j];
    const u32 m = len < cap ? len : cap;
    const u32 limit = n & ~1u;  // the reference's loop writes 2 * (n / 2) bytes, then U[n-1] separately (:5155)
    const u64 pos0 = (u64)D - d;
    const u8 * __restrict__ src = slab + (size_t)j * cap;
    for (u32 o = part * 16u; o < m; o += 256u) {
        if (o + 16u <= m && pos0 + o + 16u <= limit) {
            const uint4 q = *reinterpret_cast<const uint4 *>(src + o);
            PackedU128 w;
            w.v[0] = q.x; w.v[1] = q.y; w.v[2] = q.z; w.v[3] = q.w;
            *reinterpret_cast<PackedU128 *>(out + pos0 + o) = w;
        } else {
            for (u32 k = o; k < m && k < o + 16u; k++)
                if (pos0 + k < limit) out[pos0 + k] = src[k];
        }
    }
}

// The segments that did not fit their slab (longer than 4 x the mean: ~2 % of them, ~9 % of the rows) are walked on from the row
// the first walk left in `resume`, their bytes going straight to their place.
__global__ void __launch_bounds__(UB_BLOCK) k_ub_walk_long(UbBatch b, int cur) {
    const UbJob & J = b.job[blockIdx.y];
    const u32 bound = J.bound;
    if (blockIdx.x * UB_BLOCK >= bound) return;  // (the whole workgroup: before the barrier)
    const u32 * __restrict__ psi = J.psi;
    const u32 * __restrict__ resume = J.resume;
    const u32 * __restrict__ seg_len = J.seg_len;
    const u32 * __restrict__ dist = J.dist[cur];
    const u32 * __restrict__ succ = J.succ[cur];
    const u32 * __restrict__ sid = J.sid;
    const u32 * __restrict__ cum = J.cum;
    const u32 * __restrict__ d_total = J.d_total;
    const u32 idx = J.idx, cap = J.cap, n = J.n;
    u8 * __restrict__ out = J.out;
    __shared__ u32 c[257];
    for (int k = threadIdx.x; k < 257; k += UB_BLOCK) c[k] = cum[k];
    __syncthreads();
    const u32 j = blockIdx.x * UB_BLOCK + threadIdx.x;
    if (j >= ub_count(d_total, bound)) return;
    const u32 len = seg_len[j];
    if (len <= cap) return;
    if (succ[j] != sid[0]) return;
    const u32 D = dist[ub_sid(sid, idx, bound)];
    const u32 d = dist[j];
    if (d > D) return;
    const u32 limit = n & ~1u;
    u32 r = resume[j];
    u64 pos = (u64)D - d + cap;
    for (u32 t = cap; t < len; t++) {
        const u32 nr = psi[r];
        const u32 sym = ub_symbol_lds(c, r);
        if (pos < limit) out[pos] = (u8)sym;
        pos++;
        r = nr;
    }
}

__device__ __forceinline__ u32 ub_first_symbol(const u32 * __restrict__ cum, u32 r) {  // F[r], r >= 1
    u32 lo = 0, hi = 256;
    for (int b = 0; b < 8; b++) {
        const u32 mid = (lo + hi) >> 1;
        if (cum[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// What the reference leaves behind the chain (nothing for a genuine BWT, where D = n), and U[n-1] = first BWT byte.
// Rules and their derivation from include/libsais.h:4534-4636: oracle/bz3_oracle.c, orc_unbwt.
__global__ void __launch_bounds__(UB_BLOCK) k_ub_tail(UbBatch b, int cur) {
    const UbJob & J = b.job[blockIdx.y];
    const u8 * __restrict__ in = J.in;
    const u32 * __restrict__ psi = J.psi;
    const u32 * __restrict__ cum = J.cum;
    const u32 * __restrict__ dist = J.dist[cur];
    const u32 * __restrict__ sid = J.sid;
    const u32 idx = J.idx, bound = J.bound, n = J.n;
    u8 * __restrict__ out = J.out;
    const u32 D = dist[ub_sid(sid, idx, bound)];
    const u32 limit = n & ~1u;
    const u32 lastc = in[0];
    const u32 E = cum[lastc];  // row of the suffix that is the last character alone = LF(0)
    const u32 gid = blockIdx.x * UB_BLOCK + threadIdx.x;
    u32 start = D;
    if (D < limit && (D & 1u)) {  // E was hit on an even step of the bigram chase
        int shift = 0;
        while ((n >> shift) > (1u << 17)) shift++;
        const bool same_group = E >= 2 && ((E - 1) >> shift) == (E >> shift);
        if (gid == 0) {
            if (same_group || E + 1 > n) {
                out[D] = 0;
            } else {
                out[D - 1] = (u8)ub_first_symbol(cum, E + 1);
                out[D] = (u8)ub_first_symbol(cum, psi[E + 1]);
            }
        }
        start = D + 1;
    }
    if (start < limit) {  // stuck at table entry 0: the bigram of the first non-empty bucket, over and over
        const u32 q0 = (E == 1) ? 2u : 1u;
        const u32 hi = ub_first_symbol(cum, q0), lo = ub_first_symbol(cum, psi[q0]);
        for (u64 j = (u64)start + gid; j < limit; j += (u64)gridDim.x * UB_BLOCK)
            if (j != n - 1) out[j] = (u8)((j & 1u) ? lo : hi);  // U[n-1] belongs to thread 0 below
    }
    if (gid == 0) out[n - 1] = (u8)lastc;
}

// psi, splitter ids, the sorter's and the scans' scratch, seven splitter arrays of ub_split_bound() entries, the slabs (4 bytes per row and a
// margin).  The rule below never picks a stride under 8 rows for a block of 2^17 rows or more (every row is a splitter below that), whatever
// the lane target, so the formula depends on n alone: 17 bytes per byte of a large block, against the 60 of the forward transform, which every
// caller's arena is sized for (api_internal.hpp workspace_bytes_for) -- that is also what a stride FORCED below 8 rows (tests) draws on: 40.
size_t unbwt_workspace_bytes(u64 n) {
    const u64 rows = n + 1;
    const u64 splitters = rows < UB_EVERY_ROW ? rows : (rows >> UB_MIN_LOG_STRIDE) + 2 + UB_BOUND_MARGIN;
    return (n + 64) * 8 + radix_temp_bytes(n) + scan_temp_words(n + 1) * 4 + (splitters + 4096) * 32 + (n + (n >> 3)) * 4 + (1u << 20);
}

// tests and the stride sweep: -1 = the rule, 0..8 = that log2(stride) for every block
static std::atomic<int> g_ub_force_log_stride{-1};
void unbwt_set_log_stride(int v) { g_ub_force_log_stride.store(v >= 0 && v <= UB_MAX_LOG_STRIDE ? v : -1); }

// The lanes the device keeps resident: UNBWT_LANES_PER_CU on each of its CUs (asked of the runtime once per device).
static u32 ub_device_lanes() {
    static std::atomic<u32> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    u32 v = cached[dev].load();
    if (v == 0) {
        int cus = 0;
#ifndef BZ3_EMU
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
#endif
        if (cus <= 0) cus = 256;
        v = (u32)cus * UNBWT_LANES_PER_CU;
        cached[dev].store(v);
    }
    return v;
}

// One splitter per 2^log_stride rows.  Segment lengths are geometric (splitters are a hash of the row number), every lane walks its whole
// segment, and the walk is one dependent load after the other (an Infinity Cache hit at best: ~230 ns), so a launch lasts as long as its LONGEST
// segment: stride x ln(number of segments) round trips -- as long as every lane is resident at once.  More lanes than the device holds
// (2048 per CU: 32 waves) run in turns instead, and more splitters mean a longer list to rank and more slab words to place.  So: the smallest
// stride whose lanes the device still keeps resident.  Rounds 2 to 6 kept 65,536 to 131,072 splitters at every size (4 to 8 of a CU's 32 wave
// slots, 750 to 1,400 steps for an 8 MiB block); that rule was tuned on 256 MiB blocks alone, which take the largest stride under either.
int unbwt_log_stride(u32 rows, u32 lanes) {
    const int forced = g_ub_force_log_stride.load();
    if (forced >= 0) return forced;
    if (rows < UB_EVERY_ROW) return 0;
    int log_stride = UB_MIN_LOG_STRIDE;
    while (log_stride < UB_MAX_LOG_STRIDE && ((u64)rows >> log_stride) > lanes) log_stride++;
    return log_stride;
}

// What one job takes from the arena at a given stride, rounding of the allocator included.  At the strides the rule picks it stays under
// unbwt_workspace_bytes; a stride forced below 8 rows (tests) needs more.
static size_t ub_job_bytes(u64 n, int log_stride) {
    const u64 rows = n + 1;
    const u64 bound = ub_split_bound((u32)rows, log_stride);
    return rows * 8 + radix_temp_bytes(n) + scan_temp_words(rows) * 4 + bound * 28 + bound * (4u << log_stride) + (1u << 16);
}

// How many of the first `count` jobs go into one pass: the largest b <= UB_MAX_BATCH for which b workspaces of the largest job fit into
// `arena_free` bytes and b x (rows >> UB_MAX_LOG_STRIDE) lanes -- the fewest splitters the rule ever gives that job -- are lanes the stream
// keeps resident.  A block of 256 MiB therefore goes alone, with the launch sequence of a single block; blocks of 8 MiB go four at a time.
size_t unbwt_batch_workspace_bytes(u64 n, u32 b) {
    size_t each = unbwt_workspace_bytes(n);
    const int forced = g_ub_force_log_stride.load();
    if (forced >= 0 && ub_job_bytes(n, forced) > each) each = ub_job_bytes(n, forced);
    return each * b;
}

u32 unbwt_batch_size(const u32 * n, u32 count, size_t arena_free, u32 lanes) {
    if (count <= 1) return count;
    if (lanes == 0) lanes = ub_device_lanes();
    u32 b = 1;
    u64 largest = n[0];
    while (b < count && b < UB_MAX_BATCH) {
        const u64 big = n[b] > largest ? n[b] : largest;
        if (unbwt_batch_workspace_bytes(big, b + 1) > arena_free || (u64)(b + 1) * ((big + 1) >> UB_MAX_LOG_STRIDE) > lanes) break;
        largest = big;
        b++;
    }
    return b;
}

// Nothing in here waits for the stream: the host sizes arrays and grids from ub_split_bound() instead of reading the splitter count back, and the
// scratch goes back to the arena when the function returns, with its kernels still in flight.  That is sound because an arena belongs to one
// stream at a time: whoever takes the same bytes next launches on `s` as well, so its kernels queue behind these -- the argument of
// encode_front_b for the suffix sorter's scratch.  The callers wait for the stream right after the call, for reasons of their own
// (decode_group: see there; the hooks read the text back).
// A fixed launch sequence, whatever the data: `count` blocks go through it together, one launch per step.  Every item has n >= 2 and 0 < idx <= n.
void bwt_inverse_batch(const UbBatchItem * items, u32 count, Arena & tmp, hipStream_t s, u32 lanes) {
    if (count == 0) return;
    if (count > UB_MAX_BATCH) throw HipError{hipErrorUnknown, "inverse BWT batch of more blocks than the job table holds", __FILE__, __LINE__};
    const size_t mk = tmp.mark();
    if (lanes == 0) lanes = ub_device_lanes();
    UbBatch b;
    b.count = count;
    u32 * hists = tmp.take<u32>((size_t)256 * count);  // (one piece: one memset)
    u32 most_n = 0, most_rows = 0, most_bound = 0;
    RadixIotaJob rj[UB_MAX_BATCH];
    u32 * sids[UB_MAX_BATCH];
    u32 * totals[UB_MAX_BATCH];
    u64 lens[UB_MAX_BATCH];
    for (u32 k = 0; k < count; k++) {
        UbJob & J = b.job[k];
        if (items[k].n < 2) throw HipError{hipErrorUnknown, "inverse BWT batch with a block of fewer than 2 bytes", __FILE__, __LINE__};
        J.in = items[k].in;
        J.out = items[k].out;
        J.n = items[k].n;
        J.idx = items[k].idx;
        J.rows = J.n + 1;
        J.log_stride = unbwt_log_stride(J.rows, lanes);
        J.bound = ub_split_bound(J.rows, J.log_stride);
        J.cap = 4u << J.log_stride;  // bytes per slab: 4 x the mean segment length (splitters are one row in 2^log_stride)
        J.psi = tmp.take<u32>(J.rows);
        J.sid = tmp.take<u32>(J.rows);
        J.hist = hists + (size_t)256 * k;
        J.cum = tmp.take<u32>(257);
        J.d_total = tmp.take<u32>(1);
        most_n = J.n > most_n ? J.n : most_n;
        most_rows = J.rows > most_rows ? J.rows : most_rows;
        most_bound = J.bound > most_bound ? J.bound : most_bound;
        rj[k] = RadixIotaJob{J.in, J.psi, J.n, J.idx};
        sids[k] = J.sid;
        totals[k] = J.d_total;
        lens[k] = J.rows;
    }
    // 1. psi by one stable radix pass: value of byte k is its row k + (k >= idx), destination base 1
    HIP_CHECK(hipMemsetAsync(hists, 0, (size_t)256 * 4 * count, s));
    // (the entries past `count` repeat the first job until step 2 has filled the real ones: no uninitialised bytes in a kernel argument)
    for (u32 k = 0; k < UB_MAX_BATCH; k++) {
        UbJob & J = b.job[k];
        if (k >= count) J = b.job[0];
        J.split_row = J.seg_len = J.resume = J.succ[0] = J.succ[1] = J.dist[0] = J.dist[1] = nullptr;
        J.slab = nullptr;
    }
    launch(k_ub_hist, dim3((u32)(((u64)most_n + UB_BLOCK * 64 - 1) / (UB_BLOCK * 64)), count), dim3(UB_BLOCK), 0, s, b);
    launch(k_ub_cum, dim3(1, count), dim3(256), 0, s, b);
    radix_pass_iota_u8_many(rj, count, 1u, tmp, s);

    // 2. splitters: ids by a scan of the flags (the exact count stays in d_total), then THE walk
    const dim3 grows((most_rows + UB_BLOCK - 1) / UB_BLOCK, count);
    launch(k_ub_flags, grows, dim3(UB_BLOCK), 0, s, b);
    exclusive_scan_u32_many(sids, lens, totals, count, tmp, s);
    for (u32 k = 0; k < count; k++) {
        UbJob & J = b.job[k];
        J.split_row = tmp.take<u32>(J.bound);
        J.seg_len = tmp.take<u32>(J.bound);
        J.resume = tmp.take<u32>(J.bound);
        J.succ[0] = tmp.take<u32>(J.bound);
        J.succ[1] = tmp.take<u32>(J.bound);
        J.dist[0] = tmp.take<u32>(J.bound);
        J.dist[1] = tmp.take<u32>(J.bound);
        J.slab = tmp.take<u8>((size_t)J.bound * J.cap + 64);
    }
    for (u32 k = count; k < UB_MAX_BATCH; k++) b.job[k] = b.job[0];
    const dim3 gs((most_bound + UB_BLOCK - 1) / UB_BLOCK, count);
    launch(k_ub_collect, grows, dim3(UB_BLOCK), 0, s, b);
    launch(k_ub_walk, gs, dim3(UB_BLOCK), 0, s, b);

    // 3. rank the splitter lists: 2^rounds >= the largest bound >= every list's length (the terminal points at itself with distance 0: further
    // rounds change nothing, so a shorter list sits through the longest one's rounds unchanged)
    int cur = 0;
    for (u64 span = 1; span < most_bound; span <<= 1) {
        launch(k_ub_jump, gs, dim3(UB_BLOCK), 0, s, b, cur);
        cur ^= 1;
    }
    // 4. the parked bytes to their places, the long segments' rest straight there
    launch(k_ub_place, dim3((u32)(((u64)most_bound * 16 + UB_BLOCK - 1) / UB_BLOCK), count), dim3(UB_BLOCK), 0, s, b, cur);
    launch(k_ub_walk_long, gs, dim3(UB_BLOCK), 0, s, b, cur);
    launch(k_ub_tail, dim3(256, count), dim3(UB_BLOCK), 0, s, b, cur);
    tmp.release(mk);
}

void bwt_inverse(const u8 * d_in, u32 n, u32 idx, u8 * d_out, Arena & tmp, hipStream_t s, u32 lanes) {
    if (n == 0) return;
    if (n == 1) {
        HIP_CHECK(hipMemcpyAsync(d_out, d_in, 1, hipMemcpyDeviceToDevice, s));
        return;
    }
    const UbBatchItem one{d_in, d_out, n, idx};
    bwt_inverse_batch(&one, 1, tmp, s, lanes);
}

}  // namespace bz3
