// sort.hip -- device-wide exclusive scan + stable 8-bit-digit LSD radix sort for gfx950.
//
// Radix pass = three kernels (all HBM-streaming, no MFMA: byte/integer work):
//   k_rs_hist    : per-tile digit histogram, LDS-binned, written digit-major  hist[d * tiles + t]
//   scan         : device-wide exclusive scan of the digit-major table => global offset of every
//                  (digit, tile) bucket
//   k_rs_scatter : re-reads the tile, ranks each key among equal digits with wave64 ballots
//                  (match-any over the 8 digit bits + popcount below the lane), adds the per-wave
//                  running counts kept in LDS, orders the tile by digit in LDS and writes key+value out in runs.  The
//                  tile is walked wave-striped (wave w owns keys [1024w, 1024w+1024), 16 rounds of
//                  64 consecutive keys) so the order of equal digits is preserved: the pass is stable.
// Algorithmic traffic per pass and element: sizeof(K) (hist) + sizeof(K)+4 (read) + sizeof(K)+4 (write).
//
// Memory-level parallelism (round 2, found in the ISA): a load written as `if (i < n) x = p[i]` inside an unrolled loop compiles to
// a branch around the load and an `s_waitcnt vmcnt(0)` before its first use, i.e. ONE load in flight per wave and one exposed HBM
// round trip per round -- 16 (+16 for the values) per tile in the first version of k_rs_scatter, which is what held it at
// ~1 TB/s.  Every streaming kernel here therefore issues ALL loads of its tile first, branch-free (the index is clamped to n-1
// and the lane masked afterwards), and only then starts to consume them.
#include "prims.hpp"
#include "sort.hpp"

namespace bz3 {

// ---------------------------------------------------------------------------------------------
// exclusive scan
// ---------------------------------------------------------------------------------------------
constexpr int SC_BLOCK = 256;
constexpr int SC_ITEMS = 8;
constexpr int SC_TILE = SC_BLOCK * SC_ITEMS;

// The SC_ITEMS consecutive values of a thread: two 16-byte loads when the tile is whole and aligned, clamped scalar loads (all in
// flight together, see the note on memory-level parallelism above) otherwise.  Values past n read as 0.
__device__ __forceinline__ void scan_load_items(const u32 * __restrict__ data, u64 n, u64 base, u32 (&v)[SC_ITEMS]) {
    static_assert(SC_ITEMS == 8, "two uint4 per thread");
    if (base + SC_ITEMS <= n && (reinterpret_cast<uintptr_t>(data) & 15u) == 0) {
        const uint4 a = *reinterpret_cast<const uint4 *>(data + base);
        const uint4 b = *reinterpret_cast<const uint4 *>(data + base + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        const u64 last = n - 1;  // n >= 1: the scan is never launched on nothing
#pragma unroll
        for (int k = 0; k < SC_ITEMS; k++) v[k] = data[base + k < n ? base + k : last];
#pragma unroll
        for (int k = 0; k < SC_ITEMS; k++) v[k] = base + k < n ? v[k] : 0u;
    }
}

// The kernels' bodies are __device__ functions of the tile (`bx`): the single form runs them on blockIdx.x, the batched form (further down:
// several independent tables in one launch, grid.y = table) on the same index after it has picked its table by blockIdx.y.
__device__ __forceinline__ void scan_reduce_body(const u32 * __restrict__ data, u64 n, u32 * __restrict__ sums, u32 bx) {
    __shared__ u32 lds[SC_BLOCK / WAVE + 1];
    const u64 base = (u64)bx * SC_TILE + (u64)threadIdx.x * SC_ITEMS;
    u32 v[SC_ITEMS];
    scan_load_items(data, n, base, v);
    u32 acc = 0;
#pragma unroll
    for (int k = 0; k < SC_ITEMS; k++) acc += v[k];
    u32 tot = block_sum<SC_BLOCK>(acc, lds);
    if (threadIdx.x == 0) sums[bx] = tot;
}
__global__ void __launch_bounds__(SC_BLOCK) k_scan_reduce(const u32 * __restrict__ data, u64 n, u32 * __restrict__ sums) {
    scan_reduce_body(data, n, sums, blockIdx.x);
}

// Local exclusive scan of one tile; `sums` (may be null) holds the exclusive prefix of every tile.  one_tile: the table is this tile alone.
__device__ __forceinline__ void scan_apply_body(u32 * __restrict__ data, u64 n, const u32 * __restrict__ sums, u32 * __restrict__ total_out, u32 bx,
                                                bool one_tile) {
    __shared__ u32 lds[SC_BLOCK / WAVE + 1];
    const u64 base = (u64)bx * SC_TILE + (u64)threadIdx.x * SC_ITEMS;
    u32 v[SC_ITEMS];
    scan_load_items(data, n, base, v);
    u32 acc = 0;
#pragma unroll
    for (int k = 0; k < SC_ITEMS; k++) acc += v[k];
    u32 tot;
    u32 pre = block_excl_add<SC_BLOCK>(acc, lds, tot);
    if (sums) pre += sums[bx];
    if (base + SC_ITEMS <= n && (reinterpret_cast<uintptr_t>(data) & 15u) == 0) {
        uint4 a, b;
        a.x = pre; a.y = a.x + v[0]; a.z = a.y + v[1]; a.w = a.z + v[2];
        b.x = a.w + v[3]; b.y = b.x + v[4]; b.z = b.y + v[5]; b.w = b.z + v[6];
        *reinterpret_cast<uint4 *>(data + base) = a;
        *reinterpret_cast<uint4 *>(data + base + 4) = b;
    } else {
#pragma unroll
        for (int k = 0; k < SC_ITEMS; k++) {
            if (base + k < n) data[base + k] = pre;
            pre += v[k];
        }
    }
    if (total_out && one_tile && threadIdx.x == 0) *total_out = tot;
}
__global__ void __launch_bounds__(SC_BLOCK) k_scan_apply(u32 * __restrict__ data, u64 n, const u32 * __restrict__ sums,
                                                         u32 * __restrict__ total_out) {
    scan_apply_body(data, n, sums, total_out, blockIdx.x, gridDim.x == 1);
}

__global__ void k_add_last(const u32 * __restrict__ sums_excl, const u32 * __restrict__ last_tile_total, u32 * out) {
    // total = exclusive prefix of the last tile + that tile's own sum
    *out = *sums_excl + *last_tile_total;
}

// Mid-sized tables in ONE launch (round 5): a workgroup of 1024, every thread a contiguous chunk of the table (16-byte accesses; a thread's lines are
// reused from L1 / L2 across its iterations), one workgroup scan over the chunk sums.  Up to 256 Ki words -- the count table of a radix pass of up to
// 1024 tiles (4 Mi keys) -- this replaces reduce + apply(1 tile) + apply: three launches of ~10 us with their gaps, of which the sorter's ~40 mid-sized
// passes per block paid ~1.5 ms (profiles/r05_call6_kernels_*: 123 k_scan_apply + 68 k_scan_reduce launches per 256 MiB block).
constexpr int SC1_BLOCK = 1024;
constexpr u64 SC1_MAX = 262144;
__device__ __forceinline__ void scan_single_body(u32 * __restrict__ data, u64 n, u32 * __restrict__ total_out) {
    __shared__ u32 lds[SC1_BLOCK / WAVE + 1];
    const u64 quads = (n + 3) / 4;                                  // the table in groups of four words
    const u64 per = (quads + SC1_BLOCK - 1) / SC1_BLOCK;            // groups per thread
    const u64 q0 = (u64)threadIdx.x * per, q1 = q0 + per < quads ? q0 + per : quads;
    const bool vec = (reinterpret_cast<uintptr_t>(data) & 15u) == 0;
    auto load4 = [&](u64 q, u32 (&v)[4]) {
        if (vec && 4 * q + 4 <= n) {
            const uint4 a = *reinterpret_cast<const uint4 *>(data + 4 * q);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = 4 * q + k < n ? data[4 * q + k] : 0u;
        }
    };
    u32 acc = 0;
    for (u64 q = q0; q < q1; q++) {
        u32 v[4];
        load4(q, v);
        acc += v[0] + v[1] + v[2] + v[3];
    }
    u32 tot;
    u32 run = block_excl_add<SC1_BLOCK>(acc, lds, tot);
    for (u64 q = q0; q < q1; q++) {
        u32 v[4];
        load4(q, v);
        u32 o[4];
        o[0] = run; o[1] = o[0] + v[0]; o[2] = o[1] + v[1]; o[3] = o[2] + v[2];
        run = o[3] + v[3];
        if (vec && 4 * q + 4 <= n) {
            *reinterpret_cast<uint4 *>(data + 4 * q) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (4 * q + k < n) data[4 * q + k] = o[k];
        }
    }
    if (total_out && threadIdx.x == 0) *total_out = tot;
}
__global__ void __launch_bounds__(SC1_BLOCK) k_scan_single(u32 * __restrict__ data, u64 n, u32 * __restrict__ total_out) {
    scan_single_body(data, n, total_out);
}

// (experiments: the recursive scan for every size, as up to round 4; read once)
static bool scan_no_single() {
    static const bool v = getenv("BZ3_SCAN_NO_SINGLE") != nullptr;
    return v;
}

static void scan_rec(u32 * d, u64 n, u32 * d_total, Arena & tmp, hipStream_t s) {
    if (n == 0) {
        if (d_total) HIP_CHECK(hipMemsetAsync(d_total, 0, 4, s));
        return;
    }
    if (n <= SC_TILE) {
        launch(k_scan_apply, dim3(1), dim3(SC_BLOCK), 0, s, d, n, (const u32 *)nullptr, d_total);
        return;
    }
    if (n <= SC1_MAX && !scan_no_single()) {
        launch(k_scan_single, dim3(1), dim3(SC1_BLOCK), 0, s, d, n, d_total);
        return;
    }
    const u64 tiles = (n + SC_TILE - 1) / SC_TILE;
    size_t m = tmp.mark();
    u32 * sums = tmp.take<u32>(tiles + 1);
    launch(k_scan_reduce, dim3((u32)tiles), dim3(SC_BLOCK), 0, s, (const u32 *)d, n, sums);
    scan_rec(sums, tiles, d_total, tmp, s);  // d_total = sum of all tile sums = grand total
    launch(k_scan_apply, dim3((u32)tiles), dim3(SC_BLOCK), 0, s, d, n, (const u32 *)sums, (u32 *)nullptr);
    tmp.release(m);
}

void exclusive_scan_u32(u32 * d_data, u64 n, u32 * d_total, Arena & tmp, hipStream_t s) { scan_rec(d_data, n, d_total, tmp, s); }

// ---- several tables in one launch per step -------------------------------------------------------------------------------------------
// The job table travels by value, as a kernel argument; grid = (tiles of the longest table, table), and a workgroup whose tile lies
// beyond its own table leaves at once.  The path (one tile / one workgroup / recursive) is the longest table's; every kernel works on
// its own table's length, however short.
struct ScanBatch {
    u32 count;
    struct Job {
        u32 * data;
        u32 * sums;   // k_scan_reduce_many writes them, k_scan_apply_many reads them (null: none)
        u32 * total;  // may be null
        u64 n;        // >= 1
    } job[SORT_MAX_BATCH];
};
static_assert(sizeof(ScanBatch) <= KERNEL_TABLE_BYTES, "job table too large for a by-value kernel argument");
__global__ void __launch_bounds__(SC_BLOCK) k_scan_reduce_many(ScanBatch b) {
    const ScanBatch::Job & j = b.job[blockIdx.y];
    if ((u64)blockIdx.x * SC_TILE >= j.n) return;
    scan_reduce_body(j.data, j.n, j.sums, blockIdx.x);
}
__global__ void __launch_bounds__(SC_BLOCK) k_scan_apply_many(ScanBatch b) {
    const ScanBatch::Job & j = b.job[blockIdx.y];
    if ((u64)blockIdx.x * SC_TILE >= j.n) return;
    scan_apply_body(j.data, j.n, j.sums, j.total, blockIdx.x, j.n <= (u64)SC_TILE);
}
__global__ void __launch_bounds__(SC1_BLOCK) k_scan_single_many(ScanBatch b) {
    const ScanBatch::Job & j = b.job[blockIdx.y];
    scan_single_body(j.data, j.n, j.total);
}

static void scan_rec_many(ScanBatch b, Arena & tmp, hipStream_t s) {
    u64 longest = 0;
    for (u32 k = 0; k < b.count; k++) longest = b.job[k].n > longest ? b.job[k].n : longest;
    for (u32 k = 0; k < b.count; k++) b.job[k].sums = nullptr;
    if (longest <= SC_TILE) {
        launch(k_scan_apply_many, dim3(1, b.count), dim3(SC_BLOCK), 0, s, b);
        return;
    }
    if (longest <= SC1_MAX && !scan_no_single()) {
        launch(k_scan_single_many, dim3(1, b.count), dim3(SC1_BLOCK), 0, s, b);
        return;
    }
    const u32 tiles = (u32)((longest + SC_TILE - 1) / SC_TILE);
    size_t m = tmp.mark();
    ScanBatch sub = b, top = b;
    for (u32 k = 0; k < b.count; k++) {
        const u64 t = (b.job[k].n + SC_TILE - 1) / SC_TILE;
        u32 * sums = tmp.take<u32>(t + 1);
        top.job[k].sums = sums;
        top.job[k].total = nullptr;  // the grand total comes out of the scan of the tile sums
        sub.job[k].data = sums;
        sub.job[k].n = t;
    }
    launch(k_scan_reduce_many, dim3(tiles, b.count), dim3(SC_BLOCK), 0, s, top);
    scan_rec_many(sub, tmp, s);
    launch(k_scan_apply_many, dim3(tiles, b.count), dim3(SC_BLOCK), 0, s, top);
    tmp.release(m);
}

void exclusive_scan_u32_many(u32 * const * d_data, const u64 * n, u32 * const * d_totals, u32 count, Arena & tmp, hipStream_t s) {
    if (count == 0 || count > SORT_MAX_BATCH) throw HipError{hipErrorUnknown, "scan batch of a size the job table does not hold", __FILE__, __LINE__};
    ScanBatch b;
    b.count = count;
    for (u32 k = 0; k < SORT_MAX_BATCH; k++) {
        const u32 j = k < count ? k : 0;  // (unused entries repeat the first: no uninitialised bytes in the argument)
        if (n[j] == 0) throw HipError{hipErrorUnknown, "scan batch with an empty table", __FILE__, __LINE__};
        b.job[k] = ScanBatch::Job{d_data[j], nullptr, d_totals ? d_totals[j] : nullptr, n[j]};
    }
    scan_rec_many(b, tmp, s);
}

// ---------------------------------------------------------------------------------------------
// radix pass
// ---------------------------------------------------------------------------------------------
constexpr int RS_WAVES = RS_BLOCK / WAVE;          // 4
constexpr int RS_ROUNDS = RS_TILE / RS_BLOCK;      // 16 rounds of 64 keys per wave
constexpr int RS_WAVE_SPAN = RS_TILE / RS_WAVES;   // 1024 keys per wave

// XCD-aware tile assignment.  The dispatcher places workgroup b on XCD b % 8 (observed, MI355X_MICROARCH.md "Workgroup dispatch"; a
// speed assumption only: every tile is processed exactly once whatever the placement), and every XCD has its own L2.  A radix
// scatter writes ~16 keys of a tile to each of 256 bucket regions; the tiles that fill the neighbouring bytes of a cache line are
// the NEXT tiles.  With tile = blockIdx they sit on the other seven XCDs and every L2 writes its partial lines back on its own
// (measured in round 1: 4.6x write amplification); with a contiguous range of tiles per XCD they merge in one L2.
// The grid is 8 * ceil(tiles / 8) workgroups; the padded ones (tile >= tiles) leave at once.
__device__ __forceinline__ u32 rs_tile_of_block(u32 b, u32 tiles, bool xcd) {
    if (!xcd) return b;
    const u32 per = (tiles + 7u) / 8u;
    return (b & 7u) * per + (b >> 3);
}
__host__ __device__ inline u32 rs_grid(u32 tiles, bool xcd) { return xcd ? 8u * ((tiles + 7u) / 8u) : tiles; }

template <typename K, int BITS>
__device__ __forceinline__ u32 rs_digit(K key, int shift) {
    return (u32)(key >> shift) & ((1u << BITS) - 1u);
}

// BITS = digit width: 8 (256 bins, the default) or 9 (512 bins: the LZP predecessor build sorts its 18-bit hashes in two passes
// instead of three, round 5).  A thread owns RADIX / RS_BLOCK neighbouring digits wherever a digit needs a thread.
template <typename K, int BITS>
__device__ __forceinline__ void rs_hist_body(const K * __restrict__ keys, u64 n, int shift, u32 * __restrict__ hist, u32 tiles, u32 xcd, u32 bx) {
    constexpr int RADIX = 1 << BITS;
    __shared__ u32 bins[RADIX];
    // same tile assignment as the scatter: the counts of neighbouring tiles are neighbouring words of the digit-major table, so
    // the tiles of one XCD fill whole lines of it in that XCD's L2 (and the scatter finds its tile's keys in the L2 that read them)
    const u32 tile = rs_tile_of_block(bx, tiles, xcd != 0u);
    if (tile >= tiles) return;
#pragma unroll
    for (int d = threadIdx.x; d < RADIX; d += RS_BLOCK) bins[d] = 0;
    __syncthreads();
    const u64 tile_base = (u64)tile * RS_TILE;
    const u64 wbase = tile_base + (u64)wave_id() * RS_WAVE_SPAN + lane_id();
    const u64 last = n - 1;
    K key[RS_ROUNDS];
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; r++) {  // all 16 loads in flight before the first LDS atomic
        const u64 i = wbase + (u64)r * WAVE;
        key[r] = keys[i < n ? i : last];
    }
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; r++) {
        const u64 i = wbase + (u64)r * WAVE;
        if (i < n) atomicAdd(&bins[rs_digit<K, BITS>(key[r], shift)], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int d = threadIdx.x; d < RADIX; d += RS_BLOCK) hist[(u64)d * tiles + tile] = bins[d];
}
template <typename K, int BITS>
__global__ void __launch_bounds__(RS_BLOCK) k_rs_hist(const K * __restrict__ keys, u64 n, int shift, u32 * __restrict__ hist, u32 tiles, u32 xcd) {
    rs_hist_body<K, BITS>(keys, n, shift, hist, tiles, xcd, blockIdx.x);
}

// The tile is first put in digit order in LDS, then written out with consecutive lanes on consecutive destinations -- a digit's ~16
// keys of a tile leave as one run instead of 16 separate 8-byte stores.  Measured in round 3 on a 256 MiB block (full-n pass of
// 8-byte keys + 4-byte values): 1.46 ms = 4.4 TB/s of algorithmic traffic against 2.37 ms for the direct scatter
// (profiles/r03_kernel_stats_stages_256MiB_staged.txt), so the direct scatter is gone.
// Slot of a key inside the tile = start of its digit + keys of that digit in earlier waves + rank in its own wave, which is the
// stable order.  LDS: sizeof(K) * 4096 + 16 KiB + 6 KiB (54 KiB for 8-byte keys: two workgroups per CU).
//
// RAW (round 5): `offs` is the hist kernel's table as it left it -- per-tile COUNTS, not scanned -- and every workgroup derives its own
// 2^BITS offsets from it: digit d of tile t starts at (keys of smaller digits in all tiles) + (keys of digit d in earlier tiles), two
// sums over one row of the digit-major table per digit.  For a pass of up to RS_RAW_TILES tiles that is cheaper than the three to
// five launches of the recursive scan it replaces (415 k scan launches per bench run, most of them for the sorter's
// ~50 small passes per block); larger passes keep the scanned table.
template <typename K, bool IOTA, bool WKEYS, int BITS, bool RAW>
__global__ void __launch_bounds__(RS_BLOCK) k_rs_scatter(const K * __restrict__ kin, K * __restrict__ kout, const u32 * __restrict__ vin,
                                                               u32 * __restrict__ vout, u64 n, int shift, const u32 * __restrict__ offs, u32 tiles,
                                                               u32 iota_split, u32 out_base, u32 xcd) {
#include "sort_scatter_body.hpp"  // (shared with k_rs_scatter_many by inclusion: see the file)
}

// The pass of several independent key arrays in one launch per step (the inverse BWT's psi build: generated values, no keys out).  grid =
// (workgroups of the longest array, array); every array has its own length, count table, split and output.  A workgroup beyond its own
// array's padded grid must leave BEFORE the tile assignment: rs_tile_of_block maps such an index back onto a tile of a shorter array.
struct RsBatch8 {
    u32 count;
    struct Job {
        const u8 * keys;
        u32 * vout;
        u32 * hist;
        u64 n;  // >= 1
        u32 tiles, iota_split;
    } job[SORT_MAX_BATCH];
};
static_assert(sizeof(RsBatch8) <= KERNEL_TABLE_BYTES, "job table too large for a by-value kernel argument");
__global__ void __launch_bounds__(RS_BLOCK) k_rs_hist_many(RsBatch8 b, int shift, u32 xcd) {
    const RsBatch8::Job & j = b.job[blockIdx.y];
    if (blockIdx.x >= rs_grid(j.tiles, xcd != 0u)) return;
    rs_hist_body<u8, 8>(j.keys, j.n, shift, j.hist, j.tiles, xcd, blockIdx.x);
}
template <bool RAW>
__global__ void __launch_bounds__(RS_BLOCK) k_rs_scatter_many(RsBatch8 b, int shift, u32 out_base, u32 xcd) {
    typedef u8 K;
    constexpr bool IOTA = true, WKEYS = false;
    constexpr int BITS = 8;
    const RsBatch8::Job & j = b.job[blockIdx.y];
    if (blockIdx.x >= rs_grid(j.tiles, xcd != 0u)) return;
    const u8 * __restrict__ kin = j.keys;
    u8 * __restrict__ kout = nullptr;
    const u32 * __restrict__ vin = nullptr;
    u32 * __restrict__ vout = j.vout;
    const u32 * __restrict__ offs = j.hist;
    const u64 n = j.n;
    const u32 tiles = j.tiles, iota_split = j.iota_split;
#include "sort_scatter_body.hpp"  // (k_rs_scatter's body, on the names declared above)
}

// The same for the forward sorter's passes: 4- or 8-byte keys that are written out, values generated (IOTA) or read, every array with its own
// digit position (the suffix sorter's jobs differ in how many key bits they have).
template <typename K>
struct RsBatchKV {
    struct Job {
        const K * kin;
        K * kout;
        const u32 * vin;  // unused by the IOTA form
        u32 * vout;
        u32 * hist;
        u64 n;  // >= 1
        u32 tiles;
        int shift;
    } job[SORT_MAX_BATCH];
};
static_assert(sizeof(RsBatchKV<u32>) <= KERNEL_TABLE_BYTES && sizeof(RsBatchKV<u64>) <= KERNEL_TABLE_BYTES, "job table too large for a by-value kernel argument");
template <typename K>
__global__ void __launch_bounds__(RS_BLOCK) k_rs_hist_kv_many(RsBatchKV<K> b, u32 xcd) {
    const typename RsBatchKV<K>::Job & j = b.job[blockIdx.y];
    if (blockIdx.x >= rs_grid(j.tiles, xcd != 0u)) return;
    rs_hist_body<K, 8>(j.kin, j.n, j.shift, j.hist, j.tiles, xcd, blockIdx.x);
}
template <typename K, bool IOTA, bool RAW>
__global__ void __launch_bounds__(RS_BLOCK) k_rs_scatter_kv_many(RsBatchKV<K> b, u32 xcd) {
    constexpr bool WKEYS = true;
    constexpr int BITS = 8;
    const typename RsBatchKV<K>::Job & j = b.job[blockIdx.y];
    if (blockIdx.x >= rs_grid(j.tiles, xcd != 0u)) return;
    const K * __restrict__ kin = j.kin;
    K * __restrict__ kout = j.kout;
    const u32 * __restrict__ vin = j.vin;
    u32 * __restrict__ vout = j.vout;
    const u32 * __restrict__ offs = j.hist;
    const u64 n = j.n;
    const int shift = j.shift;
    const u32 tiles = j.tiles, iota_split = 0xFFFFFFFFu, out_base = 0u;
#include "sort_scatter_body.hpp"  // (k_rs_scatter's body, on the names declared above)
}

// Passes of up to this many tiles (512 Ki keys) skip the scan: the scatter's workgroups read the count table themselves (RAW above).
// Every workgroup reads the whole table -- tiles * 2^BITS words from L2 -- so the bound keeps that at 128 KiB (8-bit digits) per workgroup.
constexpr u32 RS_RAW_TILES = 128;

// (experiments: the scanned table for every pass, as up to round 4; read once)
static bool rs_no_raw() {
    static const bool v = getenv("BZ3_RS_NO_RAW") != nullptr;
    return v;
}

template <typename K, int BITS>
void radix_pass_bits(const K * kin, K * kout, const u32 * vin, u32 * vout, u64 n, int shift, u32 iota_split, u32 out_base, Arena & tmp,
                     hipStream_t s) {
    if (n == 0) return;
    constexpr int RADIX = 1 << BITS;
    const u32 tiles = (u32)((n + RS_TILE - 1) / RS_TILE);
    size_t m = tmp.mark();
    u32 * hist = tmp.take<u32>((size_t)tiles * RADIX);
    const u32 xcd = 1u;  // contiguous tiles per XCD (measured round 3: 2.37 against 3.58 ms per full-n pass with tile = blockIdx)
    const dim3 sgrid(rs_grid(tiles, xcd != 0u));
    launch(k_rs_hist<K, BITS>, sgrid, dim3(RS_BLOCK), 0, s, kin, n, shift, hist, tiles, xcd);
    const bool raw = tiles <= RS_RAW_TILES && !rs_no_raw();
    if (!raw) exclusive_scan_u32(hist, (u64)tiles * RADIX, nullptr, tmp, s);
    const bool iota = vin == nullptr, wkeys = kout != nullptr;
#define BZ3_RS_LAUNCH(I, W, R) \
    launch(k_rs_scatter<K, I, W, BITS, R>, sgrid, dim3(RS_BLOCK), 0, s, kin, kout, vin, vout, n, shift, (const u32 *)hist, tiles, iota_split, out_base, xcd)
#define BZ3_RS_DISPATCH(R)                                   \
    do {                                                     \
        if (iota && wkeys) BZ3_RS_LAUNCH(true, true, R);     \
        else if (iota) BZ3_RS_LAUNCH(true, false, R);        \
        else if (wkeys) BZ3_RS_LAUNCH(false, true, R);       \
        else BZ3_RS_LAUNCH(false, false, R);                 \
    } while (0)
    if (raw) BZ3_RS_DISPATCH(true);
    else BZ3_RS_DISPATCH(false);
#undef BZ3_RS_DISPATCH
#undef BZ3_RS_LAUNCH
    tmp.release(m);
}

// Raw or scanned count tables: decided by the longest array, for all of them (either is exact at any size; the bound is about speed).
void radix_pass_iota_u8_many(const RadixIotaJob * jobs, u32 count, u32 out_base, Arena & tmp, hipStream_t s) {
    if (count == 0 || count > SORT_MAX_BATCH) throw HipError{hipErrorUnknown, "radix batch of a size the job table does not hold", __FILE__, __LINE__};
    RsBatch8 b;
    b.count = count;
    size_t m = tmp.mark();
    u32 most = 0;
    u32 * tables[SORT_MAX_BATCH];
    u64 words[SORT_MAX_BATCH];
    for (u32 k = 0; k < count; k++) {
        if (jobs[k].n == 0) throw HipError{hipErrorUnknown, "radix batch with an empty array", __FILE__, __LINE__};
        const u32 tiles = (u32)((jobs[k].n + RS_TILE - 1) / RS_TILE);
        words[k] = (u64)tiles * RS_RADIX;
        tables[k] = tmp.take<u32>((size_t)words[k]);
        b.job[k] = RsBatch8::Job{jobs[k].keys, jobs[k].vout, tables[k], jobs[k].n, tiles, jobs[k].iota_split};
        most = tiles > most ? tiles : most;
    }
    for (u32 k = count; k < SORT_MAX_BATCH; k++) b.job[k] = b.job[0];
    const u32 xcd = 1u;
    const dim3 grid(rs_grid(most, true), count);
    launch(k_rs_hist_many, grid, dim3(RS_BLOCK), 0, s, b, 0, xcd);
    const bool raw = most <= RS_RAW_TILES && !rs_no_raw();
    if (!raw) exclusive_scan_u32_many(tables, words, nullptr, count, tmp, s);
    if (raw) launch(k_rs_scatter_many<true>, grid, dim3(RS_BLOCK), 0, s, b, 0, out_base, xcd);
    else launch(k_rs_scatter_many<false>, grid, dim3(RS_BLOCK), 0, s, b, 0, out_base, xcd);
    tmp.release(m);
}

// One array goes through radix_pass: the single kernels, launch for launch what a block alone has always had (the metric's 256 MiB blocks).
template <typename K>
void radix_pass_many(const RadixPairJob<K> * jobs, u32 count, Arena & tmp, hipStream_t s) {
    if (count == 0 || count > SORT_MAX_BATCH) throw HipError{hipErrorUnknown, "radix batch of a size the job table does not hold", __FILE__, __LINE__};
    if (count == 1) {
        radix_pass<K>(jobs[0].kin, jobs[0].kout, jobs[0].vin, jobs[0].vout, jobs[0].n, jobs[0].shift, 0xFFFFFFFFu, 0u, tmp, s);
        return;
    }
    RsBatchKV<K> b;
    size_t m = tmp.mark();
    u32 most = 0;
    u32 * tables[SORT_MAX_BATCH];
    u64 words[SORT_MAX_BATCH];
    const bool iota = jobs[0].vin == nullptr;
    for (u32 k = 0; k < count; k++) {
        if (jobs[k].n == 0 || !jobs[k].kout || (jobs[k].vin == nullptr) != iota) throw HipError{hipErrorUnknown, "radix batch with an empty or a mixed array", __FILE__, __LINE__};
        const u32 tiles = (u32)((jobs[k].n + RS_TILE - 1) / RS_TILE);
        words[k] = (u64)tiles * RS_RADIX;
        tables[k] = tmp.take<u32>((size_t)words[k]);
        b.job[k] = typename RsBatchKV<K>::Job{jobs[k].kin, jobs[k].kout, jobs[k].vin, jobs[k].vout, tables[k], jobs[k].n, tiles, jobs[k].shift};
        most = tiles > most ? tiles : most;
    }
    for (u32 k = count; k < SORT_MAX_BATCH; k++) b.job[k] = b.job[0];
    const u32 xcd = 1u;
    const dim3 grid(rs_grid(most, true), count);
    launch(k_rs_hist_kv_many<K>, grid, dim3(RS_BLOCK), 0, s, b, xcd);
    const bool raw = most <= RS_RAW_TILES && !rs_no_raw();
    if (!raw) exclusive_scan_u32_many(tables, words, nullptr, count, tmp, s);
    if (iota) {
        if (raw) launch(k_rs_scatter_kv_many<K, true, true>, grid, dim3(RS_BLOCK), 0, s, b, xcd);
        else launch(k_rs_scatter_kv_many<K, true, false>, grid, dim3(RS_BLOCK), 0, s, b, xcd);
    } else {
        if (raw) launch(k_rs_scatter_kv_many<K, false, true>, grid, dim3(RS_BLOCK), 0, s, b, xcd);
        else launch(k_rs_scatter_kv_many<K, false, false>, grid, dim3(RS_BLOCK), 0, s, b, xcd);
    }
    tmp.release(m);
}

void radix_hist_bits9(const u32 * keys, u64 n, int shift, u32 * hist, u32 tiles, hipStream_t s) {
    launch(k_rs_hist<u32, 9>, dim3(rs_grid(tiles, true)), dim3(RS_BLOCK), 0, s, keys, n, shift, hist, tiles, 1u);
}

template <typename K>
void radix_pass(const K * kin, K * kout, const u32 * vin, u32 * vout, u64 n, int shift, u32 iota_split, u32 out_base, Arena & tmp,
                hipStream_t s) {
    radix_pass_bits<K, 8>(kin, kout, vin, vout, n, shift, iota_split, out_base, tmp, s);
}

template <typename K>
int radix_sort_pairs(K * k0, K * k1, u32 * v0, u32 * v1, u64 n, int bit_lo, int bit_hi, Arena & tmp, hipStream_t s) {
    int cur = 0;
    for (int shift = bit_lo; shift < bit_hi; shift += 8) {
        if (cur == 0)
            radix_pass<K>(k0, k1, v0, v1, n, shift, 0xFFFFFFFFu, 0u, tmp, s);
        else
            radix_pass<K>(k1, k0, v1, v0, n, shift, 0xFFFFFFFFu, 0u, tmp, s);
        cur ^= 1;
    }
    return cur;
}

template void radix_pass<u8>(const u8 *, u8 *, const u32 *, u32 *, u64, int, u32, u32, Arena &, hipStream_t);
template void radix_pass<u32>(const u32 *, u32 *, const u32 *, u32 *, u64, int, u32, u32, Arena &, hipStream_t);
template void radix_pass<u64>(const u64 *, u64 *, const u32 *, u32 *, u64, int, u32, u32, Arena &, hipStream_t);
template void radix_pass_bits<u32, 9>(const u32 *, u32 *, const u32 *, u32 *, u64, int, u32, u32, Arena &, hipStream_t);
template void radix_pass_many<u32>(const RadixPairJob<u32> *, u32, Arena &, hipStream_t);
template void radix_pass_many<u64>(const RadixPairJob<u64> *, u32, Arena &, hipStream_t);
template int radix_sort_pairs<u32>(u32 *, u32 *, u32 *, u32 *, u64, int, int, Arena &, hipStream_t);
template int radix_sort_pairs<u64>(u64 *, u64 *, u32 *, u32 *, u64, int, int, Arena &, hipStream_t);

}  // namespace bz3
