// bwt.hip -- forward Burrows-Wheeler transform on gfx950: one block, or up to BWT_MAX_BATCH (8) blocks through one launch sequence (bwt_forward_batch).
// Replaces libsais_bwt (reference include/libsais.h:4095-4121, SA-IS: :3941-3983, :3740-3939), which is a sequential
// induced-sorting algorithm whose inner scans carry a dependency through 256 bucket cursors.  This is NOT a port of it.
//
// Design of rounds 3-4 ("sort once, then resolve groups where they lie"):
//
//   codes   : the bytes of the block are given an order-preserving prefix-free code of at most 8 bits per symbol, the optimal
//             height-limited alphabetic tree for the block's byte histogram (frequent bytes get short codes), built on the DEVICE
//             (k_vlc_init / k_vlc_level / k_vlc_codes; rounds 1-3: on the host).  Comparing the concatenated code bits of two suffixes
//             is the same as comparing their bytes, and a 56-bit window holds 7 symbols at least and ~12 of English text.
//   round 0 : key(i) = first 56 code bits of suffix i (16 symbols at most, zero padded past the end) << 8 | T[i-1]; ONE stable LSD
//             radix sort of all n (key, i) pairs over the upper 56 bits (7 passes of sort.hip).  The byte that precedes the suffix
//             rides in the low byte: it is the BWT symbol of the suffix, so the output needs no gather through the suffix array.
//   groups  : suffixes with equal 56-bit windows form a group of neighbouring slots.  V[slot] = suffix | head flag (bit 31);
//             k_bwt_heads marks them and snapshots the flags, k_bwt_spine_a / _b give every anchor tile of 512 slots (WR_A) the last
//             head before it.
//   route   : k_bwt_route -- a wave per anchor tile sends the groups that start there to one of three lists: up to 64 members -> the
//             tail list (one entry per suffix), 65 .. 256 members (WR_G) -> a descriptor for the wide kernel, more -> the big list.
//   wide    : k_bwt_wide -- a wave per descriptor, 2 or 4 suffixes per lane in registers: a step fetches the next 40 code bits of
//             every still-ambiguous suffix straight from the text (no inverse suffix array, no rank table: groups are independent of
//             each other), a bitonic network over the wave's registers sorts all sub-groups at once; what is down to <= 64 members
//             moves on to the tail list.
//   tail    : k_bwt_tail -- a wave per 64 list entries takes the whole groups that start there, a lane per suffix, ranks groups of up
//             to 12 by counting and larger ones with a 64-lane bitonic network, up to TL_CAP steps.  Text needs 2-3 steps.
//             The wide and the tail kernel read the lengths of their lists from the router's counters on the device (round 4).
//   big     : groups of > 256 suffixes (a few % of text) get one more 56-bit window each through the global radix sorter
//             (k_big_*), after which they are small and are routed again.
//   deep    : what is still ambiguous after that (long repeats: runs, periodic data) falls back to classic prefix doubling on
//             ranks (ISA built once, k_bg_* / k_isa_scatter / k_bwt_doubling_keys_grp) -- the only path that needs random 4-byte scatters.
//   output  : U[0] = T[n-1]; U[i < i0 ? i+1 : i] = payload byte of slot i for i != i0 = slot of suffix 0; idx = i0+1.
//
// Order of equal windows past the end of the block: a suffix that is a proper prefix of another sorts first (zero padding is the
// smallest continuation, and a suffix with no symbol left at its depth sorts before every live one, shorter first) -- exactly the
// order libsais produces.
//
// HBM per block of n bytes (carved from the per-device workspace): 2 x key u64[n], 2 x suffix u32[n], payload u8[n]; the deep path
// additionally ISA u32[n], 2 x slot u32[n], rank u32[n], tile words.  Algorithmic traffic: 11 B per input byte.
#include <atomic>
#include <vector>

#include "prims.hpp"
#include "sort.hpp"
#include "stages.hpp"

namespace bz3 {

constexpr int BW_BLOCK = 256;
constexpr u32 V_HEAD = 0x80000000u;  // slot starts a group
constexpr u32 V_MASK = 0x3FFFFFFFu;  // suffix number (n < 2^30: bz3_bound(511 MiB) = 546.5 M)

// Bytes of the block that are NOT among its `keep` most frequent byte values (one workgroup of 256: thread c ranks the count of byte value c).
// The BWT output has the block's histogram, and the CM stage's row-cache kernels hold ~40 order-1 rows per block: api.hip routes a block
// whose rarer values make up more than half of the row misses those kernels tolerate straight to the whole-model kernels (round 5; before, the row-cache kernels had to give it up first).
//
// ---- job tables: every kernel of this file works on up to BWT_MAX_BATCH independent blocks ("jobs") in one launch --------------------
// A kernel's arguments are the fields of its job structure, listed ONCE in an X-macro; the table of jobs travels by value as the kernel
// argument (nothing of it has to outlive the launch); grid = (workgroups of the job that needs most, job).  A workgroup picks its job by
// blockIdx.y, leaves if its index lies beyond that job's own extent (`grid_`) -- before any barrier --, and from there on the body reads
// the fields under the names, types and qualifiers they had as kernel parameters.  Jobs never wait for each other.
#define BWT_FIELD(T, name) T name;
#define BWT_LOCAL(T, name) T const name = job_.name;
#define BWT_JOB(NAME, ARGS)  \
    struct NAME {            \
        u32 grid_;           \
        ARGS(BWT_FIELD)      \
    };                       \
    static_assert(sizeof(NAME) * BWT_MAX_BATCH <= KERNEL_TABLE_BYTES, "job table too large for a by-value kernel argument")
#define BWT_ENTER(NAME, ARGS)                    \
    const NAME & job_ = jobs_.job[blockIdx.y];     \
    if (blockIdx.x >= job_.grid_) return;        \
    ARGS(BWT_LOCAL)
template <typename J>
struct JobTab {
    J job[BWT_MAX_BATCH];
};

#define OUTSIDE_ARGS(X) X(const u32 * __restrict__, hist) X(u32, keep) X(u32 * __restrict__, out)
BWT_JOB(OutsideJob, OUTSIDE_ARGS);
__global__ void __launch_bounds__(256) k_bwt_outside(JobTab<OutsideJob> jobs_) {
    BWT_ENTER(OutsideJob, OUTSIDE_ARGS)
    __shared__ u32 h[256];
    __shared__ u32 red[256 / WAVE + 1];
    const u32 c = threadIdx.x;
    h[c] = hist[c];
    __syncthreads();
    const u32 mine = h[c];
    u32 rank = 0;  // byte values that come before c in (count descending, value ascending) order
    for (u32 k = 0; k < 256u; k++) rank += (h[k] > mine || (h[k] == mine && k < c)) ? 1u : 0u;
    const u32 tot = block_sum<256>(rank >= keep ? mine : 0u, red);
    if (c == 0) *out = tot;
}

// ---- the order-preserving code ----------------------------------------------------------------------------------------------
// vlc[c] = code << 4 | len (1 <= len <= 8) for byte values present in the block, 0 otherwise.
constexpr int VLC_MAXLEN = 8;
constexpr int VLC_WINDOW = 16;  // symbols a window looks at

#define SYM_HIST_ARGS(X) X(const u8 * __restrict__, t) X(u32, n) X(u32 * __restrict__, hist)
BWT_JOB(SymHistJob, SYM_HIST_ARGS);
__global__ void __launch_bounds__(BW_BLOCK) k_bwt_sym_hist(JobTab<SymHistJob> jobs_) {
    BWT_ENTER(SymHistJob, SYM_HIST_ARGS)
    __shared__ u32 bins[256];
    bins[threadIdx.x] = 0;
    __syncthreads();
    // 64 bytes per thread, 16 at a time, every load of a group in flight before the first is counted (sort.hip explains why the
    // obvious `if (i < n) ... t[i]` loop is one exposed HBM round trip per byte); index clamped, lane masked.
    const u64 base = (u64)blockIdx.x * (BW_BLOCK * 64);
    const u64 last = (u64)n - 1;
    for (u32 g = 0; g < 4; g++) {
        u8 c[16];
#pragma unroll
        for (u32 k = 0; k < 16; k++) {
            const u64 i = base + (u64)(g * 16 + k) * BW_BLOCK + threadIdx.x;
            c[k] = t[i < n ? i : last];
        }
#pragma unroll
        for (u32 k = 0; k < 16; k++) {
            const u64 i = base + (u64)(g * 16 + k) * BW_BLOCK + threadIdx.x;
            if (i < n) atomicAdd(&bins[c[k]], 1u);
        }
    }
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(&hist[threadIdx.x], bins[threadIdx.x]);
}

// Optimal alphabetic (order-preserving) prefix-free code of height <= 8 for the byte values present, by dynamic programming over
// intervals: cost[l][i][j] = lightest tree of height <= l over the present values i .. j-1 = min over the split k of
// cost[l-1][i][k] + cost[l-1][k][j], plus the weight of the interval.  On the DEVICE since round 4 (rounds 1-3 copied the histogram to
// the host, ran the recurrence there in ~1 ms and copied the table back: a stream synchronisation and a millisecond of idle GPU per
// block, and a front end that slowed down with the host): a level is one launch with a thread per interval -- every cell of a level
// only reads the level below --, the tables (two cost planes of 257 x 257 u64, nine root planes of u16) live in the block's arena.
// Which optimal tree comes out does not matter to the BWT (any order-preserving prefix code sorts the suffixes the same way): ties
// go to the smallest split.
constexpr int VLC_S1 = 257;                         // intervals [i, j) over up to 256 present values: 0 <= i < j <= 256
constexpr u64 VLC_INF = ~0ull >> 2;
constexpr size_t VLC_PLANE = (size_t)VLC_S1 * VLC_S1;
struct VlcWork {
    u32 s;            // byte values present
    u32 sym[256];     // ... in increasing order
    u64 pre[257];     // prefix sums of their counts
};
constexpr size_t VLC_WORK_BYTES = ((sizeof(VlcWork) + 255) & ~(size_t)255) + 2 * VLC_PLANE * sizeof(u64) + (VLC_MAXLEN + 1) * VLC_PLANE * sizeof(u16) + 256;

// the present values, their prefix sums, level 0 (single values cost nothing, nothing else fits height 0), the trivial tables
#define VLC_INIT_ARGS(X) X(const u32 * __restrict__, hist) X(VlcWork * __restrict__, w) X(u64 * __restrict__, cost0) X(u32 * __restrict__, table)
BWT_JOB(VlcInitJob, VLC_INIT_ARGS);
__global__ void __launch_bounds__(256) k_vlc_init(JobTab<VlcInitJob> jobs_) {
    BWT_ENTER(VlcInitJob, VLC_INIT_ARGS)
    __shared__ u32 lds[256 / WAVE + 1];
    __shared__ u64 s_cnt[256];
    const u32 c = threadIdx.x;
    const u32 cnt = hist[c];
    u32 total;
    const u32 at = block_excl_add<256>(cnt ? 1u : 0u, lds, total);
    s_cnt[c] = 0;
    __syncthreads();
    if (cnt) {
        w->sym[at] = c;
        s_cnt[at] = cnt;
    }
    table[c] = (total == 1u && cnt) ? ((0u << 4) | 1u) : 0u;  // one value: code 0, one bit; the others are filled in by k_vlc_codes
    __syncthreads();
    if (c == 0) {
        w->s = total;
        u64 run = 0;
        for (u32 k = 0; k <= 256u; k++) {
            w->pre[k] = run;
            if (k < 256u) run += s_cnt[k];
        }
    }
    for (u32 i = 0; i < (u32)VLC_S1; i++) {  // row i of the level-0 plane
        const u32 j0 = c, j1 = c + 256u;
        cost0[(size_t)i * VLC_S1 + j0] = j0 == i + 1u ? 0ull : VLC_INF;
        if (j1 < (u32)VLC_S1) cost0[(size_t)i * VLC_S1 + j1] = j1 == i + 1u ? 0ull : VLC_INF;
    }
}
// level l from level l-1: workgroup i, thread j-1
#define VLC_LEVEL_ARGS(X) X(const VlcWork * __restrict__, w) X(u32, l) X(const u64 * __restrict__, below) X(u64 * __restrict__, cost) X(u16 * __restrict__, root)
BWT_JOB(VlcLevelJob, VLC_LEVEL_ARGS);
__global__ void __launch_bounds__(256) k_vlc_level(JobTab<VlcLevelJob> jobs_) {
    BWT_ENTER(VlcLevelJob, VLC_LEVEL_ARGS)
    const u32 s = w->s;
    const u32 i = blockIdx.x, j = threadIdx.x + 1u;
    if (i >= s) return;
    u64 best = VLC_INF;
    u32 bk = 0;
    if (j > i && j <= s) {
        const u32 len = j - i, half = 1u << (l - 1u);
        if (len == 1u) {
            best = 0;
        } else if (len <= 2u * half) {
            const u32 klo = j > i + half ? j - half : i + 1u;      // both parts must fit height l-1: at most 2^(l-1) values each
            const u32 khi = i + half < j - 1u ? i + half : j - 1u;
            for (u32 k = klo; k <= khi; k++) {
                const u64 a = below[(size_t)i * VLC_S1 + k], b = below[(size_t)k * VLC_S1 + j];
                if (a < VLC_INF && b < VLC_INF && a + b < best) {
                    best = a + b;
                    bk = k;
                }
            }
            if (best < VLC_INF) best += w->pre[j] - w->pre[i];
        }
    }
    if (j > i && j < (u32)VLC_S1) {
        cost[(size_t)i * VLC_S1 + j] = best;
        root[(size_t)i * VLC_S1 + j] = (u16)bk;
    }
}
// every present value walks down from the root of the height-8 tree: table[c] = code << 4 | length
#define VLC_CODES_ARGS(X) X(const VlcWork * __restrict__, w) X(const u16 * __restrict__, roots) X(u32 * __restrict__, table)
BWT_JOB(VlcCodesJob, VLC_CODES_ARGS);
__global__ void __launch_bounds__(256) k_vlc_codes(JobTab<VlcCodesJob> jobs_) {
    BWT_ENTER(VlcCodesJob, VLC_CODES_ARGS)
    const u32 s = w->s, x = threadIdx.x;
    if (s < 2u || x >= s) return;
    u32 i = 0, j = s, l = VLC_MAXLEN, code = 0, len = 0;
    while (j - i > 1u) {
        const u32 k = roots[(size_t)l * VLC_PLANE + (size_t)i * VLC_S1 + j];
        if (x < k) {
            j = k;
            code <<= 1;
        } else {
            i = k;
            code = (code << 1) | 1u;
        }
        l--;
        len++;
    }
    table[w->sym[x]] = (code << 4) | len;
}
// The first B code bits of the symbols in the window (wa, wb: 16 bytes, little endian; avail <= 16 of them exist), zero padded;
// cnt = symbols that lie entirely inside those bits.
template <int B, int SYMS = VLC_WINDOW>
__device__ __forceinline__ void vlc_pack(const u32 * __restrict__ tab, u64 wa, u64 wb, u32 avail, u64 & key, u32 & cnt) {
    u64 acc = 0;
    u32 bits = 0;
    cnt = 0;
#pragma unroll
    for (u32 k = 0; k < (u32)SYMS; k++) {
        const u32 e = tab[(u8)(k < 8 ? wa >> (8 * k) : wb >> (8 * (k - 8)))];
        const u32 len = e & 15u;
        const bool take = k < avail && bits < (u32)B;
        acc = take ? ((acc << len) | (u64)(e >> 4)) : acc;
        bits = take ? bits + len : bits;
        cnt = (take && bits <= (u32)B) ? k + 1u : cnt;
    }
    key = bits >= (u32)B ? (acc >> (bits - (u32)B)) : (acc << ((u32)B - bits));
}

struct __attribute__((packed)) PackedU64 { u64 v; };

// The 16 bytes at t[pos ..] as two little-endian words (any alignment); avail = how many of them exist (bytes past the end read as
// zero).  Branch-free for n >= 16, so that the loads of all the elements a thread handles are in flight together: the address is
// clamped to the last 16 bytes of the block and the words are shifted down by the difference.
__device__ __forceinline__ void load_window(const u8 * __restrict__ t, u64 pos, u64 n, u64 & a, u64 & b, u32 & avail) {
    avail = pos >= n ? 0u : (n - pos < (u64)VLC_WINDOW ? (u32)(n - pos) : (u32)VLC_WINDOW);
    if (n >= (u64)VLC_WINDOW) {
        const u64 p2 = pos + VLC_WINDOW <= n ? pos : n - VLC_WINDOW;
        u64 lo = reinterpret_cast<const PackedU64 *>(t + p2)->v;
        u64 hi = reinterpret_cast<const PackedU64 *>(t + p2 + 8)->v;
        const u64 delta = pos - p2;          // bytes to drop from the front
        u32 sh = delta >= 16 ? 128u : (u32)delta * 8u;
        if (sh >= 64u) {
            lo = hi;
            hi = 0;
            sh -= 64u;
        }
        if (sh >= 64u) {
            lo = 0;
            sh = 0;
        }
        if (sh) {
            lo = (lo >> sh) | (hi << (64u - sh));
            hi >>= sh;
        }
        a = lo;
        b = hi;
    } else {  // tiny block: byte by byte
        a = b = 0;
        for (u32 k = 0; k < avail; k++) {
            const u64 c = t[pos + k];
            if (k < 8) a |= c << (8 * k); else b |= c << (8 * (k - 8));
        }
    }
}
__device__ __forceinline__ u8 window_byte(u64 a, u64 b, u32 k) { return (u8)(k < 8 ? a >> (8 * k) : b >> (8 * (k - 8))); }

// keys[i] = (first 56 code bits of suffix i) << 8 | T[i-1]; 8 positions per thread from 24 bytes.
#define VLC_KEYS_ARGS(X) X(const u8 * __restrict__, t) X(u32, n) X(const u32 * __restrict__, vlc) X(u64 * __restrict__, keys)
BWT_JOB(VlcKeysJob, VLC_KEYS_ARGS);
__global__ void __launch_bounds__(BW_BLOCK) k_bwt_vlc_keys(JobTab<VlcKeysJob> jobs_) {
    BWT_ENTER(VlcKeysJob, VLC_KEYS_ARGS)
    __shared__ u32 tab[256];
    tab[threadIdx.x] = vlc[threadIdx.x];
    __syncthreads();
    const u64 base = ((u64)blockIdx.x * BW_BLOCK + threadIdx.x) * 8;
    if (base >= n) return;
    const u64 last = (u64)n - 1;
    u8 b[24];  // b[k] = t[base - 1 + k]
#pragma unroll
    for (int k = 0; k < 24; k++) {
        const u64 i = base + k;  // index + 1
        b[k] = t[i == 0 ? 0 : (i - 1 < n ? i - 1 : last)];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const u64 p = base + k;
        if (p < n) {
            u64 wa = 0, wb = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                wa |= (u64)b[k + 1 + q] << (8 * q);
                wb |= (u64)b[k + 9 + q] << (8 * q);
            }
            const u64 left = n - p;
            u64 key;
            u32 cnt;
            vlc_pack<56>(tab, wa, wb, left < (u64)VLC_WINDOW ? (u32)left : (u32)VLC_WINDOW, key, cnt);
            keys[p] = (key << 8) | (p == 0 ? 0ull : (u64)b[k]);
        }
    }
}

// ---- groups of the sorted list ----------------------------------------------------------------------------------------------
// Resolve-kernel geometry: a workgroup owns the groups whose head lies in its RS_S anchor slots; such a group of <= TR_G suffixes
// ends inside the TR_WIN-slot window.
constexpr int WR_A = 512;     // anchor slots per wave
constexpr int WR_G = 256;     // largest group a wave resolves (4 suffixes per lane; with 8 the wide kernel needs 200 registers: two waves per SIMD)
constexpr int WR_WAVES = 4;   // waves per workgroup (independent of each other after the code table is loaded)
constexpr int WR_CAP = 160;   // resolve steps before a group is left to the deep path
constexpr int TL_CAP = 160;   // tail steps before a group is left to the deep path (>= 800 symbols)
constexpr u32 WR_FAR = 0xFFFFu;
constexpr int TR_S = WR_A;    // granularity of tile_last / carry / dirty
constexpr int TR_G = WR_G;

// V[p] = suffix | head flag, PB[p] = payload byte, tile_last[t] = 1 + slot of the last head in anchor tile t (0: none), pos0, and
// the SNAPSHOT of the head flags as a bitmap: the resolve kernel takes the group boundaries from the snapshot, because the flags in V
// change under it (a neighbouring workgroup splits its own groups while this one is still reading its window).
#define HEADS_ARGS(X) X(const u64 * __restrict__, keys) X(u32 * __restrict__, v) X(u8 * __restrict__, pb) X(u32, n) X(u32 * __restrict__, tile_last) X(u32 * __restrict__, hbits) X(u32 * __restrict__, counters)
BWT_JOB(HeadsJob, HEADS_ARGS);
__global__ void __launch_bounds__(BW_BLOCK) k_bwt_heads(JobTab<HeadsJob> jobs_) {
    BWT_ENTER(HeadsJob, HEADS_ARGS)
    __shared__ u32 lds[BW_BLOCK / WAVE + 1];
    const u64 tbase = (u64)blockIdx.x * TR_S;
    u32 hp = 0;
    for (u32 q = threadIdx.x; q < (u32)TR_S; q += BW_BLOCK) {  // TR_S is a multiple of the workgroup size: uniform trip count
        const u64 p = tbase + q;
        bool head = true;  // past the end: heads
        if (p < n) {
            const u64 k = keys[p];
            head = p == 0 || (k >> 8) != (keys[p - 1] >> 8);
            const u32 s = v[p];
            v[p] = s | (head ? V_HEAD : 0u);
            pb[p] = (u8)k;
            if (head) hp = (u32)p + 1u;
            if (s == 0) counters[2] = (u32)p;
        }
        const u64 bal = __ballot(head);
        if (lane_id() == 0 && p - (p & 63u) < (((u64)n + 63u) & ~63ull)) {
            hbits[p >> 5] = (u32)bal;
            hbits[(p >> 5) + 1] = (u32)(bal >> 32);
        }
    }
    hp = block_max<BW_BLOCK>(hp, lds);
    if (threadIdx.x == 0) tile_last[blockIdx.x] = hp;
}

// The same reduction and snapshot from the flags in V (after a big round changed them).
#define REDUCE_HEADS_ARGS(X) X(const u32 * __restrict__, v) X(u32, n) X(u32 * __restrict__, tile_last) X(u32 * __restrict__, hbits)
BWT_JOB(ReduceHeadsJob, REDUCE_HEADS_ARGS);
__global__ void __launch_bounds__(BW_BLOCK) k_bwt_reduce_heads(JobTab<ReduceHeadsJob> jobs_) {
    BWT_ENTER(ReduceHeadsJob, REDUCE_HEADS_ARGS)
    __shared__ u32 lds[BW_BLOCK / WAVE + 1];
    const u64 tbase = (u64)blockIdx.x * TR_S;
    u32 hp = 0;
    for (u32 q = threadIdx.x; q < (u32)TR_S; q += BW_BLOCK) {
        const u64 p = tbase + q;
        bool head = true;
        if (p < n) {
            head = (v[p] & V_HEAD) != 0u;
            if (head) hp = (u32)p + 1u;
        }
        const u64 bal = __ballot(head);
        if (lane_id() == 0 && p - (p & 63u) < (((u64)n + 63u) & ~63ull)) {
            hbits[p >> 5] = (u32)bal;
            hbits[(p >> 5) + 1] = (u32)(bal >> 32);
        }
    }
    hp = block_max<BW_BLOCK>(hp, lds);
    if (threadIdx.x == 0) tile_last[blockIdx.x] = hp;
}

// carry of tile t = 1 + slot of the last head before the tile = max(carry_local[t], group_carry[t / SP_GROUP]) (0: none):
//   k_bwt_spine_a : one workgroup per SP_GROUP tiles, exclusive running maximum inside the group + the group's maximum
//   k_bwt_spine_b : one workgroup, exclusive running maximum over the groups (at most ~1000 of them)
// (one workgroup over all 520 k tiles of a 256 MiB block took as long as a radix pass)
constexpr int SP_BLOCK = 256;
constexpr int SP_PER = 4;
constexpr int SP_GROUP = SP_BLOCK * SP_PER;
template <int BLOCK>
__device__ __forceinline__ u32 sp_block_excl_max(u32 v, u32 * lds, u32 & all) {  // lds: BLOCK / 64 + 1 words; ends with a barrier
    const u32 incl = wave_incl_max(v);
    if (lane_id() == WAVE - 1) lds[wave_id()] = incl;
    u32 up = __shfl_up(incl, 1u);
    if (lane_id() == 0) up = 0u;
    __syncthreads();
    u32 carry = 0, tot = 0;
    for (int w = 0; w < BLOCK / WAVE; w++) {
        if (w < wave_id()) carry = lds[w] > carry ? lds[w] : carry;
        tot = lds[w] > tot ? lds[w] : tot;
    }
    __syncthreads();
    all = tot;
    return up > carry ? up : carry;
}
#define SPINE_A_ARGS(X) X(const u32 * __restrict__, tile_last) X(u32, tiles) X(u32 * __restrict__, carry_local) X(u32 * __restrict__, group_max)
BWT_JOB(SpineAJob, SPINE_A_ARGS);
__global__ void __launch_bounds__(SP_BLOCK) k_bwt_spine_a(JobTab<SpineAJob> jobs_) {
    BWT_ENTER(SpineAJob, SPINE_A_ARGS)
    __shared__ u32 lds[SP_BLOCK / WAVE + 1];
    const u32 t0 = blockIdx.x * SP_GROUP + threadIdx.x * SP_PER;
    u32 h[SP_PER];
#pragma unroll
    for (int k = 0; k < SP_PER; k++) h[k] = t0 + k < tiles ? tile_last[t0 + k] : 0u;
    u32 mine = 0;
#pragma unroll
    for (int k = 0; k < SP_PER; k++) mine = h[k] > mine ? h[k] : mine;
    u32 all;
    u32 run = sp_block_excl_max<SP_BLOCK>(mine, lds, all);
#pragma unroll
    for (int k = 0; k < SP_PER; k++) {
        if (t0 + k < tiles) carry_local[t0 + k] = run;
        run = h[k] > run ? h[k] : run;
    }
    if (threadIdx.x == 0) group_max[blockIdx.x] = all;
}
#define SPINE_B_ARGS(X) X(const u32 * __restrict__, group_max) X(u32, groups) X(u32 * __restrict__, group_carry)
BWT_JOB(SpineBJob, SPINE_B_ARGS);
__global__ void __launch_bounds__(1024) k_bwt_spine_b(JobTab<SpineBJob> jobs_) {
    BWT_ENTER(SpineBJob, SPINE_B_ARGS)
    __shared__ u32 lds[1024 / WAVE + 1];
    u32 run_in = 0;  // maximum over the chunks of 1024 groups before this one (one chunk for every block size the API allows)
    for (u32 base = 0; base < groups; base += 1024u) {
        const u32 g = base + threadIdx.x;
        const u32 x = g < groups ? group_max[g] : 0u;
        u32 all;
        const u32 ex = sp_block_excl_max<1024>(x, lds, all);
        if (g < groups) group_carry[g] = ex > run_in ? ex : run_in;
        run_in = all > run_in ? all : run_in;
    }
}

// ---- the resolve kernel ------------------------------------------------------------------------------------------------------
// One WAVE per 512 anchor slots, no workgroup barriers.  The wave owns the groups whose head lies in its anchor slots; it takes them
// in batches of whole groups that are neighbours in the slot order, at most 512 slots per batch (8 per lane, blocked: position
// j = lane * E + r), and resolves a batch completely before it goes on:
//   step  : every suffix that still shares its group fetches the next 40 code bits at its depth straight from the text (16 bytes, all
//           loads of a lane in flight together) -- no inverse suffix array, no rank table: groups are independent of each other;
//           sort word = [group start : 9][live : 1][40 code bits, or the length of a suffix that has ended][position : 9];
//           a bitonic network over the wave's registers (strides below E inside a lane, the others by cross-lane exchange) sorts all
//           groups of the batch at once; the payloads (suffix, depth, BWT symbol) follow through a per-wave LDS buffer; positions
//           whose word differs from their left neighbour's become group heads.
//   shrink: once the suffixes still ambiguous fit half the lanes' capacity, the final ones are written out and the rest move up
//           (E halves: a 64-element network costs a tenth of a 512-element one), so long tails of tiny deep groups stay cheap.
// Round 3 measured the first, workgroup-wide version of this kernel (2048-slot windows, block scans and barriers between the phases
// of a step) at 40 ms per 256 MiB block, nearly all of it waiting at barriers with 16 waves per CU; a wave-level step is the same
// work without a single barrier, and the small footprint (~5 KB of LDS per wave) lets many waves cover each other's gathers.
__device__ __forceinline__ u32 bw_readlane(u32 v, int lane) {
#ifdef BZ3_EMU
    return __shfl(v, lane);
#else
    return (u32)__builtin_amdgcn_readlane((int)v, lane);
#endif
}
// Sort word layout
constexpr int WW_IDX = 9, WW_KEY = 40;
__device__ __forceinline__ u64 ww_make(u32 gs, bool live, u64 key, u32 idx) {
    return ((u64)gs << (WW_IDX + WW_KEY + 1)) | ((live ? 1ull : 0ull) << (WW_IDX + WW_KEY)) | (key << WW_IDX) | (u64)idx;
}
// payload: [suffix : 30][depth : 16][BWT symbol : 8]
__device__ __forceinline__ u64 pl_make(u32 v, u32 d, u32 p) { return ((u64)v << 24) | ((u64)(d & 0xFFFFu) << 8) | (u64)(p & 0xFFu); }
__device__ __forceinline__ u32 pl_v(u64 x) { return (u32)(x >> 24); }
__device__ __forceinline__ u32 pl_d(u64 x) { return (u32)(x >> 8) & 0xFFFFu; }
__device__ __forceinline__ u32 pl_p(u64 x) { return (u32)x & 0xFFu; }

// Bitonic sort of the 64 * E words held by the wave (position j = lane * E + r), ascending.
template <int E>
__device__ __forceinline__ void wave_bitonic(u64 (&w)[E]) {
    const u32 lane = (u32)lane_id();
#pragma unroll
    for (u32 k = 2; k <= 64u * E; k <<= 1) {
#pragma unroll
        for (u32 j = k >> 1; j >= 1; j >>= 1) {
            if (j >= (u32)E) {  // partner in another lane
                const u32 lj = j / E;
                const bool upper = (lane & lj) != 0u;
                const bool asc = ((lane * E) & k) == 0u;  // k >= 2 E here: the bit lies in the lane number
#pragma unroll
                for (int r = 0; r < E; r++) {
                    const u64 y = __shfl_xor(w[r], (int)lj);
                    const u64 lo = w[r] < y ? w[r] : y, hi = w[r] < y ? y : w[r];
                    w[r] = (upper == asc) ? hi : lo;
                }
            } else {  // partner in the same lane
#pragma unroll
                for (int r = 0; r < E; r++) {
                    if (!(r & j)) {
                        const bool asc = ((lane * E + r) & k) == 0u;
                        const u64 x = w[r], y = w[r | j];
                        const u64 lo = x < y ? x : y, hi = x < y ? y : x;
                        w[r] = asc ? lo : hi;
                        w[r | j] = asc ? hi : lo;
                    }
                }
            }
        }
    }
}

// per-wave LDS
struct WrLds {
    u64 pl[WR_G];       // payloads by position (permutation / compaction buffer)
    u16 aux[WR_G];      // slot of a position (offset from the window start)
    u8 hd[WR_G];        // compaction: head flags of the positions
};

// smallest set bit position >= p in the wave's window bitmap (33 words), WR_FAR if none
__device__ __forceinline__ u32 wr_next_head(const u32 * hb, u32 p) {
    const u32 lane = (u32)lane_id();
    u32 word = lane < 33u ? hb[lane] : 0u;
    const u32 wp = p >> 5;
    if (lane < wp) word = 0;
    else if (lane == wp) word &= 0xFFFFFFFFu << (p & 31u);
    const u64 any = __ballot(word != 0u);
    if (!any) return WR_FAR;
    const int l = __ffsll((unsigned long long)any) - 1;
    const u32 wv = bw_readlane(word, l);
    return (u32)l * 32u + (u32)(__ffs(wv) - 1);
}
// largest set bit position <= t
__device__ __forceinline__ u32 wr_prev_head(const u32 * hb, u32 t) {
    const u32 lane = (u32)lane_id();
    u32 word = lane < 33u ? hb[lane] : 0u;
    const u32 wp = t >> 5;
    if (lane > wp) word = 0;
    else if (lane == wp) word &= 0xFFFFFFFFu >> (31u - (t & 31u));
    const u64 any = __ballot(word != 0u);
    if (!any) return WR_FAR;
    const int l = 63 - __clzll((unsigned long long)any);
    const u32 wv = bw_readlane(word, l);
    return (u32)l * 32u + (31u - (u32)__clz(wv));
}

struct WrCtx {
    const u8 * t;
    u32 n;
    u32 * v;
    u8 * pb;
    const u32 * tab;
    u32 * counters;
    u32 chain;
    u64 slot0;  // global slot of window position 0
    u32 * tail_v;
    u32 * tail_slot;
    u16 * tail_d;
    u8 * tail_pb;
    u32 tail_cap;
};

// One batch: window positions [c, c + L) (whole groups, L <= 512), E = suffixes per lane.  Returns when every group is resolved (or the
// step cap is reached: the groups are written back as they are and counted as given up).
template <int E>
__device__ __forceinline__ u32 wr_run(const WrCtx & cx, WrLds & lds, u64 (&pl)[E], u32 hm, u32 L, u32 step);

// the `total` ambiguous suffixes a shrink left in the wave's LDS buffer, E2 per lane
template <int E2>
__device__ __forceinline__ u32 wr_reload(const WrCtx & cx, WrLds & lds, u32 total, u32 step) {
    const u32 lane = (u32)lane_id();
    u64 q[E2];
    u32 h2 = 0;
#pragma unroll
    for (int r = 0; r < E2; r++) {
        const u32 j = lane * E2 + r;
        const bool in = j < total;
        q[r] = in ? lds.pl[j] : 0ull;
        h2 |= (in ? (u32)lds.hd[j] : 1u) << r;
    }
    wave_sync();
    return wr_run<E2>(cx, lds, q, h2, total, step);
}

// Returns the number of suffixes it left in lds.pl / aux / hd for the tail list (0: the batch is done).
template <int E>
__device__ __forceinline__ u32 wr_run(const WrCtx & cx, WrLds & lds, u64 (&pl)[E], u32 hm, u32 L, u32 step) {
    // pl[r] / bit r of hm: payload and head flag of position j = lane * E + r; lds.aux[j] = the position's slot (offset from cx.slot0);
    // positions >= L are heads without content
    const u32 lane = (u32)lane_id();
    for (;; step++) {
        // ---- which positions still share a group: not (head and followed by a head)
        const u32 nxt0 = __shfl_down(hm & 1u, 1u);
        const u32 hnext = (hm >> 1) | ((lane == 63u ? 1u : nxt0) << (E - 1));
        u32 amb = ~(hm & hnext) & ((1u << E) - 1u);
#pragma unroll
        for (int r = 0; r < E; r++)
            if (lane * E + r >= L) amb &= ~(1u << r);
        const u32 ambs = (u32)__popc(amb);
        const u32 total = wave_sum(ambs);
        if (total == 0u || step >= (u32)WR_CAP) {
            // ---- out: every position of the batch (a suffix alone in its group is final)
#pragma unroll
            for (int r = 0; r < E; r++)
                if (lane * E + r < L) {
                    const u64 p = cx.slot0 + lds.aux[lane * E + r];
                    const u32 sv = pl_v(pl[r]);
                    cx.v[p] = sv | (((hm >> r) & 1u) ? V_HEAD : 0u);
                    cx.pb[p] = (u8)pl_p(pl[r]);
                    if (sv == 0u) cx.counters[2] = (u32)p;
                }
            if (total && lane == 0) atomicAdd(&cx.counters[1], total);
            return 0u;
        }
        // ---- group starts (running maximum of the head positions) and the largest group
        u32 lasth = 0;  // 1 + position of this lane's last head
#pragma unroll
        for (int r = 0; r < E; r++)
            if ((hm >> r) & 1u) lasth = lane * E + r + 1u;
        u32 run0 = wave_incl_max(lasth);
        run0 = __shfl_up(run0, 1u);
        if (lane == 0) run0 = 0;  // (position 0 is a head)
        u32 span = 0;  // largest distance of a position from its group's head
        {
            u32 rn = run0;
#pragma unroll
            for (int r = 0; r < E; r++) {
                const u32 j = lane * E + r;
                if ((hm >> r) & 1u) rn = j + 1u;
                if (j < L && j + 1u - rn > span) span = j + 1u - rn;
            }
        }
        const bool small_groups = wave_max(span) < 64u && step > 0u;  // every group has at most 64 members: the tail kernel's
        u32 run = run0;
        if (small_groups || total <= 32u * E) {
            // ---- shrink: the final ones out, the others move up into half (or less) of the lanes' capacity
            const u32 before = wave_incl_add(ambs) - ambs;
            u32 so[E];
#pragma unroll
            for (int r = 0; r < E; r++) so[r] = lane * E + r < L ? (u32)lds.aux[lane * E + r] : 0u;
            wave_sync();  // every lane has read the slots of its positions before any is overwritten
            u32 d = before;
#pragma unroll
            for (int r = 0; r < E; r++) {
                if (lane * E + r < L) {
                    if ((amb >> r) & 1u) {
                        lds.pl[d] = pl[r];
                        lds.aux[d] = (u16)so[r];
                        lds.hd[d] = (u8)((hm >> r) & 1u);
                        d++;
                    } else {
                        const u64 p = cx.slot0 + so[r];
                        const u32 sv = pl_v(pl[r]);
                        cx.v[p] = sv | V_HEAD;
                        cx.pb[p] = (u8)pl_p(pl[r]);
                        if (sv == 0u) cx.counters[2] = (u32)p;
                    }
                }
            }
            wave_sync();
            // continue with the smallest capacity that holds them
            if (small_groups || total <= 64u) return total;  // the rest is the tail kernel's: the caller appends lds.pl / aux / hd [0, total) to its list
            if constexpr (E == 8) {
                if (total > 128u) return wr_reload<4>(cx, lds, total, step);
                return wr_reload<2>(cx, lds, total, step);
            }
            if constexpr (E == 4) return wr_reload<2>(cx, lds, total, step);
        }
        // ---- next code bits of the ambiguous suffixes, four suffixes of a lane at a time (their windows in flight together: with all eight
        // the kernel needs every register a wave can have, and one wave per SIMD hides no latency at all)
        constexpr int CH = E < 4 ? E : 4;
        u64 w[E];
#pragma unroll
        for (int r0 = 0; r0 < E; r0 += CH) {
            u64 wa[CH], wb[CH];
            u32 avl[CH], dep[CH];
#pragma unroll
            for (int k = 0; k < CH; k++) dep[k] = pl_d(pl[r0 + k]);
            if (step == 0) {
                // depth = the symbols inside the 56-bit windows the group was formed on: one from the sort of all suffixes, one more per
                // big round its members went through.  Every member walks the same symbols, so all arrive at the same depth (a member
                // whose text ends on the way arrives at the end and sorts first).
                for (u32 hop = 0; hop < cx.chain; hop++) {
#pragma unroll
                    for (int k = 0; k < CH; k++) load_window(cx.t, (u64)pl_v(pl[r0 + k]) + dep[k], cx.n, wa[k], wb[k], avl[k]);
#pragma unroll
                    for (int k = 0; k < CH; k++) {
                        u64 k56;
                        u32 cnt;
                        vlc_pack<56>(cx.tab, wa[k], wb[k], avl[k], k56, cnt);
                        dep[k] += ((amb >> (r0 + k)) & 1u) ? cnt : 0u;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < CH; k++) load_window(cx.t, (u64)pl_v(pl[r0 + k]) + dep[k], cx.n, wa[k], wb[k], avl[k]);
#pragma unroll
            for (int k = 0; k < CH; k++) {
                const int r = r0 + k;
                const u32 j = lane * E + r;
                if ((hm >> r) & 1u) run = j + 1u;
                const u32 gs = run - 1u;
                u64 key;
                u32 cnt;
                vlc_pack<WW_KEY, 12>(cx.tab, wa[k], wb[k], avl[k], key, cnt);
                const u32 sv = pl_v(pl[r]);
                const bool live = (u64)sv + dep[k] < cx.n;
                if (!live) {
                    key = (u64)(cx.n - sv);  // ended: shorter first
                    cnt = 0;
                }
                const bool am = (amb >> r) & 1u;
                w[r] = am ? ww_make(gs, live, key, j) : ww_make(j < L ? j : (u32)(64 * E - 1), false, 0ull, j);  // a final suffix stays where it is
                if (am) pl[r] = pl_make(sv, dep[k] + cnt, pl_p(pl[r]));
            }
        }
        // ---- sort; the payloads follow
#pragma unroll
        for (int r = 0; r < E; r++) lds.pl[lane * E + r] = pl[r];
        wave_bitonic<E>(w);
        wave_sync();
#pragma unroll
        for (int r = 0; r < E; r++) pl[r] = lds.pl[(u32)w[r] & ((1u << WW_IDX) - 1u)];
        wave_sync();
        // ---- new heads: where the word (without the position) differs from the left neighbour's
        const u64 left = __shfl_up(w[E - 1], 1u);
#pragma unroll
        for (int r = 0; r < E; r++) {
            const u64 prev = r ? w[r - 1] : left;
            if ((w[r] >> WW_IDX) != (prev >> WW_IDX)) hm |= 1u << r;  // (lane 0, r = 0 compares with its own last word: it is a head already)
        }
    }
}

template <int E>
__device__ __forceinline__ u32 wr_batch(const WrCtx & cx, WrLds & lds, u32 L) {  // ONE group: slots cx.slot0 .. + L
    const u32 lane = (u32)lane_id();
    u64 pl[E];
    u32 hm = 0;
    u32 xv[E];
    u8 xp[E];
#pragma unroll
    for (int r = 0; r < E; r++) {
        const u32 j = lane * E + r;
        const u64 p = cx.slot0 + (j < L ? j : L - 1u);
        xv[r] = cx.v[p];
        xp[r] = cx.pb[p];
    }
#pragma unroll
    for (int r = 0; r < E; r++) {
        const u32 j = lane * E + r;
        const bool in = j < L;
        hm |= ((in && j > 0u) ? 0u : 1u) << r;  // the group's head; positions past it are heads without content
        pl[r] = in ? pl_make(xv[r] & V_MASK, 0u, xp[r]) : 0ull;
        lds.aux[j] = (u16)(in ? j : 0u);
    }
    wave_sync();
    return wr_run<E>(cx, lds, pl, hm, L, 0u);
}

// The router: one wave per 512 anchor slots looks at the head bits and sends every group headed there where it belongs --
//   up to 64 members   : its ambiguous suffixes to the tail list (k_bwt_tail)
//   65 .. 512 members  : a (head slot, size) descriptor to the mid list (k_bwt_wide)
//   more               : its slots to the big list (k_big_*)
// It keeps nothing but a 33-word bitmap per wave, so dozens of waves share a CU (the first version did the wide work in the same
// kernel and ran two waves per SIMD: 13 ms instead of 3).
constexpr int RT_WAVES = 16;  // waves per router workgroup: one append to each list per WORKGROUP (an append per wave made the
                              // lists' counters the bottleneck: a single word takes ~90 atomics per microsecond)
struct RtLds {
    u32 hb[36];     // head bits of the window [a, a + 1024]
    u16 lg_c[10];   // groups of more than 64 headed in the anchor slots (at most 7) and the run that enters from the left: start ...
    u16 lg_e[10];   // ... end (exclusive, clipped to the anchor slots for the big ones) ...
    u32 lg_hp[10];  // ... and for the big ones the group's head slot; 0xFFFFFFFF marks a mid-size group (a descriptor)
    u32 cnt[4];     // what this wave appends: [0] tail entries, [1] mid descriptors, [2] big slots
    u32 base[4];    // where
};
#define ROUTE_ARGS(X) X(u32, n) X(const u32 * __restrict__, v) X(const u8 * __restrict__, pb) X(const u32 * __restrict__, hbits) X(const u32 * __restrict__, carry_local) X(const u32 * __restrict__, group_carry) X(const u8 * __restrict__, dirty) X(u32 * __restrict__, big_slot) X(u32 * __restrict__, big_hp) X(u32, big_cap) X(u32 * __restrict__, mid_slot) X(u16 * __restrict__, mid_size) X(u32, mid_cap) X(u32 * __restrict__, tail_v) X(u32 * __restrict__, tail_slot) X(u16 * __restrict__, tail_d) X(u8 * __restrict__, tail_pb) X(u32, tail_cap) X(u32 * __restrict__, counters)
BWT_JOB(RouteJob, ROUTE_ARGS);
__global__ void __launch_bounds__(RT_WAVES * WAVE) k_bwt_route(u32 n, const u32 * __restrict__ v, const u8 * __restrict__ pb, const u32 * __restrict__ hbits,
                                                              const u32 * __restrict__ carry_local, const u32 * __restrict__ group_carry,
                                                              const u8 * __restrict__ dirty, u32 * __restrict__ big_slot, u32 * __restrict__ big_hp, u32 big_cap,
                                                              u32 * __restrict__ mid_slot, u16 * __restrict__ mid_size, u32 mid_cap, u32 * __restrict__ tail_v,
                                                              u32 * __restrict__ tail_slot, u16 * __restrict__ tail_d, u8 * __restrict__ tail_pb, u32 tail_cap,
                                                              u32 * __restrict__ counters) {
    const u32 grid_x = gridDim.x;
    (void)grid_x;
#include "bwt_route_body.hpp"  // (shared with k_bwt_route_many by inclusion: see the file)
}
__global__ void __launch_bounds__(RT_WAVES * WAVE) k_bwt_route_many(JobTab<RouteJob> jobs_) {
    BWT_ENTER(RouteJob, ROUTE_ARGS)
    const u32 grid_x = job_.grid_;
    (void)grid_x;
#include "bwt_route_body.hpp"  // (k_bwt_route's body, on the names declared above)
}

// The wide kernel: one wave per group of 65 .. 512 suffixes (a descriptor of the router), 2 / 4 / 8 suffixes per lane in registers.
// A step or two later its sub-groups have at most 64 members and go to the tail list.
#define WIDE_ARGS(X) X(const u8 * __restrict__, t) X(u32, n) X(u32 * __restrict__, v) X(u8 * __restrict__, pb) X(const u32 * __restrict__, vlc) X(const u32 * __restrict__, mid_slot) X(const u16 * __restrict__, mid_size) X(u32, mid_cap) X(u32 * __restrict__, tail_v) X(u32 * __restrict__, tail_slot) X(u16 * __restrict__, tail_d) X(u8 * __restrict__, tail_pb) X(u32, tail_cap) X(u32 * __restrict__, counters) X(u32, chain)
BWT_JOB(WideJob, WIDE_ARGS);
__global__ void __launch_bounds__(WR_WAVES * WAVE) k_bwt_wide(const u8 * __restrict__ t, u32 n, u32 * __restrict__ v, u8 * __restrict__ pb, const u32 * __restrict__ vlc,
                                                             const u32 * __restrict__ mid_slot, const u16 * __restrict__ mid_size, u32 mid_cap, u32 * __restrict__ tail_v,
                                                             u32 * __restrict__ tail_slot, u16 * __restrict__ tail_d, u8 * __restrict__ tail_pb, u32 tail_cap,
                                                             u32 * __restrict__ counters, u32 chain) {
    const u32 grid_x = gridDim.x;
    (void)grid_x;
#include "bwt_wide_body.hpp"  // (shared with k_bwt_wide_many by inclusion: see the file)
}
__global__ void __launch_bounds__(WR_WAVES * WAVE) k_bwt_wide_many(JobTab<WideJob> jobs_) {
    BWT_ENTER(WideJob, WIDE_ARGS)
    const u32 grid_x = job_.grid_;
    (void)grid_x;
#include "bwt_wide_body.hpp"  // (k_bwt_wide's body, on the names declared above)
}

// ---- the tail: tiny groups that need many more windows ---------------------------------------------------------------------------
// What the resolve kernel hands over: batches that are down to <= 64 ambiguous suffixes (and batches that never had more).  They sit
// in one global list, every batch a run of whole groups that starts with a head.  One wave per 64 list entries takes the groups
// whose head lies in its entries (a group has at most 64 members: they end within the next 64 entries), a lane per suffix, as many
// whole groups at a time as fit the 64 lanes.  A step costs one gather from the text and a handful of cross-lane operations; nothing
// in it waits for another wave, and with ~50 registers and 2 KB of LDS dozens of these waves share a CU, so the gather latency of
// one is covered by the others -- which the resolve kernel, with eight suffixes per lane in registers, cannot offer.
#define TAIL_ARGS(X) X(const u8 * __restrict__, t) X(u32, n) X(u32 * __restrict__, v) X(u8 * __restrict__, pb) X(const u32 * __restrict__, vlc) X(const u32 * __restrict__, tail_v) X(const u32 * __restrict__, tail_slot) X(const u16 * __restrict__, tail_d) X(const u8 * __restrict__, tail_pb) X(u32 * __restrict__, counters) X(u32, chain)
BWT_JOB(TailJob, TAIL_ARGS);
__global__ void __launch_bounds__(WAVE) k_bwt_tail(const u8 * __restrict__ t, u32 n, u32 * __restrict__ v, u8 * __restrict__ pb, const u32 * __restrict__ vlc,
                                                  const u32 * __restrict__ tail_v, const u32 * __restrict__ tail_slot, const u16 * __restrict__ tail_d,
                                                  const u8 * __restrict__ tail_pb, u32 * __restrict__ counters, u32 chain) {
    const u32 grid_x = gridDim.x;
    (void)grid_x;
#include "bwt_tail_body.hpp"  // (shared with k_bwt_tail_many by inclusion: see the file)
}
__global__ void __launch_bounds__(WAVE) k_bwt_tail_many(JobTab<TailJob> jobs_) {
    BWT_ENTER(TailJob, TAIL_ARGS)
    const u32 grid_x = job_.grid_;
    (void)grid_x;
#include "bwt_tail_body.hpp"  // (k_bwt_tail's body, on the names declared above)
}

// ---- the big path: one more window for the members of groups too large for the resolve kernel --------------------------------
#define BIG_KEYS_ARGS(X) X(const u8 * __restrict__, t) X(u32, n) X(const u32 * __restrict__, v) X(const u32 * __restrict__, vlc) X(const u32 * __restrict__, big_slot) X(u32, nb) X(u32, chain) X(u64 * __restrict__, keys)
BWT_JOB(BigKeysJob, BIG_KEYS_ARGS);
__global__ void __launch_bounds__(BW_BLOCK) k_big_keys(JobTab<BigKeysJob> jobs_) {
    BWT_ENTER(BigKeysJob, BIG_KEYS_ARGS)
    __shared__ u32 tab[256];
    tab[threadIdx.x] = vlc[threadIdx.x];
    __syncthreads();
    const u32 i = blockIdx.x * BW_BLOCK + threadIdx.x;
    if (i >= nb) return;
    const u32 s = v[big_slot[i]] & V_MASK;
    u64 pos = s;
    u64 wa, wb, key;
    u32 avl, cnt;
    for (u32 hop = 0; hop < chain; hop++) {  // past the windows the group was formed on (cf. k_bwt_tail's `fresh` entries)
        load_window(t, pos, n, wa, wb, avl);
        vlc_pack<56>(tab, wa, wb, avl, key, cnt);
        pos += cnt;
    }
    load_window(t, pos, n, wa, wb, avl);
    vlc_pack<56>(tab, wa, wb, avl, key, cnt);
    const bool live = pos < n;
    keys[i] = live ? ((1ull << 56) | key) : (u64)(n - s);
}

// after the two sorts: order[j] = index into the big list of the element that comes j-th; collect what moves
#define BIG_GATHER_ARGS(X) X(const u32 * __restrict__, order) X(const u32 * __restrict__, big_slot) X(const u32 * __restrict__, big_hp) X(const u64 * __restrict__, keys) X(const u32 * __restrict__, v) X(const u8 * __restrict__, pb) X(u32, nb) X(u32 * __restrict__, gv) X(u8 * __restrict__, gpb) X(u64 * __restrict__, gkey) X(u32 * __restrict__, ghp)
BWT_JOB(BigGatherJob, BIG_GATHER_ARGS);
__global__ void __launch_bounds__(BW_BLOCK) k_big_gather(JobTab<BigGatherJob> jobs_) {
    BWT_ENTER(BigGatherJob, BIG_GATHER_ARGS)
    const u32 j = blockIdx.x * BW_BLOCK + threadIdx.x;
    if (j >= nb) return;
    const u32 src = order[j];
    const u32 slot = big_slot[src];
    gv[j] = v[slot] & V_MASK;
    gpb[j] = pb[slot];
    gkey[j] = keys[src];
    ghp[j] = big_hp[src];
}
#define BIG_ORDER_KEYS_ARGS(X) X(const u32 * __restrict__, order) X(const u32 * __restrict__, big_hp) X(u32, nb) X(u32 * __restrict__, out)
BWT_JOB(BigOrderKeysJob, BIG_ORDER_KEYS_ARGS);
__global__ void __launch_bounds__(BW_BLOCK) k_big_order_keys(JobTab<BigOrderKeysJob> jobs_) {
    BWT_ENTER(BigOrderKeysJob, BIG_ORDER_KEYS_ARGS)
    const u32 j = blockIdx.x * BW_BLOCK + threadIdx.x;
    if (j < nb) out[j] = big_hp[order[j]];
}
// the j-th element of the sorted list goes to the j-th smallest slot of the list
#define BIG_APPLY_ARGS(X) X(const u32 * __restrict__, sorted_slots) X(const u32 * __restrict__, gv) X(const u8 * __restrict__, gpb) X(const u64 * __restrict__, gkey) X(const u32 * __restrict__, ghp) X(u32, nb) X(u32 * __restrict__, v) X(u8 * __restrict__, pb) X(u8 * __restrict__, dirty) X(u32 * __restrict__, counters)
BWT_JOB(BigApplyJob, BIG_APPLY_ARGS);
__global__ void __launch_bounds__(BW_BLOCK) k_big_apply(JobTab<BigApplyJob> jobs_) {
    BWT_ENTER(BigApplyJob, BIG_APPLY_ARGS)
    const u32 j = blockIdx.x * BW_BLOCK + threadIdx.x;
    if (j >= nb) return;
    const bool head = j == 0 || ghp[j] != ghp[j - 1] || gkey[j] != gkey[j - 1];
    const u32 slot = sorted_slots[j];
    const u32 s = gv[j];
    v[slot] = s | (head ? V_HEAD : 0u);
    pb[slot] = gpb[j];
    dirty[slot / (u32)TR_S] = 1;
    if (s == 0) counters[2] = slot;
}

// U from the payload bytes: U[0] = T[n-1], slot i0 (suffix 0) is skipped.
#define FINISH_ARGS(X) X(const u8 * __restrict__, t) X(const u8 * __restrict__, pb) X(u32, n) X(const u32 * __restrict__, slot_of_suffix0) X(u8 * __restrict__, out) X(u32 * __restrict__, idx_out)
BWT_JOB(FinishJob, FINISH_ARGS);
__global__ void __launch_bounds__(BW_BLOCK) k_bwt_finish(JobTab<FinishJob> jobs_) {
    BWT_ENTER(FinishJob, FINISH_ARGS)
    const u32 i = blockIdx.x * BW_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 i0 = *slot_of_suffix0;
    if (i == 0) {
        out[0] = t[n - 1];
        *idx_out = i0 + 1;
    }
    if (i != i0) out[i < i0 ? i + 1 : i] = pb[i];
}

// ---- the deep path: prefix doubling on ranks -----------------------------------------------------------------------------------
// Regrouping of a sorted list in two passes over tiles of 2048 elements (8 consecutive elements per thread) and a one-workgroup spine:
//   reduce : per tile, the position of its last group head and the number of elements that stay active
//   spine  : exclusive running maximum / sum over the tiles
//   apply  : in-tile running maximum of the head positions (+ the tile's carry) gives every element its group head, hence its rank;
//            in-tile sum of the keep flags (+ the tile's offset) gives the slot in the compacted list; writes SA / ISA and the
//            compacted (suffix, slot, rank) triples -- the rank rides along so that the next keys need one gather instead of two.
// The list is described either by its sorted 64-bit keys (a doubling round) or by the head flags in V (entry from the resolve passes).
constexpr int BG_ITEMS = 8;
constexpr int BG_TILE = BW_BLOCK * BG_ITEMS;
struct alignas(16) BgU64x2 { u64 x, y; };
struct alignas(16) BgU32x4 { u32 x, y, z, w; };

// kv[j + 1] = keys[base + j] for j = -1 .. BG_ITEMS (indices clamped into [0, m - 1]: a clamped copy only ever meets a flag test
// that is overridden by its own bounds check).  Whole tiles: four 16-byte loads + the two neighbours, all in flight together.
__device__ __forceinline__ void bg_load_keys(const u64 * __restrict__ keys, u32 m, u64 base, u64 (&kv)[BG_ITEMS + 2]) {
    const u64 last = (u64)m - 1;
    kv[0] = keys[base > 0 ? (base - 1 < last ? base - 1 : last) : 0];
    kv[BG_ITEMS + 1] = keys[base + BG_ITEMS < last ? base + BG_ITEMS : last];
    if (base + BG_ITEMS <= m) {
        const BgU64x2 * __restrict__ q = reinterpret_cast<const BgU64x2 *>(keys + base);  // base is a multiple of 8 elements, the array 256-byte aligned
#pragma unroll
        for (int j = 0; j < BG_ITEMS / 2; j++) {
            const BgU64x2 t = q[j];
            kv[1 + 2 * j] = t.x;
            kv[2 + 2 * j] = t.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < BG_ITEMS; j++) kv[1 + j] = keys[base + j < last ? base + j : last];
    }
}
__device__ __forceinline__ void bg_load_u32(const u32 * __restrict__ a, u32 m, u64 base, u32 (&v)[BG_ITEMS]) {
    if (base + BG_ITEMS <= m) {
        const BgU32x4 * __restrict__ q = reinterpret_cast<const BgU32x4 *>(a + base);
        const BgU32x4 t0 = q[0], t1 = q[1];
        v[0] = t0.x; v[1] = t0.y; v[2] = t0.z; v[3] = t0.w;
        v[4] = t1.x; v[5] = t1.y; v[6] = t1.z; v[7] = t1.w;
    } else {
        const u64 last = (u64)m - 1;
#pragma unroll
        for (int j = 0; j < BG_ITEMS; j++) v[j] = a[base + j < last ? base + j : last];
    }
}
// Head / unique flags of the BG_ITEMS elements at base (bit j), from the keys or (VF) from the head flags in `vals`; elements past m: 0.
template <bool VF>
__device__ __forceinline__ void bg_flags(const u64 * __restrict__ keys, const u32 * __restrict__ vals, u32 m, u64 base, u32 & heads, u32 & uniqs) {
    heads = uniqs = 0;
    if (VF) {
        u32 v[BG_ITEMS];
        const u64 lb = base < m ? base : (u64)m - 1;
        bg_load_u32(vals, m, lb, v);
        const u32 nxt = vals[base + BG_ITEMS < (u64)m ? base + BG_ITEMS : (u64)m - 1];
#pragma unroll
        for (int j = 0; j < BG_ITEMS; j++) {
            const u64 k = base + j;
            if (k < m) {
                const bool head = v[j] >> 31;
                const bool nh = k + 1 == (u64)m || ((j + 1 < BG_ITEMS ? v[j + 1 < BG_ITEMS ? j + 1 : j] : nxt) >> 31);
                heads |= (head ? 1u : 0u) << j;
                uniqs |= ((head && nh) ? 1u : 0u) << j;
            }
        }
    } else {
        u64 kv[BG_ITEMS + 2];
        bg_load_keys(keys, m, base < m ? base : (u64)m - 1, kv);
#pragma unroll
        for (int j = 0; j < BG_ITEMS; j++) {
            const u64 k = base + j;
            if (k < m) {
                const bool head = k == 0 || kv[j + 1] != kv[j];
                const bool uniq = head && (k + 1 == (u64)m || kv[j + 2] != kv[j + 1]);
                heads |= (head ? 1u : 0u) << j;
                uniqs |= (uniq ? 1u : 0u) << j;
            }
        }
    }
}

#define BG_REDUCE_ARGS(X) X(const u64 * __restrict__, keys) X(const u32 * __restrict__, vals) X(u32, m) X(u32 * __restrict__, tile_head) X(u32 * __restrict__, tile_keep)
BWT_JOB(BgReduceJob, BG_REDUCE_ARGS);
template <bool VF>
__global__ void __launch_bounds__(BW_BLOCK) k_bg_reduce(JobTab<BgReduceJob> jobs_) {
    BWT_ENTER(BgReduceJob, BG_REDUCE_ARGS)
    __shared__ u32 lds[BW_BLOCK / WAVE + 1];
    const u64 base = (u64)blockIdx.x * BG_TILE + (u64)threadIdx.x * BG_ITEMS;
    u32 heads, uniqs;
    bg_flags<VF>(keys, vals, m, base, heads, uniqs);
    u32 hp = 0, keep = 0;  // hp = 1 + position of the last head seen (0 = none)
#pragma unroll
    for (int j = 0; j < BG_ITEMS; j++) {
        const u64 k = base + j;
        if (k < m) {
            if ((heads >> j) & 1u) hp = (u32)k + 1u;
            keep += ((uniqs >> j) & 1u) ? 0u : 1u;
        }
    }
    hp = block_max<BW_BLOCK>(hp, lds);
    keep = block_sum<BW_BLOCK>(keep, lds);
    if (threadIdx.x == 0) {
        tile_head[blockIdx.x] = hp;
        tile_keep[blockIdx.x] = keep;
    }
}

template <int BLOCK>
__device__ __forceinline__ u32 bg_block_excl_max(u32 v, u32 * lds) {  // lds: BLOCK / 64 words; ends with a barrier
    const u32 incl = wave_incl_max(v);
    if (lane_id() == WAVE - 1) lds[wave_id()] = incl;
    u32 up = __shfl_up(incl, 1u);
    if (lane_id() == 0) up = 0u;
    __syncthreads();
    u32 carry = 0;
    for (int w = 0; w < wave_id(); w++) carry = lds[w] > carry ? lds[w] : carry;
    __syncthreads();
    return up > carry ? up : carry;
}

// One workgroup: tile_head[t] <- maximum over the tiles before t, tile_keep[t] <- sum over the tiles before t, *total <- sum of all.
constexpr int BG_SPINE = 1024;
#define BG_SPINE_ARGS(X) X(u32 * __restrict__, tile_head) X(u32 * __restrict__, tile_keep) X(u32, tiles) X(u32 * __restrict__, total)
BWT_JOB(BgSpineJob, BG_SPINE_ARGS);
__global__ void __launch_bounds__(BG_SPINE) k_bg_spine(JobTab<BgSpineJob> jobs_) {
    BWT_ENTER(BgSpineJob, BG_SPINE_ARGS)
    __shared__ u32 lds[BG_SPINE / WAVE + 1];
    // a thread owns `per` consecutive tiles and walks them eight at a time, the loads of a batch in flight together (up to 256
    // tiles per thread at 511 MiB: one exposed round trip per tile would cost more than the passes this kernel sits between)
    const u32 per = (((tiles + BG_SPINE - 1) / BG_SPINE) + 7u) & ~7u;
    const u32 t0 = threadIdx.x * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    u32 hp = 0, sum = 0;
    for (u32 t = t0; t < t1; t += 8) {
        u32 h[8], c[8];
#pragma unroll
        for (u32 k = 0; k < 8; k++) {
            const u32 i = t + k < t1 ? t + k : t1 - 1u;  // never another thread's entries
            h[k] = tile_head[i];
            c[k] = tile_keep[i];
        }
#pragma unroll
        for (u32 k = 0; k < 8; k++)
            if (t + k < t1) {
                hp = h[k] > hp ? h[k] : hp;
                sum += c[k];
            }
    }
    u32 run_hp = bg_block_excl_max<BG_SPINE>(hp, lds);
    u32 all;
    u32 run_sum = block_excl_add<BG_SPINE>(sum, lds, all);
    for (u32 t = t0; t < t1; t += 8) {
        u32 h[8], c[8];
#pragma unroll
        for (u32 k = 0; k < 8; k++) {
            const u32 i = t + k < t1 ? t + k : t1 - 1u;
            h[k] = tile_head[i];
            c[k] = tile_keep[i];
        }
#pragma unroll
        for (u32 k = 0; k < 8; k++)
            if (t + k < t1) {
                tile_head[t + k] = run_hp;
                tile_keep[t + k] = run_sum;
                run_hp = h[k] > run_hp ? h[k] : run_hp;
                run_sum += c[k];
            }
    }
    if (threadIdx.x == 0) *total = all;
}

// DOUBLING: the upper key word is the suffix's current rank (k_bwt_doubling_keys_grp), and the first sub-group of a group keeps it: no store.
#define BG_APPLY_ARGS(X)                                                                                                                      \
    X(const u64 * __restrict__, keys) X(const u32 * __restrict__, vals) X(const u32 * __restrict__, slots) X(u32, m)                          \
    X(const u32 * __restrict__, tile_head) X(const u32 * __restrict__, tile_keep) X(u32 * __restrict__, sa) X(u32 * __restrict__, isa)        \
    X(u32 * __restrict__, vals_out) X(u32 * __restrict__, slots_out) X(u32 * __restrict__, grp_out) X(const u8 * __restrict__, t)             \
    X(u8 * __restrict__, pb) X(u32 * __restrict__, rank_out)
BWT_JOB(BgApplyJob, BG_APPLY_ARGS);
template <bool VF, bool DOUBLING>
__global__ void __launch_bounds__(BW_BLOCK) k_bg_apply(const u64 * __restrict__ keys, const u32 * __restrict__ vals, const u32 * __restrict__ slots, u32 m,
                                                      const u32 * __restrict__ tile_head, const u32 * __restrict__ tile_keep, u32 * __restrict__ sa,
                                                      u32 * __restrict__ isa, u32 * __restrict__ vals_out, u32 * __restrict__ slots_out, u32 * __restrict__ grp_out,
                                                      const u8 * __restrict__ t, u8 * __restrict__ pb, u32 * __restrict__ rank_out) {
#include "bwt_bg_apply_body.hpp"  // (shared with k_bg_apply_many by inclusion: see the file)
}
template <bool VF, bool DOUBLING>
__global__ void __launch_bounds__(BW_BLOCK) k_bg_apply_many(JobTab<BgApplyJob> jobs_) {
    BWT_ENTER(BgApplyJob, BG_APPLY_ARGS)
#include "bwt_bg_apply_body.hpp"  // (k_bg_apply's body, on the names declared above)
}

// key(k) = (current rank of suffix s, carried along by k_bg_apply) << 32 | rank of suffix s + h;   past-the-end suffixes get
// n-1-s (< h), so that a suffix that is a proper prefix of another sorts first and two such suffixes order by length.
#define DOUBLING_KEYS_ARGS(X) X(const u32 * __restrict__, vals) X(const u32 * __restrict__, grp) X(const u32 * __restrict__, isa) X(u32, m) X(u32, n) X(u32, h) X(u64 * __restrict__, keys)
BWT_JOB(DoublingKeysJob, DOUBLING_KEYS_ARGS);
__global__ void __launch_bounds__(BW_BLOCK) k_bwt_doubling_keys_grp(JobTab<DoublingKeysJob> jobs_) {
    BWT_ENTER(DoublingKeysJob, DOUBLING_KEYS_ARGS)
    const u32 k = blockIdx.x * BW_BLOCK + threadIdx.x;
    if (k >= m) return;
    const u32 s = vals[k];
    const u64 j = (u64)s + h;
    const u32 lo = (j < n) ? isa[j] + h : (n - 1u - s);
    keys[k] = ((u64)grp[k] << 32) | lo;
}

// isa[suffix] = rank for pairs that a radix pass has bucketed by the top 8 bits of the suffix number: a bucket's destinations lie in
// a window of n / 256 words (4 MB at 256 MiB), and with a contiguous range of tiles per XCD (cf. sort.hip) the XCD's L2 absorbs the
// random stores of the bucket it is working on -- measured against n stores all over the 1 GB array: see DESIGN.md.
constexpr int IS_ITEMS = 8;
#define ISA_SCATTER_ARGS(X) X(const u32 * __restrict__, suf) X(const u32 * __restrict__, rank) X(u32, n) X(u32, tiles) X(u32 * __restrict__, isa)
BWT_JOB(IsaScatterJob, ISA_SCATTER_ARGS);
__global__ void __launch_bounds__(BW_BLOCK) k_isa_scatter(JobTab<IsaScatterJob> jobs_) {
    BWT_ENTER(IsaScatterJob, ISA_SCATTER_ARGS)
    const u32 per = (tiles + 7u) / 8u;
    const u32 tile = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
    if (tile >= tiles) return;
    const u64 base = (u64)tile * (BW_BLOCK * IS_ITEMS) + threadIdx.x;
    u32 x[IS_ITEMS], r[IS_ITEMS];
#pragma unroll
    for (int k = 0; k < IS_ITEMS; k++) {
        const u64 i = base + (u64)k * BW_BLOCK;
        x[k] = suf[i < n ? i : (u64)n - 1];
        r[k] = rank[i < n ? i : (u64)n - 1];
    }
#pragma unroll
    for (int k = 0; k < IS_ITEMS; k++)
        if (base + (u64)k * BW_BLOCK < n) isa[x[k] & V_MASK] = r[k];
}

static int bits_for(u64 x) {
    int b = 0;
    while (x) { b++; x >>= 1; }
    return b ? b : 1;
}

size_t bwt_workspace_bytes(u64 n) {
    // 2 keys (16) + 2 suffix arrays (8) + payload (1) + tail list (11) + ISA (4) + 2 slot lists (8) + ranks (4) + tile words (4) + a third suffix list (4)
    return n * (16 + 8 + 1 + 11 + 4 + 8 + 4 + 4 + 4) + n / 8 + radix_temp_bytes(n) + scan_temp_words(n) * 4 + (1u << 20) + 16384 + VLC_WORK_BYTES;
}

// Test / diagnosis switches, read from the environment ONCE (rounds 1-3 called getenv per block and per pass):
//   BZ3_BWT_TRACE=1        one line per pass on stderr
//   BZ3_BWT_BIG_ROUNDS=<k> tests only: how many more windows the big groups get before the deep path takes them (0: none; default 1);
//                          within a process: bz3_hip_debug_bwt_big_rounds(k), k < 0 = default
struct BwtSwitches {
    bool trace;
    int big_rounds_default;  // BZ3_BWT_BIG_ROUNDS as read at load (1 without it)
    std::atomic<int> big_rounds;
};
static BwtSwitches & bwt_switches() {
    static BwtSwitches sw{getenv("BZ3_BWT_TRACE") != nullptr, getenv("BZ3_BWT_BIG_ROUNDS") ? atoi(getenv("BZ3_BWT_BIG_ROUNDS")) : 1,
                          {getenv("BZ3_BWT_BIG_ROUNDS") ? atoi(getenv("BZ3_BWT_BIG_ROUNDS")) : 1}};
    return sw;
}
void bwt_set_big_rounds(int k) { bwt_switches().big_rounds.store(k < 0 ? bwt_switches().big_rounds_default : k); }  // tests: bz3_hip_debug_bwt_big_rounds (k < 0: the default as read at load)
// Grids of the wide / tail kernels: fixed by the block's size (their work lists' lengths stay on the device).  Tail: n / 256 waves, a
// quarter of what the longest possible list (n entries, 64 per wave) would take: at most four strides per wave.  Wide: n / 4096
// workgroups of WR_WAVES waves; the list holds at most n / 65 descriptors, so the worst case is ~16 strides per wave -- the lists of
// real blocks are far shorter (text: a few 10^5 descriptors at 256 MiB, one or two strides).  Call 3 of round 4 measured a tail grid of
// 24,576 waves, dozens of strides per wave, 13 % slower than the exactly sized launch of rounds 1-3.  BZ3_BWT_GRIDS="wide,tail" (read
// once) overrides: experiments.
struct BwtGrids {
    u32 wide, tail;
};
static BwtGrids bwt_grids(u32 n) {
    static const BwtGrids forced = [] {
        BwtGrids g{0, 0};
        if (const char * e = getenv("BZ3_BWT_GRIDS")) (void)sscanf(e, "%u,%u", &g.wide, &g.tail);
        return g;
    }();
    if (forced.wide && forced.tail) return forced;
    const u32 tail = n / (64u * 4u), wide = n / (64u * 4u * 16u);  // (lists: <= n entries, 64 per wave; <= n / 64 descriptors, 4 per workgroup)
    return BwtGrids{wide < 8u ? 8u : wide, tail < 32u ? 32u : tail};
}

__global__ void k_bwt_set_word(u32 * p, u32 v) { *p = v; }

// The lists a pass rebuilds start empty: [0] big elements, [4] tail entries, [5] start of the first tail append that did not fit, [8] mid descriptors.
#define RESET_WORDS_ARGS(X) X(u32 * __restrict__, counters)
BWT_JOB(ResetWordsJob, RESET_WORDS_ARGS);
__global__ void __launch_bounds__(WAVE) k_bwt_reset_words(JobTab<ResetWordsJob> jobs_) {
    BWT_ENTER(ResetWordsJob, RESET_WORDS_ARGS)
    if (threadIdx.x == 0) {
        counters[0] = 0u;
        counters[4] = 0u;
        counters[5] = 0xFFFFFFFFu;
        counters[8] = 0u;
    }
}

// ---- the host side: up to BWT_MAX_BATCH blocks through ONE launch sequence -------------------------------------------------------
// The jobs of a batch diverge (one is done after pass 0, the next needs another window, a third goes to rank doubling), so every launch is
// built from the subset of jobs that need it, each with its own extent.
struct Sel {
    u32 count = 0;
    u32 idx[BWT_MAX_BATCH];
    void add(u32 i) { idx[count++] = i; }
};
template <typename J, typename F>
static void launch_jobs(void (*kernel)(JobTab<J>), dim3 block, hipStream_t s, const Sel & sel, F make) {
    if (sel.count == 0) return;
    JobTab<J> tab{};
    u32 most = 0;
    for (u32 k = 0; k < sel.count; k++) {
        tab.job[k] = make(sel.idx[k]);
        most = tab.job[k].grid_ > most ? tab.job[k].grid_ : most;
    }
    for (u32 k = sel.count; k < BWT_MAX_BATCH; k++) tab.job[k] = tab.job[0];  // (unused entries repeat the first: no uninitialised bytes in the argument)
    launch(kernel, dim3(most, sel.count), block, 0, s, tab);
}

// Four kernels keep a single form beside the table form (bwt_*_body.hpp): one job runs, through `single`, the kernel a block alone has always run.
template <typename J, typename F, typename G>
static void launch_one_or_many(void (*many)(JobTab<J>), dim3 block, hipStream_t s, const Sel & sel, F make, G single) {
    if (sel.count == 1) single(make(sel.idx[0]));
    else launch_jobs<J>(many, block, s, sel, make);
}
template <bool VF, bool DOUBLING, typename F>
static void launch_bg_apply(hipStream_t s, const Sel & sel, F make) {
    launch_one_or_many<BgApplyJob>(k_bg_apply_many<VF, DOUBLING>, dim3(BW_BLOCK), s, sel, make, [&](const BgApplyJob & j) {
        launch(k_bg_apply<VF, DOUBLING>, dim3(j.grid_), dim3(BW_BLOCK), 0, s, j.keys, j.vals, j.slots, j.m, j.tile_head, j.tile_keep, j.sa, j.isa, j.vals_out, j.slots_out, j.grp_out,
               j.t, j.pb, j.rank_out);
    });
}

// LSD sorts of several arrays over their own key bits [bit_lo, bit_hi), pass by pass: a pass is one radix_pass_many over the arrays that
// still have a digit at that position.  iota: the first pass reads `kin`, generates the values and writes side 1.
template <typename K>
struct SortJob {
    const K * kin;
    K * k[2];
    u32 * v[2];
    u64 n;
    int bit_lo, bit_hi;
    int cur;     // out: the side that holds the result
    int passes;  // out
};
template <typename K>
static void sort_many(SortJob<K> * jobs, u32 count, bool iota, Arena & tmp, hipStream_t s) {
    for (u32 k = 0; k < count; k++) jobs[k].cur = jobs[k].passes = 0;
    for (int p = 0;; p++) {
        RadixPairJob<K> rp[BWT_MAX_BATCH];
        u32 c = 0;
        for (u32 k = 0; k < count; k++) {
            SortJob<K> & j = jobs[k];
            const int shift = j.bit_lo + 8 * p;
            if (iota && p == 0) {
                rp[c++] = RadixPairJob<K>{j.kin, j.k[1], nullptr, j.v[1], j.n, shift};
                j.cur = 1;
            } else if (shift < j.bit_hi) {
                rp[c++] = RadixPairJob<K>{j.k[j.cur], j.k[j.cur ^ 1], j.v[j.cur], j.v[j.cur ^ 1], j.n, shift};
                j.cur ^= 1;
            } else {
                continue;
            }
            j.passes++;
        }
        if (c == 0) break;
        radix_pass_many<K>(rp, c, tmp, s);
    }
}

struct FwJob {
    BwtBatchItem * item;
    const u8 * in;
    u32 n;
    u64 * key[2];
    u32 * val[2];
    u8 * pb;
    u32 tiles, sp_groups;
    u32 *tile_last, *carry, *group_max, *group_carry;
    u8 * dirty;
    u32 * hbits;
    u32 * words;  // counters [0] big elements, [1] left ambiguous by the resolve / tail kernels, [2] slot of suffix 0, [3] a list overflowed, [4] tail entries, [5] start of the first tail append that did not fit; [6] scan total, [7] primary index, [8] mid descriptors
    u32 *vlc, *hist;
    u32 * V;
    int cur;
    u32 big_cap;
    u32 *big_slot, *big_hp, *bord[2], *bgk[2], *gv, *ghp;
    u64 *bkey0, *bkey[2], *gkey;
    u8 * gpb;
    u32 tail_cap, mid_cap;
    u32 *tail_v, *tail_slot, *mid_slot;
    u16 *tail_d, *mid_size;
    u8 * tail_pb;
    u32 g;       // symbols every group is known to share at least (7 per 56-bit window)
    bool deep;   // fall back to rank doubling
    u32 nb;
    BwtGrids grids;
    BwtStats st;
    // the deep path
    u32 *isa, *slot[2], *grp, *vv[2], *tile_head, *tile_keep;
    u32 m, h;
    int scur;
    u32 *vact, *vfree;
};

void bwt_forward_batch(BwtBatchItem * items, u32 count, Arena & tmp, hipStream_t s) {
    if (count == 0 || count > BWT_MAX_BATCH) throw HipError{hipErrorUnknown, "suffix sorter batch of a size the job table does not hold", __FILE__, __LINE__};
    for (u32 k = 0; k < count; k++) {
        if (items[k].n < 2) throw HipError{hipErrorUnknown, "suffix sorter batch with a block of fewer than 2 bytes", __FILE__, __LINE__};
        if (items[k].n > V_MASK) throw HipError{hipErrorUnknown, "block too large for the suffix sorter", __FILE__, __LINE__};
    }
    const size_t mk = tmp.mark();
    // the jobs' counter words and code histograms lie side by side: one memset clears them, one copy per pass reads all the words back
    u32 * words_all = tmp.take<u32>((size_t)(16 + 256) * count);
    u32 * hist_all = words_all + 16 * (size_t)count;
    FwJob jb[BWT_MAX_BATCH];
    Sel all;
    for (u32 k = 0; k < count; k++) {  // per-job scratch, job after job
        FwJob & j = jb[k];
        j = FwJob{};
        all.add(k);
        j.item = &items[k];
        if (items[k].rec) *items[k].rec = BwtRecord{};
        j.in = items[k].in;
        const u32 n = j.n = items[k].n;
        j.key[0] = tmp.take<u64>(n);
        j.key[1] = tmp.take<u64>(n);
        j.val[0] = tmp.take<u32>(n);
        j.val[1] = tmp.take<u32>(n);
        j.pb = tmp.take<u8>(n);
        j.tiles = (u32)(((u64)n + TR_S - 1) / TR_S);
        j.tile_last = tmp.take<u32>(j.tiles + 1);
        j.carry = tmp.take<u32>(j.tiles + 1);  // carry_local
        j.sp_groups = (j.tiles + SP_GROUP - 1) / SP_GROUP;
        j.group_max = tmp.take<u32>(j.sp_groups + 1);
        j.group_carry = tmp.take<u32>(j.sp_groups + 1);
        j.dirty = tmp.take<u8>(j.tiles + 2);
        j.hbits = tmp.take<u32>(((size_t)n + 63) / 64 * 2 + (size_t)TR_S / 32 + 8);  // snapshot of the head flags, whole 64-slot words of every anchor tile
        j.vlc = tmp.take<u32>(256);
        j.words = words_all + 16 * (size_t)k;
        j.hist = hist_all + 256 * (size_t)k;
        j.g = 7;
        j.grids = bwt_grids(n);
    }
    auto grid = [](u64 m) { return (u32)((m + BW_BLOCK - 1) / BW_BLOCK); };

    // ---- codes
    HIP_CHECK(hipMemsetAsync(words_all, 0, (size_t)(16 + 256) * count * sizeof(u32), s));
    launch_jobs<ResetWordsJob>(k_bwt_reset_words, dim3(WAVE), s, all, [&](u32 k) { return ResetWordsJob{1u, jb[k].words}; });
    launch_jobs<SymHistJob>(k_bwt_sym_hist, dim3(BW_BLOCK), s, all, [&](u32 k) { return SymHistJob{grid(((u64)jb[k].n + 63) / 64), jb[k].in, jb[k].n, jb[k].hist}; });
    {
        Sel with;
        for (u32 k = 0; k < count; k++)
            if (items[k].d_outside) with.add(k);
        launch_jobs<OutsideJob>(k_bwt_outside, dim3(256), s, with, [&](u32 k) { return OutsideJob{1u, jb[k].hist, (u32)BWT_ROUTE_KEEP, items[k].d_outside}; });
    }
    {
        // the code tables: a level is one launch for all jobs (stream order protects the scratch: what reuses it is launched after the last level)
        const size_t vm = tmp.mark();
        VlcWork * w[BWT_MAX_BATCH];
        u64 * cost[BWT_MAX_BATCH][2];
        u16 * roots[BWT_MAX_BATCH];
        for (u32 k = 0; k < count; k++) {
            char * base = tmp.take<char>(VLC_WORK_BYTES);
            w[k] = reinterpret_cast<VlcWork *>(base);
            cost[k][0] = reinterpret_cast<u64 *>(base + ((sizeof(VlcWork) + 255) & ~(size_t)255));
            cost[k][1] = cost[k][0] + VLC_PLANE;
            roots[k] = reinterpret_cast<u16 *>(cost[k][1] + VLC_PLANE);
        }
        launch_jobs<VlcInitJob>(k_vlc_init, dim3(256), s, all, [&](u32 k) { return VlcInitJob{1u, jb[k].hist, w[k], cost[k][0], jb[k].vlc}; });
        for (u32 l = 1; l <= (u32)VLC_MAXLEN; l++)
            launch_jobs<VlcLevelJob>(k_vlc_level, dim3(256), s, all,
                                     [&](u32 k) { return VlcLevelJob{256u, w[k], l, cost[k][(l - 1) & 1], cost[k][l & 1], roots[k] + (size_t)l * VLC_PLANE}; });
        launch_jobs<VlcCodesJob>(k_vlc_codes, dim3(256), s, all, [&](u32 k) { return VlcCodesJob{1u, w[k], roots[k], jb[k].vlc}; });
        tmp.release(vm);
    }

    // ---- round 0: all suffixes by their first 56 code bits
    launch_jobs<VlcKeysJob>(k_bwt_vlc_keys, dim3(BW_BLOCK), s, all, [&](u32 k) { return VlcKeysJob{grid(((u64)jb[k].n + 7) / 8), jb[k].in, jb[k].n, jb[k].vlc, jb[k].key[0]}; });
    {
        SortJob<u64> sj[BWT_MAX_BATCH];
        for (u32 k = 0; k < count; k++) sj[k] = SortJob<u64>{jb[k].key[0], {jb[k].key[0], jb[k].key[1]}, {jb[k].val[0], jb[k].val[1]}, jb[k].n, 8, 64, 0, 0};
        sort_many<u64>(sj, count, true, tmp, s);
        for (u32 k = 0; k < count; k++) {
            FwJob & j = jb[k];
            j.cur = sj[k].cur;
            j.st.radix_passes += sj[k].passes;
            j.st.sorted_elements += j.n;
            j.st.rounds++;
            j.V = j.val[j.cur];
        }
    }
    launch_jobs<HeadsJob>(k_bwt_heads, dim3(BW_BLOCK), s, all,
                          [&](u32 k) { return HeadsJob{jb[k].tiles, jb[k].key[jb[k].cur], jb[k].V, jb[k].pb, jb[k].n, jb[k].tile_last, jb[k].hbits, jb[k].words}; });
    auto spines = [&](const Sel & sel) {
        launch_jobs<SpineAJob>(k_bwt_spine_a, dim3(SP_BLOCK), s, sel, [&](u32 k) { return SpineAJob{jb[k].sp_groups, jb[k].tile_last, jb[k].tiles, jb[k].carry, jb[k].group_max}; });
        launch_jobs<SpineBJob>(k_bwt_spine_b, dim3(1024), s, sel, [&](u32 k) { return SpineBJob{1u, jb[k].group_max, jb[k].sp_groups, jb[k].group_carry}; });
    };
    spines(all);

    for (u32 k = 0; k < count; k++) {
        FwJob & j = jb[k];
        const u32 n = j.n;
        // the key buffers are free from here on: the big path's lists live there
        const u32 big_cap = j.big_cap = n / 4;
        j.big_slot = reinterpret_cast<u32 *>(j.key[0]);          // n/4 words
        j.big_hp = j.big_slot + big_cap;                         // n/4 words
        j.bord[0] = j.big_hp + big_cap;                          // order / sorted slots, 2 x n/4 words   (key[0]: 4 x n/4 words = 4 n bytes of 8 n)
        j.bord[1] = j.big_hp + 2 * (size_t)big_cap;
        j.bgk[0] = j.bord[1] + big_cap;                          // group keys for the second sort        (6 n bytes)
        j.bgk[1] = j.bord[1] + 2 * (size_t)big_cap;
        j.gv = j.bgk[1] + big_cap;                               // 7 n bytes
        j.ghp = j.gv + big_cap;                                  // 8 n bytes: end of key[0]
        j.bkey0 = j.key[1];                                      // n/4 keys = 2 n bytes
        j.bkey[0] = j.bkey0 + big_cap;                           // 4 n, 6 n
        j.bkey[1] = j.bkey0 + 2 * (size_t)big_cap;
        j.gkey = j.bkey0 + 3 * (size_t)big_cap;                  // 8 n: end of key[1]
        j.gpb = reinterpret_cast<u8 *>(j.val[j.cur ^ 1]);        // the other suffix buffer is free as well
        // the tail kernel's input: every suffix that shares a group of up to 64 may be in it
        j.tail_cap = n;
        j.tail_v = tmp.take<u32>(j.tail_cap);
        j.tail_slot = tmp.take<u32>(j.tail_cap);
        j.tail_d = tmp.take<u16>(j.tail_cap);
        j.tail_pb = tmp.take<u8>(j.tail_cap);
        j.mid_cap = n / 64 + 16;  // groups of more than 64
        j.mid_slot = tmp.take<u32>(j.mid_cap);
        j.mid_size = tmp.take<u16>(j.mid_cap);
    }
    u32 h_words[16 * BWT_MAX_BATCH];
    Sel act = all;   // the jobs still in the resolve loop: they go through its passes in step
    Sel deep_jobs;
    const bool trace = bwt_switches().trace;
    for (int pass = 0; act.count; pass++) {
        const u32 chain = (u32)pass + 1u;
        launch_one_or_many<RouteJob>(k_bwt_route_many, dim3(RT_WAVES * WAVE), s, act, [&](u32 k) {
            const FwJob & j = jb[k];
            return RouteJob{(j.tiles + RT_WAVES - 1) / RT_WAVES, j.n, j.V, j.pb, j.hbits, j.carry, j.group_carry, pass ? j.dirty : nullptr, j.big_slot, j.big_hp, j.big_cap, j.mid_slot, j.mid_size,
                            j.mid_cap, j.tail_v, j.tail_slot, j.tail_d, j.tail_pb, j.tail_cap, j.words};
        }, [&](const RouteJob & j) {
            launch(k_bwt_route, dim3(j.grid_), dim3(RT_WAVES * WAVE), 0, s, j.n, j.v, j.pb, j.hbits, j.carry_local, j.group_carry, j.dirty, j.big_slot, j.big_hp, j.big_cap, j.mid_slot,
                   j.mid_size, j.mid_cap, j.tail_v, j.tail_slot, j.tail_d, j.tail_pb, j.tail_cap, j.counters);
        });
        // the wide and the tail kernel take their work lists' lengths from the counters on the device: fixed grids, ONE read-back per pass and batch
        launch_one_or_many<WideJob>(k_bwt_wide_many, dim3(WR_WAVES * WAVE), s, act, [&](u32 k) {
            const FwJob & j = jb[k];
            return WideJob{j.grids.wide, j.in, j.n, j.V, j.pb, j.vlc, j.mid_slot, j.mid_size, j.mid_cap, j.tail_v, j.tail_slot, j.tail_d, j.tail_pb, j.tail_cap, j.words, chain};
        }, [&](const WideJob & j) {
            launch(k_bwt_wide, dim3(j.grid_), dim3(WR_WAVES * WAVE), 0, s, j.t, j.n, j.v, j.pb, j.vlc, j.mid_slot, j.mid_size, j.mid_cap, j.tail_v, j.tail_slot, j.tail_d, j.tail_pb, j.tail_cap,
                   j.counters, j.chain);
        });
        launch_one_or_many<TailJob>(k_bwt_tail_many, dim3(WAVE), s, act, [&](u32 k) {
            const FwJob & j = jb[k];
            return TailJob{j.grids.tail, j.in, j.n, j.V, j.pb, j.vlc, j.tail_v, j.tail_slot, j.tail_d, j.tail_pb, j.words, chain};
        }, [&](const TailJob & j) {
            launch(k_bwt_tail, dim3(j.grid_), dim3(WAVE), 0, s, j.t, j.n, j.v, j.pb, j.vlc, j.tail_v, j.tail_slot, j.tail_d, j.tail_pb, j.counters, j.chain);
        });
        if (pass == 0)
            for (u32 k = 0; k < count; k++)  // (tests: a recorder gets the block's code table with the first read-back)
                if (items[k].rec) HIP_CHECK(hipMemcpyAsync(items[k].rec->vlc, jb[k].vlc, sizeof items[k].rec->vlc, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(h_words, words_all, (size_t)16 * count * sizeof(u32), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        const int max_big = bwt_switches().big_rounds.load();  // one more window takes text from ~12 % of its suffixes in big groups to ~1 %; what is left is deep and goes to rank doubling
        Sel more;
        for (u32 q = 0; q < act.count; q++) {
            FwJob & j = jb[act.idx[q]];
            const u32 * hw = h_words + 16 * (size_t)act.idx[q];
            const u32 nb = j.nb = hw[0];
            if (BwtRecord * r = j.item->rec)
                if (r->passes < BWT_REC_PASSES) r->pass[r->passes++] = BwtRecord::Pass{j.g, hw[0], hw[1], hw[3], hw[4], hw[5], hw[8]};
            if (trace) fprintf(stderr, "[bwt] n %u pass %d depth %u: %u suffixes in groups > %d, %u groups through the wide kernel, %u suffixes through the tail kernel, %u given up, overflow %u\n", j.n, pass, j.g, nb, TR_G, hw[8], hw[4], hw[1], hw[3]);
            if (nb == 0) {  // no group left that is too large: done, unless the resolve kernel gave some up (counted over all passes)
                j.deep = hw[1] != 0;
            } else if (hw[3] || pass >= max_big || nb > j.n / 4) {  // groups too many / too deep for windows of code bits
                j.deep = true;
            } else {
                more.add(act.idx[q]);
                continue;
            }
            if (j.deep) deep_jobs.add(act.idx[q]);
        }
        act = more;
        if (act.count == 0) break;
        // ---- one more window for the members of the big groups
        launch_jobs<BigKeysJob>(k_big_keys, dim3(BW_BLOCK), s, act, [&](u32 k) { return BigKeysJob{grid(jb[k].nb), jb[k].in, jb[k].n, jb[k].V, jb[k].vlc, jb[k].big_slot, jb[k].nb, chain, jb[k].bkey0}; });
        u32 *order[BWT_MAX_BATCH], *ofree[BWT_MAX_BATCH];
        {
            SortJob<u64> sj[BWT_MAX_BATCH];
            for (u32 q = 0; q < act.count; q++) {
                FwJob & j = jb[act.idx[q]];
                j.st.rounds++;
                j.st.sorted_elements += j.nb;
                sj[q] = SortJob<u64>{j.bkey0, {j.bkey[0], j.bkey[1]}, {j.bord[0], j.bord[1]}, j.nb, 0, 57, 0, 0};
            }
            sort_many<u64>(sj, act.count, true, tmp, s);
            for (u32 q = 0; q < act.count; q++) {
                FwJob & j = jb[act.idx[q]];
                j.st.radix_passes += sj[q].passes;
                order[act.idx[q]] = j.bord[sj[q].cur];
                ofree[act.idx[q]] = j.bord[sj[q].cur ^ 1];
            }
        }
        launch_jobs<BigOrderKeysJob>(k_big_order_keys, dim3(BW_BLOCK), s, act, [&](u32 k) { return BigOrderKeysJob{grid(jb[k].nb), order[k], jb[k].big_hp, jb[k].nb, jb[k].bgk[0]}; });
        // by the group's head slot (stable: the order inside a group stays), then the slots of the list in increasing order (the resolve kernel
        // emitted them tile by tile in no particular order): keys = slots, values unused (the order buffers are free by then)
        u32 * sorted_slots[BWT_MAX_BATCH];
        for (int which = 0; which < 2; which++) {
            SortJob<u32> sj[BWT_MAX_BATCH];
            for (u32 q = 0; q < act.count; q++) {
                FwJob & j = jb[act.idx[q]];
                if (which == 1) HIP_CHECK(hipMemcpyAsync(j.bgk[0], j.big_slot, (size_t)j.nb * 4, hipMemcpyDeviceToDevice, s));
                sj[q] = SortJob<u32>{nullptr, {j.bgk[0], j.bgk[1]}, {order[act.idx[q]], ofree[act.idx[q]]}, j.nb, 0, bits_for(j.n), 0, 0};
            }
            sort_many<u32>(sj, act.count, false, tmp, s);
            for (u32 q = 0; q < act.count; q++) {
                FwJob & j = jb[act.idx[q]];
                j.st.radix_passes += sj[q].passes;
                u32 * oo[2] = {order[act.idx[q]], ofree[act.idx[q]]};
                if (which == 0) {
                    order[act.idx[q]] = oo[sj[q].cur];
                    ofree[act.idx[q]] = oo[sj[q].cur ^ 1];
                } else {
                    sorted_slots[act.idx[q]] = j.bgk[sj[q].cur];
                }
            }
            if (which == 0)
                launch_jobs<BigGatherJob>(k_big_gather, dim3(BW_BLOCK), s, act, [&](u32 k) {
                    const FwJob & j = jb[k];
                    return BigGatherJob{grid(j.nb), order[k], j.big_slot, j.big_hp, j.bkey0, j.V, j.pb, j.nb, j.gv, j.gpb, j.gkey, j.ghp};
                });
        }
        for (u32 q = 0; q < act.count; q++) HIP_CHECK(hipMemsetAsync(jb[act.idx[q]].dirty, 0, jb[act.idx[q]].tiles + 2, s));
        launch_jobs<BigApplyJob>(k_big_apply, dim3(BW_BLOCK), s, act, [&](u32 k) {
            const FwJob & j = jb[k];
            return BigApplyJob{grid(j.nb), sorted_slots[k], j.gv, j.gpb, j.gkey, j.ghp, j.nb, j.V, j.pb, j.dirty, j.words};
        });
        for (u32 q = 0; q < act.count; q++) jb[act.idx[q]].g += 7;
        launch_jobs<ResetWordsJob>(k_bwt_reset_words, dim3(WAVE), s, act, [&](u32 k) { return ResetWordsJob{1u, jb[k].words}; });  // the big list and the tail list are rebuilt by the next pass
        launch_jobs<ReduceHeadsJob>(k_bwt_reduce_heads, dim3(BW_BLOCK), s, act, [&](u32 k) { return ReduceHeadsJob{jb[k].tiles, jb[k].V, jb[k].n, jb[k].tile_last, jb[k].hbits}; });
        spines(act);
    }

    if (deep_jobs.count) {
        // ---- deep path: ISA from the flags, then prefix doubling on (rank, rank of the suffix h further on); its buffers only for the jobs that enter it
        for (u32 q = 0; q < deep_jobs.count; q++) {
            FwJob & j = jb[deep_jobs.idx[q]];
            const u32 n = j.n;
            j.isa = tmp.take<u32>(n);
            j.slot[0] = tmp.take<u32>(n);
            j.slot[1] = tmp.take<u32>(n);
            j.grp = tmp.take<u32>(n);
            j.vv[0] = j.val[j.cur ^ 1];
            j.vv[1] = tmp.take<u32>(n);
            const u32 max_tiles = (u32)(((u64)n + BG_TILE - 1) / BG_TILE);
            j.tile_head = tmp.take<u32>(2 * (size_t)max_tiles + 16);
            j.tile_keep = j.tile_head + max_tiles + 8;
            // every group still ambiguous shares at least h symbols: 7 per window of the big rounds; a group the resolve kernel gave up
            // shares the first window's 7 and 5 more per step it took (WR_CAP steps): never the shallower of the two.
            j.m = n;
            j.h = j.g < 7u + 5u * (u32)TL_CAP ? j.g : 7u + 5u * (u32)TL_CAP;
            if (trace) fprintf(stderr, "[bwt] n %u deep path from depth %u\n", n, j.h);
            if (BwtRecord * r = j.item->rec) {
                r->deep = 1u;
                r->h = j.h;
            }
        }
        auto bg_tiles = [](u32 m) { return (u32)(((u64)m + BG_TILE - 1) / BG_TILE); };
        {
            // ranks in slot order (sa = V in place: a slot holds its final suffix, without flag, once the suffix is alone in its group), then the
            // inverse suffix array from (suffix, rank) pairs bucketed by the top bits of the suffix
            // rk = key[0] (2 n words: ranks, then the bucketed suffixes kb), rb = key[1]
            launch_jobs<BgReduceJob>(k_bg_reduce<true>, dim3(BW_BLOCK), s, deep_jobs, [&](u32 k) { return BgReduceJob{bg_tiles(jb[k].m), nullptr, jb[k].V, jb[k].m, jb[k].tile_head, jb[k].tile_keep}; });
            launch_jobs<BgSpineJob>(k_bg_spine, dim3(BG_SPINE), s, deep_jobs, [&](u32 k) { return BgSpineJob{1u, jb[k].tile_head, jb[k].tile_keep, bg_tiles(jb[k].m), jb[k].words + 6}; });
            launch_bg_apply<true, false>(s, deep_jobs, [&](u32 k) {
                const FwJob & j = jb[k];
                return BgApplyJob{bg_tiles(j.m), nullptr, j.V, nullptr, j.m, j.tile_head, j.tile_keep, j.V, j.isa, j.vv[0], j.slot[0], j.grp, j.in, j.pb, reinterpret_cast<u32 *>(j.key[0])};
            });
            RadixPairJob<u32> rp[BWT_MAX_BATCH];
            for (u32 q = 0; q < deep_jobs.count; q++) {
                FwJob & j = jb[deep_jobs.idx[q]];
                u32 * rk = reinterpret_cast<u32 *>(j.key[0]);
                const int nbits = bits_for((u64)j.n - 1);
                rp[q] = RadixPairJob<u32>{j.V, rk + j.n, rk, reinterpret_cast<u32 *>(j.key[1]), j.n, nbits > 8 ? nbits - 8 : 0};
                j.st.radix_passes++;
            }
            radix_pass_many<u32>(rp, deep_jobs.count, tmp, s);
            launch_jobs<IsaScatterJob>(k_isa_scatter, dim3(BW_BLOCK), s, deep_jobs, [&](u32 k) {
                const FwJob & j = jb[k];
                const u32 itiles = (u32)(((u64)j.n + BW_BLOCK * IS_ITEMS - 1) / (BW_BLOCK * IS_ITEMS));
                return IsaScatterJob{8u * ((itiles + 7u) / 8u), reinterpret_cast<u32 *>(j.key[0]) + j.n, reinterpret_cast<u32 *>(j.key[1]), j.n, itiles, j.isa};
            });
        }
        for (u32 q = 0; q < deep_jobs.count; q++) {
            FwJob & j = jb[deep_jobs.idx[q]];
            j.scur = 0;
            j.vact = j.vv[0];
            j.vfree = j.vv[1];
        }
        Sel dbl = deep_jobs;  // the jobs still doubling
        while (dbl.count) {
            HIP_CHECK(hipMemcpyAsync(h_words, words_all, (size_t)16 * count * sizeof(u32), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            Sel go;
            for (u32 q = 0; q < dbl.count; q++) {
                FwJob & j = jb[dbl.idx[q]];
                const u32 m_next = h_words[16 * (size_t)dbl.idx[q] + 6];
                if (BwtRecord * r = j.item->rec)
                    if (r->rounds < BWT_REC_ROUNDS) r->round[r->rounds++] = BwtRecord::Round{j.h, m_next};
                if (m_next == 0) continue;
                j.m = m_next;
                j.st.rounds++;
                if (trace) fprintf(stderr, "[bwt] n %u doubling round at depth %u: %u active suffixes\n", j.n, j.h, j.m);
                go.add(dbl.idx[q]);
            }
            dbl = go;
            if (dbl.count == 0) break;
            // the active suffixes are in vact, their slots in slot[scur], their ranks in grp
            launch_jobs<DoublingKeysJob>(k_bwt_doubling_keys_grp, dim3(BW_BLOCK), s, dbl, [&](u32 k) { return DoublingKeysJob{grid(jb[k].m), jb[k].vact, jb[k].grp, jb[k].isa, jb[k].m, jb[k].n, jb[k].h, jb[k].key[0]}; });
            int side[BWT_MAX_BATCH];
            for (u32 q = 0; q < dbl.count; q++) side[q] = 0;
            for (int which = 0; which < 2; which++) {  // by the rank h further on, then (stable) by the current rank
                SortJob<u64> sj[BWT_MAX_BATCH];
                for (u32 q = 0; q < dbl.count; q++) {
                    FwJob & j = jb[dbl.idx[q]];
                    u32 * pv[2] = {j.vact, j.vfree};
                    const int c = side[q];
                    const int bits = which == 0 ? bits_for((u64)j.n + j.h) : bits_for(j.n);
                    sj[q] = SortJob<u64>{nullptr, {j.key[c], j.key[c ^ 1]}, {pv[c], pv[c ^ 1]}, j.m, which * 32, which * 32 + bits, 0, 0};
                }
                sort_many<u64>(sj, dbl.count, false, tmp, s);
                for (u32 q = 0; q < dbl.count; q++) {
                    side[q] ^= sj[q].cur;
                    jb[dbl.idx[q]].st.radix_passes += sj[q].passes;
                }
            }
            u64 * skey[BWT_MAX_BATCH];
            u32 * vsorted[BWT_MAX_BATCH];
            for (u32 q = 0; q < dbl.count; q++) {
                FwJob & j = jb[dbl.idx[q]];
                u32 * pv[2] = {j.vact, j.vfree};
                skey[dbl.idx[q]] = j.key[side[q]];
                vsorted[dbl.idx[q]] = pv[side[q]];
                j.vfree = pv[side[q] ^ 1];
                j.st.sorted_elements += j.m;
            }
            launch_jobs<BgReduceJob>(k_bg_reduce<false>, dim3(BW_BLOCK), s, dbl, [&](u32 k) { return BgReduceJob{bg_tiles(jb[k].m), skey[k], nullptr, jb[k].m, jb[k].tile_head, jb[k].tile_keep}; });
            launch_jobs<BgSpineJob>(k_bg_spine, dim3(BG_SPINE), s, dbl, [&](u32 k) { return BgSpineJob{1u, jb[k].tile_head, jb[k].tile_keep, bg_tiles(jb[k].m), jb[k].words + 6}; });
            launch_bg_apply<false, true>(s, dbl, [&](u32 k) {
                const FwJob & j = jb[k];
                return BgApplyJob{bg_tiles(j.m), skey[k], vsorted[k], j.slot[j.scur], j.m, j.tile_head, j.tile_keep, j.V, j.isa, j.vfree, j.slot[j.scur ^ 1], j.grp, j.in, j.pb, nullptr};
            });
            for (u32 q = 0; q < dbl.count; q++) {
                FwJob & j = jb[dbl.idx[q]];
                j.scur ^= 1;
                j.vact = j.vfree;
                j.vfree = vsorted[dbl.idx[q]];
                if (j.h >= 0x40000000u) throw HipError{hipErrorUnknown, "suffix sort did not converge", __FILE__, __LINE__};
                j.h *= 2;
            }
        }
    }
    // the slot of suffix 0: where the resolve kernels saw it, or isa[0]
    launch_jobs<FinishJob>(k_bwt_finish, dim3(BW_BLOCK), s, all, [&](u32 k) {
        const FwJob & j = jb[k];
        return FinishJob{grid(j.n), j.in, j.pb, j.n, j.deep ? j.isa : j.words + 2, items[k].out, items[k].d_idx ? items[k].d_idx : j.words + 7};
    });
    bool wait = false;
    for (u32 k = 0; k < count; k++) wait = wait || !items[k].d_idx;
    if (wait) {
        HIP_CHECK(hipMemcpyAsync(h_words, words_all, (size_t)16 * count * sizeof(u32), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    for (u32 k = 0; k < count; k++) {
        items[k].idx = items[k].d_idx ? 0 : (s32)h_words[16 * (size_t)k + 7];
        if (items[k].stats) *items[k].stats = jb[k].st;
        if (items[k].rec) items[k].rec->st = jb[k].st;
    }
    tmp.release(mk);
}

// Tests only: a record as BWT_RECORD_WORDS flat words, with the geometry a test needs beside it (so that no test hard-codes a constant of this file):
//   [0] BWT_RECORD_WORDS  [1] n  [2] went deep  [3] deep path's first depth h  [4] passes of the resolve loop  [5] doubling rounds recorded
//   [6] BwtStats rounds  [7] radix passes  [8], [9] sorted elements (low, high word)  [10] big rounds allowed (the switch as it stands)
//   [12] WR_A  [13] WR_G  [14] largest group of the tail list  [15] largest group the tail ranks by counting  [16] TL_CAP  [17] WR_CAP  [18] VLC_WINDOW
//   [19] VLC_MAXLEN  [20] SP_GROUP  [21] capacity of the big list (n / 4)  [22] WW_KEY: code bits of a wide step  [23] code bits of a tail step
//   [24] code bits of a window  [25] BG_TILE  [26] RT_WAVES  [27] BWT_REC_PASSES  [28] BWT_REC_ROUNDS
//   [32 ..) the code table, 256 words; then 8 words per pass: g, [0], [1], [3], [4], [5], [8], 0; then 2 words per doubling round: h, m
constexpr u32 TL_GROUP = 64, TL_COUNT = 12, TL_KEY = 40, BW_KEY = 56;  // the literals of bwt_route_body.hpp (e - h <= 64) and bwt_tail_body.hpp (maxsz <= 12u, vlc_pack<40>), vlc_pack<56>
void bwt_record_flatten(const BwtRecord & r, u32 n, u32 * out) {
    for (u32 k = 0; k < BWT_RECORD_WORDS; k++) out[k] = 0;
    const u32 head[] = {BWT_RECORD_WORDS, n, r.deep, r.h, r.passes, r.rounds, (u32)r.st.rounds, (u32)r.st.radix_passes, (u32)r.st.sorted_elements, (u32)(r.st.sorted_elements >> 32),
                        (u32)bwt_switches().big_rounds.load(), 0u, (u32)WR_A, (u32)WR_G, TL_GROUP, TL_COUNT, (u32)TL_CAP, (u32)WR_CAP, (u32)VLC_WINDOW, (u32)VLC_MAXLEN, (u32)SP_GROUP, n / 4,
                        (u32)WW_KEY, TL_KEY, BW_KEY, (u32)BG_TILE, (u32)RT_WAVES, BWT_REC_PASSES, BWT_REC_ROUNDS};
    static_assert(sizeof head / sizeof head[0] <= 32, "the record's head is 32 words");
    for (u32 k = 0; k < sizeof head / sizeof head[0]; k++) out[k] = head[k];
    u32 * w = out + 32;
    for (u32 k = 0; k < 256; k++) *w++ = r.vlc[k];
    for (u32 k = 0; k < BWT_REC_PASSES; k++, w += 8) {
        const BwtRecord::Pass & p = r.pass[k];
        const u32 v[8] = {p.g, p.big, p.given_up, p.overflow, p.tail, p.tail_valid, p.mid, 0u};
        for (u32 q = 0; q < 8; q++) w[q] = v[q];
    }
    for (u32 k = 0; k < BWT_REC_ROUNDS; k++) {
        *w++ = r.round[k].h;
        *w++ = r.round[k].m;
    }
}

// d_idx == nullptr: synchronous, returns the primary index.  d_idx != nullptr: the primary index is left THERE (a device word that outlives
// the arena) and the call returns 0 without waiting for the stream -- the block's header is written by a kernel that reads it (round 4).
// A batch of one through bwt_forward_batch: there is one code path.
s32 bwt_forward(const u8 * d_in, u32 n, u8 * d_out, Arena & tmp, hipStream_t s, BwtStats * stats, u32 * d_idx, u32 * d_outside) {
    if (d_outside && n < 2) HIP_CHECK(hipMemsetAsync(d_outside, 0, 4, s));
    if (n == 0) {
        if (d_idx) launch(k_bwt_set_word, dim3(1), dim3(1), 0, s, d_idx, 0u);
        return 0;
    }
    if (n == 1) {
        HIP_CHECK(hipMemcpyAsync(d_out, d_in, 1, hipMemcpyDeviceToDevice, s));
        if (d_idx) {
            launch(k_bwt_set_word, dim3(1), dim3(1), 0, s, d_idx, 1u);
            return 0;
        }
        HIP_CHECK(hipStreamSynchronize(s));
        return 1;
    }
    BwtBatchItem one{d_in, n, d_out, d_idx, d_outside, stats, 0};
    bwt_forward_batch(&one, 1, tmp, s);
    return one.idx;
}

// How many of the first `count` blocks (sizes n[k]) one run takes: the largest b <= BWT_MAX_BATCH whose b workspaces of the run's largest block fit
// what the arena has free, and only for blocks of at most BWT_BATCH_MAX_N bytes (stages.hpp: the largest size the sweep covers; above it a run of
// one keeps the launch sequence a block has always had).  bwt_set_batch forces b (tests / sweeps; memory still bounds it).
static std::atomic<int> g_bwt_batch{-1};
void bwt_set_batch(int b) { g_bwt_batch.store(b < 0 ? -1 : b > (int)BWT_MAX_BATCH ? (int)BWT_MAX_BATCH : b < 1 ? 1 : b); }
u32 bwt_batch_size(const u32 * n, u32 count, size_t arena_free) {
    if (count == 0) return 0;
    const int forced = g_bwt_batch.load();
    u32 want = forced > 0 ? (u32)forced : BWT_MAX_BATCH;
    if (want > count) want = count;
    for (u32 b = want; b > 1; b--) {
        u32 largest = 0;
        for (u32 k = 0; k < b; k++) largest = n[k] > largest ? n[k] : largest;
        if (forced <= 0 && largest > BWT_BATCH_MAX_N) continue;
        if ((size_t)b * bwt_workspace_bytes((u64)largest + 64) <= arena_free) return b;
    }
    return 1;
}

}  // namespace bz3
