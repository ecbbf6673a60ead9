// frame.hpp -- kernels of the device-resident frame API (bz3_hip_compress_device / bz3_hip_decompress_device, api_frames.hip).
//
// A frame (src/libbz3.c:876-997) is a 13-byte header, then per block an 8-byte chunk header (coded size, original size)
// and the coded bytes.  Moving a window of blocks between the caller's buffers and the states' slots is a list of
// byte segments at arbitrary alignments on both sides: k_copy_segments moves them all in one launch.  Decoding
// needs the chunk headers, which form a chain (each one's offset depends on the sizes before it): k_frame_walk_many
// follows the chains of many frames, one lane per frame, and hands the host every chunk's offsets and first 17 bytes
// in one read-back.
#pragma once
#include "../../include/libbz3.h"
#include "frame_check.hpp"
#include "hipx.hpp"

namespace bz3 {

// ---- k_copy_segments -------------------------------------------------------------------------------------------------
// One segment: `len` bytes from absolute device address `src` to `dst`.  Segments of one launch do not overlap on the
// destination side (they may share a 16-byte granule: the bytes of a shared granule are written with byte stores).
// `mode`: 0 or 1, a plain copy; an element size of 2, 4 or 8 (| PLANES_INVERSE), a byte-plane split (merge) of the segment
// (planes.hpp: such a launch goes to k_move_segments).  `base`: 0, or the address of `len` bytes on the caller's side of the move that
// are subtracted from the source bytes before a split (mode without PLANES_INVERSE) or added after a merge (with it), byte by byte
// mod 256 (planes.hpp: a launch with such a segment goes to k_delta_segments).
struct CopySeg {
    u64 src, dst, len, mode, base;
};
constexpr u32 COPY_THREADS = 256;
constexpr u32 COPY_GRANULES_PER_LANE = 4;
constexpr u32 COPY_TILE_GRANULES = COPY_THREADS * COPY_GRANULES_PER_LANE;  // 16 KiB of destination per workgroup

// Destination granules (16-byte aligned) a segment touches, and the workgroups (tiles) it takes.
__host__ __device__ inline u64 copy_granules(u64 dst, u64 len) { return len ? ((dst + len + 15) >> 4) - (dst >> 4) : 0; }
__host__ __device__ inline u64 copy_tiles(u64 dst, u64 len) { return (copy_granules(dst, len) + COPY_TILE_GRANULES - 1) / COPY_TILE_GRANULES; }

__device__ __forceinline__ u32 align_byte(u32 hi, u32 lo, u32 r) {  // ((hi:lo) >> 8 r)[31:0], v_alignbyte_b32
#ifdef BZ3_EMU
    return (u32)((((u64)hi << 32) | lo) >> (8 * (r & 3)));
#else
    return __builtin_amdgcn_alignbyte(hi, lo, r);
#endif
}

// One tile of one segment.  Q = (src - dst) / 4 mod 4: which word of the lower aligned source granule holds the first source
// byte of every destination granule (uniform over a segment, hence a template parameter: the word selection is static).
// A full destination granule whose source bytes straddle two aligned source granules is built from both of them with
// v_alignbyte_b32 and written with one 16-byte store; both granules hold bytes of the segment.  The partial head and tail
// granules are copied byte by byte.  No granule is ever loaded that holds no byte of the segment.
template <int Q>
__device__ __forceinline__ uint4 shift_granules(uint4 lo, uint4 hi, u32 r) {  // bytes [4 Q + r, 4 Q + r + 16) of lo:hi
    const u32 w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint4 o;
    o.x = align_byte(w[Q + 1], w[Q + 0], r);
    o.y = align_byte(w[Q + 2], w[Q + 1], r);
    o.z = align_byte(w[Q + 3], w[Q + 2], r);
    o.w = align_byte(w[Q + 4], w[Q + 3], r);
    return o;
}

template <int Q>
__device__ __forceinline__ void copy_tile(const u8 * src, u8 * dst, u64 len, u64 g_first, u64 g_end) {
    const u64 d0 = (u64)dst, d1 = d0 + len;
    const u64 delta = (u64)src - d0;  // source address = destination address + delta (mod 2^64)
    const u32 r = (u32)(delta & 3);
    const bool aligned = (delta & 15) == 0;
    if (g_end - g_first == COPY_TILE_GRANULES && (g_first << 4) >= d0 && (g_end << 4) <= d1) {  // every granule of the tile is full: loads first, then stores
        uint4 lo[COPY_GRANULES_PER_LANE], hi[COPY_GRANULES_PER_LANE];
#pragma unroll
        for (u32 k = 0; k < COPY_GRANULES_PER_LANE; k++) {
            const uint4 * sp = (const uint4 *)((((g_first + k * COPY_THREADS + threadIdx.x) << 4) + delta) & ~(u64)15);
            lo[k] = sp[0];
            if (!aligned) hi[k] = sp[1];
        }
#pragma unroll
        for (u32 k = 0; k < COPY_GRANULES_PER_LANE; k++)
            *(uint4 *)((g_first + k * COPY_THREADS + threadIdx.x) << 4) = aligned ? lo[k] : shift_granules<Q>(lo[k], hi[k], r);
        return;
    }
    for (u32 k = 0; k < COPY_GRANULES_PER_LANE; k++) {
        const u64 g = g_first + k * COPY_THREADS + threadIdx.x;
        if (g >= g_end) break;
        const u64 a = g << 4;  // destination granule [a, a + 16)
        if (a >= d0 && a + 16 <= d1) {
            const uint4 * sp = (const uint4 *)((a + delta) & ~(u64)15);
            *(uint4 *)a = aligned ? sp[0] : shift_granules<Q>(sp[0], sp[1], r);
        } else {
            const u64 b0 = a > d0 ? a : d0, b1 = a + 16 < d1 ? a + 16 : d1;
            for (u64 b = b0; b < b1; b++) *(u8 *)b = *(const u8 *)(b + delta);
        }
    }
}

// Workgroup b copies tile b - tile_start[i] of segment i, where tile_start[i] <= b < tile_start[i + 1] (binary search over the
// nseg + 1 prefix sums the host computed).
__device__ __forceinline__ void copy_segment_tile(const CopySeg & sg, u32 tile) {
    const u64 g0 = sg.dst >> 4, g_end = (sg.dst + sg.len + 15) >> 4;
    const u64 g_first = g0 + (u64)tile * COPY_TILE_GRANULES;
    const u64 g_last = g_first + COPY_TILE_GRANULES < g_end ? g_first + COPY_TILE_GRANULES : g_end;
    const u8 * src = (const u8 *)sg.src;
    u8 * dst = (u8 *)sg.dst;
    switch ((u32)(((sg.src - sg.dst) >> 2) & 3)) {
        case 0: copy_tile<0>(src, dst, sg.len, g_first, g_last); break;
        case 1: copy_tile<1>(src, dst, sg.len, g_first, g_last); break;
        case 2: copy_tile<2>(src, dst, sg.len, g_first, g_last); break;
        default: copy_tile<3>(src, dst, sg.len, g_first, g_last); break;
    }
}

__global__ void __launch_bounds__(COPY_THREADS) k_copy_segments(const CopySeg * __restrict__ segs, const u32 * __restrict__ tile_start, u32 nseg) {
    const u32 b = blockIdx.x;
    u32 lo = 0, hi = nseg;  // invariant: tile_start[lo] <= b < tile_start[hi]
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (tile_start[mid] <= b) lo = mid;
        else hi = mid;
    }
    copy_segment_tile(segs[lo], b - tile_start[lo]);
}

// ---- k_frame_walk_many -----------------------------------------------------------------------------------------------
// The chunk headers of n frames, one lane per frame (the headers of one frame form a chain: every header's offset depends
// on the one before it).  Lane i resumes frame i from its state (off = offset of the next chunk header, done = chunks
// behind, planned = output bytes before it); off == 0 is the first visit, which reads and checks the 13-byte frame header
// first (src/libbz3.c:930-960) and then walks from offset 13.  It walks up to `limit` chunks, writes their records from
// rec[rec_base] on and its resume state to tails[i].
//
// A range walk (WalkArg::range != 0; bz3_hip_decompress_device_range, api_frames.hip) wants only the chunks that hold a byte of the
// output bytes [lo, hi): the lane stops before it reads a header with planned >= hi, and it advances over a chunk that ends at
// or before lo (planned + orig <= lo) or is empty with its header checked as any other, but without a record and without using
// any of `limit`, so a frame may hold any number of such chunks before its range.  The capacity check is not made
// (the host passes buf_max = SIZE_MAX): a range is clipped, never too big.
//
// A range walk with a period (WalkArg::count > 1; bz3_hip_decompress_device_strided, api_frames.hip) wants the output bytes of `count`
// runs of `run` bytes that start `stride` bytes apart from lo on (stride >= run > 0), the last of them cut at hi.  A chunk is recorded
// iff it meets a run: i0 is the first run that ends behind the chunk's first byte, and the chunk meets it iff that run exists and
// starts before the chunk's end.  A chunk that lies in a gap between two runs is header-checked and skipped like one before the range.
// One 64-bit division per chunk, on the one lane that follows the chain.  A launch in which no frame has a period is
// k_frame_walk_many as it was; one with such a frame is k_frame_walk_strided, where a lane with count <= 1 executes the walk above.
//
// A range walk with a piece table (WalkArg::m > 0; bz3_hip_decompress_device_select, api_frames.hip) wants of each of `count` periods, `stride`
// bytes apart from lo on, the m pieces [s_j, s_j + l_j) of the period, ascending, disjoint and none empty, the last period cut at hi.  The
// table lies in device memory, m + 1 entries of two u64: (s_j, P_j) with P_j = l_0 + ... + l_{j-1}, and the closing entry (unused, P_m), so
// that l_j = P_{j+1} - P_j.  A chunk is recorded iff it meets a piece: q is the period that holds the chunk's first byte (0 before lo), j
// the first piece of that period that ends behind it (binary search), piece 0 of period q + 1 where there is none; the chunk meets it iff
// that period exists and the piece starts before the chunk's end and below hi.  A chunk in a gap between two pieces, or between the last piece
// of a period and the first of the next, is header-checked and skipped.  One 64-bit division and one binary search per chunk, on the one lane
// that follows the chain.  A launch with such a frame is k_frame_walk_select, where the other lanes execute the walks above.
struct WalkChunk {
    u64 in_off;   // offset of the chunk header in the frame
    u64 out_off;  // output bytes of the chunks before it (planned)
    s32 size, orig;
    u8 hdr[17];   // the first 17 bytes of the chunk's coded bytes (zeros beyond the end of the frame)
    u8 pad[3];
    u32 index;    // the chunk's number in its frame (the walk's `done` when it read the header)
};
struct WalkArg {
    u64 in, in_size, buf_max;  // the frame (device address, bytes), the output capacity
    u64 off, planned;          // resume state (off == 0: first visit)
    u32 done, limit, rec_base;
    u32 block_size, n_blocks;  // from the frame header (ignored on a first visit)
    u32 range;                 // != 0: a range walk over the output bytes [lo, hi)
    u64 lo, hi;
    u64 run, stride, count;    // count > 1: only the chunks that meet one of `count` runs of `run` bytes, `stride` apart from lo on
    u64 pieces;                // m > 0: the device address of the piece table; only the chunks that meet a piece of one of `count` periods
    u32 m, pad;
};
struct WalkTail {
    u64 off, planned;  // resume state after the last well-formed chunk read
    u32 done;
    u32 count;  // chunks written to the records
    s32 err;    // BZ3_OK, or the first header error (the walk stopped at it)
    u32 block_size, n_blocks;  // the frame header's fields
    u32 pad;
};
static_assert(sizeof(WalkChunk) % 16 == 0 && sizeof(WalkArg) % 8 == 0 && sizeof(WalkTail) % 8 == 0, "walk records are packed arrays");
constexpr u32 WALK_THREADS = 64;

// The first piece of a table of m that ends behind byte r of its period, or m.
__host__ __device__ inline u32 first_piece_behind(const u64 * tab, u32 m, u64 r) {
    u32 lo = 0, hi = m;  // invariant: the pieces before lo end at or before r, those from hi on behind it
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (tab[2 * mid] + (tab[2 * mid + 3] - tab[2 * mid + 1]) > r) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// PERIOD: some frame of the launch walks with a period (k_frame_walk_strided); without it the fields of the period are never looked at.
// SELECT: some frame of the launch walks with a piece table (k_frame_walk_select); likewise.
template <bool PERIOD, bool SELECT = false>
__device__ __forceinline__ void frame_walk(const WalkArg * __restrict__ args, u32 n, WalkChunk * __restrict__ rec, WalkTail * __restrict__ tails) {
    const u32 i = blockIdx.x * WALK_THREADS + threadIdx.x;
    if (i >= n) return;
    const WalkArg a = args[i];
    const u8 * frame = (const u8 *)a.in;
    u64 off = a.off, planned = a.planned;
    u32 done = a.done, block_size = a.block_size, n_blocks = a.n_blocks, c = 0;
    int err = BZ3_OK;
    if (off == 0) {  // the frame header, in the order of decompress: size and magic (:930-936), then what bz3_new accepts (:953-960)
        if (a.in_size < 13 || frame[0] != 'B' || frame[1] != 'Z' || frame[2] != '3' || frame[3] != 'v' || frame[4] != '1') {
            err = BZ3_ERR_MALFORMED_HEADER;
        } else {
            block_size = (u32)frame[5] | ((u32)frame[6] << 8) | ((u32)frame[7] << 16) | ((u32)frame[8] << 24);
            n_blocks = (u32)frame[9] | ((u32)frame[10] << 8) | ((u32)frame[11] << 16) | ((u32)frame[12] << 24);
            if (block_size < 65u * 1024 || block_size > 511u * 1024 * 1024) err = BZ3_ERR_INIT;
            off = 13;
        }
    }
    while (err == BZ3_OK && c < a.limit && done < n_blocks) {
        if (a.range && planned >= a.hi) break;  // headers at or beyond the end of the range are never read
        s32 size = 0, orig = 0;
        err = frame_chunk_check(frame + off, a.in_size - off, block_size, (size_t)a.buf_max, (size_t)planned, &size, &orig);
        if (err != BZ3_OK) break;
        const u64 data = off + 8;
        bool wanted = !a.range || (orig > 0 && planned + (u64)orig > a.lo);
        if (SELECT && wanted && a.m > 0) {
            const u64 * tab = (const u64 *)a.pieces;
            u64 q = planned < a.lo ? 0 : (planned - a.lo) / a.stride;
            u32 j = first_piece_behind(tab, a.m, planned < a.lo ? 0 : planned - a.lo - q * a.stride);
            if (j == a.m) {
                q++;
                j = 0;
            }
            const u64 start = a.lo + q * a.stride + tab[2 * j];  // (q < count: it fits, bz3_hip.h)
            wanted = q < a.count && start < planned + (u64)orig && start < a.hi;
        } else if (PERIOD && wanted && a.count > 1) {
            const u64 i0 = planned < a.lo + a.run ? 0 : (planned - a.lo - a.run) / a.stride + 1;
            wanted = i0 < a.count && a.lo + i0 * a.stride < planned + (u64)orig;
        }
        if (wanted) {
            WalkChunk & w = rec[a.rec_base + c];
            w.in_off = off;
            w.out_off = planned;
            w.size = size;
            w.orig = orig;
            w.index = done;
            for (u32 k = 0; k < 17; k++) w.hdr[k] = data + k < a.in_size ? frame[data + k] : (u8)0;
            c++;
        }
        off = data + (u64)size;
        planned += (u64)orig;
        done++;
    }
    WalkTail & t = tails[i];
    t.off = off;
    t.planned = planned;
    t.done = done;
    t.count = c;
    t.err = err;
    t.block_size = block_size;
    t.n_blocks = n_blocks;
}

__global__ void __launch_bounds__(WALK_THREADS) k_frame_walk_many(const WalkArg * __restrict__ args, u32 n, WalkChunk * __restrict__ rec,
                                                                  WalkTail * __restrict__ tails) {
    frame_walk<false>(args, n, rec, tails);
}

// k_frame_walk_many for a launch in which some frame walks with a period.  (A kernel of its own, as the segment kernels of planes.hpp are:
// the walks without a period keep the code and the registers they had.)
__global__ void __launch_bounds__(WALK_THREADS) k_frame_walk_strided(const WalkArg * __restrict__ args, u32 n, WalkChunk * __restrict__ rec,
                                                                     WalkTail * __restrict__ tails) {
    frame_walk<true>(args, n, rec, tails);
}

// The same for a launch in which some frame walks with a piece table.
__global__ void __launch_bounds__(WALK_THREADS) k_frame_walk_select(const WalkArg * __restrict__ args, u32 n, WalkChunk * __restrict__ rec,
                                                                    WalkTail * __restrict__ tails) {
    frame_walk<true, true>(args, n, rec, tails);
}

}  // namespace bz3
