// planes.hpp -- byte-plane split / merge of a frame's blocks (bz3_hip_compress_device_planes / bz3_hip_decompress_device_planes, api_frames.hip).
//
// For a block of s bytes of k-byte elements, m = s / k:
//     split_k(b)[q m + e] = b[e k + q]   (0 <= q < k, 0 <= e < m),     split_k(b)[j] = b[j]   (m k <= j < s: the tail stays in place)
// merge_k is its inverse.  The frame path copies every block into a slot and back anyway (frame.hpp k_copy_segments); a segment with
// an element size is split (compress, scatter side) or merged (decompress, gather side) during that copy instead.  Both sides of
// both directions may sit at any alignment: the interleaved side is the caller's buffer (in + j block_size, out + planned), and
// plane q starts at slot + q m, which is 16-byte aligned only where m is.
//
// One workgroup moves a tile of PLANES_TILE_ELEMS elements in two phases:
//   1. a lane takes 16 elements into registers with 16-byte loads (k contiguous granules of the interleaved side, or one granule of
//      each plane; a side that is not 16-byte aligned is built from the aligned granules around it with v_alignbyte_b32, as copy_tile
//      does), transposes bytes with v_perm_b32 and writes k aligned 16-byte rows to LDS, laid out as the destination wants them;
//   2. a lane takes destination granules (16-byte aligned in global memory), reads their 16 bytes from LDS at whatever byte offset
//      that is (five dword reads, v_alignbyte_b32) and writes them with one 16-byte store.
// 255 of the 256 lanes' elements make a tile: the destination granule that straddles the end of a tile belongs to the tile it
// starts in, which therefore holds up to 15 elements of the next one (the 256th lane's).  Byte stores are left for the partial
// granules at the two ends of a plane (split) or of the block (merge) and for the tail.  As in copy_tile, no granule is loaded that
// holds no byte of the segment, and no byte outside the segment's destination is written.
//
// Delta segments (CopySeg::base != 0; bz3_hip_*_device_delta, api_frames.hip).  D(x, b)[i] = (x[i] - b[i]) mod 256 for every byte.  A split
// segment with a base stores split_k(src - base), a merge segment merge_k(src) + base; the base lies on the interleaved (caller's)
// side, at the offsets of that side, with an alignment of its own.  The difference is taken in phase 1, on the registers that hold
// the interleaved bytes (before the transpose of a split, after the one of a merge), four bytes per operation (sub_bytes /
// add_bytes: gfx950 has no packed byte subtract); the base's granules are loaded as the interleaved side's are.  k = 1 needs no
// LDS: delta1_tile is copy_tile with a second read stream.
//
// In place.  A merge may write its output over the base (dst == base, the decode call's `out == base`) because every base byte a
// workgroup needs is read by that workgroup before anyone writes it:
//   * the bytes a tile stores, [s0, s1), are disjoint from every other tile's and every other segment's, so only the tile itself
//     ever writes them;
//   * they lie within the 256 lanes' elements [ea, ea + PLANES_LOAD_ELEMS) (s1 <= d0 + (ea + PLANES_TILE_ELEMS) k + 15), so all of
//     them are read from the base in phase 1, before the tile's barrier, and stored in phase 2, after it;
//   * what else phase 1 reads of the base -- the rest of the 256th lane's elements, the bytes of the straddling granule below s0,
//     the neighbours inside an aligned granule -- belongs to other tiles, which may have overwritten it already: those sums land in
//     LDS outside [s0 - origin, s1 - origin) and phase 2 never reads them;
//   * a tail byte is read and written by one thread, in that order, and used by no other;
//   * delta1_tile reads the base at the destination's own granules (dst == base: the same alignment), each by the thread that then
//     stores it.
// Any other overlap of base and destination is the caller's error (api_frames.hip refuses it).
//
// Clipped merge (CopySeg::mode & PLANES_CLIP; bz3_hip_decompress_device_range, api_frames.hip).  A range of a frame cuts its first and its
// last chunk: of merge_k(slot[0, s)) only the bytes [a, b) are wanted, at dst[0, b - a), plus base[0, b - a) where there is a base
// (dst and base address the clip's first byte; the chunk's byte c pairs with dst[c - a] and base[c - a]).  clip_merge_tile is
// merge_tile with the chunk's own m = s / k as the plane stride and three changes:
//   * only the tiles that hold an element byte of [a, b) are launched (clip_first_tile, clip_tiles), the first of them stores the
//     clip's part of the tail;
//   * a lane whose 16 elements lie inside [a, b) loads and transposes them as before; a lane whose elements straddle a or b moves
//     the bytes inside the clip one by one (at most two lanes of a segment), a lane outside it loads nothing.  So every granule
//     loaded from the slot holds a byte of the chunk, and every granule loaded from the base a byte of base[0, b - a): nothing
//     around a range's base is relied on (without a base the straddling lanes may take the 16-byte path: all they load is the slot);
//   * the tiles' store ranges are cut at the 16-byte boundaries of dst as before, and clamped to [dst, dst + min(b, m k) - a).
// In place (dst == base): the argument above holds word for word with [s0, s1) clamped to the clip.  The bytes a tile stores are its
// own, they lie within its 256 lanes' elements and inside [a, b), so every one of them was read from the base in phase 1 by a lane
// of this tile (16-byte path: the lane lies inside the clip; byte path: the byte does), before the barrier; what else phase 1 read
// of the base belongs to other tiles and lands in LDS outside [s0 - origin, s1 - origin); a tail byte is read and written by one
// thread.  dst and base share the clip's coordinates, so dst == base pairs every byte with itself.
//
// Clipped split (CopySeg::mode & PLANES_CLIP without PLANES_INVERSE; bz3_hip_update_device_range, api_frames.hip).  The write mirror of the
// clipped merge: dst is a slot that holds split_k of a decoded chunk of s bytes (m = s / k, the tail in place), and of the chunk only the
// bytes [a, b) get new values, src[0, b - a) (less base[0, b - a) where there is a base): src and base address the clip's first byte.  The
// segment stores dst[q m + e] = src[e k + q - a] for every (e, q) with a <= e k + q < b, the tail bytes c in [max(a, m k), b) to dst[c], and
// NO OTHER BYTE OF THE SLOT: the rest is the old chunk, which the encode that follows reads.  clip_split_tile is split_tile with these changes:
//   * only the tiles that hold an element byte of [a, b) are launched (clip_first_tile, clip_tiles), the first of them stores the clip's
//     part of the tail;
//   * a lane whose 16 elements lie inside [a, b) loads, subtracts and transposes them as before; a lane whose elements straddle a or b moves
//     the bytes inside the clip one by one (at most two lanes of a segment), a lane outside it loads nothing.  The interleaved side is the
//     caller's here, so this holds with or without a base: every granule loaded from src or base holds a byte of src[0, b - a) or
//     base[0, b - a), and nothing around the caller's row buffer is relied on;
//   * plane q holds the clip's elements [ceil((a - q) / k), ceil((min(b, m k) - q) / k)), ranges that differ by at most one element between the
//     planes.  A tile's store range in plane q is its usual one, cut at the 16-byte boundaries of dst + q m, then clamped to that element
//     range; the first tile launched starts at the clamp whatever its own first granule is (the tile before it, which would own those bytes,
//     is not launched; they are elements of this tile).  Full granules inside the range are 16-byte stores and the partial ones at the clamp
//     byte stores, never a read-modify-write of a granule: the neighbouring bytes are the old chunk's, or another tile's.
// k = 1 is a plain copy, or the delta1_tile copy with a base, at dst + a, and a == 0 && b == s the ordinary split segment (GatherList::patch,
// api_frames.hip).  No scratch; the LDS of the other segment kernels.
//
// Gather merges (CopySeg::mode & (PLANES_STRIDED | PLANES_SELECT); gather_tile).  A strided and a select merge want of a chunk a set of its bytes
// that a formula c(u), increasing in u, names (the two paragraphs below).  In the output they are CONTIGUOUS, dst[0, nbytes), so the chunk is one
// segment with one destination range, whatever the number of runs or pieces in it.  Chunk byte c lives at slot[(c % k) m + c / k] for c < m k
// (m = len / k), at slot[c] in the tail: merge_k.  gather_tile tiles the DESTINATION: a workgroup owns the destination bytes
// [4080 k t, 4080 k (t + 1)) cut at dst's 16-byte boundaries as merge_tile's are, lane l fills LDS with the 16 k destination bytes from
// u0 = 4080 k t + 16 k l on, in destination order, and phase 2 is store_from_lds.  The two merges differ in one thing, the cursor a lane walks the
// chunk with (StridedCursor, SelectCursor): it locates c(u0) and what is left of the run or piece there with one division, and then steps.  A lane
// whose 16 k bytes are 16 whole elements of one run or piece (they lie inside it, inside [0, nbytes) and inside the element part of the chunk, and
// the first of them is byte 0 of an element) takes k plane granules and interleave<K> (k = 1: one load16_any) and, with a base, load_elems16 of
// the base and add_bytes (merged_elems16); every other lane (one that crosses a run's or a piece's boundary, the chunk's tail or the segment's end,
// or whose bytes do not start an element) moves its bytes one by one.  RUNS AND PIECES SHORTER THAN 16 ELEMENTS THEREFORE GO WHOLLY THROUGH THE
// BYTE PATH: correct and slow ("Strided range decode").  Every granule loaded from the slot holds a byte of the chunk (16-byte path:
// c + 16 k <= m k, and plane granule q covers slot[q m + c / k, + 16)); every granule loaded from the base holds a byte of base[0, nbytes)
// (16-byte path: u0 + 16 k <= nbytes, and load_elems16 takes the aligned granules around exactly those bytes; byte path: bytes u < nbytes); and
// nothing outside dst[0, nbytes) is written (phase 2 is store_from_lds over the tile's share of [dst, dst + nbytes)).  No scratch.
// In place (dst == base): dst and base share the segment's coordinates, so dst == base pairs every byte with itself.  The bytes a tile
// stores, [s0, s1), are its own (the tiles' store ranges partition dst[0, nbytes), the segments' destinations are disjoint); they lie
// within the destination bytes of its 256 lanes, [4080 k t, 4080 k t + 4096 k) (s1 <= dst + 4080 k (t + 1) + 15), so every one of
// them was read from the base in phase 1 by a lane of this tile (16-byte path: the lane's 16 k bytes lie inside [0, nbytes); byte
// path: the byte does), before the barrier, and is stored in phase 2, after it.  load_elems16 keeps of the aligned granules it reads
// only the lane's own 16 k bytes, so what else phase 1 takes from the base are the 256th lane's bytes and the bytes below s0, which
// belong to other tiles, may have been overwritten already and land in LDS outside [s0 - origin, s1 - origin), where phase 2 never
// reads.  The argument speaks of the tiling, the lanes' destination bytes and phase 2 alone: which SOURCE byte a cursor gives a destination byte
// does not enter it.
//
// Strided merge (PLANES_STRIDED; bz3_hip_decompress_device_strided, api_frames.hip).  A strided range wants of a chunk a periodic set of its
// bytes: chunk byte c0, the `first` bytes from it on (the rest of the run c0 lies in), then runs of `run` bytes whose starts lie `stride` bytes
// apart, nbytes in all.  Destination byte u comes from chunk byte
//     c(u) = c0 + u                                                    (u < first)
//     c(u) = c0 + first + (stride - run) + (v / run) stride + v % run  (v = u - first)
// StridedCursor divides in 32 bits: every quantity is below the chunk's 2^31 bytes; a run longer than that is clamped (segments_tile), which
// changes no c(u).
//
// Select merge (PLANES_SELECT; bz3_hip_decompress_device_select, api_frames.hip).  An index request wants of a chunk the bytes of a LIST of
// pieces per period: the periods start `stride` bytes apart, piece j of a period is its bytes [s_j, s_j + l_j), the pieces ascend and are
// disjoint, P_j = l_0 + ... + l_{j-1}, L = P_m.  The table of the m + 1 pairs (s_j, P_j) -- the last one closes it with P_m -- lies in device
// memory and is only ever read.  With x = r0 + u, destination byte u comes from chunk byte
//     c(u) = rel + (q0 + x / L) stride + s_j + (x % L - P_j),     j the piece with P_j <= x % L < P_{j+1}
// (rel = the request's offset less the chunk's, mod 2^64; q0, r0: the period and the place in it of destination byte 0).  The host has checked
// that c(0) and c(nbytes - 1) lie in [0, len); c increases, so every c(u) does.  SelectCursor locates its first byte with one division (32 bits
// where L < 2^31, else a comparison: x < L + 2^31 then) and one binary search over P, and from there steps through the pieces linearly,
// skipping empty ones, with the chunk byte of the period's start in hand.  The LDS is that of k_strided_segments.
//
// Select split (CopySeg::mode & PLANES_SELECT without PLANES_INVERSE; bz3_hip_update_device_select, api_frames.hip).  The write mirror of the select
// merge: dst is a slot that holds split_k of a chunk of len bytes, and the chunk bytes c(u) of the formula above, u < nbytes, get the new values
// src[u] (less base[u] where there is a base): src and base are the CONTIGUOUS side and address the segment's first byte.  Chunk byte c is stored
// where split_k keeps it, dst[(c % k) m + c / k] below m k and dst[c] in the tail, and NO OTHER BYTE OF THE SLOT is: the rest is the old chunk,
// which the encode that follows reads.  select_split_tile tiles the SOURCE as gather_tile tiles its destination, and a lane walks the chunk
// with the same SelectCursor.  A lane whose 16 k bytes are 16 whole elements of the chunk inside one piece (gather_tile's condition) takes load_elems16,
// sub_bytes and deinterleave, the fast path of clip_split_tile (split_elems16); every other lane moves its bytes one by one, so PIECES SHORTER THAN 16 ELEMENTS GO WHOLLY
// THROUGH THE BYTE PATH: correct and slow.  Every granule loaded from src or base holds a byte of the lane's own 16 k bytes of src[0, nbytes) or
// base[0, nbytes).  The stores leave the lane directly, without the LDS stage of the other tiles: the wanted bytes of different lanes are disjoint
// but a tile's share of a plane is no contiguous range (neighbouring lanes may lie in different pieces and periods), and the bytes between two
// lanes' shares are the old chunk's, so there is no granule a second phase could own without reading them back.  The rule is therefore: the 16
// bytes a lane has for one plane are ONE 16-byte store where they are an aligned granule, and 16 byte stores otherwise; never a read-modify-write.
// No scratch; the kernel's LDS is that of the clipped and whole splits beside it.
//
// Replane (CopySeg::mode & PLANES_REPLANE; bz3_hip_resize_device, api_frames.hip).  A resize keeps the first a bytes of a decoded chunk of o bytes in
// a chunk of o' bytes, a <= min(o, o').  The decoded chunk sits in its slot as split_k over m = o / k, the chunk to be coded needs them as split_k
// over m' = o' / k.  With pos(c; L) = (c % k) (L / k) + c / k below (L / k) k and pos(c; L) = c in the tail, the segment stores
//     dst[pos(c; o')] = src[pos(c; o)]   for c < a,
// and NO OTHER BYTE OF dst: the bytes from a on come from the clipped split of the same launch, which writes none below a.  Out of place, from
// the slot the chunk was decoded into to the slot it is coded from: in place plane q would shift by q (m' - m) across workgroups.  The bulk is k
// runs of a / k bytes, plane q of src to plane q of dst, at unrelated alignments: each goes through copy_tile (aligned granule loads,
// v_alignbyte_b32, 16-byte stores, byte stores at the partial granules of a run's two ends), a tile index naming (plane, tile within plane).  What
// is left is the partial element at a, fewer than k bytes, which may lie in the tail of either layout: single threads move them.  k = 1 is a
// plain copy, and nothing at all where the two slots coincide (GatherList::replane, api_frames.hip).  No LDS of its own, no scratch.
#pragma once
#include <type_traits>

#include "frame.hpp"

namespace bz3 {

constexpr u32 PLANES_TILE_ELEMS = (COPY_THREADS - 1) * 16;  // elements whose destination granules a workgroup owns
constexpr u32 PLANES_LOAD_ELEMS = COPY_THREADS * 16;        // elements a workgroup loads (the last 16 for the straddling granules)
constexpr u32 PLANE_STRIDE = PLANES_LOAD_ELEMS + 16;        // LDS bytes per plane (split): phase 2 reads up to 20 bytes from offset < 4080
constexpr u32 PLANES_LDS_BYTES = 8 * PLANE_STRIDE;          // >= 8 * PLANES_LOAD_ELEMS + 16, the merge layout
constexpr u64 PLANES_INVERSE = 0x100;                       // CopySeg::mode = elem_size | PLANES_INVERSE for merge
constexpr u64 PLANES_CLIP = 0x200;                          // a merge of which only the bytes [a, b) are stored (k_range_segments and the kernels above it); without PLANES_INVERSE a split that replaces only them (k_patch_segments)
constexpr u64 PLANES_STRIDED = 0x400;                       // a merge of which a periodic byte set is stored (k_strided_segments and k_select_segments)
constexpr u32 STRIDED_PARAMS = 5;                           // u64 per segment in its side table: c0, first, run, stride, nbytes
constexpr u64 PLANES_SELECT = 0x800;                        // a merge of which the bytes of a piece list per period are stored (k_select_segments alone); without PLANES_INVERSE a split that replaces only them (k_patch_select_segments)
constexpr u32 SELECT_PARAMS = 7;                            // u64 per segment in its side table: rel, stride, q0, r0, nbytes, the piece table's address, m
constexpr u64 PLANES_REPLANE = 0x1000;                      // a slot-to-slot move of a chunk's first a bytes from the planes of its old length to those of its new one (k_replane_segments alone); its row of the clip table holds len_old and a

__host__ __device__ inline bool planes_elem_size_ok(u64 k) { return k == 1 || k == 2 || k == 4 || k == 8; }
// Workgroups of a split / merge segment: one per PLANES_TILE_ELEMS elements; a block shorter than an element still has its tail.
__host__ __device__ inline u64 planes_tiles(u64 len, u64 k) {
    const u64 t = (len / k + PLANES_TILE_ELEMS - 1) / PLANES_TILE_ELEMS;
    return len ? (t ? t : 1) : 0;
}
__host__ __device__ inline u64 segment_tiles(const CopySeg & sg) {
    return (sg.mode & 0xff) > 1 ? planes_tiles(sg.len, sg.mode & 0xff) : copy_tiles(sg.dst, sg.len);
}

__device__ __forceinline__ u32 byte_perm(u32 hi, u32 lo, u32 sel) {  // byte i of the result = byte sel[i] (0..7) of hi:lo, v_perm_b32
#ifdef BZ3_EMU
    const u64 v = ((u64)hi << 32) | lo;
    u32 o = 0;
    for (u32 i = 0; i < 4; i++) o |= (u32)((v >> (8 * ((sel >> (8 * i)) & 7))) & 0xff) << (8 * i);
    return o;
#else
    return __builtin_amdgcn_perm(hi, lo, sel);
#endif
}

// Bytes [sh, sh + 16) of lo:hi, 0 <= sh < 16 (sh is uniform over a wave: the word selection is two rounds of conditional moves).
__device__ __forceinline__ uint4 shift_bytes(uint4 lo, uint4 hi, u32 sh) {
    u32 w0 = lo.x, w1 = lo.y, w2 = lo.z, w3 = lo.w, w4 = hi.x, w5 = hi.y, w6 = hi.z, w7 = hi.w;
    if (sh & 4) { w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; w5 = w6; w6 = w7; }
    if (sh & 8) { w0 = w2; w1 = w3; w2 = w4; w3 = w5; w4 = w6; }
    uint4 o;
    o.x = align_byte(w1, w0, sh & 3);
    o.y = align_byte(w2, w1, sh & 3);
    o.z = align_byte(w3, w2, sh & 3);
    o.w = align_byte(w4, w3, sh & 3);
    return o;
}

// 16 bytes from any address: the one or two aligned granules that hold them.
__device__ __forceinline__ uint4 load16_any(u64 addr) {
    const uint4 * g = (const uint4 *)(addr & ~(u64)15);
    const u32 sh = (u32)(addr & 15);
    return sh ? shift_bytes(g[0], g[1], sh) : g[0];
}

// Byte-wise difference / sum of two dwords.  The low seven bits of every byte are subtracted (added) with the top bits set (cleared)
// so that no borrow (carry) leaves a byte; the top bit of every byte is x ^ y ^ borrow (carry), an exclusive or.
__host__ __device__ inline u32 sub_bytes(u32 x, u32 y) { return ((x | 0x80808080u) - (y & 0x7f7f7f7fu)) ^ ((x ^ ~y) & 0x80808080u); }
__host__ __device__ inline u32 add_bytes(u32 x, u32 y) { return ((x & 0x7f7f7f7fu) + (y & 0x7f7f7f7fu)) ^ ((x ^ y) & 0x80808080u); }
template <bool INV>
__device__ __forceinline__ uint4 delta16(uint4 x, uint4 b) {  // x + b (INV) or x - b, 16 bytes
    return INV ? make_uint4(add_bytes(x.x, b.x), add_bytes(x.y, b.y), add_bytes(x.z, b.z), add_bytes(x.w, b.w))
               : make_uint4(sub_bytes(x.x, b.x), sub_bytes(x.y, b.y), sub_bytes(x.z, b.z), sub_bytes(x.w, b.w));
}

// 16 elements of K bytes from any address into 4 K words: the K (aligned) or K + 1 aligned granules that hold them.
template <int K>
__device__ __forceinline__ void load_elems16(u64 addr, u32 (&w)[4 * K]) {
    const uint4 * g = (const uint4 *)(addr & ~(u64)15);
    const u32 sh = (u32)(addr & 15);
    uint4 v[K + 1];
#pragma unroll
    for (int i = 0; i < K; i++) v[i] = g[i];
    if (sh) {
        v[K] = g[K];  // holds the lane's last sh bytes
#pragma unroll
        for (int i = 0; i < K; i++) v[i] = shift_bytes(v[i], v[i + 1], sh);
    }
#pragma unroll
    for (int i = 0; i < K; i++) {
        w[4 * i] = v[i].x;
        w[4 * i + 1] = v[i].y;
        w[4 * i + 2] = v[i].z;
        w[4 * i + 3] = v[i].w;
    }
}

// 16 bytes of LDS from any byte offset: five aligned dwords.
__device__ __forceinline__ uint4 lds16_any(const u8 * lds, u32 x) {
    const u32 * w = (const u32 *)(lds + (x & ~3u));
    uint4 o;
    o.x = align_byte(w[1], w[0], x & 3);
    o.y = align_byte(w[2], w[1], x & 3);
    o.z = align_byte(w[3], w[2], x & 3);
    o.w = align_byte(w[4], w[3], x & 3);
    return o;
}

// 4 x 4 byte transpose: byte c of r[j] -> byte j of r[c].  Its own inverse.
__device__ __forceinline__ void transpose4(u32 & r0, u32 & r1, u32 & r2, u32 & r3) {
    const u32 a = byte_perm(r1, r0, 0x05010400), b = byte_perm(r1, r0, 0x07030602);  // [r0.0 r1.0 r0.1 r1.1], [r0.2 r1.2 r0.3 r1.3]
    const u32 c = byte_perm(r3, r2, 0x05010400), d = byte_perm(r3, r2, 0x07030602);
    r0 = byte_perm(c, a, 0x05040100);
    r1 = byte_perm(c, a, 0x07060302);
    r2 = byte_perm(d, b, 0x05040100);
    r3 = byte_perm(d, b, 0x07060302);
}

// w: 16 elements of K bytes, interleaved (4 K words); p[q]: byte q of the 16 elements (4 words).
template <int K>
__device__ __forceinline__ void deinterleave(const u32 (&w)[4 * K], u32 (&p)[K][4]) {
#pragma unroll
    for (int n = 0; n < 4; n++) {
        if (K == 2) {
            p[0][n] = byte_perm(w[2 * n + 1], w[2 * n], 0x06040200);
            p[1][n] = byte_perm(w[2 * n + 1], w[2 * n], 0x07050301);
        } else {  // words h, h + K/4, h + 2 K/4, h + 3 K/4 of four consecutive elements hold their bytes 4 h .. 4 h + 3
#pragma unroll
            for (int h = 0; h < K / 4; h++) {
                u32 r0 = w[K * n + h], r1 = w[K * n + K / 4 + h], r2 = w[K * n + 2 * (K / 4) + h], r3 = w[K * n + 3 * (K / 4) + h];
                transpose4(r0, r1, r2, r3);
                p[(4 * h + 0) % K][n] = r0;
                p[(4 * h + 1) % K][n] = r1;
                p[(4 * h + 2) % K][n] = r2;
                p[(4 * h + 3) % K][n] = r3;
            }
        }
    }
}

template <int K>
__device__ __forceinline__ void interleave(const u32 (&p)[K][4], u32 (&w)[4 * K]) {
#pragma unroll
    for (int n = 0; n < 4; n++) {
        if (K == 2) {
            w[2 * n] = byte_perm(p[1][n], p[0][n], 0x05010400);
            w[2 * n + 1] = byte_perm(p[1][n], p[0][n], 0x07030602);
        } else {
#pragma unroll
            for (int h = 0; h < K / 4; h++) {
                u32 r0 = p[(4 * h + 0) % K][n], r1 = p[(4 * h + 1) % K][n], r2 = p[(4 * h + 2) % K][n], r3 = p[(4 * h + 3) % K][n];
                transpose4(r0, r1, r2, r3);
                w[K * n + h] = r0;
                w[K * n + K / 4 + h] = r1;
                w[K * n + 2 * (K / 4) + h] = r2;
                w[K * n + 3 * (K / 4) + h] = r3;
            }
        }
    }
}

// Phase 2 of both directions: the bytes [s0, s1) of global memory from LDS, where the byte at address `origin` is lds[0].  Granule
// i of the lane is (s0 & ~15) + 16 (lane + 256 i); granules inside [s0, s1) get one 16-byte store, the partial ones byte stores.
template <int ROUNDS>
__device__ __forceinline__ void store_from_lds(const u8 * lds, u64 origin, u64 s0, u64 s1) {
#pragma unroll
    for (int i = 0; i < ROUNDS; i++) {
        const u64 a = (s0 & ~(u64)15) + 16 * (u64)(threadIdx.x + COPY_THREADS * i);
        if (a >= s1) break;
        if (a >= s0 && a + 16 <= s1) {
            *(uint4 *)a = lds16_any(lds, (u32)(a - origin));
        } else {
            const u64 b0 = a > s0 ? a : s0, b1 = a + 16 < s1 ? a + 16 : s1;
            for (u64 b = b0; b < b1; b++) *(u8 *)b = lds[b - origin];
        }
    }
}

__device__ __forceinline__ u64 align16_up_to(u64 a, u64 end) {
    a = (a + 15) & ~(u64)15;
    return a < end ? a : end;
}

// ---- a lane's 16 elements --------------------------------------------------------------------------------------------------------------
// The 16-byte paths of phase 1.  Merge side: the 16 elements from element index e on of the K planes at `src`, m bytes apart (K == 1: the 16
// bytes at src + e), interleaved into 4 K words; with D, plus the 16 K bytes at address `base`.  The caller has checked that e + 16 <= m and,
// with D, that the 16 K base bytes are the lane's own.
template <int K, bool D>
__device__ __forceinline__ void merged_elems16(const u8 * src, u64 m, u64 e, u64 base, u32 (&w)[4 * K]) {
    if constexpr (K == 1) {
        const uint4 v = load16_any((u64)src + e);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    } else {
        u32 p[K][4];
#pragma unroll
        for (int q = 0; q < K; q++) {
            const uint4 v = load16_any((u64)src + q * m + e);
            p[q][0] = v.x;
            p[q][1] = v.y;
            p[q][2] = v.z;
            p[q][3] = v.w;
        }
        interleave<K>(p, w);
    }
    if (D) {
        u32 b[4 * K];
        load_elems16<K>(base, b);
#pragma unroll
        for (int i = 0; i < 4 * K; i++) w[i] = add_bytes(w[i], b[i]);
    }
}

// Those 4 K words as the lane's K rows of the merge layout of LDS (16 K bytes per lane, in destination order).
template <int K>
__device__ __forceinline__ void rows_to_lds(u8 * lds, const u32 (&w)[4 * K]) {
#pragma unroll
    for (int i = 0; i < K; i++) *(uint4 *)(lds + 16 * (K * threadIdx.x + i)) = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}

// The mirror, split side: the 16 elements of K bytes at address `src`, less with D the 16 K bytes at address `base`, deinterleaved: p[q] is byte q
// of the 16 elements.
template <int K, bool D>
__device__ __forceinline__ void split_elems16(u64 src, u64 base, u32 (&p)[K][4]) {
    u32 w[4 * K];
    load_elems16<K>(src, w);
    if (D) {
        u32 b[4 * K];
        load_elems16<K>(base, b);
#pragma unroll
        for (int i = 0; i < 4 * K; i++) w[i] = sub_bytes(w[i], b[i]);
    }
    if constexpr (K == 1) {
#pragma unroll
        for (int n = 0; n < 4; n++) p[0][n] = w[n];
    } else {
        deinterleave<K>(w, p);
    }
}

// Those K granules as the lane's granule of every plane of the split layout of LDS (PLANE_STRIDE bytes per plane).
template <int K>
__device__ __forceinline__ void planes_to_lds(u8 * lds, const u32 (&p)[K][4]) {
#pragma unroll
    for (int q = 0; q < K; q++) *(uint4 *)(lds + q * PLANE_STRIDE + 16 * threadIdx.x) = make_uint4(p[q][0], p[q][1], p[q][2], p[q][3]);
}

// Tile `tile` of a split: elements [ea, ea + PLANES_TILE_ELEMS) of the block at `src` into the planes at `dst`; with D, of the
// block's byte-wise difference from the bytes at `base`.
template <int K, bool D>
__device__ __forceinline__ void split_tile(const u8 * src, const u8 * base, u8 * dst, u64 len, u64 tile, u8 * lds) {
    const u64 m = len / K, ea = tile * PLANES_TILE_ELEMS;
    const u64 e = ea + 16 * (u64)threadIdx.x;
    if (e + 16 <= m) {
        u32 p[K][4];
        split_elems16<K, D>((u64)src + e * K, (u64)base + e * K, p);
        planes_to_lds<K>(lds, p);
    } else {
        for (u64 i = e; i < m; i++)
            for (int q = 0; q < K; q++) lds[q * PLANE_STRIDE + (i - ea)] = D ? (u8)(src[i * K + q] - base[i * K + q]) : src[i * K + q];
    }
    __syncthreads();
    const bool last = ea + PLANES_TILE_ELEMS >= m;
#pragma unroll
    for (int q = 0; q < K; q++) {
        const u64 p0 = (u64)dst + q * m, pend = p0 + m;
        const u64 s0 = tile == 0 ? p0 : align16_up_to(p0 + ea, pend);
        const u64 s1 = last ? pend : align16_up_to(p0 + ea + PLANES_TILE_ELEMS, pend);
        store_from_lds<1>(lds + q * PLANE_STRIDE, p0 + ea, s0, s1);
    }
    if (tile == 0 && threadIdx.x < len - m * K) {
        const u64 t = m * K + threadIdx.x;
        dst[t] = D ? (u8)(src[t] - base[t]) : src[t];
    }
}

// Tile `tile` of a merge: elements [ea, ea + PLANES_TILE_ELEMS) of the planes at `src` into the block at `dst`; with D, plus the
// bytes at `base` (which may be `dst`: every read of the base is phase 1's or the tail thread's own, see the head of this file).
template <int K, bool D>
__device__ __forceinline__ void merge_tile(const u8 * src, const u8 * base, u8 * dst, u64 len, u64 tile, u8 * lds) {
    const u64 m = len / K, ea = tile * PLANES_TILE_ELEMS;
    const u64 e = ea + 16 * (u64)threadIdx.x;
    if (e + 16 <= m) {
        u32 w[4 * K];
        merged_elems16<K, D>(src, m, e, (u64)base + e * K, w);
        rows_to_lds<K>(lds, w);
    } else {
        for (u64 i = e; i < m; i++)
            for (int q = 0; q < K; q++) lds[(i - ea) * K + q] = D ? (u8)(src[q * m + i] + base[i * K + q]) : src[q * m + i];
    }
    __syncthreads();
    const bool last = ea + PLANES_TILE_ELEMS >= m;
    const u64 d0 = (u64)dst, dend = d0 + m * K;
    const u64 s0 = tile == 0 ? d0 : align16_up_to(d0 + ea * K, dend);
    const u64 s1 = last ? dend : align16_up_to(d0 + (ea + PLANES_TILE_ELEMS) * K, dend);
    store_from_lds<K>(lds, d0 + ea * K, s0, s1);  // at most 255 K + 1 granules
    if (tile == 0 && threadIdx.x < len - m * K) {
        const u64 t = m * K + threadIdx.x;
        dst[t] = D ? (u8)(src[t] + base[t]) : src[t];
    }
}

// One tile of a segment with an element size (CopySeg::mode); D: and a base.
template <bool D>
__device__ __forceinline__ void planes_tile(const CopySeg & sg, u64 tile, u8 * lds) {
    const u8 * src = (const u8 *)sg.src;
    const u8 * base = (const u8 *)sg.base;
    u8 * dst = (u8 *)sg.dst;
    switch ((u32)sg.mode) {
        case 2: split_tile<2, D>(src, base, dst, sg.len, tile, lds); break;
        case 4: split_tile<4, D>(src, base, dst, sg.len, tile, lds); break;
        case 8: split_tile<8, D>(src, base, dst, sg.len, tile, lds); break;
        case 2 | PLANES_INVERSE: merge_tile<2, D>(src, base, dst, sg.len, tile, lds); break;
        case 4 | PLANES_INVERSE: merge_tile<4, D>(src, base, dst, sg.len, tile, lds); break;
        case 8 | PLANES_INVERSE: merge_tile<8, D>(src, base, dst, sg.len, tile, lds); break;
        default: break;
    }
}

// The segment that holds workgroup b of a launch: tile_start[lo] <= b < tile_start[lo + 1].
__device__ __forceinline__ u32 segment_of_tile(const u32 * __restrict__ tile_start, u32 nseg, u32 b) {
    u32 lo = 0, hi = nseg;  // invariant: tile_start[lo] <= b < tile_start[hi]
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (tile_start[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// k_copy_segments for a launch in which some segment has an element size: segments without one take copy_tile as before, the
// others split_tile / merge_tile.  tile_start counts a segment's workgroups with segment_tiles.  (A kernel of its own so that launches
// of plain copies keep k_copy_segments, which holds no LDS.)
__global__ void __launch_bounds__(COPY_THREADS) k_move_segments(const CopySeg * __restrict__ segs, const u32 * __restrict__ tile_start, u32 nseg) {
    __shared__ uint4 lds[PLANES_LDS_BYTES / 16];
    const u32 lo = segment_of_tile(tile_start, nseg, blockIdx.x);
    const CopySeg sg = segs[lo];
    if ((sg.mode & 0xff) > 1) planes_tile<false>(sg, blockIdx.x - tile_start[lo], (u8 *)lds);
    else copy_segment_tile(sg, blockIdx.x - tile_start[lo]);
}

// ---- delta segments ---------------------------------------------------------------------------------------------------------------
// One tile of a segment with a base and no element size: copy_tile's tiling (COPY_TILE_GRANULES destination granules from g_first), a
// destination granule = the source's 16 bytes minus (INV: plus) the base's, each built from the one or two aligned granules that hold
// them (both hold bytes of the segment, or of the base range, because the destination granule lies inside the segment), one 16-byte
// store; byte by byte at the partial granules of the two ends.
template <bool INV>
__device__ __forceinline__ void delta1_tile(const u8 * src, const u8 * base, u8 * dst, u64 len, u64 g_first, u64 g_end) {
    const u64 d0 = (u64)dst, d1 = d0 + len;
    const u64 ds = (u64)src - d0, db = (u64)base - d0;  // source / base address = destination address + ds / db (mod 2^64)
    if (g_end - g_first == COPY_TILE_GRANULES && (g_first << 4) >= d0 && (g_end << 4) <= d1) {  // every granule of the tile is full: loads first, then stores
        uint4 x[COPY_GRANULES_PER_LANE], b[COPY_GRANULES_PER_LANE];
#pragma unroll
        for (u32 k = 0; k < COPY_GRANULES_PER_LANE; k++) {
            const u64 a = (g_first + k * COPY_THREADS + threadIdx.x) << 4;
            x[k] = load16_any(a + ds);
            b[k] = load16_any(a + db);
        }
#pragma unroll
        for (u32 k = 0; k < COPY_GRANULES_PER_LANE; k++) *(uint4 *)((g_first + k * COPY_THREADS + threadIdx.x) << 4) = delta16<INV>(x[k], b[k]);
        return;
    }
    for (u32 k = 0; k < COPY_GRANULES_PER_LANE; k++) {
        const u64 g = g_first + k * COPY_THREADS + threadIdx.x;
        if (g >= g_end) break;
        const u64 a = g << 4;  // destination granule [a, a + 16)
        if (a >= d0 && a + 16 <= d1) {
            *(uint4 *)a = delta16<INV>(load16_any(a + ds), load16_any(a + db));
        } else {
            const u64 b0 = a > d0 ? a : d0, b1 = a + 16 < d1 ? a + 16 : d1;
            for (u64 b = b0; b < b1; b++) *(u8 *)b = INV ? (u8)(*(const u8 *)(b + ds) + *(const u8 *)(b + db)) : (u8)(*(const u8 *)(b + ds) - *(const u8 *)(b + db));
        }
    }
}

// ---- diff segments ------------------------------------------------------------------------------------------------------------------
// Do a[0, len) and b[0, len) differ in any byte?  A diff segment is CopySeg{src = a, dst = 0, len, mode = its flag's index, base = b}: two read
// streams and no destination.  The tiling is delta1_tile's with `a` in the destination's place: copy_tiles(a, len) tiles of COPY_TILE_GRANULES
// aligned granules of `a`, one per lane and round.  A granule of `a` that lies inside the run is one aligned 16-byte load, and the 16 bytes of
// `b` that pair with it are load16_any's one or two aligned granules, which both hold bytes of b[0, len) because the 16 bytes do and, where there
// are two, straddle their seam.  The partial granules at the run's two ends are compared byte by byte over [max(a, granule), min(a + len, granule
// + 16)) alone, so a byte before or behind the run is never read, let alone compared: no granule is loaded that holds no byte of the run.
// Returns the OR of the lane's XORs.
__device__ __forceinline__ u32 diff_tile(const u8 * a, const u8 * b, u64 len, u64 g_first, u64 g_end) {
    const u64 a0 = (u64)a, a1 = a0 + len;
    const u64 db = (u64)b - a0;  // b's address = a's address + db (mod 2^64)
    u32 acc = 0;
    if (g_end - g_first == COPY_TILE_GRANULES && (g_first << 4) >= a0 && (g_end << 4) <= a1) {  // every granule of the tile is full: all loads first
        uint4 x[COPY_GRANULES_PER_LANE], y[COPY_GRANULES_PER_LANE];
#pragma unroll
        for (u32 k = 0; k < COPY_GRANULES_PER_LANE; k++) {
            const u64 p = (g_first + k * COPY_THREADS + threadIdx.x) << 4;
            x[k] = *(const uint4 *)p;
            y[k] = load16_any(p + db);
        }
#pragma unroll
        for (u32 k = 0; k < COPY_GRANULES_PER_LANE; k++) acc |= (x[k].x ^ y[k].x) | (x[k].y ^ y[k].y) | (x[k].z ^ y[k].z) | (x[k].w ^ y[k].w);
        return acc;
    }
    for (u32 k = 0; k < COPY_GRANULES_PER_LANE; k++) {
        const u64 g = g_first + k * COPY_THREADS + threadIdx.x;
        if (g >= g_end) break;
        const u64 p = g << 4;  // a's granule [p, p + 16)
        if (p >= a0 && p + 16 <= a1) {
            const uint4 x = *(const uint4 *)p, y = load16_any(p + db);
            acc |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
        } else {
            const u64 b0 = p > a0 ? p : a0, b1 = p + 16 < a1 ? p + 16 : a1;
            for (u64 q = b0; q < b1; q++) acc |= (u32)(*(const u8 *)q ^ *(const u8 *)(q + db));
        }
    }
    return acc;
}

// flags[segs[i].mode] becomes 1 where the two runs of diff segment i differ; the caller zeroes `flags` on the stream before the launch, and a flag
// no workgroup stores to stays 0.  tile_start counts a segment's workgroups with copy_tiles(src, len).  No LDS and no barrier: of every wave that
// found a difference, the lowest lane that did stores the 1 (an ordinary vector store; several waves and workgroups may store the same value).
__global__ void __launch_bounds__(COPY_THREADS) k_diff_segments(const CopySeg * __restrict__ segs, const u32 * __restrict__ tile_start, u32 nseg, u32 * __restrict__ flags) {
    const u32 lo = segment_of_tile(tile_start, nseg, blockIdx.x);
    const CopySeg sg = segs[lo];
    const u64 g_first = (sg.src >> 4) + (u64)(blockIdx.x - tile_start[lo]) * COPY_TILE_GRANULES, g_end = (sg.src + sg.len + 15) >> 4;
    const u64 g_last = g_first + COPY_TILE_GRANULES < g_end ? g_first + COPY_TILE_GRANULES : g_end;
    const u32 acc = diff_tile((const u8 *)sg.src, (const u8 *)sg.base, sg.len, g_first, g_last);
    const u64 found = __ballot(acc != 0);
    if (acc != 0 && (found & (((u64)1 << (threadIdx.x & 63)) - 1)) == 0) flags[sg.mode] = 1;
}

// ---- clipped merge ------------------------------------------------------------------------------------------------------------------
// The tiles of a merge of `len` bytes that hold an element byte of its bytes [a, b), a < b <= len: tiles first .. first + count - 1 of
// planes_tiles(len, k).  A clip that holds tail bytes only still takes one tile, which stores them.
__host__ __device__ inline u64 clip_first_tile(u64 len, u64 k, u64 a) {
    const u64 t = a / (k * PLANES_TILE_ELEMS), n = planes_tiles(len, k);
    return t < n ? t : n - 1;
}
__host__ __device__ inline u64 clip_tiles(u64 len, u64 k, u64 a, u64 b) {
    const u64 mk = len / k * k, bm = b < mk ? b : mk;  // the clip's element bytes end at bm
    return bm > a ? (bm - 1) / (k * PLANES_TILE_ELEMS) - a / (k * PLANES_TILE_ELEMS) + 1 : 1;
}

// Tile clip_first_tile + rel of a merge of the `len` bytes at `src`, of which the bytes [ca, cb) go to dst[0, cb - ca); with D, plus
// base[0, cb - ca) (which may be `dst`).  See the head of this file.
template <int K, bool D>
__device__ __forceinline__ void clip_merge_tile(const u8 * src, const u8 * base, u8 * dst, u64 len, u64 ca, u64 cb, u64 rel, u8 * lds) {
    const u64 m = len / K, ea = (clip_first_tile(len, K, ca) + rel) * PLANES_TILE_ELEMS;
    const u64 e = ea + 16 * (u64)threadIdx.x;
    const u64 bm = cb < m * K ? cb : m * K;
    const u64 l0 = e * K, l1 = (e + 16) * K;  // the chunk bytes of the lane's elements
    if (l0 < bm && l1 > ca) {
        if (e + 16 <= m && (!D || (l0 >= ca && l1 <= cb))) {
            u32 w[4 * K];
            merged_elems16<K, D>(src, m, e, (u64)base + (l0 - ca), w);
            rows_to_lds<K>(lds, w);
        } else {
            for (u64 i = e; i < m && i < e + 16; i++)
                for (int q = 0; q < K; q++) {
                    const u64 c = i * K + q;
                    if (c >= ca && c < cb) lds[c - ea * K] = D ? (u8)(src[q * m + i] + base[c - ca]) : src[q * m + i];
                }
        }
    }
    __syncthreads();
    if (bm > ca) {
        const u64 d0 = (u64)dst, dend = d0 + (bm - ca);  // the chunk's byte c lives at d0 + (c - ca)
        const u64 t0 = ea * K, t1 = (ea + PLANES_TILE_ELEMS) * K;
        const u64 s0 = t0 <= ca ? d0 : align16_up_to(d0 + (t0 - ca), dend);
        const u64 s1 = t1 >= bm ? dend : t1 <= ca ? d0 : align16_up_to(d0 + (t1 - ca), dend);
        store_from_lds<K>(lds, d0 + t0 - ca, s0, s1);  // (the origin may lie below dst: only differences from it are used)
    }
    if (rel == 0 && threadIdx.x < len - m * K) {
        const u64 t = m * K + threadIdx.x;
        if (t >= ca && t < cb) dst[t - ca] = D ? (u8)(src[t] + base[t - ca]) : src[t];
    }
}

// ---- clipped split ------------------------------------------------------------------------------------------------------------------
// Tile clip_first_tile + rel of a split INTO the `len` bytes at `dst`, which hold split_k of a chunk: of the chunk's bytes only [ca, cb) are
// replaced, by src[0, cb - ca); with D, less base[0, cb - ca).  See the head of this file.
template <int K, bool D>
__device__ __forceinline__ void clip_split_tile(const u8 * src, const u8 * base, u8 * dst, u64 len, u64 ca, u64 cb, u64 rel, u8 * lds) {
    const u64 m = len / K, ea = (clip_first_tile(len, K, ca) + rel) * PLANES_TILE_ELEMS;
    const u64 e = ea + 16 * (u64)threadIdx.x;
    const u64 bm = cb < m * K ? cb : m * K;
    const u64 l0 = e * K, l1 = (e + 16) * K;  // the chunk bytes of the lane's elements
    if (l0 < bm && l1 > ca) {
        if (l0 >= ca && l1 <= bm) {  // (l1 <= bm <= m K: the lane's 16 elements are whole elements of the chunk)
            u32 p[K][4];
            split_elems16<K, D>((u64)src + (l0 - ca), (u64)base + (l0 - ca), p);
            planes_to_lds<K>(lds, p);
        } else {
            for (u64 i = e; i < m && i < e + 16; i++)
                for (int q = 0; q < K; q++) {
                    const u64 c = i * K + q;
                    if (c >= ca && c < cb) lds[q * PLANE_STRIDE + (i - ea)] = D ? (u8)(src[c - ca] - base[c - ca]) : src[c - ca];
                }
        }
    }
    __syncthreads();
    if (bm > ca) {
#pragma unroll
        for (int q = 0; q < K; q++) {
            // plane q holds the clip's elements [e0, e1): those e with ca <= e K + q < bm
            const u64 e0 = ca > (u64)q ? (ca - q + K - 1) / K : 0, e1 = bm > (u64)q ? (bm - q + K - 1) / K : 0;
            const u64 p0 = (u64)dst + q * m, pend = p0 + m;
            const u64 s0 = rel == 0 ? p0 + e0 : align16_up_to(p0 + ea, pend);  // (the first tile launched starts the clip, wherever its own granules start)
            const u64 t1 = align16_up_to(p0 + ea + PLANES_TILE_ELEMS, pend);
            const u64 s1 = t1 < p0 + e1 ? t1 : p0 + e1;
            if (s0 < s1) store_from_lds<1>(lds + q * PLANE_STRIDE, p0 + ea, s0, s1);
        }
    }
    if (rel == 0 && threadIdx.x < len - m * K) {
        const u64 t = m * K + threadIdx.x;
        if (t >= ca && t < cb) dst[t] = D ? (u8)(src[t - ca] - base[t - ca]) : src[t - ca];
    }
}

// ---- gather merges: strided and select ---------------------------------------------------------------------------------------------------
// Workgroups of a gather merge (or of a select split) of nbytes contiguous bytes: one per PLANES_TILE_ELEMS k of them.
__host__ __device__ inline u64 strided_tiles(u64 nbytes, u64 k) { return (nbytes + k * PLANES_TILE_ELEMS - 1) / (k * PLANES_TILE_ELEMS); }

// A cursor walks the chunk bytes c(u) of a segment's contiguous side from a lane's first byte u0 on (the head of this file): `c` is the chunk
// byte of the lane's current byte, `left` what is left of its run or piece from there, step(more) goes on one byte (more: the lane has another
// byte to move).  Chunk bytes are taken mod 2^32: every c(u) that is read or written lies below the chunk's 2^31 bytes.

// The strided walk: chunk byte c0, `first` bytes from it on, then runs of `run` bytes with `gap` = stride - run bytes between them.
struct StridedRuns {
    u32 c0, first, run, gap;
};
struct StridedCursor {
    using Walk = StridedRuns;
    u32 c, left;
    const u32 run, gap;
    __device__ __forceinline__ StridedCursor(const StridedRuns & r, u32 u0) : run(r.run), gap(r.gap) {  // one division
        if (u0 < r.first) {
            c = r.c0 + u0;
            left = r.first - u0;
        } else {
            const u32 v = u0 - r.first, q = v / run;
            c = r.c0 + u0 + (q + 1) * gap;
            left = run - (v - q * run);
        }
    }
    __device__ __forceinline__ void step(bool) {
        c++;
        if (--left == 0) {
            c += gap;
            left = run;
        }
    }
};

// The piece of a table of m (pairs (s_j, P_j), closed by P_m) that holds byte r < P_m of the period's wanted bytes: P_j <= r < P_{j+1}.
__host__ __device__ inline u32 piece_of(const u64 * tab, u32 m, u64 r) {
    u32 lo = 0, hi = m;  // invariant: P_lo <= r < P_hi
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (tab[2 * mid + 1] <= r) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The select walk over a segment's SELECT_PARAMS sp: one division (32 bits where L < 2^31, else a comparison: x < L + 2^31 then) and one binary
// search over P locate the lane's first byte; from there it steps through the pieces linearly, skipping empty ones, with the chunk byte of the
// period's start in hand.
struct SelectCursor {
    using Walk = const u64 *;
    const u64 * __restrict__ tab;
    const u32 np, stride;
    u32 j, cb, c, left;  // the piece, the chunk byte of its period's first byte
    __device__ __forceinline__ SelectCursor(const u64 * __restrict__ sp, u32 u0) : tab((const u64 *)sp[5]), np((u32)sp[6]), stride((u32)sp[1]) {
        const u64 L = tab[2 * np + 1], x = sp[3] + u0;
        u64 q, r;  // x = q L + r
        if (L >> 31) {
            q = x >= L ? 1 : 0;
            r = x - (q ? L : 0);
        } else {
            q = (u32)x / (u32)L;
            r = (u32)x - (u32)q * (u32)L;
        }
        j = piece_of(tab, np, r);
        cb = (u32)(sp[0] + (sp[2] + q) * sp[1]);
        const u64 in = r - tab[2 * j + 1], rest = tab[2 * j + 3] - r;  // bytes of piece j before and from the lane's first byte
        c = cb + (u32)(tab[2 * j] + in);
        left = rest < 0x7fffffffu ? (u32)rest : 0x7fffffffu;  // (beyond the chunk's 2^31 bytes: no byte of the segment lies behind it)
    }
    __device__ __forceinline__ void step(bool more) {
        c++;
        if (--left == 0 && more) {  // the next piece that is not empty (there is one: L > 0), in the next period behind the last
            u64 l;
            do {
                if (++j == np) {
                    j = 0;
                    cb += stride;
                }
                l = tab[2 * j + 3] - tab[2 * j + 1];
            } while (l == 0);
            c = cb + (u32)tab[2 * j];
            left = l < 0x7fffffffu ? (u32)l : 0x7fffffffu;
        }
    }
};

// Tile `tile` of a gather merge of the `len` < 2^31 bytes at `src`: destination bytes [0, nbytes) from the chunk bytes c(u) that a Cursor over
// `walk` names (the head of this file, "Gather merges"), to dst; with D, plus base[0, nbytes) (which may be `dst`).  Workgroups:
// strided_tiles(nbytes, k).
template <int K, bool D, class Cursor>
__device__ __forceinline__ void gather_tile(const u8 * src, const u8 * base, u8 * dst, u32 len, u32 nbytes, const typename Cursor::Walk & walk, u32 tile, u8 * lds) {
    const u32 m = len / K, ua = tile * (PLANES_TILE_ELEMS * K);
    const u32 u0 = ua + 16 * K * threadIdx.x;
    if (u0 < nbytes) {
        Cursor cur(walk, u0);
        if (cur.left >= 16 * K && u0 + 16 * K <= nbytes && cur.c % K == 0 && cur.c + 16 * K <= m * K) {
            u32 w[4 * K];
            merged_elems16<K, D>(src, m, cur.c / K, (u64)base + u0, w);
            rows_to_lds<K>(lds, w);
        } else {
            const u32 u1 = u0 + 16 * K < nbytes ? u0 + 16 * K : nbytes;
            for (u32 u = u0; u < u1; u++) {
                const u8 x = src[cur.c < m * K ? (cur.c % K) * m + cur.c / K : cur.c];
                lds[u - ua] = D ? (u8)(x + base[u]) : x;
                cur.step(u + 1 < u1);
            }
        }
    }
    __syncthreads();
    const u64 d0 = (u64)dst, dend = d0 + nbytes;
    const u64 s0 = tile == 0 ? d0 : align16_up_to(d0 + ua, dend);
    const u64 s1 = ua + PLANES_TILE_ELEMS * K >= nbytes ? dend : align16_up_to(d0 + ua + PLANES_TILE_ELEMS * K, dend);
    store_from_lds<K>(lds, d0 + ua, s0, s1);  // at most 255 K + 1 granules
}

// ---- the segment kernels -------------------------------------------------------------------------------------------------------------
// The kinds of segment a launch may hold, in the order they were added: every kind's kernel handles the kinds below it as well.
enum SegLevel : int { SEG_DELTA = 0, SEG_CLIP = 1, SEG_STRIDED = 2, SEG_SELECT = 3 };

// f(K, D) with the segment's element size and whether it has a base as constants (K() and D() are constant expressions): the one switch of every
// partial tile.  It is written into every branch that calls it: its value computed once above the branches costs four to six SGPRs.
template <int K>
using ElemSize = std::integral_constant<int, K>;
template <class F>
__device__ __forceinline__ void with_elem_size_and_base(const CopySeg & sg, F && f) {
    switch ((u32)(sg.mode & 0xff) | (sg.base ? 16u : 0u)) {
        case 1: f(ElemSize<1>(), std::false_type()); break;
        case 2: f(ElemSize<2>(), std::false_type()); break;
        case 4: f(ElemSize<4>(), std::false_type()); break;
        case 8: f(ElemSize<8>(), std::false_type()); break;
        case 1 | 16: f(ElemSize<1>(), std::true_type()); break;
        case 2 | 16: f(ElemSize<2>(), std::true_type()); break;
        case 4 | 16: f(ElemSize<4>(), std::true_type()); break;
        case 8 | 16: f(ElemSize<8>(), std::true_type()); break;
        default: break;
    }
}

// One tile of a segment that is moved whole: a copy, a split or a merge, with or without a base.
__device__ __forceinline__ void whole_segment_tile(const CopySeg & sg, u32 tile, u8 * lds) {
    if (!sg.base) {
        if ((sg.mode & 0xff) > 1) planes_tile<false>(sg, tile, lds);
        else copy_segment_tile(sg, tile);
    } else if ((sg.mode & 0xff) > 1) {
        planes_tile<true>(sg, tile, lds);
    } else {
        const u64 g_first = (sg.dst >> 4) + (u64)tile * COPY_TILE_GRANULES, g_end = (sg.dst + sg.len + 15) >> 4;
        const u64 g_last = g_first + COPY_TILE_GRANULES < g_end ? g_first + COPY_TILE_GRANULES : g_end;
        if (sg.mode & PLANES_INVERSE) delta1_tile<true>((const u8 *)sg.src, (const u8 *)sg.base, (u8 *)sg.dst, sg.len, g_first, g_last);
        else delta1_tile<false>((const u8 *)sg.src, (const u8 *)sg.base, (u8 *)sg.dst, sg.len, g_first, g_last);
    }
}

// One workgroup of a launch whose highest segment kind is LEVEL: the tile of its segment, by the segment's mode.  clips[2 i], clips[2 i + 1]
// are segment i's [a, b) (read for segments with PLANES_CLIP alone, LEVEL >= SEG_CLIP), periods[5 i .. 5 i + 4] its c0, first, run, stride and
// nbytes (PLANES_STRIDED, LEVEL >= SEG_STRIDED), selects[7 i .. 7 i + 6] its SELECT_PARAMS (PLANES_SELECT, LEVEL == SEG_SELECT); tile_start counts
// a segment's workgroups with strided_tiles, strided_tiles, clip_tiles and segment_tiles in that order.  A branch above LEVEL is not compiled,
// so a kernel holds the code of its own kinds alone.
template <int LEVEL>
__device__ __forceinline__ void segments_tile(const CopySeg * __restrict__ segs, const u32 * __restrict__ tile_start, u32 nseg, const u64 * __restrict__ clips,
                                              const u64 * __restrict__ periods, const u64 * __restrict__ selects, u8 * lds) {
    const u32 lo = segment_of_tile(tile_start, nseg, blockIdx.x);
    const CopySeg sg = segs[lo];
    const u32 tile = blockIdx.x - tile_start[lo];
    const u8 * src = (const u8 *)sg.src;
    const u8 * base = (const u8 *)sg.base;
    u8 * dst = (u8 *)sg.dst;
    if (LEVEL >= SEG_SELECT && (sg.mode & PLANES_SELECT)) {
        const u64 * sp = selects + (u64)SELECT_PARAMS * lo;
        with_elem_size_and_base(sg, [&](auto K, auto D) { gather_tile<K(), D(), SelectCursor>(src, base, dst, (u32)sg.len, (u32)sp[4], sp, tile, lds); });
    } else if (LEVEL >= SEG_STRIDED && (sg.mode & PLANES_STRIDED)) {
        const u64 * pp = periods + (u64)STRIDED_PARAMS * lo;
        const u32 c0 = (u32)pp[0], first = (u32)pp[1], nbytes = (u32)pp[4];
        const u32 run = pp[2] < 0x7fffffffu ? (u32)pp[2] : 0x7fffffffu;  // (a run beyond the chunk's 2^31 bytes: no destination byte lies behind it)
        const u32 gap = nbytes > first ? (u32)(pp[3] - pp[2]) : 0;
        with_elem_size_and_base(sg, [&](auto K, auto D) { gather_tile<K(), D(), StridedCursor>(src, base, dst, (u32)sg.len, nbytes, {c0, first, run, gap}, tile, lds); });
    } else if (LEVEL >= SEG_CLIP && (sg.mode & PLANES_CLIP)) {
        const u64 ca = clips[2 * lo], cb = clips[2 * lo + 1];
        switch ((u32)(sg.mode & 0xff) | (sg.base ? 16u : 0u)) {  // (written out: through with_elem_size_and_base k_range_segments and k_strided_segments take two more SGPRs)
            case 2: clip_merge_tile<2, false>(src, base, dst, sg.len, ca, cb, tile, lds); break;
            case 4: clip_merge_tile<4, false>(src, base, dst, sg.len, ca, cb, tile, lds); break;
            case 8: clip_merge_tile<8, false>(src, base, dst, sg.len, ca, cb, tile, lds); break;
            case 2 | 16: clip_merge_tile<2, true>(src, base, dst, sg.len, ca, cb, tile, lds); break;
            case 4 | 16: clip_merge_tile<4, true>(src, base, dst, sg.len, ca, cb, tile, lds); break;
            case 8 | 16: clip_merge_tile<8, true>(src, base, dst, sg.len, ca, cb, tile, lds); break;
            default: break;
        }
    } else {
        whole_segment_tile(sg, tile, lds);
    }
}

// The four kernels of launches in which some segment has a base, is a clipped, a strided or a select merge.  Kernels of their own, as
// k_move_segments is, so that a launch without the higher kinds keeps the code and the registers of the kernel below: the wrappers declare
// the LDS and pass the tables they have.
__global__ void __launch_bounds__(COPY_THREADS) k_delta_segments(const CopySeg * __restrict__ segs, const u32 * __restrict__ tile_start, u32 nseg) {
    __shared__ uint4 lds[PLANES_LDS_BYTES / 16];
    segments_tile<SEG_DELTA>(segs, tile_start, nseg, nullptr, nullptr, nullptr, (u8 *)lds);
}

__global__ void __launch_bounds__(COPY_THREADS) k_range_segments(const CopySeg * __restrict__ segs, const u32 * __restrict__ tile_start, u32 nseg,
                                                                 const u64 * __restrict__ clips) {
    __shared__ uint4 lds[PLANES_LDS_BYTES / 16];
    segments_tile<SEG_CLIP>(segs, tile_start, nseg, clips, nullptr, nullptr, (u8 *)lds);
}

__global__ void __launch_bounds__(COPY_THREADS) k_strided_segments(const CopySeg * __restrict__ segs, const u32 * __restrict__ tile_start, u32 nseg,
                                                                   const u64 * __restrict__ clips, const u64 * __restrict__ periods) {
    __shared__ uint4 lds[PLANES_LDS_BYTES / 16];
    segments_tile<SEG_STRIDED>(segs, tile_start, nseg, clips, periods, nullptr, (u8 *)lds);
}

__global__ void __launch_bounds__(COPY_THREADS) k_select_segments(const CopySeg * __restrict__ segs, const u32 * __restrict__ tile_start, u32 nseg,
                                                                  const u64 * __restrict__ clips, const u64 * __restrict__ periods, const u64 * __restrict__ selects) {
    __shared__ uint4 lds[PLANES_LDS_BYTES / 16];
    segments_tile<SEG_SELECT>(segs, tile_start, nseg, clips, periods, selects, (u8 *)lds);
}

// ---- select split --------------------------------------------------------------------------------------------------------------------
// Tile `tile` of a select split INTO the `len` < 2^31 bytes at `dst`, which hold split_k of a chunk: the chunk bytes c(u), u < nbytes (the head of
// this file, "Select split"; sp: the segment's SELECT_PARAMS), get src[u]; with D, less base[u].  Workgroups: strided_tiles(nbytes, k); the first
// 255 lanes of one own 16 k source bytes each (the tiling of the gather merge's destination, which needs its 256th lane for the straddling
// granule alone: here nothing straddles).  No LDS and no barrier: every store leaves the lane that loaded the byte.
template <int K, bool D>
__device__ __forceinline__ void select_split_tile(const u8 * src, const u8 * base, u8 * dst, u32 len, const u64 * __restrict__ sp, u32 tile) {
    const u32 m = len / K, nbytes = (u32)sp[4];
    const u32 u0 = tile * (PLANES_TILE_ELEMS * K) + 16 * K * threadIdx.x;
    if (threadIdx.x >= COPY_THREADS - 1 || u0 >= nbytes) return;
    SelectCursor cur(sp, u0);
    if (cur.left >= 16 * K && u0 + 16 * K <= nbytes && cur.c % K == 0 && cur.c + 16 * K <= m * K) {
        u32 p[K][4];
        split_elems16<K, D>((u64)src + u0, (u64)base + u0, p);
#pragma unroll
        for (int i = 0; i < K; i++) {  // plane i: the lane's 16 bytes, one granule where they are one
            const u64 a = (u64)dst + (u64)i * m + cur.c / K;
            if ((a & 15) == 0) {
                *(uint4 *)a = make_uint4(p[i][0], p[i][1], p[i][2], p[i][3]);
            } else {
#pragma unroll
                for (int t = 0; t < 16; t++) *(u8 *)(a + t) = (u8)(p[i][t / 4] >> (8 * (t % 4)));
            }
        }
    } else {
        const u32 u1 = u0 + 16 * K < nbytes ? u0 + 16 * K : nbytes;
        for (u32 u = u0; u < u1; u++) {
            dst[cur.c < m * K ? (cur.c % K) * m + cur.c / K : cur.c] = D ? (u8)(src[u] - base[u]) : src[u];
            cur.step(u + 1 < u1);
        }
    }
}

// ---- replane ---------------------------------------------------------------------------------------------------------------------------
// Where split_k keeps byte c of a chunk of len bytes: pos(c; len) of the head of this file, "Replane".
__host__ __device__ inline u64 plane_pos(u64 c, u64 len, u64 k) {
    const u64 m = len / k;
    return c < m * k ? (c % k) * m + c / k : c;
}
// Workgroups of a replane segment that keeps the chunk bytes [0, a): k plane runs of a / k bytes, each with the tiles a run of that length takes
// at the worst destination alignment (a run touches at most (n + 30) / 16 granules), so that a tile index names its plane by one division; a
// segment with nothing but stray bytes still has the tile that moves them.
__host__ __device__ inline u64 replane_plane_tiles(u64 a, u64 k) { return a / k ? (((a / k + 30) >> 4) + COPY_TILE_GRANULES - 1) / COPY_TILE_GRANULES : 0; }
__host__ __device__ inline u64 replane_tiles(u64 a, u64 k) {
    const u64 t = k * replane_plane_tiles(a, k);
    return a ? (t ? t : 1) : 0;
}

// Tile `tile` of a replane from the slot at `src`, which holds split_k of a chunk of len_old bytes, to the slot at `dst`, which is to hold split_k of
// a chunk of len_new bytes with the same first a bytes, a <= min(len_old, len_new), k = 2, 4 or 8: plane q's first a / k bytes are one run from
// src + q (len_old / k) to dst + q (len_new / k), moved by copy_tile, tile / per naming the plane and tile % per the tile within it; the bytes
// of the partial element at a (fewer than k; they may lie in either chunk's tail) are moved one by one by the first threads of tile 0.  No
// other byte of dst is written, and no granule is loaded that holds no byte of a run.
__device__ __forceinline__ void replane_tile(const u8 * src, u8 * dst, u64 len_old, u64 len_new, u64 a, u32 k, u32 tile) {
    const u32 sh = k == 2 ? 1 : k == 4 ? 2 : 3;
    const u64 n = a >> sh;
    const u32 per = (u32)replane_plane_tiles(a, k);
    if (per) {
        const u32 q = tile / per;
        const CopySeg run = {(u64)src + q * (len_old >> sh), (u64)dst + q * (len_new >> sh), n, 0, 0};
        if (q < k && (u64)(tile - q * per) < copy_tiles(run.dst, n)) copy_segment_tile(run, tile - q * per);
    }
    if (tile == 0 && threadIdx.x < a - (n << sh)) {
        const u64 c = (n << sh) + threadIdx.x;
        dst[plane_pos(c, len_new, k)] = src[plane_pos(c, len_old, k)];
    }
}

// One workgroup of an update's patch launch: a select split (SELECT alone compiles it), a replane (REPLANE alone compiles it), whose len_old and a
// are clips[2 i], clips[2 i + 1], a clipped split, whose [a, b) are clips[2 i], clips[2 i + 1], or a segment that is moved whole.
template <bool SELECT, bool REPLANE = false>
__device__ __forceinline__ void patch_segments_tile(const CopySeg * __restrict__ segs, const u32 * __restrict__ tile_start, u32 nseg, const u64 * __restrict__ clips,
                                                    const u64 * __restrict__ selects, u8 * lds) {
    const u32 lo = segment_of_tile(tile_start, nseg, blockIdx.x);
    const CopySeg sg = segs[lo];
    const u32 tile = blockIdx.x - tile_start[lo];
    const u8 * src = (const u8 *)sg.src;
    const u8 * base = (const u8 *)sg.base;
    u8 * dst = (u8 *)sg.dst;
    if (REPLANE && (sg.mode & PLANES_REPLANE)) return replane_tile(src, dst, clips[2 * lo], sg.len, clips[2 * lo + 1], (u32)(sg.mode & 0xff), tile);
    if (SELECT && (sg.mode & PLANES_SELECT)) {
        const u64 * sp = selects + (u64)SELECT_PARAMS * lo;
        return with_elem_size_and_base(sg, [&](auto K, auto D) { select_split_tile<K(), D()>(src, base, dst, (u32)sg.len, sp, tile); });
    }
    if (!(sg.mode & PLANES_CLIP)) return whole_segment_tile(sg, tile, lds);
    const u64 ca = clips[2 * lo], cb = clips[2 * lo + 1];
    with_elem_size_and_base(sg, [&](auto K, auto D) {
        if constexpr (K() > 1) clip_split_tile<K(), D()>(src, base, dst, sg.len, ca, cb, tile, lds);  // (a k = 1 clip is an ordinary segment)
    });
}

// The kernel of an update's patch launch (bz3_hip_update_device_range, api_frames.hip): clipped splits beside segments that are moved whole.  It
// holds no merge that is clipped, strided or selected, and the kernels above hold no clipped split: a launch has segments of one family
// (copy_segments sees to it).
__global__ void __launch_bounds__(COPY_THREADS) k_patch_segments(const CopySeg * __restrict__ segs, const u32 * __restrict__ tile_start, u32 nseg,
                                                                 const u64 * __restrict__ clips) {
    __shared__ uint4 lds[PLANES_LDS_BYTES / 16];
    patch_segments_tile<false>(segs, tile_start, nseg, clips, nullptr, (u8 *)lds);
}

// The same for a patch launch that holds a select split (bz3_hip_update_device_select, api_frames.hip), whose SELECT_PARAMS are selects[7 i .. 7 i + 6].
// A kernel of its own, as every kind's is, so that a patch launch without one keeps k_patch_segments.
__global__ void __launch_bounds__(COPY_THREADS) k_patch_select_segments(const CopySeg * __restrict__ segs, const u32 * __restrict__ tile_start, u32 nseg,
                                                                        const u64 * __restrict__ clips, const u64 * __restrict__ selects) {
    __shared__ uint4 lds[PLANES_LDS_BYTES / 16];
    patch_segments_tile<true>(segs, tile_start, nseg, clips, selects, (u8 *)lds);
}

// The same for a patch launch that holds a replane segment (bz3_hip_resize_device, api_frames.hip), whose len_old and a are clips[2 i],
// clips[2 i + 1]: the kept head of a decoded chunk moves to the byte planes of its new length while the clipped split beside it lays the new
// bytes behind it.  A kernel of its own, so that a patch launch without one keeps k_patch_segments.
__global__ void __launch_bounds__(COPY_THREADS) k_replane_segments(const CopySeg * __restrict__ segs, const u32 * __restrict__ tile_start, u32 nseg,
                                                                   const u64 * __restrict__ clips) {
    __shared__ uint4 lds[PLANES_LDS_BYTES / 16];
    patch_segments_tile<false, true>(segs, tile_start, nseg, clips, nullptr, (u8 *)lds);
}

}  // namespace bz3
