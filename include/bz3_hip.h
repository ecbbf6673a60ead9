/*
 * bz3_hip.h -- extensions of the libbz3.h C ABI that only make sense for a GPU backend.
 * Plain C, plain pointers and sizes; no torch / HIP types in any signature (device memory is passed
 * as void* addresses, e.g. torch.Tensor.data_ptr()).
 *
 *  - device-resident block entry points: same contract as bz3_encode_block(s)/bz3_decode_block(s)
 *    (reference src/libbz3.c:585-654, :656-809, :845-870) but `buffer` is a DEVICE pointer, so a
 *    pipeline that already has its data in HBM (or bench.py) skips the PCIe hops;
 *  - device selection for the multi-GPU block sharding of SURVEY.md section 8e;
 *  - per-stage entry points on host buffers, used by the parity tests to diff each HIP stage
 *    against its reference stage (crc32sum, mrlec, mrled, lzp_compress, lzp_decompress,
 *    libsais_bwt, libsais_unbwt, encode_bytes, decode_bytes);
 *  - per-stage timings of the last block a state processed;
 *  - the frame API (bz3_compress / bz3_decompress) on device memory.
 */
#ifndef BZ3_HIP_H
#define BZ3_HIP_H
#include <stddef.h>
#include <stdint.h>
#include "libbz3.h"
#define BZ3_HIP 1 /* this libbzip3 is the HIP implementation: the bz3_hip_* entry points exist */

#ifdef __cplusplus
extern "C" {
#endif

/* Number of usable HIP devices (0 when the runtime finds none). */
BZIP3_API int bz3_hip_device_count(void);
/* Pin every state created afterwards BY THIS PROCESS to `device` (>= 0), or restore round-robin (-1).
 * Returns 0, or -1 for an invalid device.  Environment BZ3_HIP_DEVICE=<n> has the same effect. */
BZIP3_API int bz3_hip_bind_device(int device);
/* Device a state is bound to. */
BZIP3_API int bz3_hip_state_device(struct bz3_state * state);

/* CM kernel variant (process-wide).  0 = the whole 145.5 KiB model in LDS, one block per CU; 1 / 2 = row-cache
 * kernels (the order-1 rows a block uses are cached in LDS -- 96 or 44/56 of them --, the others spill to HBM:
 * two / three blocks per CU; a block whose working set does not fit is handed back to variant 0 automatically);
 * -1 = automatic (default), by batch size: up to one block per CU variant 0, up to two per CU variant 1, beyond that variant 2.
 * Environment BZ3_HIP_CM_MODE=auto|full|rows|rows3 has the same effect.  Output bytes do not depend on the variant.
 * Returns 0, or -1 for an invalid mode. */
BZIP3_API int bz3_hip_set_cm_mode(int mode);
/* Test hook: how many more code windows the suffix sorter gives groups that are too large for its in-LDS kernels before rank doubling
 * takes them (0 = none: straight to the deep path; k < 0 = the default, 1).  Output bytes do not depend on it. */
BZIP3_API void bz3_hip_debug_bwt_big_rounds(int k);
/* Test hook of the inverse BWT: one splitter per 2^log_stride rows for every block (0..8; -1 = the rule, which sizes the splitter walk to the
 * lanes the device keeps resident).  Output bytes do not depend on it. */
BZIP3_API void bz3_hip_debug_set_unbwt_log_stride(int log_stride);
/* Number of blocks the row-cache kernels have handed back to the full-model kernels so far (statistics). */
BZIP3_API unsigned bz3_hip_cm_blocks_given_up(void);
/* Number of blocks sent STRAIGHT to the whole-model CM kernels so far (statistics): blocks of batches that take a row-cache variant (more blocks than
 * CUs) with many live byte values (encode) or a payload that hardly shrank (decode).  A batch of at most one block per CU is never split. */
BZIP3_API unsigned bz3_hip_cm_blocks_routed_full(void);

/* The CM kernel variant (0..8, 12 as above) a batch of `blocks` blocks on `device` is coded (encode != 0) or decoded with under the
 * current mode; -1 for an invalid device. */
BZIP3_API int bz3_hip_cm_variant_for(int device, int blocks, int encode);

/* Test hook: the largest number of per-GPU groups of one batch call that have been running at the same time since the
 * last reset (a batch whose states live on G GPUs runs G groups concurrently, one host thread per GPU). */
BZIP3_API int bz3_hip_debug_peak_concurrent_groups(int reset);

/* Test hook: shape of the ring the last bz3_encode_blocks / bz3_hip_encode_blocks_device group ran its front end through:
 * blocks per window | context slots << 16 | (workspace handed back when the call ended) << 30 (0 before the first call).  The serial LZP drivers of a window run on a side stream
 * while the whole-GPU stages of the other slots' windows run on the group's stream; the shape follows the free memory. */
BZIP3_API int bz3_hip_debug_front_end_ring(void);
/* Keep-workspace mode for lean states (same as BZ3_HIP_KEEP_WS=1 in the environment, but switchable: 1 on, 0 off, -1 back to the environment):
 * a GPU-filling lean batch's workspace survives the call, the decode call that follows reuses it and carves the swap buffers of its tail windows
 * from it -- instead of a hipFree and two multi-GB hipMallocs per round trip (30-45 ms per GiB).  The memory stays with the library until
 * bz3_hip_release_cached_memory(), within the headroom rule below.  bench.py turns it on for its timed steps. */
BZIP3_API int bz3_hip_set_keep_workspace(int on);
/* Two-thread front end of the encoder (round 6; 1 on, 0 off, -1 back to the environment: BZ3_HIP_FRONT_DUO, read once).  A batch of 16 blocks or more runs the first
 * half of every block's front end (CRC, mRLE, LZP preparation) on a second host thread and stream, up to ring-slots - 1 windows ahead of the second half (LZP emission,
 * suffix sort) on the calling thread: each half stops for read-backs the host needs, and the kernels of one fill the other's bubbles.  Costs a second scratch region
 * (~30 bytes per byte of the largest block).  Output bytes do not depend on it.  bz3_hip_debug_front_end_ring() reports bit 29 when the last call took this form. */
BZIP3_API int bz3_hip_set_front_end_duo(int on);
/* Headroom: the device memory the library leaves to the host program (the caller owns its memory; the library's workspace, its pool of swap buffers and --
 * with keep-workspace -- a GPU-filling batch's whole ring are caches).  Rule: when a batch call returns, at least `bytes` of the device are free
 * (hipMemGetInfo), or the library holds nothing cached on that device.  The rings are sized for it and the rule is enforced when a call ends (idle pooled swap
 * buffers go back to the driver first, the workspace second).  Default 4 GiB; environment BZ3_HIP_WS_HEADROOM_MB; bytes < 0 = back to the environment;
 * 0 = no rule (the library may keep whatever it grew to). */
BZIP3_API void bz3_hip_set_workspace_headroom(long long bytes);
BZIP3_API size_t bz3_hip_workspace_headroom(void);
/* Statistics: how often the rule had to be enforced since the last reset -- returns the pool trims, *releases receives the workspace releases. */
BZIP3_API unsigned bz3_hip_debug_headroom_events(int reset, unsigned * releases);
/* tests only: LZP contexts the encoder's front-end ring may hold (api_internal.hpp ring_contexts_for), the arena's slack beyond a request, and the bytes the
 * library holds cached on `device` right now (workspace + idle pooled swap buffers). */
BZIP3_API size_t bz3_hip_debug_ring_contexts(size_t free_bytes, size_t have, size_t need, size_t fixed, size_t ctx_bytes, size_t cap, int lean, size_t headroom);
BZIP3_API size_t bz3_hip_debug_arena_slack(size_t bytes);
BZIP3_API unsigned bz3_hip_debug_cm_launches(int reset); /* statistics: CM kernel launches of the batch paths since the last reset */
BZIP3_API size_t bz3_hip_debug_workspace_bytes(size_t block_bytes, int which); /* 0: per-block scratch of the stages, 1: one LZP context of the encoder's ring */
BZIP3_API size_t bz3_hip_debug_cached_bytes(int device);
/* Statistics of the keep-workspace experiment (environment BZ3_HIP_KEEP_WS=1: a lean batch's workspace survives the call and the decoder's tail carves
 * its swap buffers from it): swap buffers served from the arena instead of the pool since the last reset. */
BZIP3_API int bz3_hip_debug_arena_swap_buffers(int reset);

/* Lean states (process-wide switch, read by bz3_new; environment BZ3_HIP_LEAN=1 has the same effect).  A state
 * normally owns its swap buffer (the reference's swap_buffer, bz3_bound(block_size) bytes of HBM) for life, so a
 * batch of N blocks holds 2 N block-sized buffers.  A lean state owns none: it borrows one from a per-GPU pool only
 * while its block is in the whole-GPU stages, the CM encoder works in place in the caller's buffer (input at the end
 * of the bz3_bound(size) bytes the API guarantees, coded bytes growing from the start), and the CM decoder reads a
 * staged copy of the coded payload -- about 1.2 block-sized buffers per block in flight, which is what lets 3 x 256
 * blocks of 256 MiB share one MI355X.  Output bytes, return values and error codes are the same.  Returns 0. */
BZIP3_API int bz3_hip_set_lean_states(int on);
/* Frees the per-GPU workspace and the idle pooled swap buffers (they are otherwise kept for the next call). */
BZIP3_API void bz3_hip_release_cached_memory(void);

/* Device-resident variants: `buffer` / `buffers[i]` are device addresses on the state's GPU with the
 * same capacities the host API requires (bz3_bound(size) for encode; buffer_size for decode). */
BZIP3_API int32_t bz3_hip_encode_block_device(struct bz3_state * state, void * buffer, int32_t size);
BZIP3_API int32_t bz3_hip_decode_block_device(struct bz3_state * state, void * buffer, size_t buffer_size, int32_t compressed_size,
                                              int32_t orig_size);
BZIP3_API void bz3_hip_encode_blocks_device(struct bz3_state * states[], void * buffers[], int32_t sizes[], int32_t n);
BZIP3_API void bz3_hip_decode_blocks_device(struct bz3_state * states[], void * buffers[], size_t buffer_sizes[], int32_t sizes[],
                                            int32_t orig_sizes[], int32_t n);

/* Frames in device memory: bz3_compress / bz3_decompress (src/libbz3.c:876-997) with `in` and `out` in device memory of ONE GPU.
 * Same frame bytes, same return codes, same *out_size semantics (capacity on entry, bytes written on return; on a decode error: the bytes
 * of the chunks decoded before it).  Synchronous: the caller's writes to `in` must be complete before the call (synchronise your stream),
 * `out` is complete when it returns.  `in` is never written.  The GPU is the one that owns `in` (compress: `out`); both buffers must be
 * device memory of that GPU, else BZ3_ERR_INIT (an empty `in`, or an `out` of capacity 0 on decode, is not looked at).  The states of
 * the call live on that GPU whatever bz3_hip_bind_device says.  Blocks go through in windows of up to 256 per call (fewer where the
 * device's free memory beyond the headroom rule does not hold 256 slots and swap buffers); the headroom rule holds when the call returns. */
BZIP3_API int bz3_hip_compress_device(uint32_t block_size, const void * in, void * out, size_t in_size, size_t * out_size);
BZIP3_API int bz3_hip_decompress_device(const void * in, void * out, size_t in_size, size_t * out_size);
/* Walks the chunk headers of a frame in device memory with bz3_decompress's header checks (no decoding): *decoded_size = sum of the
 * original sizes of the well-formed chunks; returns BZ3_OK when all n_blocks chunks are present and well-formed, else the error
 * bz3_decompress would report first for the frame's headers (MALFORMED_HEADER / TRUNCATED_DATA; BZ3_ERR_INIT for a block size bz3_new
 * refuses or a pointer that is not device memory). */
BZIP3_API int bz3_hip_frame_decoded_size_device(const void * in, size_t in_size, size_t * decoded_size);
/* n independent frames on ONE GPU in one call: frame i gets exactly the bytes, return code and out_sizes[i] that
 * bz3_hip_compress_device(block_size, ins[i], outs[i], in_sizes[i], &out_sizes[i]) (bz3_hip_decompress_device(ins[i], outs[i],
 * in_sizes[i], &out_sizes[i])) would give it alone (out_sizes[i]: capacity on entry, bytes written on return; errors included: a short
 * output, a corrupt chunk after committed ones, header errors in the reference's order).  One frame's failure never changes another
 * frame's result, and a failing frame's later blocks go into no later window.  Blocks of all frames go through windows of up to 256
 * blocks in frame order, across frame boundaries, so one window's CM launch codes blocks of many frames; every block is checked
 * against its own frame's block size (compress: the :877 rule per frame; decode: each frame's header).  rcs[i] receives frame i's code;
 * returns BZ3_OK if all are BZ3_OK, else the code of the lowest-indexed failing frame.  n == 0 returns BZ3_OK and touches nothing.
 * Before any write, BZ3_ERR_INIT for the whole call, in every rcs[i] and with every out_sizes[i] = 0: n < 0; a NULL array with n > 0;
 * a non-empty buffer (ins[i] with in_sizes[i] > 0, outs[i] with out_sizes[i] > 0) that is not device memory of the GPU the first
 * non-empty buffer lives on (an empty buffer is not looked at).  Synchronous, with the headroom rule, as the single-frame calls. */
BZIP3_API int bz3_hip_compress_device_many(uint32_t block_size, int32_t n, const void * const ins[], const size_t in_sizes[],
                                           void * const outs[], size_t out_sizes[], int rcs[]);
BZIP3_API int bz3_hip_decompress_device_many(int32_t n, const void * const ins[], const size_t in_sizes[],
                                             void * const outs[], size_t out_sizes[], int rcs[]);
/* bz3_hip_frame_decoded_size_device for n frames, in one walk: decoded_sizes[i] and rcs[i] as the single call gives them; the return
 * code and the whole-call checks as bz3_hip_decompress_device_many (with no output buffers). */
BZIP3_API int bz3_hip_frame_decoded_sizes_device(int32_t n, const void * const ins[], const size_t in_sizes[],
                                                 size_t decoded_sizes[], int rcs[]);
/* Test hook: one launch of the segment copy kernel (frame.hpp k_copy_segments) on the device that owns `dst`: n (src_off, dst_off, len)
 * triples (host array of 3 n u64) relative to `src` / `dst`, non-overlapping on the destination side.  Returns 0, or BZ3_ERR_INIT. */
BZIP3_API int32_t bz3_hip_debug_copy_segments(const void * src, void * dst, const uint64_t * segs, int32_t n);

/* Byte-plane frames: the device frame calls above for typed data.  For a block of s bytes of elem_size-byte elements (k = elem_size,
 * m = s / k), split_k(b)[q m + e] = b[e k + q] for 0 <= q < k, 0 <= e < m, and split_k(b)[j] = b[j] for m k <= j < s (the tail of
 * s % k bytes stays in place); merge_k is its inverse, k = 1 the identity.  S(x) applies split_k to every block bz3_compress cuts x
 * into (src/libbz3.c:877-914: block j is x[j bs, (j + 1) bs), the last one in_size % bs bytes), never across blocks.  The compress
 * calls write exactly bz3_compress(block_size, S(x)): an ordinary .bz3 frame, which any bzip3 decodes to S(x).  The decompress
 * calls decode a frame and apply merge_k to every chunk, of the original size its chunk header gives (not the header's block size).
 * The element size is not stored in the frame: pass the one the frame was made with.  Everything else is the contract of the calls
 * without _planes, with S(x) in the place of x: return codes, *out_size, the bytes committed before an error (whole merged chunks),
 * the pointer checks, the independence of the frames of a _many call, windows, the headroom rule.  elem_size must be 1, 2, 4 or 8,
 * else BZ3_ERR_INIT for the whole call before any write (_many: in every rcs[i], every out_sizes[i] = 0); 1 gives the bytes of the
 * calls without _planes; a NULL elem_sizes in the _many calls is 1 for every frame.  The split and the merge happen in the launches that move a window's blocks into and out of their slots
 * (planes.hpp), so no pass over the data and no buffer of the size of the input is added. */
BZIP3_API int bz3_hip_compress_device_planes(uint32_t block_size, uint32_t elem_size, const void * in, void * out, size_t in_size,
                                             size_t * out_size);
BZIP3_API int bz3_hip_decompress_device_planes(uint32_t elem_size, const void * in, void * out, size_t in_size, size_t * out_size);
BZIP3_API int bz3_hip_compress_device_planes_many(uint32_t block_size, int32_t n, const uint32_t elem_sizes[], const void * const ins[],
                                                  const size_t in_sizes[], void * const outs[], size_t out_sizes[], int rcs[]);
BZIP3_API int bz3_hip_decompress_device_planes_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[],
                                                    const size_t in_sizes[], void * const outs[], size_t out_sizes[], int rcs[]);
/* Test hook: bz3_hip_debug_copy_segments with n (src_off, dst_off, len, elem_size | inverse << 8) quadruples (host array of 4 n u64):
 * a segment is copied (elem_size 1), split (inverse 0) or merged (inverse 1) in one launch.  Returns 0, or BZ3_ERR_INIT. */
BZIP3_API int32_t bz3_hip_debug_planes(const void * src, void * dst, const uint64_t * segs, int32_t n);

/* Delta frames: the byte-plane calls above for data of which an earlier version (the base) is in device memory of the same GPU.
 * D(x, b)[i] = (x[i] - b[i]) mod 256 for every byte i of x, b holding as many bytes as x; its inverse is (d[i] + b[i]) mod 256.  The
 * compress calls write exactly bz3_compress(block_size, S(D(in, base))), S as defined above for elem_size (1: the identity): an
 * ordinary .bz3 frame, which stores neither the element size nor anything about the base.  D is position-wise, so block j pairs with
 * the base bytes [j bs, j bs + len_j); what src/libbz3.c:914 drops stays dropped.  The decompress calls decode a frame, apply merge_k
 * to every chunk and add the base bytes at the chunk's output offsets.  Everything else is the contract of the _planes calls with
 * S(D(x, b)) in the place of S(x): return codes, *out_size, whole restored chunks committed before an error and nothing else of `out`
 * touched, the independence of the frames of a _many call, windows across frames, the headroom rule.
 *   base == NULL (bases == NULL, bases[i] == NULL): the frame has no base and the call is exactly its _planes call.
 *   compress: `base` holds in_size bytes; it is never written.
 *   decompress: `base` holds base_size bytes and the frame's capacity is min(*out_size, base_size): a chunk that would run past the
 *     base fails with BZ3_ERR_DATA_TOO_BIG, as one that runs past `out` does, after the chunks before it are committed.  `out` may be
 *     exactly `base` (the same address: the base is updated in place, and after an error the bytes beyond *out_size are still the
 *     base's) or must not overlap it.
 *   BZ3_ERR_INIT before any write (_many: for the whole call, in every rcs[i], every out_sizes[i] = 0): a non-empty base that is not
 *     device memory of the call's GPU; on decompress an `out` that overlaps its base without starting at the same address; on compress an
 *     `out` that overlaps the frame's base or its input.  Overlaps between different frames of a _many call are not looked for.
 * The difference is taken in the launches that move a window's blocks into and out of their slots (planes.hpp): one more read
 * stream, no pass over the data and no buffer of the size of the input is added.  Decoding against another base than the one the
 * frame was made with returns other bytes and no error: keep a checksum of the base (bz3_hip_crc32c_device) beside the frame. */
BZIP3_API int bz3_hip_compress_device_delta(uint32_t block_size, uint32_t elem_size, const void * in, const void * base, void * out,
                                            size_t in_size, size_t * out_size);
BZIP3_API int bz3_hip_decompress_device_delta(uint32_t elem_size, const void * in, const void * base, size_t base_size, void * out,
                                              size_t in_size, size_t * out_size);
BZIP3_API int bz3_hip_compress_device_delta_many(uint32_t block_size, int32_t n, const uint32_t elem_sizes[], const void * const ins[],
                                                 const void * const bases[], const size_t in_sizes[], void * const outs[],
                                                 size_t out_sizes[], int rcs[]);
BZIP3_API int bz3_hip_decompress_device_delta_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[],
                                                   const size_t in_sizes[], const void * const bases[], const size_t base_sizes[],
                                                   void * const outs[], size_t out_sizes[], int rcs[]);
/* The checksum of the block headers (crc32sum, src/libbz3.c: CRC-32C, state `init`, no inversion; the codec uses init = 1) over n bytes
 * of device memory at any alignment, computed on the GPU that owns them.  Returns BZ3_OK with the value in *crc (n == 0: init), or
 * BZ3_ERR_INIT for a pointer that is not device memory.  Synchronous. */
BZIP3_API int bz3_hip_crc32c_device(const void * p, size_t n, uint32_t init, uint32_t * crc);
/* The same checksum of n buffers in ONE pass: crcs[i] is exactly what bz3_hip_crc32c_device(ptrs[i], sizes[i], init_i, &c) returns, with
 * init_i = inits[i], or 1 (the codec's) for every buffer when inits == NULL.  The buffers may repeat, overlap and have any alignment; a
 * buffer of size 0 yields its init and its pointer, which may be NULL, is never looked at.  All non-empty buffers are device memory of ONE
 * GPU, that of the first non-empty one, and the call runs there.  No byte outside [ptrs[i], ptrs[i] + sizes[i]) of any buffer is read and
 * nothing is written to the buffers.  Per call: one upload of a table of n entries, at most two kernel launches and one read-back of n
 * words, whatever n is (the single call above is the n = 1 case).  Returns BZ3_OK (also for n == 0), or BZ3_ERR_INIT before anything is
 * written to crcs: n < 0; ptrs, sizes or crcs NULL with n > 0; a non-empty buffer that is not device memory of that GPU; more than 32 TiB
 * in one call.  Synchronous. */
BZIP3_API int bz3_hip_crc32c_device_many(int32_t n, const void * const * ptrs, const size_t * sizes, const uint32_t * inits, uint32_t * crcs);
BZIP3_API unsigned bz3_hip_debug_crc_launches(int reset); /* statistics: kernels launched by bz3_hip_crc32c_device[_many] since the last reset */
/* Test hook: bz3_hip_debug_planes with a base: n (src_off, base_off, dst_off, len, elem_size | inverse << 8) quintuples (host array of
 * 5 n u64) relative to `src` / `base` / `dst`; base_off = UINT64_MAX: the segment has no base.  A segment with a base stores
 * split_k(src - base) (inverse 0) or merge_k(src) + base (inverse 1), the base paired with the interleaved side.  `dst` may be `base`
 * with dst_off == base_off for inverse segments.  Returns 0, or BZ3_ERR_INIT. */
BZIP3_API int32_t bz3_hip_debug_delta(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n);

/* Range decode: the bytes [offset, offset + w) of what a frame decodes to, at the cost of the chunks that hold them.  For a frame f and
 * an element size k let X be what bz3_hip_decompress_device_planes(k, f, ...) writes with unlimited capacity: chunk j (of the frame
 * header's n_blocks) occupies [p_j, p_j + o_j) of X, o_j from its chunk header, p_j = o_0 + ... + o_{j-1}, T their sum.  w is *out_size
 * on entry, with a base min(*out_size, base_size); end = offset + w, saturating at 2^64 - 1.  The call is pread(2) on X:
 *   it writes out[i] = X[offset + i] for 0 <= i < r, r = max(0, min(T, end) - offset) -- with a base (X[offset + i] + base[i]) mod 256 --
 *   and returns BZ3_OK with *out_size = r.  A range that runs past the end of the frame is short, not an error: this is the ONE
 *   difference from the full call at offset 0, which reports BZ3_ERR_DATA_TOO_BIG where the range call clips; BZ3_ERR_DATA_TOO_BIG is
 *   never returned here.
 *   `base` holds the base's bytes OF THE RANGE: base[i] pairs with out[i].  `out` may be exactly `base` (updated in place) or must not
 *   overlap it; any other overlap is BZ3_ERR_INIT before any write, as in the _delta calls.  The overlap is judged on the w bytes the
 *   call can touch of each: out[0, w) and base[0, w), so a generous *out_size beside a small base is no overlap.
 *   The frame header is always checked, as in the full call (src/libbz3.c:930-960).  The header of chunk j is read and checked iff
 *   w > 0 and p_j < end, with the three header checks of bz3_decompress that do not concern capacity (:963-980), against the frame's
 *   block size; headers at or beyond `end` are never read and their errors are not reported.
 *   Chunk j is DECODED iff [p_j, p_j + o_j) and [offset, end) share a byte.  Chunks before the range are header-checked and skipped: a
 *   corrupt payload in them is not noticed.  Empty chunks are never decoded.  A decoded chunk is decoded whole: its CRC and every
 *   per-block check apply as in the full call, with its frame's block size.
 *   The result is the first event in chunk order, a header error or a failed chunk: its code is returned, the range bytes of the
 *   chunks before it are committed, *out_size is their count (a prefix of the range), nothing else of `out` is written.
 *   Nothing outside out[0, r) is ever written; `in` and a base that is not `out` are never written.
 * No index is stored: the chunk headers before the range are followed on the device by one lane (a few microseconds per chunk).
 * _many: n independent ranges of n frames (the same frame may appear more than once) on ONE GPU; offsets == NULL is offset 0 for every
 * frame, elem_sizes, bases and bases[i] may be NULL as in bz3_hip_decompress_device_delta_many, whose whole-call checks, return value,
 * rcs[], independence of frames, windows across frame boundaries and headroom rule hold here word for word.  The windows hold only the
 * chunks to be decoded: 256 frames that need one chunk each share one CM launch, and the states of a call are sized from the chunks
 * its first walk selects.  The single call is the n = 1 case. */
BZIP3_API int bz3_hip_decompress_device_range(uint32_t elem_size, const void * in, size_t in_size, uint64_t offset, const void * base,
                                              size_t base_size, void * out, size_t * out_size);
BZIP3_API int bz3_hip_decompress_device_range_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[],
                                                   const uint64_t offsets[], const void * const bases[], const size_t base_sizes[],
                                                   void * const outs[], size_t out_sizes[], int rcs[]);
/* Test hook: one launch of the gather of a range call: n (src_off, base_off, dst_off, len, elem_size | 1 << 8, a, b) septuples (host
 * array of 7 n u64) relative to `src` / `base` / `dst`.  Of merge_k(the len bytes at src_off) the bytes [a, b), a <= b <= len, are stored
 * at dst_off, plus the b - a bytes at base_off unless base_off is UINT64_MAX: base_off and dst_off address the clip's first byte.  `dst`
 * may be `base` with dst_off == base_off.  The inverse direction only; anything else is BZ3_ERR_INIT.  One launch takes mixed
 * elem_size.  Returns 0, or BZ3_ERR_INIT. */
BZIP3_API int32_t bz3_hip_debug_range(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n);

/* Strided range decode: a slice along any dimension of what a frame decodes to -- `count` runs of `run` bytes whose starts lie `stride`
 * bytes apart from `offset` on -- at the cost of the chunks that hold a byte of a run.  X, p_j, o_j and T are as in the range contract
 * above.  W = count * run; w = min(*out_size, W), with a base min(*out_size, base_size, W); for t < w
 *     phi(t) = offset + (t / run) * stride + t % run,
 * which is strictly increasing; end = phi(w - 1) + 1.  The call is pread(2) of the bytes phi(0), phi(1), ... of X:
 *   it writes out[t] = X[phi(t)] for t < r -- with a base (X[phi(t)] + base[t]) mod 256 --, r the number of t < w with phi(t) < T (a
 *   prefix, because phi increases), and returns BZ3_OK with *out_size = r.  BZ3_ERR_DATA_TOO_BIG is never returned.
 *   `base` holds the base's bytes OF THE SLICE, in output order: base[t] pairs with out[t].  `out` may be exactly `base`; any other
 *   overlap of out[0, w) and base[0, w) is BZ3_ERR_INIT before any write.
 *   Validity (a violation is BZ3_ERR_INIT for the whole call before any write, exactly as a bad elem_size is): stride >= run wherever
 *   count > 1 and run > 0; count * run must not overflow 64 bits; offset + (count - 1) * stride + run must not overflow 64 bits.  run == 0
 *   or count == 0 is allowed and means W = 0 (nothing else of such a period is looked at): the frame header alone is checked, as for
 *   w = 0 in the range call.
 *   The frame header is always checked.  The header of chunk j is read and checked iff w > 0 and p_j < end, with the three checks of
 *   the range call.  Chunk j is DECODED iff o_j > 0 and [p_j, p_j + o_j) holds phi(t) for some t < w; it is then decoded whole, with
 *   its CRC and every per-block check.  A chunk that lies before the first run, or IN A GAP BETWEEN TWO RUNS, is header-checked and
 *   skipped: a corrupt payload there is not noticed.
 *   The result is the first event in chunk order, a header error or a failed chunk: its code is returned, the output bytes t with
 *   phi(t) below that chunk's p_j are committed (a prefix), *out_size is their count, nothing else of `out` is written.
 *   Equivalence: a request with count == 1 or with stride == run is the contiguous range (offset, W): it returns byte for byte what
 *   bz3_hip_decompress_device_range returns for *out_size = min(*out_size, W), with the same return code and *out_size, through the
 *   same launches.
 * Within a decoded chunk the wanted bytes are gathered by one launch per window (planes.hpp k_strided_segments), a chunk being one
 * segment however many runs it holds.  Runs of 16 elements or more move 16 elements per lane; shorter ones byte by byte.
 * _many follows bz3_hip_decompress_device_range_many word for word: n independent frames on ONE GPU (the same frame may appear more than
 * once), NULL elem_sizes, bases and bases[i] as there, the same whole-call checks, rcs[], windows across frames and headroom rule.
 * params holds four u64 per frame: offset, run, stride, count; NULL params is BZ3_ERR_INIT.  The single call is the n = 1 case. */
BZIP3_API int bz3_hip_decompress_device_strided(uint32_t elem_size, const void * in, size_t in_size, uint64_t offset, uint64_t run,
                                                uint64_t stride, uint64_t count, const void * base, size_t base_size, void * out,
                                                size_t * out_size);
BZIP3_API int bz3_hip_decompress_device_strided_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[],
                                                     const uint64_t params[], const void * const bases[], const size_t base_sizes[],
                                                     void * const outs[], size_t out_sizes[], int rcs[]);
/* Test hook: one launch of the gather of a strided call: n tuples of 10 u64 (src_off, base_off, dst_off, len, elem_size | 1 << 8, c0,
 * first, run, stride, nbytes) relative to `src` / `base` / `dst`.  Of merge_k(the len bytes at src_off) the nbytes bytes c(0), c(1), ...
 * are stored at dst_off, plus the nbytes bytes at base_off unless base_off is UINT64_MAX: c(u) = c0 + u for u < first, else with
 * v = u - first, c(u) = c0 + first + (stride - run) + (v / run) * stride + v % run; 1 <= first <= run <= stride.  A tuple with
 * nbytes <= first is one contiguous piece and becomes the clipped or whole segment of bz3_hip_debug_range; stride == run is not
 * normalised away and reaches the strided kernel.  `dst` may be `base` with dst_off == base_off.  BZ3_ERR_INIT for a tuple whose last
 * chunk byte c(nbytes - 1) is not below len, for len >= 2^31 and for what bz3_hip_debug_range refuses.  Returns 0, or BZ3_ERR_INIT. */
BZIP3_API int32_t bz3_hip_debug_strided(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n);

/* Index decode: an arbitrary ascending set of rows, experts or columns of what a frame decodes to -- `count` periods whose starts lie
 * `stride` bytes apart from `offset` on, and of every period the same m pieces (s_j, l_j): piece j is the bytes [s_j, s_j + l_j) of its
 * period -- at the cost of the chunks that hold a byte of a piece.  `pieces` is a HOST array of 2 m u64: s_0, l_0, s_1, l_1, ...  X, p_j,
 * o_j and T are as in the range contract above (the j of p_j and o_j numbers chunks, the j of s_j, l_j and P_j pieces).
 * P_j = l_0 + ... + l_{j-1}, L = P_m; W = count * L; w = min(*out_size, W), with a base min(*out_size, base_size, W); for t < w
 *     phi(t) = offset + (t / L) * stride + s_j + (t % L - P_j),     j the piece with P_j <= t % L < P_{j+1},
 * which is strictly increasing (see Validity); end = phi(w - 1) + 1.  The call is pread(2) of the bytes phi(0), phi(1), ... of X:
 *   it writes out[t] = X[phi(t)] for t < r -- with a base (X[phi(t)] + base[t]) mod 256 --, r the number of t < w with phi(t) < T (a
 *   prefix, because phi increases), and returns BZ3_OK with *out_size = r.  BZ3_ERR_DATA_TOO_BIG is never returned.
 *   `base` holds the base's bytes OF THE INDEX SET, in output order: base[t] pairs with out[t].  `out` may be exactly `base`; any other
 *   overlap of out[0, w) and base[0, w) is BZ3_ERR_INIT before any write.
 *   Validity (a violation is BZ3_ERR_INIT for the whole call before any write, exactly as a bad elem_size is): s_j + l_j must not
 *   overflow 64 bits; s_j + l_j <= s_{j+1}: the pieces ascend and are disjoint (l_j = 0 is allowed); s_{m-1} + l_{m-1} <= stride
 *   wherever count > 1 and L > 0; count * L and offset + (count - 1) * stride + s_{m-1} + l_{m-1} must not overflow 64 bits; pieces == NULL
 *   with m > 0.  m == 0, L == 0 or count == 0 is allowed and means W = 0 (nothing else of such a request is looked at): the frame header
 *   alone is checked, as for w = 0 in the range call.
 *   The frame header is always checked.  The header of chunk j is read and checked iff w > 0 and p_j < end, with the three checks of
 *   the range call.  Chunk j is DECODED iff o_j > 0 and [p_j, p_j + o_j) holds phi(t) for some t < w; it is then decoded whole and ONCE,
 *   however many pieces and periods it holds, with its CRC and every per-block check.  A chunk that lies before the first piece, or IN
 *   ANY GAP -- between two pieces of a period, or between the last piece of one period and the first of the next -- is header-checked
 *   and skipped: a corrupt payload there is not noticed.
 *   The result is the first event in chunk order, a header error or a failed chunk: its code is returned, the output bytes t with
 *   phi(t) below that chunk's p_j are committed (a prefix), *out_size is their count, nothing else of `out` is written.
 *   Nothing outside out[0, r) is ever written; `in`, `pieces` and a base that is not `out` are never written.
 *   Normal form and equivalence: empty pieces are dropped; pieces with s_j + l_j == s_{j+1} are joined; w cuts count and the last
 *   period's pieces.  A request left with one piece is the strided request (offset + s_0, l_0, stride, count): it returns byte for byte
 *   what bz3_hip_decompress_device_strided returns for *out_size = min(*out_size, W), with the same return code and *out_size, through
 *   the same launches (and that call in turn takes the range call's for one run or stride == run).
 * A frame with two or more pieces walks with its piece table in device memory (16 bytes per piece, uploaded once per call beside the
 * walk's arguments; frame.hpp k_frame_walk_select: one division and one binary search per chunk header).  Within a decoded chunk the
 * wanted bytes are gathered by one launch per window (planes.hpp k_select_segments), a chunk being one segment however many pieces and
 * periods it holds.  Lanes whose 16 elements lie inside one piece move 16 elements at once; the others byte by byte.
 * _many follows bz3_hip_decompress_device_range_many word for word: n independent frames on ONE GPU (the same frame may appear more than
 * once), NULL elem_sizes, bases and bases[i] as there, the same whole-call checks, rcs[], independence of frames, windows across frames
 * and headroom rule.  params holds four u64 per frame: offset, stride, count, m; pieces[i] is frame i's host array of 2 m_i u64.  NULL
 * params, or NULL pieces or pieces[i] where m_i > 0, is BZ3_ERR_INIT.  The single call is the n = 1 case. */
BZIP3_API int bz3_hip_decompress_device_select(uint32_t elem_size, const void * in, size_t in_size, uint64_t offset, uint64_t stride,
                                               uint64_t count, uint64_t m, const uint64_t * pieces, const void * base, size_t base_size,
                                               void * out, size_t * out_size);
BZIP3_API int bz3_hip_decompress_device_select_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[],
                                                    const uint64_t params[], const uint64_t * const pieces[], const void * const bases[],
                                                    const size_t base_sizes[], void * const outs[], size_t out_sizes[], int rcs[]);
/* Test hook: one launch of the gather of a select call: n tuples of 12 u64 (src_off, base_off, dst_off, len, elem_size | 1 << 8, rel,
 * stride, q0, r0, nbytes, first_piece, m) relative to `src` / `base` / `dst`, and one host array `pieces` of 2 n_pieces u64 (s, l) of
 * which a tuple takes the m pieces from first_piece on.  Of merge_k(the len bytes at src_off) the nbytes bytes c(0), c(1), ... are
 * stored at dst_off, plus the nbytes bytes at base_off unless base_off is UINT64_MAX: with x = r0 + u,
 *     c(u) = rel + (q0 + x / L) * stride + s_j + (x % L - P_j),     j the piece with P_j <= x % L < P_{j+1},
 * rel a two's-complement u64 (the request's offset less the chunk's).  The pieces are NOT normalised: empty ones and neighbours that
 * touch stay in the table, so a uniform list reaches the select kernel.  A tuple whose nbytes lie within one piece is one contiguous
 * piece and becomes the clipped or whole segment of bz3_hip_debug_range.  `dst` may be `base` with dst_off == base_off.  BZ3_ERR_INIT for
 * what bz3_hip_debug_strided refuses of the first five fields, for a piece list that is invalid (above; and where the tuple's bytes
 * span two periods, s_{m-1} + l_{m-1} > stride), for r0 >= L, and for a tuple whose c(0) or c(nbytes - 1) lies outside [0, len).
 * Returns 0, or BZ3_ERR_INIT. */
BZIP3_API int32_t bz3_hip_debug_select(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n,
                                       const uint64_t * pieces, uint64_t n_pieces);

/* Range update: the write mirror of range decode.  The bytes [offset, offset + w) of what a frame decodes to are replaced, and of the frame only
 * the chunks that hold them are coded again.  f, k, X, p_j, o_j and T are as in the range-decode contract above, c_j is chunk j's coded size from
 * its chunk header.  Chunk j is TOUCHED iff w > 0 and [p_j, p_j + o_j) shares a byte with [offset, offset + w); a touched chunk is CUT if the
 * range does not hold all of [p_j, p_j + o_j), and COVERED otherwise.  Empty chunks (o_j == 0) are never touched.
 *   Result.  On BZ3_OK, out[0, *out_size) is a frame f' with f's 13 header bytes and f's number of chunks.  An untouched chunk is chunk j of f,
 *   copied verbatim (8 header bytes and c_j coded bytes): its payload is never decoded, and corruption in it is not noticed.  A touched chunk
 *   is exactly the chunk bz3_hip_compress_device_delta writes for a block of o_j bytes with the content X'[p_j, p_j + o_j), split with k and coded
 *   against the frame's block size; its chunk header carries the new coded size and o_j.  X' is X with the bytes [offset, offset + w) replaced by
 *   data[0, w) -- with a base by (data[i] - base[i]) mod 256.  `base` holds the base's bytes OF THE RANGE, as in the range-decode call: base[i]
 *   pairs with data[i]; NULL means none.  Consequence: if f == bz3_compress(bs, S(x)), then f' == bz3_compress(bs, S(x')) byte for byte.
 *   Order of work.  The frame header and EVERY chunk header are walked and checked first, with the checks of the whole-frame decode that do not
 *   concern capacity (the plain walk: a few microseconds per chunk, and all records are needed to place the copies); a malformed header BEHIND
 *   the range is therefore reported, which is where the update is stricter than range decode.  Then every cut chunk of the call is decoded
 *   whole, with its CRC and per-block checks as in the full call.  Only after both steps is anything written to `out`: on a header error, or
 *   a cut chunk that fails to decode, the call returns that code with *out_size = 0 and `out` untouched.  On an encode error afterwards (not
 *   expected) *out_size = 0 and out[0, cap) is unspecified.  `in`, `data` and `base` are never written; nothing outside out[0, cap) is ever
 *   written (cap: *out_size on entry).
 *   Range.  offset + w must not overflow and must be <= T, else BZ3_ERR_DATA_TOO_BIG before any write: an update never grows a tensor
 *   (bz3_hip_resize_device below appends and truncates).  w == 0
 *   gives a verbatim copy of the frame (its chunks, without anything that follows the last one in `in`); the headers are still checked.
 *   Capacity.  need = 13 + sum over j of (8 + (touched_j ? bz3_bound(o_j) : c_j)), known after the walk; cap < need is BZ3_ERR_DATA_TOO_BIG
 *   before any write.
 *   Overlap.  out[0, cap) must not overlap in[0, in_size), data[0, w) or base[0, w): BZ3_ERR_INIT before any write.
 * _many: n independent updates on ONE GPU; the same `in` may appear more than once; offsets, elem_sizes, bases and bases[i] may be NULL with their
 * usual meanings (0, 1, none).  Whole-call checks, return value, rcs[], independence of frames and the headroom rule are those of
 * bz3_hip_decompress_device_range_many; a frame that fails leaves out_sizes[i] = 0.  The touched chunks of all frames share windows in frame
 * order: 256 frames with one touched chunk each are one CM decode launch at most and one CM encode launch, and the states are sized from the
 * touched chunks, never from n_blocks.  A call whose touched chunks exceed one window decodes its cut chunks twice: once to check them before the
 * first write, once in the window that codes them.  The single call is the n = 1 case. */
BZIP3_API int bz3_hip_update_device_range(uint32_t elem_size, const void * in, size_t in_size, uint64_t offset, const void * data, size_t w,
                                          const void * base, void * out, size_t * out_size);
BZIP3_API int bz3_hip_update_device_range_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[],
                                               const uint64_t offsets[], const void * const datas[], const size_t ws[],
                                               const void * const bases[], void * const outs[], size_t out_sizes[], int rcs[]);
/* Test hook: one launch of the patch of an update call: n (src_off, base_off, dst_off, len, elem_size, a, b) septuples (host array of 7 n u64)
 * relative to `src` / `base` / `dst`, the layout of bz3_hip_debug_range in the forward direction.  The `len` bytes at dst_off are a slot that
 * holds split_k of a chunk; the chunk's bytes [a, b), a <= b <= len, get the values of the b - a bytes at src_off, less the b - a bytes at base_off
 * unless base_off is UINT64_MAX: src_off and base_off address the clip's first byte.  No other byte of the slot, and nothing of `src` or `base`,
 * is written.  One launch takes mixed elem_size.  Returns 0, or BZ3_ERR_INIT. */
BZIP3_API int32_t bz3_hip_debug_patch(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n);

/* Resize: append to or truncate what a frame decodes to, coding again only its tail.  f, k, X, p_j, o_j, c_j and T are as in the range-update
 * contract above.  X' = X[0, keep) ++ data[0, w) -- with a base the appended bytes are (data[i] - base[i]) mod 256; `base` holds the base's bytes OF
 * THE APPENDED RANGE, as in the range update, NULL means none -- and T' = keep + w.  keep == T is an append, w == 0 a truncation, both together the
 * verbatim copy.
 *   Effective block size (src/libbz3.c:877-878): eff(bs, t) = max(65 KiB, bs > t ? bz3_bound(t) : bs).  B = eff(block_size, T').
 *   Regular input.  f must be what bz3_compress(block_size, .) writes for T bytes: the header's block size equals eff(block_size, T), every chunk but
 *   the last has o_j equal to it, the last has 0 < o_j <= it, and n_blocks == 0 iff T == 0.  Anything else is BZ3_ERR_INIT before any write; in
 *   particular a frame that lost a block to the reference's in_size % block_size == 0 quirk (:914) is refused.
 *   Lossless output.  If T' >= B and T' % B == 0 the reference would drop a block: the call returns BZ3_ERR_INIT before any write and never writes a
 *   frame that loses bytes.  B > 511 MiB is BZ3_ERR_INIT, as in the compress call.
 *   Result.  On BZ3_OK, out[0, *out_size) is exactly bz3_compress(block_size, S_k(X')): 13 header bytes with B and ceil(T' / B), then the chunks of
 *   X' cut at multiples of B.  New chunk i is COPIED if the header block size of f equals B and old chunk i has the same extent and ends at or
 *   below keep: its 8 + c_i bytes are copied verbatim, its payload is never decoded, and corruption in it is not noticed.  Every other new chunk is
 *   REBUILT.  At most one rebuilt chunk per frame holds kept bytes, the one that holds X'[keep - 1]; only for it is an old chunk decoded, the single
 *   old chunk that holds those bytes, whole and once, with the CRC and per-block checks of the full decode.  The other rebuilt chunks are built
 *   from `data` alone.  A changed effective block size (a one-block frame of T < block_size that grows, a frame cut back below block_size) leaves
 *   nothing to copy: that is the rule above at work, not a path of its own.
 *   Order of work, failure and overlap follow the range update's.  All headers are walked and checked first; then the cut chunks of the whole call
 *   are decoded; only then is anything written to any `out`.  A frame that fails in either step has its code, *out_size = 0 and an untouched `out`.
 *   keep > T is BZ3_ERR_DATA_TOO_BIG.  need = 13 + sum over the new chunks of (8 + (copied ? c_i : bz3_bound(o'_i))), and cap < need (cap: *out_size
 *   on entry) is BZ3_ERR_DATA_TOO_BIG before any write.  out[0, cap) must not overlap in[0, in_size), data[0, w) or base[0, w), else BZ3_ERR_INIT.
 *   Nothing outside out[0, cap) is written; `in`, `data` and `base` are never written.
 * _many: the whole-call checks, rcs[], the independence of frames and the headroom rule are those of bz3_hip_update_device_range_many; block_sizes
 * and keeps are required, elem_sizes, bases and bases[i] may be NULL (1, none).  The rebuilt chunks of all frames share windows in frame order and
 * the states are sized from that list: 256 frames that each append into their last chunk are at most one CM decode launch and one CM encode launch.
 * A call whose rebuilt chunks exceed one window decodes its cut chunks twice, as the range update does.  The kept head of a cut chunk moves from the
 * byte planes of its old length to those of its new one on the device (planes.hpp, "Replane"), from the slot it was decoded into to the slot it is
 * coded from: one more slot per cut chunk with k > 1.  The single call is the n = 1 case. */
BZIP3_API int bz3_hip_resize_device(uint32_t block_size, uint32_t elem_size, const void * in, size_t in_size, uint64_t keep, const void * data, size_t w,
                                    const void * base, void * out, size_t * out_size);
BZIP3_API int bz3_hip_resize_device_many(int32_t n, const uint32_t block_sizes[], const uint32_t elem_sizes[], const void * const ins[],
                                         const size_t in_sizes[], const uint64_t keeps[], const void * const datas[], const size_t ws[],
                                         const void * const bases[], void * const outs[], size_t out_sizes[], int rcs[]);
/* Test hook: one launch of the replane of a resize call: n (src_off, dst_off, len_old, len_new, elem_size, a) sextuples (host array of 6 n u64)
 * relative to `src` / `dst`.  The len_old bytes at src_off are a slot that holds split_k of a chunk; the chunk's bytes [0, a), a <= min(len_old,
 * len_new), are stored where a slot of len_new bytes at dst_off keeps them: chunk byte c lives at slot[(c % k) * (len / k) + c / k] below
 * (len / k) * k and at slot[c] in the tail.  No other byte of `dst`, and nothing of `src`, is written.  One launch takes mixed elem_size.  Returns 0,
 * or BZ3_ERR_INIT. */
BZIP3_API int32_t bz3_hip_debug_replane(const void * src, void * dst, const uint64_t * segs, int32_t n);

/* Index update: the write mirror of index decode.  Chosen rows, columns or experts of what a frame decodes to are replaced in one call, and of the
 * frame only the chunks that hold them are coded again.  phi, L, W = count * L, P_j, `pieces` (a HOST array of 2 m u64) and the piece index j are
 * exactly those of the index-decode contract above; X, p_j, o_j, c_j and T those of the range-update contract.  A strided update (a slice along an
 * inner dimension) is the m == 1 case.
 *   Result.  X' is X with X'[phi(t)] = data[t] for every t < W -- with a base, X'[phi(t)] = (data[t] - base[t]) mod 256.  `base` holds the base's
 *   bytes OF THE INDEX SET in output order, as in index decode: base[t] pairs with data[t]; NULL means none.  On BZ3_OK, out[0, *out_size) is a
 *   frame f' with f's 13 header bytes and f's number of chunks.  An untouched chunk is copied verbatim and never decoded.  A touched chunk is
 *   exactly what bz3_hip_compress_device_delta writes for a block with the content X'[p_j, p_j + o_j), as in the range update.  Consequence: if
 *   f == bz3_compress(bs, S(x)), then f' == bz3_compress(bs, S(x')) byte for byte.
 *   Touched, cut and covered chunks.  Chunk j is TOUCHED iff o_j > 0 and [p_j, p_j + o_j) holds phi(t) for some t < W.  It is COVERED iff every
 *   one of its o_j bytes is such a phi(t): a covered chunk is rebuilt from `data` alone, and its old payload is not looked at.  Otherwise it is
 *   CUT.  A cut chunk is decoded first, whole and ONCE, however many pieces and periods it holds.  A frame may have any number of cut chunks: a
 *   column update cuts all of them.
 *   Validity (a violation is BZ3_ERR_INIT for the whole call before any write).  Every validity rule of bz3_hip_decompress_device_select[_many]
 *   applies to offset, stride, count, m and pieces.  w != W is invalid: an update names all its bytes.  The bad-elem_size, pointer and device checks
 *   are those of the range update.  out[0, cap) must not overlap in[0, in_size), data[0, W) or base[0, W) (cap: *out_size on entry).
 *   Range and capacity.  If W > 0 and phi(W - 1) + 1 > T, the call returns BZ3_ERR_DATA_TOO_BIG before any write: an update never grows a tensor
 *   (bz3_hip_resize_device does).
 *   W == 0 (m == 0, L == 0 or count == 0; nothing else of such a request is looked at) gives the verbatim copy of the frame, with the headers
 *   still checked.  need = 13 + sum over j of (8 + (touched_j ? bz3_bound(o_j) : c_j)), and cap < need is BZ3_ERR_DATA_TOO_BIG before any write: the
 *   range update's formula, unchanged.
 *   Order of work and failure are the range update's: the frame header and EVERY chunk header are walked and checked first (the plain walk); then
 *   every cut chunk of the call is decoded; only then is anything written to `out`.  A frame that fails in either step has its code,
 *   *out_size = 0 and an untouched `out`; on an encode error afterwards (not expected) *out_size = 0 and out[0, cap) is unspecified.  `in`, `data`,
 *   `base` and `pieces` are never written; nothing outside out[0, cap) is ever written.
 *   Normal form and equivalence.  The request is normalised as index decode normalises: empty pieces are dropped and pieces with
 *   s_j + l_j == s_{j+1} are joined.  A request left in range form -- one piece with count == 1 or stride == L -- returns byte for byte what
 *   bz3_hip_update_device_range returns for (offset + s_0, data, W), with the same return code and *out_size, through the same launches.
 * Every other request patches its chunks with its piece table in device memory (16 bytes per piece, uploaded once per call beside the walk's
 * arguments).  Within a touched chunk the new bytes are one contiguous piece of `data`, scattered into the chunk's byte planes by one launch per
 * window (planes.hpp k_patch_select_segments), a chunk being one segment however many pieces and periods it holds.  Lanes whose 16 elements are
 * whole elements of the chunk inside one piece move 16 elements at once; the others byte by byte: pieces shorter than 16 elements are correct
 * and slow.
 * _many: the whole-call checks, rcs[] and the independence of frames follow bz3_hip_update_device_range_many; params holds four u64 per frame:
 * offset, stride, count, m; pieces[i] is frame i's host array of 2 m_i u64; ws[i] must be W_i.  NULL params, or NULL pieces or pieces[i] where
 * m_i > 0, is BZ3_ERR_INIT.  The touched chunks of all frames share windows in frame order, and the states are sized from the touched list, never
 * from n_blocks.  A call whose touched chunks exceed one window decodes its cut chunks twice, as the range update does: once to check them before
 * the first write, once in the window that codes them.  (Parking the decoded chunks instead is open.)  The single call is the n = 1 case. */
BZIP3_API int bz3_hip_update_device_select(uint32_t elem_size, const void * in, size_t in_size, uint64_t offset, uint64_t stride, uint64_t count,
                                           uint64_t m, const uint64_t * pieces, const void * data, size_t w, const void * base, void * out,
                                           size_t * out_size);
BZIP3_API int bz3_hip_update_device_select_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[],
                                                const uint64_t params[], const uint64_t * const pieces[], const void * const datas[],
                                                const size_t ws[], const void * const bases[], void * const outs[], size_t out_sizes[], int rcs[]);
/* Test hook: bz3_hip_debug_select in the forward direction, one launch of the patch of an index update: n tuples of 12 u64 (src_off, base_off,
 * dst_off, len, elem_size, rel, stride, q0, r0, nbytes, first_piece, m) relative to `src` / `base` / `dst`, and one host array `pieces` of
 * 2 n_pieces u64 (s, l) of which a tuple takes the m pieces from first_piece on.  The `len` bytes at dst_off are a slot that holds split_k of a
 * chunk; for u < nbytes the chunk's byte c(u) -- the formula of bz3_hip_debug_select -- gets the value of byte u at src_off, less byte u at
 * base_off unless base_off is UINT64_MAX.  Chunk byte c lives at slot[(c % k) * (len / k) + c / k] below (len / k) * k and at slot[c] in the tail.
 * No other byte of the slot, and nothing of `src` or `base`, is written.  The pieces are NOT normalised, so a uniform list reaches the select
 * split; a tuple whose bytes lie within one piece becomes the clipped or whole segment of bz3_hip_debug_patch.  BZ3_ERR_INIT for what
 * bz3_hip_debug_select refuses, and for any bit above the element size in the fifth field (the inverse bit among them).  Returns 0, or
 * BZ3_ERR_INIT. */
BZIP3_API int32_t bz3_hip_debug_patch_select(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n,
                                             const uint64_t * pieces, uint64_t n_pieces);

/* Sync: repack a tensor against its previous version when nobody knows where it changed.  `in` is a frame f, `old` the `size` bytes f decodes
 * to (with a base: f decodes to (old[i] - base[i]) mod 256, split with k), `data` the `size` bytes of the new version.  The call finds the chunks
 * whose bytes changed by comparing `data` with `old` on the device and codes only those again.  f, k, X, p_j, o_j, c_j and T are those of the
 * range-update contract above.
 *   Dirty.  Chunk j is DIRTY iff o_j > 0 and data[p_j, p_j + o_j) != old[p_j, p_j + o_j) byte-wise (an exact comparison, not a checksum), and
 *   CLEAN otherwise.
 *   Result.  On BZ3_OK, out[0, *out_size) is a frame f' with f's 13 header bytes and f's number of chunks.  A clean chunk is chunk j of f, copied
 *   verbatim (8 header bytes and c_j coded bytes): it is never decoded, and corruption in it is not noticed.  A dirty chunk is exactly the chunk
 *   bz3_hip_compress_device_delta writes for a block with the content data[p_j, p_j + o_j) -- with a base, less base[p_j, p_j + o_j): `base` holds
 *   `size` bytes, THE WHOLE BASE, and pairs with `data` at equal offsets; NULL means none --, split with k and coded against the frame's block size.
 *   NO chunk is ever decoded by this call, and the old payload of a dirty chunk is not read.  Consequence: if `old` is what f decodes to and
 *   f == bz3_compress(bs, S_k(D(old, base))), then f' == bz3_compress(bs, S_k(D(data, base))) byte for byte.  The caller vouches that `old` is what
 *   f decodes to; the call cannot tell, as it cannot tell a wrong base.
 *   Count.  *recoded (recoded may be NULL) is the number of dirty chunks on BZ3_OK, and 0 for a frame that fails before a write.
 *   Order of work.  The frame header and EVERY chunk header are walked and checked first with the plain walk, as in the range update: a malformed
 *   header anywhere is reported.  The comparison runs beside the walk; then size and capacity are judged; only then is anything written.  A frame
 *   that fails has its code, *out_size = 0 and an untouched `out`; on an encode error afterwards (not expected) *out_size = 0 and out[0, cap) is
 *   unspecified.  `in`, `data`, `old` and `base` are never written; nothing outside out[0, cap) is ever written (cap: *out_size on entry).
 *   Size.  size != T is BZ3_ERR_DATA_TOO_BIG before any write (bz3_hip_resize_device is the call that changes a size).  old == NULL or
 *   data == NULL with size > 0 is BZ3_ERR_INIT.  data == old is legal and gives the verbatim copy of the frame.
 *   Capacity.  need = 13 + sum over j of (8 + (dirty_j ? bz3_bound(o_j) : c_j)); cap < need is BZ3_ERR_DATA_TOO_BIG before any write.
 *   Overlap.  out[0, cap) must not overlap in[0, in_size), data[0, size), old[0, size) or base[0, size): BZ3_ERR_INIT before any write.  `data` and
 *   `old` may overlap each other.
 * _many: n independent syncs on ONE GPU; the whole-call checks, return value, rcs[], the independence of frames and the headroom rule are those of
 * bz3_hip_update_device_range_many; datas, olds and sizes are required, elem_sizes, bases, bases[i] and recoded may be NULL (1, none, not wanted).
 * The dirty chunks of all frames share windows in frame order, and the states are sized from the dirty list (min(dirty, 256)), never from
 * n_blocks: a call without a dirty chunk creates no state and launches no CM kernel.  The comparison is one launch (planes.hpp k_diff_segments)
 * and one read-back of the flags per walk round of 4096 chunk records.  The single call is the n = 1 case. */
BZIP3_API int bz3_hip_sync_device(uint32_t elem_size, const void * in, size_t in_size, const void * data, const void * old, size_t size,
                                  const void * base, void * out, size_t * out_size, uint32_t * recoded);
BZIP3_API int bz3_hip_sync_device_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[],
                                       const void * const datas[], const void * const olds[], const size_t sizes[], const void * const bases[],
                                       void * const outs[], size_t out_sizes[], uint32_t recoded[], int rcs[]);
/* Test hook: one launch of the comparison of a sync call: n (a_off, b_off, len) triples relative to `a` / `b` (host array of 3 n u64);
 * flags: host array of n u32, flags[i] = 1 iff the two runs differ, else 0 (len == 0: 0).  Both sides are read as aligned 16-byte granules, and no
 * granule is read that holds no byte of a run.  Nothing is written to `a` or `b`.  Returns 0, or BZ3_ERR_INIT. */
BZIP3_API int32_t bz3_hip_debug_diff(const void * a, const void * b, const uint64_t * segs, int32_t n, uint32_t * flags);

/* Stage timings (milliseconds) of the last block processed by `state`.  Timing a stage means waiting for the stream, so since round 4 only
 * the FIRST state of a batch (per GPU) is timed: its CRC / RLE / BWT entries are stage times, its LZP entry includes the window's driver
 * launch; for every other state of the batch CRC / BWT read 0 and RLE / LZP are launch (enqueue) times, not kernel times.  CM is the batch's
 * launch on every state. */
enum {
    BZ3_HIP_T_CRC = 0,
    BZ3_HIP_T_RLE = 1,
    BZ3_HIP_T_LZP = 2,
    BZ3_HIP_T_BWT = 3,  /* decode: the inverse BWTs of a window run up to four blocks at a time; a block's value is its run's wall time / the run's blocks */
    BZ3_HIP_T_CM = 4,   /* CM kernel alone, measured with HIP events on the state's stream */
    BZ3_HIP_T_COPY = 5, /* host<->device and device<->device block copies */
    BZ3_HIP_T_COUNT = 8
};
BZIP3_API void bz3_hip_last_timings(struct bz3_state * state, float ms[BZ3_HIP_T_COUNT]);
/* BWT statistics of the last encoded block: doubling rounds, radix passes, elements pushed through the sorter. */
BZIP3_API void bz3_hip_last_bwt_stats(struct bz3_state * state, int32_t * rounds, int32_t * radix_passes, uint64_t * sorted_elements);

/* Single-block calls (bz3_encode_block / bz3_decode_block) that arrive from several host threads within this window are collected into
 * ONE batch per direction (the reference's own batch API is N threads with one block each, src/libbz3.c:831-856; here a batch is one
 * CM launch instead of N).  Default 200 us; 0 = no waiting (callers that arrive while a batch runs still form the next batch). */
BZIP3_API void bz3_hip_set_collect_window_us(int us);
BZIP3_API unsigned bz3_hip_debug_collected_batches(int reset, unsigned * largest); /* statistics: batches run for single-block callers */

/* ---- per-stage hooks on HOST buffers (tests / profiling).  Return values mirror the reference stage. */
BZIP3_API uint32_t bz3_hip_stage_crc32c(const uint8_t * data, size_t n, uint32_t init);             /* crc32sum        */
BZIP3_API int32_t bz3_hip_stage_mrle_encode(const uint8_t * in, int32_t n, uint8_t * out);          /* mrlec           */
BZIP3_API int bz3_hip_stage_mrle_decode(const uint8_t * in, uint8_t * out, int32_t outlen, int32_t maxin); /* mrled    */
BZIP3_API int32_t bz3_hip_stage_lzp_encode(const uint8_t * in, int32_t n, uint8_t * out);           /* lzp_compress    */
BZIP3_API int32_t bz3_hip_stage_lzp_decode(const uint8_t * in, int32_t n, uint8_t * out, int32_t max); /* lzp_decompress */
/* tests only: bz3_hip_stage_lzp_encode, and in stats what the encoder's serial driver did: [0] the position it stopped at (>= n - 72), [1] matches taken,
 * [2] loop iterations, [3] flagged positions resolved (all zero where n < 72), then its constants: [4] events resolved per iteration, [5] positions per
 * bitmap window.  Output bytes are those of the stage hook. */
BZIP3_API int32_t bz3_hip_debug_lzp_encode(const uint8_t * in, int32_t n, uint8_t * out, uint32_t stats[6]);
BZIP3_API int32_t bz3_hip_stage_bwt(const uint8_t * in, uint8_t * out, int32_t n);                  /* libsais_bwt     */
BZIP3_API int32_t bz3_hip_stage_unbwt(const uint8_t * in, uint8_t * out, int32_t n, int32_t idx);   /* libsais_unbwt   */
/* tests only: the two CU masks of the decoder's partition (side streams / everything else) for `cus` CUs of which `reserve` are set aside; returns the words per mask */
BZIP3_API int32_t bz3_hip_debug_cu_masks(int cus, int reserve, uint32_t * side, uint32_t * rest);
/* tests only: sort.hip's device-wide exclusive prefix sum, in place on a host buffer */
BZIP3_API int32_t bz3_hip_debug_scan_u32(uint32_t * data, uint32_t n, uint32_t * total);
/* tests only: sort.hip's stable LSD radix sort of (keys[i], i) over key bits [0, key_bits), digits of 8 or 9 bits; returns the passes run */
BZIP3_API int32_t bz3_hip_debug_sort_u32(const uint32_t * keys, uint32_t n, int key_bits, int digit_bits, uint32_t * sorted_keys, uint32_t * sorted_index);
/* Tests and sweeps only: the inverse BWT of `count` blocks on host buffers in one call, through the batched pass of the decoder's tail in runs of
 * at most four blocks, in the order given (blocks of fewer than 2 bytes are handled apart).  Synchronous.  0, or -1 if a block's (n, idx) is one
 * libsais_unbwt refuses.  bz3_hip_stage_last_ms() then covers all runs of the call. */
BZIP3_API int32_t bz3_hip_debug_unbwt_many(const uint8_t * const * in, uint8_t * const * out, const int32_t * n, const int32_t * idx, int32_t count);
/* Tests and sweeps only: the forward BWT of `count` blocks on host buffers in one call, through the batched sorter of the encoder's front end in
 * runs of at most eight blocks, in the order given (blocks of fewer than 2 bytes are handled apart).  Synchronous.  idx_out[k] receives block k's
 * primary index.  0, or -1 on bad arguments.  bz3_hip_stage_last_ms() then covers all runs of the call. */
BZIP3_API int32_t bz3_hip_debug_bwt_many(const uint8_t * const * in, uint8_t * const * out, const int32_t * n, int32_t * idx_out, int32_t count);
/* Tests only: bz3_hip_stage_bwt of one block plus a record of what the suffix sorter did with it: its code table, the counter words of every pass of
 * the resolve loop, whether and from which depth it went to rank doubling, (depth, active suffixes) per doubling round, the statistics, and the
 * geometry constants of bwt.hip a test needs (layout: bwt.hip bwt_record_flatten; Python: bzip3_amd.StageApi.bwt_record).  rec receives rec[0] words
 * (rec_words must be at least that many: -2 otherwise, with the size in rec[0]).  *idx_out receives the primary index.  _record_many: the same for the
 * blocks of one bz3_hip_debug_bwt_many call, rec_words words apart.  0, -1 on bad arguments. */
BZIP3_API int32_t bz3_hip_debug_bwt_record(const uint8_t * in, int32_t n, uint8_t * out, int32_t * idx_out, uint32_t * rec, uint32_t rec_words);
BZIP3_API int32_t bz3_hip_debug_bwt_record_many(const uint8_t * const * in, uint8_t * const * out, const int32_t * n, int32_t * idx_out, int32_t count, uint32_t * rec, uint32_t rec_words);
/* Tests and sweeps only: blocks per run of the batched forward BWT (1..8 where memory allows); -1 = the rule (bwt_batch_size). */
BZIP3_API void bz3_hip_debug_set_bwt_batch(int b);
BZIP3_API float bz3_hip_stage_last_ms(void); /* wall ms of the transform inside the last bz3_hip_stage_bwt / _unbwt call (allocations and PCIe copies excluded) */
BZIP3_API int32_t bz3_hip_stage_cm_encode(const uint8_t * in, int32_t n, uint8_t * out);            /* encode_bytes    */
BZIP3_API void bz3_hip_stage_cm_decode(const uint8_t * in, int32_t in_size, uint8_t * out, int32_t n); /* decode_bytes  */

/* Streaming file codec (the reference CLI's driver loop, src/main.c:351-407, as a pipeline): reads blocks
 * from in_fd, codes `blocks_per_batch` of them at a time on the GPU(s) while the next batch is being read and the previous
 * one written, writes the reference's file format to out_fd ("BZ3v1", u32le block size, then per block u32le coded size,
 * u32le original size, block bytes -- byte-identical to `bzip3 -e -b`, decodable by `bzip3 -d`, and vice versa).
 * Returns 0, or a BZ3_ERR_* code (of the first failing block; the blocks before it have been written), or BZ3_HIP_ERR_IO.
 * Host buffers: page-locked up to BZ3_HIP_STREAM_PINNED_MIB MiB in total (environment, read once per process; default 4096 = 4 GiB), plain
 * malloc'ed buffers beyond that or when the host refuses -- larger configurations (blocks_per_batch x block size x 3 buffers above the
 * budget) therefore mix pinned and pageable buffers and copy the pageable ones through the runtime's staging at roughly half the rate;
 * raise the variable where the host has the lockable memory. */
#define BZ3_HIP_ERR_IO (-100)
BZIP3_API int bz3_hip_encode_stream(int in_fd, int out_fd, int32_t block_size, int32_t blocks_per_batch);
BZIP3_API int bz3_hip_decode_stream(int in_fd, int out_fd, int32_t blocks_per_batch);

/* Profiling: `copies` identical CM decode jobs in one launch through the current CM kernel variant; returns the launch
 * time in milliseconds, `out` receives the n (>= 256) decoded bytes of copy 0; with BZ3_CM_DEBUG=3 `counters` (u64[16] per
 * copy, may be NULL) receives the decoder's phase cycle counters instead of valid output (bzip3_amd/csrc/api_hooks.hip). */
BZIP3_API float bz3_hip_stage_cm_decode_many(const uint8_t * in, int32_t in_size, uint8_t * out, int32_t n, int32_t copies, uint64_t * counters);

/* The same for the encoder: `copies` identical CM encode jobs in one launch; *coded = coded size of copy 0, its bytes in `out`
 * (capacity bz3_bound(n)).  BZ3_CM_DEBUG=1 / 2: coder wave / model waves alone (output invalid). */
BZIP3_API float bz3_hip_stage_cm_encode_many(const uint8_t * in, int32_t n, uint8_t * out, int32_t * coded, int32_t copies);

#ifdef __cplusplus
}
#endif
#endif
