// frame_check.hpp -- the chunk-header rules of a frame, for the host loop (bz3_decompress, api.hip) and the device walk (frame.hpp).
#pragma once
#include "../../include/libbz3.h"
#include "hipx.hpp"

namespace bz3 {

// The four checks of one chunk header in bz3_decompress (src/libbz3.c:963-985), in the reference's order.  `p` points at
// the chunk header, `in_left` bytes of the frame remain from there, `planned` bytes of output precede the chunk.
// Shared by the host loop (bz3_decompress) and the device walk (k_frame_walk_many), so the rules exist once.
__host__ __device__ inline int frame_chunk_check(const u8 * p, size_t in_left, u32 block_size, size_t buf_max, size_t planned,
                                                 s32 * size, s32 * orig_size) {
    if (in_left < 8) return BZ3_ERR_MALFORMED_HEADER;  // :963
    const s32 sz = (s32)((u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24));
    if (sz < 0 || (u32)sz > block_size) return BZ3_ERR_MALFORMED_HEADER;  // :969
    if (in_left < (size_t)sz + 8) return BZ3_ERR_TRUNCATED_DATA;         // :974
    const s32 orig = (s32)((u32)p[4] | ((u32)p[5] << 8) | ((u32)p[6] << 16) | ((u32)p[7] << 24));
    if (orig < 0) return BZ3_ERR_MALFORMED_HEADER;                        // :980
    if (buf_max < planned + (size_t)orig) return BZ3_ERR_DATA_TOO_BIG;   // :985
    *size = sz;
    *orig_size = orig;
    return BZ3_OK;
}

}  // namespace bz3
