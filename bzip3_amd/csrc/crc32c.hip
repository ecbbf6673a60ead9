// crc32c.hip -- CRC-32C (reflected 0x82F63B78), arbitrary start state, no final xor, on gfx950.
// Replaces crc32sum + crc32Table (reference src/libbz3.c:37-72; called with state 1 at :593/:686/:803).
//
// The reference walks one table lookup per byte, serially.  Here the register update is treated as
// GF(2) polynomial algebra:   U(s, A) = s * x^(8|A|) + A(x) * x^32   (mod P),
// so a block splits into independent 16 KiB segments.  One wave owns one segment: lane l reads the
// l-th 32-bit word of each 256-byte row (fully coalesced), folds rows with Horner's rule
// (acc = acc * x^2048 + word), is aligned to the segment end by a per-lane constant x^(32(63-l)),
// xor-reduced across the wave, shifted to the end of the message by x^e (e assembled from a table of
// x^(2^b) with a 6-step cross-lane multiply-reduce) and xor-ed into one accumulator word.
// No lookup tables in LDS, no serial dependency across lanes.  Traffic: 1 byte read per input byte.
#include <algorithm>

#include "prims.hpp"
#include "stages.hpp"

namespace bz3 {

constexpr u32 CRC_POLY = 0x82F63B78u;
constexpr u32 CRC_ONE = 0x80000000u;  // the polynomial "1" in reflected bit order
constexpr int CRC_SEG_WORDS = 4096;   // 16 KiB per wave
constexpr int CRC_ROWS = CRC_SEG_WORDS / WAVE;

__host__ __device__ inline u32 gf_mul(u32 a, u32 b) {  // a(x) * b(x) mod P, reflected representation
    u32 p = 0;
#pragma unroll
    for (int i = 31; i >= 0; i--) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}

void crc_build_tables(CrcTables & t) {
    u32 x1 = CRC_ONE >> 1;  // x^1
    t.pow2[0] = x1;
    for (int b = 1; b < 64; b++) t.pow2[b] = gf_mul(t.pow2[b - 1], t.pow2[b - 1]);
    u32 x32 = t.pow2[5];
    u32 acc = CRC_ONE;
    for (int l = 63; l >= 0; l--) {
        t.lane[l] = acc;
        acc = gf_mul(acc, x32);
    }
    t.row = t.pow2[11];  // 2^11 = 2048 bits = one 64-word row
}

// x^e for a wave-uniform exponent e (in bits); all lanes return the result.
__device__ __forceinline__ u32 gf_xpow(u64 e, const u32 * __restrict__ pow2) {
    u32 f = ((e >> lane_id()) & 1ull) ? pow2[lane_id()] : CRC_ONE;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) f = gf_mul(f, __shfl_xor(f, d));
    return f;
}

// One wave folds `rows` full 64-word rows starting at word `w0`; result is the polynomial of those
// rows (no x^32 factor), valid in every lane.
__device__ __forceinline__ u32 crc_fold_rows(const u32 * __restrict__ words, u64 w0, int rows, const CrcTables * __restrict__ t) {
    u32 acc = 0;
    const u32 xrow = t->row;
    for (int r = 0; r < rows; r++) acc = gf_mul(acc, xrow) ^ words[w0 + (u64)r * WAVE + lane_id()];
    acc = gf_mul(acc, t->lane[lane_id()]);
    return wave_xor(acc);
}

__global__ void __launch_bounds__(256) k_crc_segments(const u32 * __restrict__ words, u32 nseg, u64 total_bits_after_main,
                                                     const CrcTables * __restrict__ t, u32 * __restrict__ accum) {
    const u32 g = blockIdx.x * (blockDim.x / WAVE) + wave_id();
    if (g >= nseg) return;  // wave-uniform exit
    u32 seg = crc_fold_rows(words, (u64)g * CRC_SEG_WORDS, CRC_ROWS, t);
    // shift to the end of the whole message: bits of all later segments + bits after the main part + 32
    const u64 e = (u64)(nseg - 1 - g) * CRC_SEG_WORDS * 32ull + total_bits_after_main + 32ull;
    seg = gf_mul(seg, gf_xpow(e, t->pow2));
    if (lane_id() == 0) atomicXor(accum, seg);
}

// One wave: folds the init state, the ragged remainder (< one segment) and the byte tail into *accum,
// then publishes the final CRC in *out.
__global__ void __launch_bounds__(64) k_crc_finish(const u8 * __restrict__ data, u64 n, u64 main_bytes, u32 init,
                                                  const CrcTables * __restrict__ t, u32 * __restrict__ accum, u32 * __restrict__ out) {
    const u64 rest = n - main_bytes;
    const u32 * words = reinterpret_cast<const u32 *>(data);
    const int rows = (int)(rest / 256);
    u32 state = *accum ^ gf_mul(init, gf_xpow(n * 8ull, t->pow2));
    if (rows > 0) {
        u32 part = crc_fold_rows(words, main_bytes / 4, rows, t);
        part = gf_mul(part, gf_xpow((rest - (u64)rows * 256) * 8ull + 32ull, t->pow2));
        state ^= part;
    }
    // bytes not covered by whole rows: plain bitwise update, but it must be expressed relative to the
    // message end too: U(0, tail) added to the state (state already carries the x^(8|tail|) shifts).
    if (lane_id() == 0) {
        u32 reg = 0;
        for (u64 i = main_bytes + (u64)rows * 256; i < n; i++) {
            reg ^= data[i];
#pragma unroll
            for (int k = 0; k < 8; k++) reg = (reg >> 1) ^ (CRC_POLY & (0u - (reg & 1u)));
        }
        *out = state ^ reg;
    }
}

// d_scratch: 2 words (accumulator, result).  Result is left in d_scratch[1].
void crc32c_device(const u8 * d_data, u64 n, u32 init, const CrcTables * d_tables, u32 * d_scratch, hipStream_t s) {
    HIP_CHECK(hipMemsetAsync(d_scratch, 0, 8, s));
    const u32 nseg = (u32)(n / (CRC_SEG_WORDS * 4));
    const u64 main_bytes = (u64)nseg * CRC_SEG_WORDS * 4;
    if (nseg > 0) {
        launch(k_crc_segments, dim3((nseg + 3) / 4), dim3(256), 0, s, reinterpret_cast<const u32 *>(d_data), nseg, (n - main_bytes) * 8ull,
               d_tables, d_scratch);
    }
    launch(k_crc_finish, dim3(1), dim3(64), 0, s, d_data, n, main_bytes, init, d_tables, d_scratch, d_scratch + 1);
}

// ---- many buffers in one pass (bz3_hip_crc32c_device_many) ------------------------------------------------------------------
// Every buffer is cut as above from its first 4-byte boundary on: `head` bytes (0-3) before it, then whole 16 KiB segments, whole
// 256-byte rows, a byte tail.  The segments of all buffers form one list (CrcBuf::first_seg is the exclusive prefix sum); one wave
// owns one segment of it, finds its buffer by binary search over the prefix sums and xors its share into that buffer's word of
// `crcs`.  A second launch, one wave per buffer, adds what is left and leaves the checksum in crcs[i].  No load falls outside
// [ptr, ptr + size) of any buffer and nothing but `crcs` is written.
__device__ __forceinline__ u32 crc_head_bytes(u64 ptr, u64 size) {
    const u64 h = (0 - ptr) & 3;
    return (u32)(h < size ? h : size);
}

__global__ void __launch_bounds__(256) k_crc_many_segments(const CrcBuf * __restrict__ bufs, u32 n, u32 total_seg,
                                                          const CrcTables * __restrict__ t, u32 * __restrict__ crcs) {
    const u32 g = blockIdx.x * (blockDim.x / WAVE) + wave_id();
    if (g >= total_seg) return;  // wave-uniform exit
    u32 lo = 0, hi = n;          // the last buffer whose first segment is <= g (buffers without segments share their successor's)
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (bufs[mid].first_seg <= g) lo = mid;
        else hi = mid;
    }
    const CrcBuf b = bufs[lo];
    const u32 head = crc_head_bytes(b.ptr, b.size);
    const u64 body = b.size - head;
    const u64 nseg = body / (CRC_SEG_WORDS * 4);
    const u64 l = g - b.first_seg;
    u32 seg = crc_fold_rows(global_ptr<const u32>(b.ptr + head), l * CRC_SEG_WORDS, CRC_ROWS, t);
    // shift to the end of the buffer: the later segments, the rows and bytes behind them, and the 32 of U()
    const u64 e = ((nseg - 1 - l) * CRC_SEG_WORDS * 4 + (body - nseg * CRC_SEG_WORDS * 4)) * 8ull + 32ull;
    seg = gf_mul(seg, gf_xpow(e, t->pow2));
    if (lane_id() == 0) atomicXor(crcs + lo, seg);
}

__global__ void __launch_bounds__(256) k_crc_many_finish(const CrcBuf * __restrict__ bufs, u32 n, const CrcTables * __restrict__ t,
                                                        u32 * __restrict__ crcs) {
    const u32 i = blockIdx.x * (blockDim.x / WAVE) + wave_id();
    if (i >= n) return;  // wave-uniform exit
    const CrcBuf b = bufs[i];
    if (b.size == 0) {  // its pointer is never dereferenced
        if (lane_id() == 0) crcs[i] = b.init;
        return;
    }
    const u8 * data = global_ptr<const u8>(b.ptr);
    const u32 head = crc_head_bytes(b.ptr, b.size);
    u32 reg = b.init;
    if (lane_id() == 0) {
        for (u32 k = 0; k < head; k++) {
            reg ^= data[k];
#pragma unroll
            for (int j = 0; j < 8; j++) reg = (reg >> 1) ^ (CRC_POLY & (0u - (reg & 1u)));
        }
    }
    reg = __shfl(reg, 0);  // the init of the rest
    data += head;
    const u64 body = b.size - head;
    const u64 main_bytes = body / (CRC_SEG_WORDS * 4) * (CRC_SEG_WORDS * 4);
    const u64 rest = body - main_bytes;
    const int rows = (int)(rest / 256);
    u32 state = crcs[i] ^ gf_mul(reg, gf_xpow(body * 8ull, t->pow2));
    if (rows > 0) {
        u32 part = crc_fold_rows(reinterpret_cast<const u32 *>(data), main_bytes / 4, rows, t);
        part = gf_mul(part, gf_xpow((rest - (u64)rows * 256) * 8ull + 32ull, t->pow2));
        state ^= part;
    }
    if (lane_id() == 0) {  // the byte tail, as in k_crc_finish
        u32 tail = 0;
        for (u64 k = main_bytes + (u64)rows * 256; k < body; k++) {
            tail ^= data[k];
#pragma unroll
            for (int j = 0; j < 8; j++) tail = (tail >> 1) ^ (CRC_POLY & (0u - (tail & 1u)));
        }
        crcs[i] = state ^ tail;
    }
}

u64 crc_many_segments(const void * ptr, u64 size) {
    const u64 head = std::min<u64>(size, (0 - (u64)(uintptr_t)ptr) & 3);
    return (size - head) / (CRC_SEG_WORDS * 4);
}

unsigned crc32c_device_many(const CrcBuf * d_bufs, u32 n, u32 total_seg, const CrcTables * d_tables, u32 * d_crcs, hipStream_t s) {
    if (!n) return 0;
    HIP_CHECK(hipMemsetAsync(d_crcs, 0, (size_t)n * sizeof(u32), s));
    if (total_seg) launch(k_crc_many_segments, dim3((total_seg + 3) / 4), dim3(256), 0, s, d_bufs, n, total_seg, d_tables, d_crcs);
    launch(k_crc_many_finish, dim3((n + 3) / 4), dim3(256), 0, s, d_bufs, n, d_tables, d_crcs);
    return total_seg ? 2 : 1;
}

}  // namespace bz3
