// sort_scatter_body.hpp -- the body of sort.hip's radix scatter kernels, included INSIDE k_rs_scatter (one array: the forward sorter, the LZP
// predecessor build) and k_rs_scatter_many (several arrays in one launch: the inverse BWT's psi build).  Not a header in the usual sense: the
// text is shared by inclusion, not through a __device__ function, because the single kernels must compile to exactly what they were -- moved
// into a function and inlined back, the same statements schedule differently (118 instead of 138 VGPRs for 8-byte keys), and the forward
// sorter's kernels are not to change with the inverse transform's batching.
// Expects, in scope: the template parameters K, IOTA, WKEYS, BITS, RAW; kin, kout, vin, vout, n, shift, offs, tiles, iota_split, out_base, xcd.
// The workgroup's index along the array is blockIdx.x in both.
    constexpr int RADIX = 1 << BITS;
    constexpr int DPT = RADIX / RS_BLOCK;  // digits per thread: d = DPT * threadIdx.x + j
    static_assert(RADIX % RS_BLOCK == 0 && DPT >= 1, "a thread owns whole digits");
    __shared__ u32 cnt[RS_WAVES][RADIX];
    __shared__ u32 dstart[RADIX];   // first slot of a digit inside the tile
    __shared__ u32 gdelta[RADIX];   // global destination of a digit's first key - dstart (mod 2^32)
    __shared__ u32 scan_lds[RS_BLOCK / WAVE + 1];
    __shared__ K skey[RS_TILE];
    __shared__ u32 sval[RS_TILE];
    const u32 tile = rs_tile_of_block(blockIdx.x, tiles, xcd != 0u);
    if (tile >= tiles) return;
    const int w = wave_id(), l = lane_id();
#pragma unroll
    for (int k = 0; k < RS_WAVES; k++)
#pragma unroll
        for (int d = threadIdx.x; d < RADIX; d += RS_BLOCK) cnt[k][d] = 0;
    __syncthreads();

    const u64 tile_base = (u64)tile * RS_TILE;
    const u64 wbase = tile_base + (u64)w * RS_WAVE_SPAN + l;
    K key[RS_ROUNDS];
    u32 local[RS_ROUNDS];
    const u64 lt = lanemask_lt();
    const u64 last = n - 1;
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; r++) {
        const u64 i = wbase + (u64)r * WAVE;
        key[r] = kin[i < n ? i : last];
    }
    // RAW: this thread's digits' rows of the count table, requested before the ranking below so that their latency hides behind it
    u32 row_total[DPT], row_before[DPT];
    if (RAW) {
#pragma unroll
        for (int j = 0; j < DPT; j++) {
            const u32 * __restrict__ row = offs + (u64)(DPT * threadIdx.x + j) * tiles;
            u32 tot = 0, bef = 0;
#pragma unroll 4
            for (u32 t = 0; t < tiles; t++) {
                const u32 c = row[t];
                tot += c;
                bef += t < tile ? c : 0u;
            }
            row_total[j] = tot;
            row_before[j] = bef;
        }
    }
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; r++) {
        const u64 i = wbase + (u64)r * WAVE;
        const bool valid = i < n;
        const u32 d = rs_digit<K, BITS>(key[r], shift);
        u64 peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < BITS; b++) {
            const bool bit = (d >> b) & 1u;
            const u64 bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        const u32 below = (u32)__popcll(peers & lt);
        const u32 pre = valid ? cnt[w][d] : 0u;
        wave_sync();
        if (valid && below == 0) cnt[w][d] = pre + (u32)__popcll(peers);
        wave_sync();
        local[r] = pre + below;
    }
    u32 val[RS_ROUNDS];
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; r++) {
        const u64 i = wbase + (u64)r * WAVE;
        val[r] = IOTA ? (u32)i + ((u32)i >= iota_split ? 1u : 0u) : vin[i < n ? i : last];
    }
    __syncthreads();
    {
        u32 run[DPT];
        u32 mine = 0;
#pragma unroll
        for (int j = 0; j < DPT; j++) {
            const u32 d = DPT * threadIdx.x + j;
            u32 acc = 0;
#pragma unroll
            for (int k = 0; k < RS_WAVES; k++) {
                u32 c = cnt[k][d];
                cnt[k][d] = acc;
                acc += c;
            }
            run[j] = acc;
            mine += acc;
        }
        u32 total;
        u32 start = block_excl_add<RS_BLOCK>(mine, scan_lds, total);  // ends with a barrier
        u32 gbase = 0;
        if (RAW) {
            u32 rt = 0;
#pragma unroll
            for (int j = 0; j < DPT; j++) rt += row_total[j];
            u32 all;
            gbase = block_excl_add<RS_BLOCK>(rt, scan_lds, all);  // keys of smaller digits, all tiles
        }
#pragma unroll
        for (int j = 0; j < DPT; j++) {
            const u32 d = DPT * threadIdx.x + j;
            dstart[d] = start;
            if (RAW) {
                gdelta[d] = gbase + row_before[j] + out_base - start;
                gbase += row_total[j];
            } else {
                gdelta[d] = offs[(u64)d * tiles + tile] + out_base - start;
            }
            start += run[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; r++) {
        const u32 d = rs_digit<K, BITS>(key[r], shift);
        local[r] += dstart[d] + cnt[w][d];
    }
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; r++) {
        const u64 i = wbase + (u64)r * WAVE;
        if (i < n) {
            skey[local[r]] = key[r];
            sval[local[r]] = val[r];
        }
    }
    __syncthreads();
    const u64 left = n - tile_base;
    const u32 count = left < (u64)RS_TILE ? (u32)left : (u32)RS_TILE;
#pragma unroll
    for (int q = 0; q < RS_ROUNDS; q++) {
        const u32 j = (u32)q * RS_BLOCK + threadIdx.x;
        if (j < count) {
            const K k = skey[j];
            const u32 pos = gdelta[rs_digit<K, BITS>(k, shift)] + j;
            if (WKEYS) kout[pos] = k;
            vout[pos] = sval[j];
        }
    }
