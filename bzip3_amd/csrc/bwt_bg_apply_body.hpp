// bwt_bg_apply_body.hpp -- the body of bwt.hip's k_bg_apply, included INSIDE its two forms: k_bg_apply (one block: the arguments are kernel
// parameters) and k_bg_apply_many (several blocks in one launch: the arguments are the fields of the workgroup's entry of the job table).  Not a
// header in the usual sense: the text is shared by inclusion because from the job table the same statements compile to a different program
// (68 / 50 instead of 82 VGPRs, a sixth fewer instructions; presumably __restrict__ binds the compiler on kernel parameters and not on the
// locals the table form declares), and a block alone, the metric's 256 MiB block, is to run what it always ran.
// Expects, in scope: the template parameters VF, DOUBLING; keys, vals, slots, m, tile_head, tile_keep, sa, isa, vals_out, slots_out, grp_out, t, pb,
// rank_out.  The workgroup's tile is blockIdx.x in both.
    __shared__ u32 lds[BW_BLOCK / WAVE + 1];
    __shared__ u32 st_v[BG_TILE], st_s[BG_TILE], st_g[BG_TILE];  // the tile's part of the compacted list, staged so that it leaves coalesced
    const u64 base = (u64)blockIdx.x * BG_TILE + (u64)threadIdx.x * BG_ITEMS;
    const u64 lbase = base < m ? base : (u64)m - 1;  // threads past the end load something valid and use none of it
    u32 heads, uniqs;
    bg_flags<VF>(keys, vals, m, base, heads, uniqs);
    u32 v[BG_ITEMS], sl[BG_ITEMS], hi[BG_ITEMS];
    bg_load_u32(vals, m, lbase, v);
#pragma unroll
    for (int j = 0; j < BG_ITEMS; j++) {
        v[j] &= V_MASK;
        hi[j] = 0;
    }
    if (DOUBLING) {
        u64 kv[BG_ITEMS + 2];
        bg_load_keys(keys, m, lbase, kv);
#pragma unroll
        for (int j = 0; j < BG_ITEMS; j++) hi[j] = (u32)(kv[j + 1] >> 32);
    }
    if (slots) {
        bg_load_u32(slots, m, lbase, sl);
    } else {
#pragma unroll
        for (int j = 0; j < BG_ITEMS; j++) sl[j] = (u32)(base + j);
    }
    const u32 carry_hp = tile_head[blockIdx.x], tile_off = tile_keep[blockIdx.x];
    u32 hp = 0, keep = 0;
#pragma unroll
    for (int j = 0; j < BG_ITEMS; j++) {
        const u64 k = base + j;
        if (k < m) {
            if ((heads >> j) & 1u) hp = (u32)k + 1u;
            keep += ((uniqs >> j) & 1u) ? 0u : 1u;
        }
    }
    u32 run_hp = bg_block_excl_max<BW_BLOCK>(hp, lds);
    run_hp = carry_hp > run_hp ? carry_hp : run_hp;
    u32 all;  // elements of this tile that stay active
    u32 out = block_excl_add<BW_BLOCK>(keep, lds, all);  // this thread's first slot in the tile's part of the compacted list
    // rank of an element = slot of its group's head.  The head of the group that reaches into this thread's elements from the left
    // costs one gather; from the first head on, the slots are in registers (sl[j] = k itself when the list is the whole array).
    u32 run_rank = 0;  // run_hp == 0 only where element 0 of the list starts the thread, and that one is a head
    if (run_hp > 0 && base < m) run_rank = slots ? slots[run_hp - 1u] : run_hp - 1u;
    u32 rank[BG_ITEMS];
#pragma unroll
    for (int j = 0; j < BG_ITEMS; j++) {
        const u64 k = base + j;
        rank[j] = 0;
        if (k < m) {
            if ((heads >> j) & 1u) run_rank = sl[j];
            rank[j] = run_rank;
        }
    }
#pragma unroll
    for (int j = 0; j < BG_ITEMS; j++) {
        const u64 k = base + j;
        if (k < m) {
            if (VF) rank_out[k] = rank[j];  // in slot order; the inverse suffix array is filled from these by isa_from_ranks (bucketed, not n random stores)
            else if (!DOUBLING || rank[j] != hi[j]) isa[v[j]] = rank[j];
            if ((uniqs >> j) & 1u) {
                if (!VF) {  // (VF: the list IS the array, the suffix is in its slot already -- and neighbours still read its flag)
                    sa[sl[j]] = v[j];
                    pb[sl[j]] = v[j] ? t[v[j] - 1u] : (u8)0;  // the slot's BWT symbol: the output is assembled from these bytes
                }
            } else {
                st_v[out] = v[j];
                st_s[out] = sl[j];
                st_g[out] = rank[j];
                out++;
            }
        }
    }
    __syncthreads();
    // (a thread's kept elements are consecutive slots: written directly, every store instruction of a wave would touch 64 scattered
    // words; from LDS consecutive lanes write consecutive words)
    for (u32 idx = threadIdx.x; idx < all; idx += BW_BLOCK) {
        vals_out[tile_off + idx] = st_v[idx];
        slots_out[tile_off + idx] = st_s[idx];
        grp_out[tile_off + idx] = st_g[idx];
    }
