// bwt_wide_body.hpp -- the body of bwt.hip's k_bwt_wide, included INSIDE its two forms: k_bwt_wide (one block: the arguments are kernel parameters) and
// k_bwt_wide_many (several blocks in one launch: the arguments are the fields of the workgroup's entry of the job table).  Shared by inclusion, like
// bwt_bg_apply_body.hpp (which says why): a block alone runs the kernel it has always run.
// Expects, in scope: the kernel's former parameters under their names, and grid_x = the workgroups of this block's grid.
    __shared__ u32 tab[256];
    __shared__ WrLds wl[WR_WAVES];
    __shared__ u32 pend[WR_WAVES], pbase[WR_WAVES], pfit;
    // The number of descriptors is where the router left it, on the device (round 4: the host used to read it back to size this
    // launch -- a stream synchronisation per pass); the grid is fixed and walks the list.
    const u32 nmid = counters[8] < mid_cap ? counters[8] : mid_cap;
    if (blockIdx.x * WR_WAVES >= nmid) return;
    tab[threadIdx.x] = vlc[threadIdx.x];
    __syncthreads();
    const u32 lane = (u32)lane_id();
    WrLds & lds = wl[wave_id()];
    for (u32 g0 = blockIdx.x * WR_WAVES; g0 < nmid; g0 += grid_x * WR_WAVES) {  // (uniform trip count per workgroup: barriers inside)
        const u32 g = g0 + (u32)wave_id();
        u32 pending = 0;
        u64 slot0 = 0;
        if (g < nmid) {
            const u32 L = mid_size[g];
            slot0 = mid_slot[g];
            WrCtx cx{t, n, v, pb, tab, counters, chain, slot0, tail_v, tail_slot, tail_d, tail_pb, tail_cap};
            if (L <= 128u) pending = wr_batch<2>(cx, lds, L);
            else pending = wr_batch<4>(cx, lds, L);
        }
        // ---- one append to the tail list per workgroup (an append per wave made the list's counter the bottleneck)
        if (lane == 0) pend[wave_id()] = pending;
        __syncthreads();
        if (threadIdx.x == 0) {
            u32 tot = 0;
            for (int w = 0; w < WR_WAVES; w++) {
                pbase[w] = tot;
                tot += pend[w];
            }
            u32 fits = 1;
            if (tot) {
                const u32 b0 = atomicAdd(&counters[4], tot);
                fits = b0 + tot <= tail_cap ? 1u : 0u;
                if (!fits) {
                    counters[3] = 1u;
                    atomicMin(&counters[5], b0);  // the list is valid up to the first append that did not fit
                    atomicAdd(&counters[1], tot);
                }
                for (int w = 0; w < WR_WAVES; w++) pbase[w] += b0;
            }
            pfit = fits;
        }
        __syncthreads();
        const u32 base = pbase[wave_id()];
        for (u32 q = lane; q < pending; q += WAVE) {
            const u64 x = lds.pl[q];
            if (pfit) {
                tail_v[base + q] = pl_v(x) | (lds.hd[q] ? V_HEAD : 0u);
                tail_slot[base + q] = (u32)(slot0 + lds.aux[q]);
                tail_d[base + q] = (u16)pl_d(x);
                tail_pb[base + q] = (u8)pl_p(x);
            } else {  // back where they are: the deep path takes them
                const u64 p = slot0 + lds.aux[q];
                v[p] = pl_v(x) | (lds.hd[q] ? V_HEAD : 0u);
                pb[p] = (u8)pl_p(x);
            }
        }
        __syncthreads();  // pend / pbase / the waves' LDS are reused by the next descriptors
    }
