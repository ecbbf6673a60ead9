// bwt_tail_body.hpp -- the body of bwt.hip's k_bwt_tail, included INSIDE its two forms: k_bwt_tail (one block: the arguments are kernel parameters) and
// k_bwt_tail_many (several blocks in one launch: the arguments are the fields of the workgroup's entry of the job table).  Shared by inclusion, like
// bwt_bg_apply_body.hpp (which says why): a block alone runs the kernel it has always run.
// Expects, in scope: the kernel's former parameters under their names, and grid_x = the workgroups of this block's grid.
    __shared__ u32 tab[256];
    __shared__ u64 s_word[WAVE];
    __shared__ u32 s_v[WAVE];
    __shared__ u16 s_d[WAVE];
    __shared__ u8 s_pb[WAVE];
    const u32 lane = (u32)lane_id();
    // The length of the list is where the router and the wide kernel left it, on the device ([5]: where the first append that did
    // not fit would have started); the grid is fixed and every wave walks the list in strides (round 4: no read-back to size the launch).
    const u32 total_entries = counters[4] < counters[5] ? counters[4] : counters[5];
    if (blockIdx.x * WAVE >= total_entries) return;
#pragma unroll
    for (int k = 0; k < 4; k++) tab[lane + 64u * k] = vlc[lane + 64u * k];
    __syncthreads();
  for (u32 off = blockIdx.x * WAVE; off < total_entries; off += grid_x * WAVE) {  // this wave's 64 entries; their groups end before off + 128
    u32 cursor, cnt;
    {
        const u32 i0 = off + lane, i1 = off + WAVE + lane;
        const u64 h0 = __ballot(i0 >= total_entries || (tail_v[i0 < total_entries ? i0 : 0u] >> 31) != 0u);
        const u64 h1 = __ballot(i1 >= total_entries || (tail_v[i1 < total_entries ? i1 : 0u] >> 31) != 0u);
        if (!h0) continue;  // these 64 entries continue a group headed in the previous wave's entries
        cursor = (u32)__ffsll((unsigned long long)h0) - 1u;
        cnt = h1 ? (u32)WAVE + (u32)__ffsll((unsigned long long)h1) - 1u : 2u * WAVE;
        if (off + cnt > total_entries) cnt = total_entries - off;
    }
    while (cursor < cnt) {
        const u32 i = cursor + lane;
        const bool have = i < cnt;
        const u32 x = have ? tail_v[off + i] : V_HEAD;
        // the batch: whole groups only.  If the entry behind the 64 loaded ones continues a group, that group waits for the next batch.
        const u64 hm = __ballot((x >> 31) != 0u);
        u32 e;
        if (cursor + WAVE >= cnt) e = cnt - cursor;
        else if (tail_v[off + cursor + WAVE] >> 31) e = WAVE;
        else e = 63u - (u32)__clzll((unsigned long long)hm);  // >= 1: no group here is larger than 64
        const bool act = lane < e;
        u32 sv = x & V_MASK;
        u32 sd = have ? (u32)tail_d[off + i] : 0u;
        const u32 slot = have ? tail_slot[off + i] : 0u;
        u32 sp = have ? (u32)tail_pb[off + i] : 0u;
        bool headf = !act || (x >> 31);
        bool resolved = false;
        const bool fresh = act && sd == 0u;  // came straight from the slot array: depth = the windows its group was formed on
        if (__ballot(fresh)) {
            for (u32 hop = 0; hop < chain; hop++) {
                u64 wa, wb, k56;
                u32 avl, c56;
                load_window(t, (u64)sv + sd, n, wa, wb, avl);
                vlc_pack<56>(tab, wa, wb, avl, k56, c56);
                sd += fresh ? c56 : 0u;
            }
        }
        for (u32 step = 0; step < (u32)TL_CAP; step++) {
            const u64 H = __ballot(headf);  // bit 0 is set: the batch starts with a head
            const u32 gs = 63u - (u32)__clzll((unsigned long long)(H & ((2ull << lane) - 1ull)));
            const u64 above = lane == 63u ? 0ull : (H >> (lane + 1u));
            const u32 ge = above ? lane + (u32)__ffsll((unsigned long long)above) : (u32)WAVE;
            const u32 sz = act ? (ge < e ? ge : e) - gs : 1u;
            const u32 maxsz = wave_max(sz);
            if (maxsz <= 1u) {
                resolved = true;
                break;
            }
            u64 wa, wb, key;
            u32 avl, c;
            load_window(t, (u64)sv + sd, n, wa, wb, avl);
            vlc_pack<40>(tab, wa, wb, avl, key, c);
            const bool live = (u64)sv + sd < n;
            if (!live) {
                key = (u64)(n - sv);
                c = 0;
            }
            const u64 w = ((live ? 1ull : 0ull) << 40) | key;
            u64 w2, wl;
            if (maxsz <= 12u) {
                // small groups: rank by counting (a cross-lane read per member of the largest group)
                u32 below = 0;
                for (u32 k = 0; k < maxsz; k++) {
                    const u32 q = gs + k;
                    const u64 wq = __shfl(w, (int)(q & 63u));
                    if (k < sz) below += (wq < w || (wq == w && q < lane)) ? 1u : 0u;
                }
                const u32 np = act ? gs + below : lane;
                s_word[np] = w;
                s_v[np] = sv;
                s_d[np] = (u16)(sd + c);
                s_pb[np] = (u8)sp;
                __syncthreads();
                w2 = s_word[lane];
                wl = s_word[lane ? lane - 1u : 0u];
                sv = s_v[lane];
                sd = s_d[lane];
                sp = s_pb[lane];
                __syncthreads();
            } else {
                // larger groups: one 64-lane bitonic network over [group start : 6][word : 41][lane : 6] sorts all groups at once
                // (21 stages whatever the group sizes; counting costs a cross-lane read per member: 64 of them for a group of 64)
                u64 x[1] = {((u64)(act ? gs : lane) << 47) | (w << 6) | (u64)lane};
                s_v[lane] = sv;
                s_d[lane] = (u16)(sd + c);
                s_pb[lane] = (u8)sp;
                wave_bitonic<1>(x);
                __syncthreads();
                const u32 src = (u32)x[0] & 63u;
                sv = s_v[src];
                sd = s_d[src];
                sp = s_pb[src];
                __syncthreads();
                w2 = (x[0] >> 6) & ((1ull << 41) - 1ull);
                const u64 xl = __shfl_up(x[0], 1u);
                wl = (xl >> 6) & ((1ull << 41) - 1ull);
            }
            headf = headf || w2 != wl;  // (a lane alone in its group only ever compares its own word: it stays a head)
        }
        if (act) {
            v[slot] = sv | (headf ? V_HEAD : 0u);
            pb[slot] = (u8)sp;
            if (sv == 0) counters[2] = slot;
        }
        if (!resolved) {
            const u64 H = __ballot(headf);
            const u64 nxt = (H >> 1) | (1ull << 63);
            const u64 amb = ~(H & nxt) & (e == 64u ? ~0ull : ((1ull << e) - 1ull));  // lanes not alone in their group
            if (lane == 0 && amb) atomicAdd(&counters[1], (u32)__popcll((unsigned long long)amb));
        }
        cursor += e;
    }
  }
