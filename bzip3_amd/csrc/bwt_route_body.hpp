// bwt_route_body.hpp -- the body of bwt.hip's k_bwt_route, included INSIDE its two forms: k_bwt_route (one block: the arguments are kernel parameters) and
// k_bwt_route_many (several blocks in one launch: the arguments are the fields of the workgroup's entry of the job table).  Shared by inclusion, like
// bwt_bg_apply_body.hpp (which says why): a block alone runs the kernel it has always run.
// Expects, in scope: the kernel's former parameters under their names, and grid_x = the workgroups of this block's grid.
    __shared__ RtLds wl[RT_WAVES];
    __shared__ u32 ok[3];  // the workgroup's appends fit their lists
    const u32 lane = (u32)lane_id();
    const u32 tile = blockIdx.x * RT_WAVES + (u32)wave_id();
    const u64 a = (u64)tile * WR_A;
    RtLds & lds = wl[wave_id()];
    const bool active = a < n && !(dirty && !(dirty[tile] | dirty[tile + 1]));
    const u32 wend = !active ? 0u : ((u64)n - a < 1025ull ? (u32)((u64)n - a) : 1025u);  // window positions that exist (the first slot past the end is a head)
    if (lane < 4u) lds.cnt[lane] = 0;
    // head bits of [a, a + 1024] from the snapshot; slots past the end are heads
    if (active && lane < 33u) {
        const u64 first = a + 32ull * lane;
        const u64 limit = ((u64)n + 63u) & ~63ull;  // the snapshot is written in whole 64-slot words
        lds.hb[lane] = first < limit ? hbits[first >> 5] : 0xFFFFFFFFu;
    }
    wave_sync();
    // 64 head bits starting at window position `start` (may be negative: nothing is known before the window)
    auto bits64 = [&](int start) -> u64 {
        const int s0 = start < 0 ? 0 : start;
        const u32 wi = (u32)s0 >> 5, sh = (u32)s0 & 31u;
        const u64 lo = ((u64)lds.hb[wi + 1 < 33u ? wi + 1 : 32u] << 32) | lds.hb[wi < 33u ? wi : 32u];
        const u64 hi = lds.hb[wi + 2 < 33u ? wi + 2 : 32u];
        u64 x = sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
        if (wi + 1 >= 33u) x &= 0xFFFFFFFFull >> sh;  // (beyond the window: unknown, read as no head)
        if (start < 0) x = start > -64 ? x << (u32)(-start) : 0ull;
        return x;
    };
    // ---- groups of up to 64 suffixes go to the tail kernel (one suffix per lane, ~50 registers, dozens of waves per CU: measured four
    // times the throughput per suffix of the wide path).  Every slot decides for itself from the head bits around it: its group's head h
    // (within 63 slots before it) and end e (within 64 after it); it goes if h lies in this wave's anchor slots and 2 <= e - h <= 64.
    u32 flags = 0, tcnt = 0;  // bit k: position lane + 64 k goes
    u64 row_ballot[9];
    u32 row_base[9];
    u32 nlg = 0;  // large groups / runs noted in lds.lg_*
    if (active) {
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const u32 p = lane + 64u * k;
            const u64 w1 = bits64((int)p - 63), w2 = bits64((int)p + 1);
            bool go = false;
            if (w1 && w2 && p < wend) {
                const u32 h = p - (u32)__clzll((unsigned long long)w1);
                const u32 e = p + (u32)__ffsll((unsigned long long)w2);
                go = h < (u32)WR_A && e - h >= 2u && e - h <= 64u;
            }
            row_ballot[k] = __ballot(go);
            flags |= (go ? 1u : 0u) << k;
        }
#pragma unroll
        for (int k = 0; k < 9; k++) {
            row_base[k] = tcnt;
            tcnt += (u32)__popcll((unsigned long long)row_ballot[k]);
        }
        // ---- the slots before the first head continue a group headed before this window (tile > 0: slot 0 is always a head)
        u32 nmid = 0, nbig = 0;
        const u32 c0 = wr_next_head(lds.hb, 0u);
        if (c0 > 0u) {
            const u32 cl = carry_local[tile], cg = group_carry[tile / (u32)SP_GROUP];
            const u32 hp = (cl > cg ? cl : cg) - 1u;  // (tile > 0: slot 0 is a head, so there is one)
            const bool big = c0 == WR_FAR || (u32)a + c0 - hp > (u32)WR_G;
            u32 stop = c0 < (u32)WR_A ? c0 : (u32)WR_A;
            stop = stop < wend ? stop : wend;
            if (big && stop > 0u) {
                if (lane == 0) {
                    lds.lg_c[nlg] = 0;
                    lds.lg_e[nlg] = (u16)stop;
                    lds.lg_hp[nlg] = hp;
                }
                nlg++;
                nbig += stop;
            }
        }
        // ---- groups of more than 64 headed here: a descriptor for the wide kernel (up to 512 members), or the big list
        for (u32 k = 0; k < 8u; k++) {
            const u32 p = lane + 64u * k;
            const bool head = (lds.hb[p >> 5] >> (p & 31u)) & 1u;
            u64 large = __ballot(head && p < wend && bits64((int)p + 1) == 0ull);  // no other head within the next 64 slots
            while (large) {
                const u32 l = (u32)__ffsll((unsigned long long)large) - 1u;
                large &= large - 1ull;
                const u32 c = l + 64u * k;
                const u32 nh = wr_next_head(lds.hb, c + 1u);  // end of the group
                const bool big = nh == WR_FAR || nh - c > (u32)WR_G;  // too large for a wave
                u32 stop = big ? (nh < (u32)WR_A ? nh : (u32)WR_A) : nh;
                stop = stop < wend ? stop : wend;
                if (lane == 0) {
                    lds.lg_c[nlg] = (u16)c;
                    lds.lg_e[nlg] = (u16)stop;
                    lds.lg_hp[nlg] = big ? (u32)a + c : 0xFFFFFFFFu;
                }
                nlg++;
                if (big) nbig += stop - c;
                else nmid++;
            }
        }
        if (lane == 0) {
            lds.cnt[0] = tcnt;
            lds.cnt[1] = nmid;
            lds.cnt[2] = nbig;
        }
    }
    __syncthreads();
    // ---- one reservation per list for the whole workgroup
    if (threadIdx.x < 3u) {
        const u32 q = threadIdx.x;
        u32 tot = 0;
        for (int w = 0; w < RT_WAVES; w++) {
            wl[w].base[q] = tot;
            tot += wl[w].cnt[q];
        }
        u32 fits = 1;
        if (tot) {
            u32 * ctr = q == 0 ? &counters[4] : q == 1 ? &counters[8] : &counters[0];
            const u32 cap = q == 0 ? tail_cap : q == 1 ? mid_cap : big_cap;
            const u32 b0 = atomicAdd(ctr, tot);
            fits = b0 + tot <= cap ? 1u : 0u;
            if (!fits) {
                counters[3] = 1u;
                if (q == 0) atomicMin(&counters[5], b0);  // the tail list is valid up to the first append that did not fit
                if (q != 2) atomicAdd(&counters[1], 1u);  // (suffixes that stay where they are: the deep path takes them)
            }
            for (int w = 0; w < RT_WAVES; w++) wl[w].base[q] += b0;
        }
        ok[q] = fits;
    }
    __syncthreads();
    if (!active) return;
    if (tcnt && ok[0]) {
        const u32 base = lds.base[0];
#pragma unroll
        for (int k = 0; k < 9; k++)
            if ((flags >> k) & 1u) {
                const u32 p = lane + 64u * k;
                const u32 d = base + row_base[k] + (u32)__popcll((unsigned long long)(row_ballot[k] & (((u64)1 << lane) - 1ull)));
                const u64 slot = a + p;
                tail_v[d] = (v[slot] & V_MASK) | (((lds.hb[p >> 5] >> (p & 31u)) & 1u) ? V_HEAD : 0u);
                tail_slot[d] = (u32)slot;
                tail_d[d] = 0;  // the tail kernel walks the windows the group was formed on
                tail_pb[d] = pb[slot];
            }
    }
    u32 dm = lds.base[1], db = lds.base[2];
    for (u32 i = 0; i < nlg; i++) {
        const u32 c = lds.lg_c[i], e = lds.lg_e[i], hp = lds.lg_hp[i];
        if (hp == 0xFFFFFFFFu) {
            if (ok[1] && lane == 0) {
                mid_slot[dm] = (u32)a + c;
                mid_size[dm] = (u16)(e - c);
            }
            dm++;
        } else {
            if (ok[2])
                for (u32 q = c + lane; q < e; q += WAVE) {
                    big_slot[db + (q - c)] = (u32)a + q;
                    big_hp[db + (q - c)] = hp;
                }
            db += e - c;
        }
    }
