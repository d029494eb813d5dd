// fz_kernel_bodies.inc — the statement lists of the kernels that exist twice: for the unsegmented / strided geometries
// (fz_scan_kernel, fz_verify_kernel, fz_verify_wf_kernel, fz_verify_big_kernel, fz_mp_verify_kernel, fz_mp_verify_subs_kernel)
// and for ragged segments, a batch of sequences packed back to back (fz_batch_*_kernel, fz_mp_batch_*_kernel; fz_device.h).  Included by fz_kernels.h inside each kernel, with
// FZ_KERNEL_BODY naming the section and `constexpr bool RAG` (and the kernel's template parameters) in scope: one text,
// two kernels — a shared inline function instead moved the register allocation of the existing instances.
#if FZ_KERNEL_BODY == 1      // ---- fz_scan_kernel / fz_lean_scan_kernel / fz_batch_scan_kernel
    // (also in scope: `constexpr bool DUPH` — the equal-n-gram slot sets exist — and `constexpr int MAXK`, the widest register band)
    constexpr bool WF = WFG == 16 || WFG == 32;       // lane-per-cell verification inside the scan, WFG lanes per candidate
    constexpr int BITS = (WFG == 1 || WFG == 2 || WFG == 4) ? WFG : 0;   // bit-vector verification inside the scan, one candidate per lane:
                                                                         // one / two 64-bit words per column, 4 = one 32-bit word
    // WFG = 3: the Hamming count of WFG = 0 (substitutions-only searches) under the queue discipline of the bit-vector forms
    // (full passes, block-range passes over dense tiles), for patterns that let expect dense candidates
    constexpr bool ADAPT = BITS != 0 || WFG == 3;
    constexpr int VF = WFG == 3 ? -1 : BITS;              // what fz_wave_verify runs: -1 Hamming count only, 0 by mode, 1 / 2 bit vectors
    static_assert(WFG == 0 || ADAPT || WF, "0: register band / Hamming count; 3: Hamming count; 1, 2, 4: bit-vector columns; 16, 32: lanes per candidate");
    static_assert(!(SEG && RAG), "strided and ragged segments are two geometries");
    static_assert(WFG == 0 || (FUSED && !SEG), "the lane-per-cell and bit-vector forms are fused forms of the in-memory search");
    constexpr bool PREF = FUSED && !SEG && !WF;       // candidate windows are prefetched by LDS-DMA
    constexpr uint32_t peq_bytes = BITS ? FZ_PEQ_BYTES(BITS ? BITS : 1) : 0u;   // the two Peq tables behind the pattern
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t mpad = FUSED ? (a.m + 15u) & ~15u : 0u;   // only the fused verification reads the pattern from LDS (m <= FZ_MAX_M there)
    // [32] hash living in the slot.  The kernel has no static LDS, so the dynamic area, and with it this
    // table, starts at LDS address 0 and a slot's byte offset is its address (saves one VALU add per
    // lookup); trap if a toolchain ever lays LDS out differently.
    uint32_t *lut = reinterpret_cast<uint32_t *>(smem);
    if (reinterpret_cast<uintptr_t>((FzLdsU8 *)smem) != 0) __builtin_trap();
    uint8_t *pat_lds = smem + FZ_TABLE_BYTES;
    if constexpr (FUSED)
        for (uint32_t i = threadIdx.x; i < a.m; i += FZ_FILTER_THREADS) pat_lds[i] = a.pat[i];
    if constexpr (BITS != 0) {
        // Peq tables (fz_device.h: fz_verify_lev_bits): zero, then one LDS atomic per pattern position and table
        constexpr int NWc = BITS ? BITS : 1;
        uint32_t *peq = reinterpret_cast<uint32_t *>(smem + FZ_TABLE_BYTES + mpad);
        constexpr uint32_t wdw = FZ_BITS_WIDTH(NWc) / 32u;                   // dwords per table word
        for (uint32_t i = threadIdx.x; i < peq_bytes / 4u; i += FZ_FILTER_THREADS) peq[i] = 0u;
        __syncthreads();
        if (threadIdx.x < a.m) {
            const uint32_t q = threadIdx.x, c = pat_lds[q];
            const uint32_t bf = fz_bits_fwd_bit<NWc>(a.m, q), br = fz_bits_rev_bit<NWc>(a.m, q);
            atomicOr(&peq[c * wdw + (bf >> 5)], 1u << (bf & 31u));
            atomicOr(&peq[(256u + c) * wdw + (br >> 5)], 1u << (br & 31u));
        }
    }
    if (threadIdx.x < FZ_LUT_SLOTS) {
        uint32_t t = ((threadIdx.x + 1u) & (FZ_LUT_SLOTS - 1u)) << a.lut_shift;   // free slot: a value of the next slot
        uint32_t who = 0xffu;                                                     // ... and the block that lives in the slot
        uint32_t set = 0;                                                         // ... or, with equal n-grams in the launch, all of them
        for (uint32_t g = a.nblk; g-- > 0;)
            if (((a.H[g] >> a.lut_shift) & (FZ_LUT_SLOTS - 1u)) == threadIdx.x) { t = a.H[g]; who = g; set |= 0x10000u << g; }
        lut[threadIdx.x] = t;
        if constexpr (DUPH) lut[FZ_LUT_SLOTS + threadIdx.x] = (a.flags & FZ_FLAG_DUP_HASHES) ? (who | set) : who;
        else lut[FZ_LUT_SLOTS + threadIdx.x] = who;
    }
    // DUPH = false (the lean instances): no launch with equal block hashes gets here, the slot-set branch below does not exist
    bool dup_hashes = false;
    if constexpr (DUPH) dup_hashes = (a.flags & FZ_FLAG_DUP_HASHES) != 0;
    // this workgroup's walk over the tiles (fz_device.h: FzWalk): first, first + stride, .. below limit is the logical walk,
    // kept here as `left` = limit - (the logical tile of this step), so `left > 0` is the walk's `tile < limit`; `ptile` is
    // the tile whose bytes the step reads — the logical one, or its mirror in a reversed launch — and moves by `pstride`
    // (four scalar dwords where the logical walk alone kept five: the host keeps a shard below 2^31 tiles, so tile numbers
    // and their differences are 32-bit values).  The flushes decode queue entries with the physical walk's copy in LDS
    // (fz_code_local)
    // (batches and file chunks are never scanned backwards, enqueue_shard: their instances keep the forward walk alone)
    const FzWalk wk = fz_scan_walk(a.nreg, a.reg_wg0, a.reg_nwg, a.reg_tile0, a.reg_end, gridDim.x, ntiles, blockIdx.x,
                                   !RAG && !SEG && (a.flags & FZ_FLAG_REVERSE) != 0);
    const int32_t stride = (int32_t)wk.stride, pstride = wk.phys_stride;
    if (threadIdx.x == 0) {
        uint32_t *walk = reinterpret_cast<uint32_t *>(smem + FZ_WALK_LDS);
        walk[0] = (uint32_t)wk.phys_first; walk[1] = (uint32_t)wk.phys_stride;
    }
    __syncthreads();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t qcap = PREF ? a.qcap : (uint32_t)FZ_QCAP;   // queue entries per wave
    const FzWaveLds w = PREF ? fz_wave_lds_pref(smem + FZ_TABLE_BYTES + mpad + peq_bytes, FZ_TABLE_BYTES + mpad + peq_bytes, wave, qcap, a.win_pieces)
                        : WF ? fz_wave_lds(smem + FZ_TABLE_BYTES + mpad, wave, fz_wf_fused_dwords(a.win_dwords, WF ? WFG : 16), 0u, 1u, true)
                             : fz_wave_lds(smem + FZ_TABLE_BYTES + mpad, wave, FUSED ? a.win_dwords : 0u,
                                           FUSED ? a.band_w : 0u, a.vlanes, true);
    const uint32_t hash_k = a.hash_k;
    // byte address of a hash's slot = (h >> (lut_shift - 2)) & 0x7c: two VGPR-only VALU ops (a shift
    // amount in an SGPR or an SDWA byte select would issue at half the rate, benchmarks/valu_rates.hip)
    uint32_t slot_shift;
    asm volatile("v_mov_b32 %0, %1" : "=v"(slot_shift) : "s"(a.lut_shift - 2u));
    const uint32_t mask1 = a.mask1;
    const uint32_t lane = fz_lane();
    const uint32_t lane_off = threadIdx.x * 16u;
    uint32_t qn = 0;                                  // wave-uniform queue fill
    uint32_t qf = 0;                                  // PREF: entries [0, qf) have their windows requested
    uint32_t confirmed = 0;                           // wave-uniform statistics
    uint32_t titer = 0;                               // tile iteration of this workgroup
    int32_t left = (int32_t)(wk.limit - wk.first);    // <= 0: no tile (left)
    uint32_t ptile = (uint32_t)wk.phys_first;
    // has_near_match_* (substitutions_only.py:218-233 stops at the first match): a workgroup that starts after a record
    // has been counted skips its tiles (thousands of short workgroups per launch: the ones not yet started are the saving)
    if ((a.flags & FZ_FLAG_ANY) && __hip_atomic_load(&counters[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) left = 0;
    bool slow = false;                                // a tile is being re-scanned by enumeration
    uint32_t slow_pos = 0;
    // Bit-vector form: the queue is worked off in full passes (fz_bits_flush) and filled as far as the tiles' recent yield
    // lets expect it to hold: `ylast` = entries the last tile queued (wave-uniform).  The expectation only steers; a tile that
    // overflows the queue all the same is scanned again behind a flush (and by enumeration if it overflows an empty queue).
    uint32_t ylast = 0;
    // ... and where the data is denser than any queue (DNA with 4-character n-grams: hundreds of hits per tile and wave), a
    // tile is taken in several passes, each for the blocks [b0, b0 + bw) of the launch only: a tile that overflows the EMPTY
    // queue halves bw and starts again, tiles that queue little double it.  Only a tile that overflows the empty queue with
    // one block (a run of one character meeting an n-gram of that character) is enumerated.
    uint32_t b0 = 0, bw = FZ_MAX_BLOCKS_PER_LAUNCH;

    // the filter over one row (row R of the tile)
    auto test_row = [&](const uint4 &v, const uint2 &h, auto Rc) {
        constexpr int r = decltype(Rc)::value;
        // byte offsets tested per wave-uniform branch: 8 in the hit-emitting form when the n-grams have 8 bytes or
        // more (DH == 5) — such n-grams are rare in any data, the branch is hardly ever taken and one compare serves
        // twice the offsets (exact search of a 20-byte pattern: 0.199 -> 0.194 ms per GiB); 4 otherwise (on DNA with
        // 6-byte n-grams 17 % of the 4-offset groups fire: with 8 the rare path's compares double, 0.223 -> 0.246 ms;
        // the fused form has no registers to spare for 8 hashes: 26 VGPRs spilled)
        constexpr int GRP = FZ_GROUP ? FZ_GROUP : (NWIN == 2 && DH == 5 && !FUSED ? 8 : 4);
        const uint32_t w6[6] = {v.x, v.y, v.z, v.w, h.x, h.y};
#pragma unroll
        for (int j = 0; j < 16 / GRP; ++j) {     // GRP byte offsets per ballot
            uint32_t hv[GRP], lv[GRP];                    // window hashes and the hashes living in their table slots
#pragma unroll
            for (int i = 0; i < GRP; ++i) {
                const int o = GRP * j + i;
                const uint32_t x = FZ_WIN(w6, o);
                if (NWIN == 1) hv[i] = (x & mask1) * hash_k;                             // v_mul_lo_u32
                else hv[i] = __umul24(FZ_WIN(w6, o + DH), hash_k) + x;                   // v_mad_u32_u24
                uint32_t slot4;
                if constexpr (SA) asm("v_and_b32 %0, " FZ_LUT_ADDR_MASK_STR ", %1" : "=v"(slot4) : "v"(hv[i]));
                else asm("v_lshrrev_b32 %0, %1, %2\n\tv_and_b32 %0, " FZ_LUT_ADDR_MASK_STR ", %0" : "=v"(slot4) : "v"(slot_shift), "v"(hv[i]));
                lv[i] = *reinterpret_cast<FzLdsU32 *>(slot4);            // lut sits at LDS address 0
            }
            // (measured and not kept: one v_cmp per offset with the lane masks OR-ed on the scalar unit instead of
            //  xor / min3 / min / one v_cmp per four offsets — 15.5 instead of 22.5 VALU per group, 0.2222 vs 0.2195 ms)
            uint32_t am[GRP];
#pragma unroll
            for (int i = 0; i < GRP; ++i) am[i] = hv[i] ^ lv[i];
            uint32_t acc = min(min(am[0], am[1]), min(am[2], am[3]));
            if constexpr (GRP == 8) acc = min(acc, min(min(am[4], am[5]), min(am[6], am[7])));
            const bool fire = __ballot(acc == 0) != 0;
            if (__builtin_expect(fire, 0)) {              // wave-uniform, rare: some lane, some offset
#pragma unroll
                for (int i = 0; i < GRP; ++i) {
                    const unsigned long long mi = __ballot(hv[i] == lv[i]);      // which offset (scalar branch)
                    if (mi) {
                        // which block: the window's hash equals the one in its slot, and the dword behind the hash
                        // table says whose that is (one LDS read instead of a compare per block)
                        uint32_t slot4;
                        if constexpr (SA) asm("v_and_b32 %0, " FZ_LUT_ADDR_MASK_STR ", %1" : "=v"(slot4) : "v"(hv[i]));
                        else asm("v_lshrrev_b32 %0, %1, %2\n\tv_and_b32 %0, " FZ_LUT_ADDR_MASK_STR ", %0" : "=v"(slot4) : "v"(slot_shift), "v"(hv[i]));
                        const uint32_t g = *reinterpret_cast<FzLdsU32 *>(slot4 + FZ_LUT_BYTES);
                        // the queue code is recomputed here: a (tid << 4 | titer << 18) kept in a VGPR across the tile
                        // saves three ops per firing but is the register that spills (measured: 0.218 -> 0.221 ms)
                        uint32_t pos = threadIdx.x;
                        asm volatile("v_lshlrev_b32 %0, 4, %0" : "+v"(pos));
                        if (DUPH && __builtin_expect(dup_hashes, 0)) {
                            // equal n-grams (equal hashes) share a slot: the dword behind the hash table then carries, from
                            // bit 16 up, the SET of the launch's blocks that live in the slot, and a firing lane queues one
                            // entry per member (rounds 1 - 5 compared the window's hash with every block of the launch, offset
                            // by offset: ~8 scalar instructions per block and offset of a fired group — a DNA pattern with a
                            // repeated 4-character n-gram ran 4 x slower than one without)
                            uint32_t set = hv[i] == lv[i] ? g >> 16 : 0u;
                            pos += (uint32_t)(r * FZ_ROW_BYTES + GRP * j + i);
                            while (__ballot(set != 0u)) {
                                const uint32_t gb = (uint32_t)__ffs((int)set) - 1u;       // (an empty set: 0xffffffff, never taken)
                                const bool take = set != 0u && (!ADAPT || gb - b0 < bw);
                                const unsigned long long mk = __ballot(take);
                                const uint32_t slot = qn + fz_rank(mk);
                                if (take && slot < qcap) w.queue[slot] = fz_code(pos, gb, titer);
                                qn += (uint32_t)__popcll(mk);
                                set &= set - 1u;
                            }
                        } else if constexpr (ADAPT) {
                            // only the blocks of this pass over the tile (b0, bw below): g = 0xff (a free slot) never passes
                            const bool take = hv[i] == lv[i] && g - b0 < bw;
                            const unsigned long long mt = __ballot(take);
                            const uint32_t slot = qn + fz_rank(mt);
                            if (take && slot < qcap)
                                w.queue[slot] = fz_code(pos + (uint32_t)(r * FZ_ROW_BYTES + GRP * j + i), g, titer);
                            qn += (uint32_t)__popcll(mt);
                        } else {
                            const uint32_t slot = qn + fz_rank(mi);
                            if (hv[i] == lv[i] && slot < qcap)
                                w.queue[slot] = fz_code(pos + (uint32_t)(r * FZ_ROW_BYTES + GRP * j + i), g, titer);
                            qn += (uint32_t)__popcll(mi);
                        }
                    }
                }
            }
        }
    };

    for (;;) {
        if (slow) {
            // enumerate (row, offset, block) candidates of this step's tile, 64 lanes at a time
            const uint32_t nb = ADAPT ? min(bw, a.nblk - b0) : a.nblk;      // (bit-vector form: the blocks of this pass)
            const uint32_t steps = FZ_FILTER_ROWS * 16u * nb;
            while (slow_pos < steps && qn + 64u <= qcap) {
                const uint32_t blk = (ADAPT ? b0 : 0u) + slow_pos % nb;
                const uint32_t ro = slow_pos / nb;
                w.queue[qn + lane] = fz_code((ro >> 4) * FZ_ROW_BYTES + lane_off + (ro & 15u), blk, titer);
                qn += 64u;
                ++slow_pos;
            }
            if (slow_pos >= steps) {
                slow = false;
                if (ADAPT && b0 + bw < a.nblk) b0 += bw;
                else { b0 = 0; left -= stride; ptile += (uint32_t)pstride; ++titer; }
            }
        } else if (left > 0 && (ADAPT ? (qn == 0u || qn + ylast + (ylast >> 2) + 8u <= qcap) : qn <= qcap / 2)) {
            uint4 va[2], vb[2];
            uint2 ha[2], hb[2];
            bool pre;                                 // va / ha hold rows 0-1 of the next tile
            {
                const uint8_t *tsrc = buf + fz_bcast64((uint64_t)ptile * FZ_TILE_BYTES);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    va[r] = *reinterpret_cast<const uint4 *>(tsrc + r * FZ_ROW_BYTES + lane_off);
                    ha[r] = *reinterpret_cast<const uint2 *>(tsrc + r * FZ_ROW_BYTES + lane_off + 16);
                }
            }
            do {
                const uint8_t *tsrc = buf + fz_bcast64((uint64_t)ptile * FZ_TILE_BYTES);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    vb[r] = *reinterpret_cast<const uint4 *>(tsrc + (r + 2) * FZ_ROW_BYTES + lane_off);
                    hb[r] = *reinterpret_cast<const uint2 *>(tsrc + (r + 2) * FZ_ROW_BYTES + lane_off + 16);
                }
                __builtin_amdgcn_sched_barrier(0);    // all loads are issued before the first use
                const uint32_t q_tile = qn;
                test_row(va[0], ha[0], std::integral_constant<int, 0>{});
                test_row(va[1], ha[1], std::integral_constant<int, 1>{});
                const bool same_tile = ADAPT && b0 + bw < a.nblk;       // the next pass is over this tile again (its other blocks)
                // (wave-uniform: pinned to scalar registers, which `same_tile` alone does not tell the compiler)
                const int32_t lnext = same_tile ? left : left - stride;
                const uint32_t pnext = fz_uniform(same_tile ? ptile : ptile + (uint32_t)pstride);
                if constexpr (ADAPT) pre = lnext > 0 && qn + 3u * (qn - q_tile) + 8u <= qcap;   // this pass's second half + the next pass
                else pre = lnext > 0 && qn <= qcap / 2;
                {   // unconditional (a branch here would make the compiler wait for the prefetch at the join):
                    // without a next tile the loads re-read this one (L2 hits, results unused)
                    const uint8_t *nsrc = buf + fz_bcast64((uint64_t)(pre ? pnext : ptile) * FZ_TILE_BYTES);
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        va[r] = *reinterpret_cast<const uint4 *>(nsrc + r * FZ_ROW_BYTES + lane_off);
                        ha[r] = *reinterpret_cast<const uint2 *>(nsrc + r * FZ_ROW_BYTES + lane_off + 16);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                test_row(vb[0], hb[0], std::integral_constant<int, 2>{});
                test_row(vb[1], hb[1], std::integral_constant<int, 3>{});
                if (qn > qcap) {                      // this tile overflowed the queue: drop its
                    qn = q_tile;                      // partial entries and re-scan it by enumeration
                    if constexpr (ADAPT) {        // ... or, bit-vector form:
                        if (q_tile != 0u) {           // once more behind a flush of what the queue held,
                            ylast = qcap;
                            break;
                        }
                        const uint32_t nb = min(bw, a.nblk - b0);
                        if (nb > 1u) {                // once more for half of the blocks (the queue is empty: no flush)
                            bw = (nb + 1u) >> 1;
                            ylast = qcap >> 1;
                            break;
                        }
                    }
                    slow = true;
                    slow_pos = 0;
                    break;
                }
                if constexpr (ADAPT) ylast = qn - q_tile;
                if (PREF && qn > qf) {
                    if (ptile) fz_prefetch_tile(buf, a, w, qf, qn, (uint64_t)ptile * FZ_TILE_BYTES);
                    else fz_prefetch_windows(buf, a, w, qf, qn);          // the buffer's first tile (a reversed walk's last): windows clamped at the start
                    qf = qn;
                }
                if constexpr (ADAPT) {
                    if (same_tile) {
                        b0 += bw;
                    } else {
                        b0 = 0;
                        if (bw < a.nblk && ylast <= (qcap >> 3)) bw <<= 1;   // little queued: twice the blocks per pass from the next tile on
                        left = lnext;
                        ptile = pnext;
                        ++titer;
                    }
                } else {
                    left = lnext;
                    ptile = pnext;
                    ++titer;
                }
            } while (pre);                            // else: the end of the sequence, or a flush is due
        }
        const bool done = !slow && left <= 0;
        if (PREF && done) break;                      // what is queued now is verified by the pooled flush below
        if constexpr (WF) {
            // lane-per-cell verification (Levenshtein budgets 5 .. 15): own queue in mid-scan, the workgroup's pool at the end
            confirmed += fz_flush_wf<WF ? WFG : 16, RAG>(buf, a, smem, pat_lds, w, smem + FZ_TABLE_BYTES + mpad,
                                                    fz_wave_lds_bytes(fz_wf_fused_dwords(a.win_dwords, WF ? WFG : 16), 0u, 1u, true),
                                                    reinterpret_cast<volatile uint32_t *>(smem + 2u * FZ_LUT_BYTES), wave, qn, done, recs, counters);
        } else if (qn) {
            if (PREF && qn > qf) fz_prefetch_windows(buf, a, w, qf, qn);
            if constexpr (ADAPT) {
                confirmed += fz_bits_flush<VF, RAG>(buf, a, pat_lds, smem + FZ_TABLE_BYTES + mpad, w, qn, recs, counters);
                qf = qn;                              // what stays queued has its window
                continue;
            } else {
                confirmed += fz_queue_flush<FUSED, SEG, RAG, MAXK>(buf, a, pat_lds, w, qn, hits, recs, counters);
            }
        }
        qn = 0;
        qf = 0;
        if (done) break;
    }
    if constexpr (PREF) {
        if (qn > qf) fz_prefetch_windows(buf, a, w, qf, qn);
        confirmed += fz_pooled_flush<MAXK, VF, RAG>(buf, a, pat_lds, smem + FZ_TABLE_BYTES + mpad + peq_bytes, fz_wave_lds_pref_bytes(qcap, a.win_pieces),
                                              reinterpret_cast<volatile uint32_t *>(smem + 2u * FZ_LUT_BYTES), wave, qn, recs, counters,
                                              smem + FZ_TABLE_BYTES + mpad);
    }

    // (measured and not kept: one no-return atomic per workgroup — ticket and tallies in one word — with the last-indexed
    // workgroup polling for the others instead of every workgroup waiting for its ticket: 0.2172 vs 0.2183 ms, within noise)
    if (FUSED && lane == 0 && confirmed) atomicAdd(&counters[8 + (blockIdx.x & 63u)], (unsigned long long)confirmed);
    fz_finish_launch(a, counters, lut);
#elif FZ_KERNEL_BODY == 2    // ---- fz_verify_kernel / fz_batch_verify_kernel
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t mpad = (a.m + 15u) & ~15u;
    uint8_t *pat_lds = smem;
    fz_copy_pattern(pat_lds, a, threadIdx.x, blockDim.x);
    __syncthreads();
    const FzWaveLds w = fz_wave_lds(smem + mpad, threadIdx.x >> 6, a.win_dwords, a.band_w, a.vlanes, false);
    unsigned long long nh = counters[0];
    if (nh > a.hit_cap) nh = a.hit_cap;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint32_t ncand = fz_segment_candidates_of<RAG>(a.geom);
    for (uint64_t q0 = wave * a.vlanes; q0 < nh; q0 += waves * a.vlanes) {
        const uint64_t q = q0 + fz_lane();
        const bool have = fz_lane() < a.vlanes && q < nh;
        const uint64_t hit = have ? hits[q] : 0;
        for (uint32_t c = 0; c < ncand; ++c) {
            const FzSeg sg = fz_segment_of<RAG>(a.geom, fz_hit_index(hit), c);
            const bool valid = have && fz_hit_in_range_s(a, fz_hit_block(hit) * a.L, fz_hit_index(hit), sg);
            if (!__ballot(valid)) continue;
            fz_wave_verify<FZ_REG_BAND_MAX, false>(buf, a, pat_lds, w, fz_lane(), hit, sg, valid, recs, counters);
        }
    }
    fz_finish_launch(a, counters, reinterpret_cast<uint32_t *>(smem));
#elif FZ_KERNEL_BODY == 3    // ---- fz_verify_wf_kernel / fz_batch_verify_wf_kernel
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr uint32_t NH = 64u / (uint32_t)GW;                         // hits per wave
    const uint32_t mpad = (a.m + 15u) & ~15u;
    uint8_t *pat_lds = smem + 16;                                       // 16 bytes of slack below p[0] (reversed reads)
    fz_copy_pattern(pat_lds, a, threadIdx.x, blockDim.x);
    __syncthreads();
    const uint32_t lane = fz_lane();
    const uint32_t grp = lane / (uint32_t)GW, gl = lane % (uint32_t)GW;
    const uint32_t wbytes = a.win_dwords * 4u;
    uint8_t *gwin = smem + 16 + mpad + 16 + ((threadIdx.x >> 6) * NH + grp) * (wbytes + 16u);
    unsigned long long nh = counters[0];
    if (nh > a.hit_cap) nh = a.hit_cap;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint32_t ncand = fz_segment_candidates_of<RAG>(a.geom);
    // workgroups without a hit leave at once and take no finish ticket (a ticket is an atomic on one word)
    const uint64_t per_wg = (uint64_t)NH * (blockDim.x >> 6);
    uint32_t active_wgs = (uint32_t)((nh + per_wg - 1) / per_wg < gridDim.x ? (nh + per_wg - 1) / per_wg : gridDim.x);
    if (active_wgs == 0) active_wgs = 1;
    if (blockIdx.x >= active_wgs) return;
    const bool compact = nh * ncand > FZ_WF_COMPACT_MIN;               // (uniform: every wave takes the same form)
    for (uint64_t q0 = wave * NH; q0 < nh; q0 += waves * NH) {
        const uint64_t q = q0 + grp;
        const bool have = q < nh;
        const uint64_t hit = have ? hits[q] : 0;
        const uint32_t g = fz_hit_block(hit);
        const uint64_t idx = fz_hit_index(hit);
        const uint32_t s = g * a.L;
        for (uint32_t c = 0; c < ncand; ++c) {
            const FzSeg sg = fz_segment_of<RAG>(a.geom, idx, c);
            const bool valid = have && fz_hit_in_range_s(a, s, idx, sg);
            const unsigned long long slot = q * ncand + c;
            if (!compact && have && !valid && gl == 0 && slot < a.rec_cap) recs[slot].dist = FZ_REC_NONE;   // not a hit of this segment
            if (!__ballot(valid)) continue;
            // the hit's window [wlo, whi), staged as plain bytes: byte g of the sequence at gwin[g - wbase]
            uint64_t wlo = 0, whi = 0, wbase = 0;
            if (valid) {
                const uint64_t reach = (uint64_t)s + a.k;
                wlo = idx - sg.sa > reach ? idx - reach : sg.sa;
                if (wlo < a.geom.buf_off) wlo = a.geom.buf_off;
                whi = idx - s + a.m + a.k;
                const uint64_t lim = a.geom.buf_off + a.geom.buf_len;
                if (whi > lim) whi = lim;
                if (whi > sg.se) whi = sg.se;
                wbase = a.geom.buf_off + ((wlo - a.geom.buf_off) & ~(uint64_t)3);
            }
            const uint32_t nd = valid ? (uint32_t)((whi - wbase + 3) >> 2) : 0u;
            const int64_t lbase = (int64_t)(wbase - a.geom.buf_off);
            for (uint32_t dd = gl; dd < nd; dd += (uint32_t)GW)
                reinterpret_cast<uint32_t *>(gwin)[dd] = *reinterpret_cast<const uint32_t *>(buf + lbase + (int64_t)dd * 4);
            fz_wave_lds_sync();
            // LDS byte offsets relative to smem (invalid groups read offset 0)
            const int wrel = (int)(gwin - smem);
            auto lds_of = [&](uint64_t gidx) -> int { return valid ? wrel + (int)(int64_t)(gidx - wbase) : 0; };
            // right: p[s+L:] vs t[idx+L : min(se, idx-s+m+k)]
            uint64_t rbeg = idx + a.L, rend = idx + a.m + a.k - s;
            if (rend > sg.se) rend = sg.se;
            if (rbeg > sg.se) rbeg = sg.se;
            if (rend < rbeg) rend = rbeg;
            const uint32_t rwin = (uint32_t)(rend - rbeg), rlen = a.m - s - a.L;
            uint32_t dR = 0, r = 0, dL = 0, l = 0;
            const uint32_t cellr = fz_wf_rows<GW>(smem, gl, a.k, (int)(pat_lds - smem) + (int)(s + a.L), 1, rlen, lds_of(rbeg), 1, rwin,
                                                  a.k, valid);
            const bool ok1 = fz_wf_pick<GW>(cellr, gl, a.k, rlen, rwin, a.k, valid, dR, r);
            // left: reversed p[:s] vs reversed t[max(sa, idx-s-(k-dR)) : idx], budget k - dR
            const uint32_t bl = ok1 ? a.k - dR : 0u;
            const uint64_t want = (uint64_t)s + bl;
            const uint64_t lbeg = (idx - sg.sa > want) ? idx - want : sg.sa;
            const uint32_t lwin = ok1 ? (uint32_t)(idx - lbeg) : 0u;
            const uint32_t celll = fz_wf_rows<GW>(smem, gl, a.k, (int)(pat_lds - smem) + (int)s - 1, -1, s, lds_of(idx) - 1, -1, lwin,
                                                  bl, ok1);
            const bool ok = fz_wf_pick<GW>(celll, gl, a.k, s, lwin, bl, ok1, dL, l);
            if (!compact) {
                if (valid && gl == 0 && slot < a.rec_cap) {
                    FzRec rec;
                    rec.key = hit; rec.l = l; rec.r = r; rec.dist = ok ? dL + dR : FZ_REC_NONE; rec.aux = sg.j;
                    recs[slot] = rec;
                }
            } else {
                const bool mine = ok && gl == 0;
                const unsigned long long mask = __ballot(mine);
                if (mask) {
                    unsigned long long base = 0;
                    if (lane == 0) base = atomicAdd(&counters[1], (unsigned long long)__popcll(mask));
                    base = fz_bcast64(base);
                    const unsigned long long at = base + fz_rank(mask);
                    if (mine && at < a.rec_cap) {
                        FzRec rec;
                        rec.key = hit; rec.l = l; rec.r = r; rec.dist = dL + dR; rec.aux = sg.j;
                        recs[at] = rec;
                    }
                }
            }
            fz_wave_lds_sync();
        }
    }
    // the record count the host sees = number of slots (or of appended records); only workgroups that had hits take a finish ticket
    if (!compact && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&counters[1], nh * ncand);
    fz_finish_launch(a, counters, reinterpret_cast<uint32_t *>(smem), active_wgs);
#elif FZ_KERNEL_BODY == 4    // ---- fz_verify_big_kernel / fz_batch_verify_big_kernel
    __shared__ uint32_t flag;
    const uint32_t lane = fz_lane();
    const uint8_t *pat = reinterpret_cast<const uint8_t *>(a.pat_g);   // the host stages the pattern in HBM for this kernel
    unsigned long long nh = counters[0];
    if (nh > a.hit_cap) nh = a.hit_cap;
    const uint32_t ncand = fz_segment_candidates_of<RAG>(a.geom);
    for (uint64_t q = blockIdx.x; q < nh; q += gridDim.x) {
        const uint64_t hit = hits[q];
        const uint32_t g = fz_hit_block(hit);
        const uint64_t idx = fz_hit_index(hit);
        const uint32_t s = g * a.L;
        for (uint32_t c = 0; c < ncand; ++c) {
            const FzSeg sg = fz_segment_of<RAG>(a.geom, idx, c);
            if (!fz_hit_in_range_s(a, s, idx, sg)) continue;                               // wave-uniform
            FzRec rec;
            bool ok;
            if (a.mode == FZ_MODE_SUBS) {
                // Hamming distance of the window [idx - s, idx - s + m) (_substitutions_only_ngrams_template.h:103-121)
                const uint8_t *t = buf + (int64_t)(idx - s - a.geom.buf_off);
                uint32_t nd = 0;
                for (uint32_t q0 = 0; q0 < a.m; q0 += 4096u) {
                    for (uint32_t qq = q0 + lane; qq < a.m && qq < q0 + 4096u; qq += 64u) nd += (pat[qq] != t[qq]) ? 1u : 0u;
                    if (!__ballot(nd <= a.k)) break;                                        // some lane alone is over the budget
                }
                uint32_t tot = nd;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) tot += (uint32_t)__shfl_xor((int)tot, d, 64);
                ok = tot <= a.k;                                                            // (after an early exit tot is partial, but > k)
                rec.l = s; rec.r = a.m - s - a.L; rec.dist = tot;
            } else {
                // levenshtein_ngram.py:177-198: right expansion with budget k, then left with what is left of it
                const uint32_t rlen = a.m - s - a.L;
                uint64_t rbeg = idx + a.L, rend = idx + a.m + a.k - s;
                if (rend > sg.se) rend = sg.se;
                if (rbeg > sg.se) rbeg = sg.se;
                if (rend < rbeg) rend = rbeg;
                uint32_t dR = 0, r = 0, dL = 0, l = 0;
                ok = fz_big_expand<CPL>(pat + s + a.L, 1, rlen, buf + (int64_t)(rbeg - a.geom.buf_off), 1, (uint32_t)(rend - rbeg),
                                        a.k, a.k, dR, r);
                if (ok) {
                    const uint32_t bl = a.k - dR;
                    const uint64_t want = (uint64_t)s + bl;
                    const uint64_t lbeg = (idx - sg.sa > want) ? idx - want : sg.sa;
                    ok = fz_big_expand<CPL>(pat + s - 1, -1, s, buf + (int64_t)(idx - a.geom.buf_off) - 1, -1, (uint32_t)(idx - lbeg),
                                            a.k, bl, dL, l);
                }
                rec.l = l; rec.r = r; rec.dist = dL + dR;
            }
            if (ok && lane == 0) {
                const unsigned long long slot = atomicAdd(&counters[1], 1ull);
                rec.key = hit;
                rec.aux = sg.j;
                if (slot < a.rec_cap) recs[slot] = rec;
            }
        }
    }
    fz_finish_launch(a, counters, &flag);
#elif FZ_KERNEL_BODY == 5    // ---- fz_mp_verify_kernel / fz_mp_batch_verify_kernel
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t *tab = reinterpret_cast<uint32_t *>(smem);
    for (uint32_t i = threadIdx.x; i < FZ_MP_VERIFY_WORDS; i += FZ_FILTER_THREADS) tab[i] = desc[FZ_MP_DESC_ENT + i];
    __syncthreads();
    const uint32_t *ent = tab;
    const uint32_t *pm = tab + (FZ_MP_DESC_M - FZ_MP_DESC_ENT);
    const uint8_t *pats = reinterpret_cast<const uint8_t *>(tab + (FZ_MP_DESC_PAT - FZ_MP_DESC_ENT));
    const uint32_t lane = fz_lane();
    uint8_t *wbytes = smem + FZ_MP_VERIFY_WORDS * 4u + (threadIdx.x >> 6) * fz_mp_verify_wave_bytes(a.win_dwords);
    uint32_t *win = reinterpret_cast<uint32_t *>(wbytes);
    uint16_t *ring = reinterpret_cast<uint16_t *>(wbytes + a.win_dwords * 256u);
    const uint64_t waves = (uint64_t)gridDim.x * FZ_WAVES_PER_BLOCK;
    const uint64_t wave = (uint64_t)blockIdx.x * FZ_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const uint64_t n = a.geom.n;
    const uint64_t data_end = a.geom.buf_off + a.geom.buf_len;
    uint32_t confirmed = 0;
    for (uint32_t l = 0; l < FZ_MP_LISTS; ++l) {
        unsigned long long nh = counters[FZ_MP_CTR_LIST(l)];
        if (nh > a.hit_cap) nh = a.hit_cap;
        const uint64_t *lh = hits + (uint64_t)l * a.hit_cap;
        // (the lists start at different waves: a short list keeps other waves busy than its neighbour's)
        for (uint64_t q0 = ((wave + 251u * l) % waves) * 64u; q0 < nh; q0 += waves * 64u) {
            const uint64_t q = q0 + lane;
            const bool have = q < nh;
            const uint64_t hit = have ? lh[q] : 0ull;
            const uint32_t e = ent[fz_hit_block(hit) & (FZ_MP_MAX_BLOCKS - 1u)];
            const uint32_t pid = e & 0xffu, g = (e >> 8) & 0xffu, s = e >> 16;
            const uint32_t m = pm[pid & (FZ_MP_MAX_PATS - 1u)];
            const uint8_t *p = pats + (pid & (FZ_MP_MAX_PATS - 1u)) * FZ_MP_MAX_M;
            const uint64_t idx = fz_hit_index(hit);
            bool valid;
            // the window staged, and the sequence the candidate is verified in.  (Initialised: left undefined until the branch
            // below, they moved the SGPR allocation of the unsegmented kernel.)
            uint64_t wlo = 0, whi = 0, wbase = 0, sa = 0, se = 0;
            if constexpr (RAG) {
                // the candidate's own sequence: one lookup per lane (a binary search bounded by the tile index, ~7 dependent
                // loads for 150-byte reads), before anything is staged; then the block's range, ownership and the window's
                // clamps inside [sg.sa, sg.se) (fz_mp_rag_accept).  An n-gram across a seam is rejected by the range test.
                valid = have && fz_hit_block(hit) < a.nent && m != 0u;
                FzSeg sg;
                sg.sa = sg.se = 0; sg.j = 0; sg.ok = 0;
                if (valid) sg = fz_segment_ragged(fz_ragged(a.geom), n, idx);
                FzMpRagCand c;
                valid = valid && fz_mp_rag_accept(FZ_MODE_LEV, a.geom, sg, m, a.k, a.L, s, idx, c);
                if (!__ballot(valid)) continue;
                wlo = c.wlo; whi = c.whi; sa = sg.sa; se = sg.se;
                wbase = a.geom.buf_off + ((wlo - a.geom.buf_off) & ~(uint64_t)3);
            } else {
                // acceptance range of the block (levenshtein_ngram.py:171-176) in the whole sequence [0, n), and ownership
                uint32_t lo_rel, hi_sub;
                fz_block_range(FZ_MODE_LEV, m, a.k, a.L, s, lo_rel, hi_sub);
                valid = have && fz_hit_block(hit) < a.nent && m != 0u && idx >= lo_rel && n >= hi_sub && idx + a.L <= n - hi_sub &&
                        idx >= a.geom.own_lo && idx < a.geom.own_hi && idx >= a.geom.buf_off && idx + a.L <= data_end;
                if (!__ballot(valid)) continue;
                // the window [max(0, idx - s - k), min(n, idx - s + m + k)) clipped to the buffer, dword-aligned, into LDS
                const uint64_t reach = (uint64_t)s + a.k;
                wlo = idx > reach ? idx - reach : 0ull;
                if (wlo < a.geom.buf_off) wlo = a.geom.buf_off;
                wbase = a.geom.buf_off + ((wlo - a.geom.buf_off) & ~(uint64_t)3);
                whi = idx - s + m + a.k;
                if (whi > data_end) whi = data_end;
                if (whi > n) whi = n;
                sa = 0ull; se = n;
            }
            uint32_t nd = valid ? (uint32_t)((whi - wbase + 3) >> 2) : 0u;
            if (nd > a.win_dwords) nd = a.win_dwords;
            const int64_t lbase = (int64_t)(wbase - a.geom.buf_off);
            for (uint32_t d0 = 0; d0 < a.win_dwords; d0 += 8) {
                uint32_t x[8];
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j)
                    x[j] = (d0 + j < nd) ? *reinterpret_cast<const uint32_t *>(buf + lbase + (int64_t)(d0 + j) * 4) : 0u;
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j)
                    if (d0 + j < nd) win[(d0 + j) * 64u + lane] = x[j];
            }
            fz_wave_lds_sync();
            const FzLdsWindow t{reinterpret_cast<const uint8_t *>(win + lane), wbase, 256u};
            if (valid) {
                const uint8_t *ng = p + s;
                for (uint32_t b = 0; b < a.L; ++b)
                    if (ng[b] != t.at(idx + b)) { valid = false; break; }
            }
            confirmed += (uint32_t)__popcll(__ballot(valid));
            FzRec rec;
            bool ok = false;
            if (valid) {
                FzLdsScores sc{ring + lane, 64u};
                if constexpr (RAG) ok = fz_verify_lev<FZ_REG_BAND_MAX>(sc, t, sa, se, p, m, a.k, a.L, s, idx, rec);
                else ok = fz_verify_lev<FZ_REG_BAND_MAX>(sc, t, 0ull, n, p, m, a.k, a.L, s, idx, rec);
            }
            const unsigned long long mask = __ballot(ok);
            if (mask) {
                unsigned long long base = 0;
                if (lane == 0) base = atomicAdd(&counters[FZ_MP_CTR_RECS], (unsigned long long)__popcll(mask));
                base = fz_bcast64(base);
                if (ok) {
                    rec.key = fz_hit_pack(g, idx);
                    rec.aux = pid;
                    const unsigned long long slot = base + fz_rank(mask);
                    if (slot < a.rec_cap) recs[slot] = rec;
                }
            }
            fz_wave_lds_sync();
        }
    }
    if (lane == 0 && confirmed) atomicAdd(&counters[8u + (blockIdx.x & 63u)], (unsigned long long)confirmed);
#elif FZ_KERNEL_BODY == 6    // ---- fz_mp_verify_subs_kernel / fz_mp_batch_verify_subs_kernel
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t *tab = reinterpret_cast<uint32_t *>(smem);
    constexpr uint32_t kPat = FZ_MP_DESC_PAT - FZ_MP_DESC_ENT, kRow = FZ_MP_MAX_M / 4u;
    static_assert(FZ_MP_MAX_PATS == 64u, "the transposed pattern table has one column per pattern");
    for (uint32_t i = threadIdx.x; i < FZ_MP_VERIFY_WORDS; i += FZ_FILTER_THREADS) {
        const uint32_t v = desc[FZ_MP_DESC_ENT + i];
        if (i < kPat) tab[i] = v;
        else tab[kPat + ((i - kPat) % kRow) * FZ_MP_MAX_PATS + (i - kPat) / kRow] = v;
    }
    __syncthreads();
    const uint32_t *ent = tab;
    const uint32_t *pm = tab + (FZ_MP_DESC_M - FZ_MP_DESC_ENT);
    const uint32_t *pat4 = tab + kPat;
    const uint32_t lane = fz_lane();
    uint32_t *win = reinterpret_cast<uint32_t *>(smem + FZ_MP_VERIFY_WORDS * 4u) + (threadIdx.x >> 6) * a.win_dwords * 64u;
    const uint32_t m_max = (a.win_dwords - 1u) * 4u;       // (the longest pattern rounded up to dwords)
    const uint64_t waves = (uint64_t)gridDim.x * FZ_WAVES_PER_BLOCK;
    const uint64_t wave = (uint64_t)blockIdx.x * FZ_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const uint64_t n = a.geom.n;
    const uint64_t data_end = a.geom.buf_off + a.geom.buf_len;
    uint32_t confirmed = 0;
    for (uint32_t l = 0; l < FZ_MP_LISTS; ++l) {
        unsigned long long nh = counters[FZ_MP_CTR_LIST(l)];
        if (nh > a.hit_cap) nh = a.hit_cap;
        const uint64_t *lh = hits + (uint64_t)l * a.hit_cap;
        for (uint64_t q0 = ((wave + 251u * l) % waves) * 64u; q0 < nh; q0 += waves * 64u) {
            const uint64_t q = q0 + lane;
            const bool have = q < nh;
            const uint64_t hit = have ? lh[q] : 0ull;
            const uint32_t e = ent[fz_hit_block(hit) & (FZ_MP_MAX_BLOCKS - 1u)];
            const uint32_t pid = e & (FZ_MP_MAX_PATS - 1u), g = (e >> 8) & 0xffu, s = e >> 16;
            const uint32_t m = pm[pid];
            const uint64_t idx = fz_hit_index(hit);
            bool valid;
            if constexpr (RAG) {
                // the candidate's own sequence (one lookup per lane, before anything is staged), then the window
                // [idx - s, idx - s + m) inside it, ownership, the whole window resident (fz_mp_rag_accept)
                valid = have && fz_hit_block(hit) < a.nent && m != 0u && m <= m_max && s + a.L <= m;
                FzSeg sg;
                sg.sa = sg.se = 0; sg.j = 0; sg.ok = 0;
                if (valid) sg = fz_segment_ragged(fz_ragged(a.geom), n, idx);
                FzMpRagCand c;
                valid = valid && fz_mp_rag_accept(FZ_MODE_SUBS, a.geom, sg, m, a.k, a.L, s, idx, c);
            } else {
                // the block's hit range (template.h:97-101): s <= idx and idx - s + m <= n; ownership; the whole window resident
                uint32_t lo_rel, hi_sub;
                fz_block_range(FZ_MODE_SUBS, m, a.k, a.L, s, lo_rel, hi_sub);
                valid = have && fz_hit_block(hit) < a.nent && m != 0u && m <= m_max && s + a.L <= m &&
                        idx >= lo_rel && n >= hi_sub && idx + a.L <= n - hi_sub &&
                        idx >= a.geom.own_lo && idx < a.geom.own_hi && idx - lo_rel >= a.geom.buf_off && idx + a.L + hi_sub <= data_end;
            }
            if (!__ballot(valid)) continue;
            const uint64_t i0 = valid ? idx - s : a.geom.buf_off;
            const uint64_t wbase = a.geom.buf_off + ((i0 - a.geom.buf_off) & ~(uint64_t)3);
            const uint32_t sh = (uint32_t)(i0 - wbase);
            uint32_t nd = valid ? (uint32_t)((i0 + m - wbase + 3) >> 2) : 0u;      // <= (m + 6) / 4 <= win_dwords
            if (nd > a.win_dwords) nd = a.win_dwords;
            const int64_t lbase = (int64_t)(wbase - a.geom.buf_off);
            for (uint32_t d0 = 0; d0 < a.win_dwords; d0 += 8) {
                uint32_t x[8];
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j)
                    x[j] = (d0 + j < nd) ? *reinterpret_cast<const uint32_t *>(buf + lbase + (int64_t)(d0 + j) * 4) : 0u;
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j)
                    if (d0 + j < a.win_dwords) win[(d0 + j) * 64u + lane] = x[j];
            }
            fz_wave_lds_sync();
            const FzLdsColumn t{win + lane};
            const uint32_t *p4 = pat4 + pid;
            valid = valid && fz_mp_block_equal(t, sh, p4, FZ_MP_MAX_PATS, a.L, valid ? s : 0u);
            confirmed += (uint32_t)__popcll(__ballot(valid));
            FzRec rec;
            const bool ok = fz_mp_verify_subs(t, sh, p4, FZ_MP_MAX_PATS, m, m_max, a.k, a.L, s, valid, rec);
            const unsigned long long mask = __ballot(ok);
            if (mask) {
                unsigned long long base = 0;
                if (lane == 0) base = atomicAdd(&counters[FZ_MP_CTR_RECS], (unsigned long long)__popcll(mask));
                base = fz_bcast64(base);
                if (ok) {
                    rec.key = fz_hit_pack(g, idx);
                    rec.aux = pid;
                    const unsigned long long slot = base + fz_rank(mask);
                    if (slot < a.rec_cap) recs[slot] = rec;
                }
            }
            fz_wave_lds_sync();
        }
    }
    if (lane == 0 && confirmed) atomicAdd(&counters[8u + (blockIdx.x & 63u)], (unsigned long long)confirmed);
#elif FZ_KERNEL_BODY == 7    // ---- fz_mp_verify_cls_kernel / fz_mp_batch_verify_cls_kernel
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t *tab = reinterpret_cast<uint32_t *>(smem);
    constexpr uint32_t kPat = FZ_MP_DESC_PAT - FZ_MP_DESC_ENT, kRow = FZ_MP_MAX_M / 4u, kRows = FZ_MP_MAX_PATS * kRow;
    constexpr uint32_t kMsk = kPat + kRows, kTm = kMsk + kRows;
    static_assert(FZ_MP_MAX_PATS == 64u, "the transposed tables have one column per pattern");
    static_assert(kTm == FZ_MP_CLS_DESC_TMASK - FZ_MP_DESC_ENT && kTm + 64u == FZ_MP_CLS_VERIFY_WORDS, "the class descriptor's layout");
    for (uint32_t i = threadIdx.x; i < FZ_MP_CLS_VERIFY_WORDS; i += FZ_FILTER_THREADS) {
        const uint32_t v = desc[FZ_MP_DESC_ENT + i];
        if (i < kPat || i >= kTm) tab[i] = v;
        else {                                             // pattern rows, then mask rows: both transposed
            const uint32_t base = i < kMsk ? kPat : kMsk, r = i - base;
            tab[base + (r % kRow) * FZ_MP_MAX_PATS + r / kRow] = v;
        }
    }
    __syncthreads();
    const uint32_t *ent = tab;
    const uint32_t *pm = tab + (FZ_MP_DESC_M - FZ_MP_DESC_ENT);
    const uint32_t *pat4 = tab + kPat;
    const uint32_t *msk4 = tab + kMsk;
    const uint8_t *tmask = reinterpret_cast<const uint8_t *>(tab + kTm);
    const uint32_t lane = fz_lane();
    uint32_t *win = reinterpret_cast<uint32_t *>(smem + FZ_MP_CLS_VERIFY_WORDS * 4u) + (threadIdx.x >> 6) * a.win_dwords * 64u;
    const uint32_t m_max = (a.win_dwords - 1u) * 4u;       // (the longest pattern rounded up to dwords)
    const uint64_t waves = (uint64_t)gridDim.x * FZ_WAVES_PER_BLOCK;
    const uint64_t wave = (uint64_t)blockIdx.x * FZ_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const uint64_t n = a.geom.n;
    const uint64_t data_end = a.geom.buf_off + a.geom.buf_len;
    uint32_t confirmed = 0;
    for (uint32_t l = 0; l < FZ_MP_LISTS; ++l) {
        unsigned long long nh = counters[FZ_MP_CTR_LIST(l)];
        if (nh > a.hit_cap) nh = a.hit_cap;
        const uint64_t *lh = hits + (uint64_t)l * a.hit_cap;
        for (uint64_t q0 = ((wave + 251u * l) % waves) * 64u; q0 < nh; q0 += waves * 64u) {
            const uint64_t q = q0 + lane;
            const bool have = q < nh;
            const uint64_t hit = have ? lh[q] : 0ull;
            const uint32_t e = ent[fz_hit_block(hit) & (FZ_MP_MAX_BLOCKS - 1u)];
            const uint32_t pid = e & (FZ_MP_MAX_PATS - 1u), g = (e >> 8) & 0xffu, s = e >> 16;
            const uint32_t m = pm[pid];
            const uint64_t idx = fz_hit_index(hit);
            bool valid;
            if constexpr (RAG) {
                // the candidate's own sequence, then the window [idx - s, idx - s + m) inside it, ownership, the whole
                // window resident (fz_mp_rag_accept: the substitutions acceptance — a class changes no window)
                valid = have && fz_hit_block(hit) < a.nent && m != 0u && m <= m_max && s + a.L <= m;
                FzSeg sg;
                sg.sa = sg.se = 0; sg.j = 0; sg.ok = 0;
                if (valid) sg = fz_segment_ragged(fz_ragged(a.geom), n, idx);
                FzMpRagCand c;
                valid = valid && fz_mp_rag_accept(FZ_MODE_SUBS, a.geom, sg, m, a.k, a.L, s, idx, c);
            } else {
                uint32_t lo_rel, hi_sub;
                fz_block_range(FZ_MODE_SUBS, m, a.k, a.L, s, lo_rel, hi_sub);
                valid = have && fz_hit_block(hit) < a.nent && m != 0u && m <= m_max && s + a.L <= m &&
                        idx >= lo_rel && n >= hi_sub && idx + a.L <= n - hi_sub &&
                        idx >= a.geom.own_lo && idx < a.geom.own_hi && idx - lo_rel >= a.geom.buf_off && idx + a.L + hi_sub <= data_end;
            }
            if (!__ballot(valid)) continue;
            const uint64_t i0 = valid ? idx - s : a.geom.buf_off;
            const uint64_t wbase = a.geom.buf_off + ((i0 - a.geom.buf_off) & ~(uint64_t)3);
            const uint32_t sh = (uint32_t)(i0 - wbase);
            uint32_t nd = valid ? (uint32_t)((i0 + m - wbase + 3) >> 2) : 0u;      // <= (m + 6) / 4 <= win_dwords
            if (nd > a.win_dwords) nd = a.win_dwords;
            const int64_t lbase = (int64_t)(wbase - a.geom.buf_off);
            for (uint32_t d0 = 0; d0 < a.win_dwords; d0 += 8) {
                uint32_t x[8];
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j)
                    x[j] = (d0 + j < nd) ? *reinterpret_cast<const uint32_t *>(buf + lbase + (int64_t)(d0 + j) * 4) : 0u;
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j)
                    if (d0 + j < a.win_dwords) win[(d0 + j) * 64u + lane] = x[j];
            }
            fz_wave_lds_sync();
            const FzLdsColumn t{win + lane};
            const uint32_t *p4 = pat4 + pid, *k4 = msk4 + pid;
            valid = valid && fz_mp_block_match_cls(t, sh, p4, k4, FZ_MP_MAX_PATS, tmask, a.L, valid ? s : 0u);
            confirmed += (uint32_t)__popcll(__ballot(valid));
            FzRec rec;
            const bool ok = fz_mp_verify_cls(t, sh, p4, k4, FZ_MP_MAX_PATS, tmask, m, m_max, a.k, a.L, s, valid, rec);
            const unsigned long long mask = __ballot(ok);
            if (mask) {
                unsigned long long base = 0;
                if (lane == 0) base = atomicAdd(&counters[FZ_MP_CTR_RECS], (unsigned long long)__popcll(mask));
                base = fz_bcast64(base);
                if (ok) {
                    rec.key = fz_hit_pack(g, idx);
                    rec.aux = pid;
                    const unsigned long long slot = base + fz_rank(mask);
                    if (slot < a.rec_cap) recs[slot] = rec;
                }
            }
            fz_wave_lds_sync();
        }
    }
    if (lane == 0 && confirmed) atomicAdd(&counters[8u + (blockIdx.x & 63u)], (unsigned long long)confirmed);
#else
#error "FZ_KERNEL_BODY names no section"
#endif
