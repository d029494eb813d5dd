// fz_kernels.h — hand-written HIP kernels for gfx950 (MI355X, CDNA4).  Included by fzhip.hip.
//
//   fz_scan_kernel    ONE streaming pass over the resident sequence:
//     K1 filter   every byte offset is tested against all G n-gram blocks at once (replaces G x
//                 search_exact_byteslike passes, _common.c:75-102 / memmem.c:92-160): a one-op
//                 hash of the first min(L,8) window bytes (v_alignbyte / v_mad_u32_u24) selects one
//                 of 32 slots of a table in LDS that holds the blocks' hashes (ds_read_b32: one slot
//                 per bank, so the lookup is bank-conflict free by construction), one v_xor
//                 compares, v_min3 accumulates, one ballot per 4 offsets: the cost does not depend
//                 on G; survivors go through a per-wave LDS queue to an exact re-check;
//     K2 verify   confirmed hits wait in a per-wave LDS staging area and are verified 64 at a
//                 time, one lane per hit, inside the same kernel: the <= m+2k window bytes are
//                 fetched once into LDS, then the bounded edit-distance expansion right and left
//                 (c_expand_*, _levenshtein_ngrams.pyx:9-154) or the Hamming count
//                 (_substitutions_only_ngrams_template.h:103-121) runs out of LDS / registers.
//                 Only match records leave the chip.
//                 (Measured and rejected in round 2, DESIGN.md §4: a persistent grid whose waves draw
//                 4 KiB chunks from ticket counters, and queueing only a fired group's position with
//                 the offset/block resolved at the flush — equal without candidates, 0.04 ms slower on
//                 DNA: every wave then flushes at the same time, at the end.)
//   fz_verify_kernel  the lane-per-candidate verification over a hit list in HBM, for parameter
//                 ranges that do not fit beside the filter (large m + 2k, budgets above 31).
//   fz_verify_wf_kernel  budgets 5..31: lane-per-DP-cell.  GW = 16 / 32 / 64 lanes own the 2k+1 band
//                 cells of one candidate's DP row; the left-neighbour recurrence is a prefix-min
//                 over the lanes (DPP row shifts), the upper neighbour one DPP shift.
//   fz_lp_kernel      one wave per work item: the reference's greedy candidate-set automata
//                 (generic search per n-gram hit; generic / Levenshtein linear-programming fallbacks
//                 tiled over the whole sequence), candidate lists in LDS, order preserved.
//   fz_hamming_kernel every window's Hamming distance (substitutions-only LP fallback).
//
// HBM-bound integer/byte work: no MFMA.  What matters (MI355X guide): 16-byte coalesced loads,
// >= 2048 workgroups' worth of loads in flight, no per-byte branching, n-gram constants in a
// 128-byte LDS table, wave-uniform rare paths, ONE global atomic per bulk append (a single counter
// word sustains only ~90 atomics/us chip-wide), no agent-scope fences.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <type_traits>
#include "fz_device.h"

#define FZ_FILTER_THREADS 256
#define FZ_WAVES_PER_BLOCK (FZ_FILTER_THREADS / 64)
#define FZ_FILTER_ROWS 4                                   // 16-byte rows per thread per tile
#define FZ_ROW_BYTES (FZ_FILTER_THREADS * 16)              // 4 KiB
#define FZ_TILE_BYTES (FZ_ROW_BYTES * FZ_FILTER_ROWS)      // 16 KiB (4 rows)
#define FZ_TILE_BITS 14                                    // log2(FZ_TILE_BYTES)
#define FZ_TITER_MAX ((1u << (32 - FZ_TILE_BITS - FZ_BLK_BITS)) - 1) // tile iterations a queue code can carry
#define FZ_PAD_FRONT 256                                   // zero bytes before buf[0]
#define FZ_PAD_BACK 256                                    // zero bytes the kernels may over-read (halo loads, whole 16-byte window pieces)
#ifndef FZ_GROUP
#define FZ_GROUP 0                                         // lab knob: force 4 or 8 byte offsets per wave-uniform branch (0: by n-gram length)
#endif
#define FZ_WF_COMPACT_MIN 8192ull                          // fz_verify_wf_kernel: record slots above which records are appended, not slotted
#define FZ_QCAP 256                                        // fast-hit queue entries per wave
#ifndef FZ_LUT_BITS
#define FZ_LUT_BITS 5                                      // 32 slots: one per LDS bank (6 = the round-1 table, 2-way conflicts)
#endif
#define FZ_LUT_SLOTS (1u << FZ_LUT_BITS)                   // slots of the block-hash table
#define FZ_LUT_BYTES (FZ_LUT_SLOTS * 4u)
#define FZ_TABLE_BYTES (2u * FZ_LUT_BYTES + 32u)           // the hash table + one dword per slot: the block that lives there,
                                                           // four dwords of the pooled flush, the workgroup's tile walk (below)
#define FZ_WALK_LDS (2u * FZ_LUT_BYTES + 16u)              // LDS address of {first tile, tile stride}: the scan kernel's
                                                           // dynamic LDS starts at address 0
                                                           // + the four waves' final queue fills (pooled last flush)
                                                           // (same byte offset as the hash: no address arithmetic in the rare path)
#define FZ_FLAG_DUP_HASHES 1u                              // FzScanArgs.flags: two blocks of the launch have the same hash
#define FZ_FLAG_FOLD 4u                                    // per-hit automaton: fold the matches of a hit into (hull, best match) pairs on
                                                           // the device (consolidate_overlapping_matches, common.py:145-189, first stage)
#define FZ_FLAG_ANY 2u                                     // has_near_match_*: the caller only asks WHETHER a record exists — work that starts
                                                           // after the first record has been counted is skipped
#define FZ_FLAG_REVERSE 8u                                 // the scan reads the mirror of every tile of its walk (fz_device.h: FzWalk): the
                                                           // workgroups that start first read the end of the buffer first
#if FZ_LUT_BITS == 5
#define FZ_LUT_ADDR_MASK_STR "0x7c"                        // (FZ_LUT_SLOTS - 1) * 4: byte address of a slot
#else
#define FZ_LUT_ADDR_MASK_STR "0xfc"
#endif

// 32-bit little-endian window starting `b` bytes into the 64-bit value hi:lo (v_alignbyte_b32).
__device__ __forceinline__ uint32_t fz_win(uint32_t lo, uint32_t hi, int b) {
    return b == 0 ? lo : __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)b);
}
#define FZ_WIN(w, o) fz_win((w)[(o) >> 2], (w)[((o) >> 2) + 1], (o) & 3)

typedef __attribute__((address_space(3))) const uint32_t FzLdsU32;   // LDS seen through a raw 32-bit LDS address
typedef __attribute__((address_space(3))) uint8_t FzLdsU8;

__device__ __forceinline__ uint32_t fz_lane() { return threadIdx.x & 63u; }

// The pattern into LDS: from the kernel-argument block, or (patterns longer than FZ_MAX_M, fz_verify_big_kernel's
// callers) from HBM.  Two loops under one uniform branch, NOT a select per byte between the two sources: a select
// between an argument-block address and a global one makes hipcc copy the whole 1.5 KB argument struct to scratch
// memory (1472 bytes per lane in every kernel that did it; the exact-search scan ran 3.4x slower).
__device__ __forceinline__ void fz_copy_pattern(uint8_t *dst, const FzScanArgs &a, uint32_t tid, uint32_t nthreads) {
    if (a.pat_g) {
        const uint8_t *pg = reinterpret_cast<const uint8_t *>(a.pat_g);
        for (uint32_t i = tid; i < a.m; i += nthreads) dst[i] = pg[i];
    } else {
        for (uint32_t i = tid; i < a.m; i += nthreads) dst[i] = a.pat[i];
    }
}

__device__ __forceinline__ uint32_t fz_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Make this wave's earlier LDS writes visible to its own later LDS reads (wave-synchronous code:
// no other wave shares these LDS regions, so no s_barrier is needed).
__device__ __forceinline__ void fz_wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// 32-bit window at an arbitrary (unaligned) local byte position: two aligned dword loads.
__device__ __forceinline__ uint32_t fz_load_win(const uint8_t *__restrict__ buf, int64_t local) {
    const int64_t base = local & ~(int64_t)3;
    const uint32_t lo = *reinterpret_cast<const uint32_t *>(buf + base);
    const uint32_t hi = *reinterpret_cast<const uint32_t *>(buf + base + 4);
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(local & 3));
}

// (The lab instrumentation of rounds 2 - 5 — device time stamps per workgroup phase / per n-gram hit, kernels with a part of
// the candidate handling left out, the miscompiled loop shape of fz_levlp_step_slots — is not in this file: benchmarks/
// lab_patches/lab_instrumentation.patch re-inserts it, benchmarks/lab_build.sh applies it to a scratch copy.)

// Per-wave LDS areas, carved from dynamic LDS by fz_wave_lds() / fz_wave_lds_pref().
struct FzWaveLds {
    uint32_t *queue;      // [qcap]  fast hits: tile-local offset | block << 14 | tile iteration << (14 + FZ_BLK_BITS)
    uint32_t *win;        // staged layout:     [win_dwords * vlanes]  dword d of the hit in slot l at d*vlanes+l
                          // prefetched layout: [win_pieces][qcap][16 bytes]  piece c of queue entry e at (c*qcap+e)*16
    uint16_t *scores;     // [band_w * vlanes]  ring of DP score slots (slot s of lane l at s*vlanes+l); none when prefetched
    uint32_t win_lds;     // LDS byte address of `win` (the LDS-DMA destination base; wave-uniform)
};

__host__ __device__ inline uint32_t fz_wave_lds_bytes(uint32_t win_dwords, uint32_t band_w, uint32_t vlanes,
                                                      bool with_queue) {
    uint32_t b = 0;
    if (with_queue) b += FZ_QCAP * 4;
    b += win_dwords * vlanes * 4;
    b += ((band_w * vlanes * 2) + 15u) & ~15u;
    return b;
}

// Fused lane-per-cell verification: 64 / gw contiguous byte windows per wave (window + 16 bytes of slack each), in dwords.
__host__ __device__ inline uint32_t fz_wf_fused_dwords(uint32_t win_dwords, uint32_t gw) { return (64u / gw) * (win_dwords + 4u); }

__device__ __forceinline__ FzWaveLds fz_wave_lds(uint8_t *base, uint32_t wave, uint32_t win_dwords, uint32_t band_w,
                                                 uint32_t vlanes, bool with_queue) {
    uint8_t *p = base + (size_t)wave * fz_wave_lds_bytes(win_dwords, band_w, vlanes, with_queue);
    FzWaveLds w;
    w.queue = nullptr;
    if (with_queue) { w.queue = reinterpret_cast<uint32_t *>(p); p += FZ_QCAP * 4; }
    w.win = reinterpret_cast<uint32_t *>(p); p += win_dwords * vlanes * 4;
    w.scores = reinterpret_cast<uint16_t *>(p);
    w.win_lds = 0;
    return w;
}

// Fused in-memory scan: every queue entry owns win_pieces 16-byte pieces of its sequence window, filled by
// LDS-DMA while the scan goes on (fz_prefetch_windows).
__host__ __device__ inline uint32_t fz_wave_lds_pref_bytes(uint32_t qcap, uint32_t win_pieces) {
    return qcap * 4u + win_pieces * qcap * 16u;
}

// `base_lds` = LDS byte address of `base` (the scan kernel's dynamic LDS starts at address 0).
__device__ __forceinline__ FzWaveLds fz_wave_lds_pref(uint8_t *base, uint32_t base_lds, uint32_t wave, uint32_t qcap,
                                                      uint32_t win_pieces) {
    const uint32_t off = wave * fz_wave_lds_pref_bytes(qcap, win_pieces);
    FzWaveLds w;
    w.queue = reinterpret_cast<uint32_t *>(base + off);
    w.win = reinterpret_cast<uint32_t *>(base + off + qcap * 4u);
    w.scores = nullptr;
    w.win_lds = base_lds + off + qcap * 4u;
    return w;
}

// LDS-resident accessors used by fz_verify_* on the GPU.
struct FzLdsScores {
    uint16_t *base;                                        // already offset by the lane
    uint32_t stride;                                       // = vlanes
    __device__ __forceinline__ uint32_t get(uint32_t slot) const { return base[slot * stride]; }
    __device__ __forceinline__ void set(uint32_t slot, uint32_t v) { base[slot * stride] = (uint16_t)v; }
};
struct FzLdsWindow {
    const uint8_t *base;                                   // lane's dword 0, as bytes
    uint64_t wbase;                                        // global index of byte 0 of the window
    uint32_t stride4;                                      // = vlanes * 4: bytes between a lane's consecutive dwords
    __device__ __forceinline__ uint8_t at(uint64_t gidx) const {
        const uint32_t off = (uint32_t)(gidx - wbase);
        return base[(off >> 2) * stride4 + (off & 3u)];
    }
};

// A window that LDS-DMA laid down: 16-byte piece c of the entry at base + c * rstride.
struct FzDmaWindow {
    const uint8_t *base;                                   // piece 0 of this entry
    uint64_t wbase;                                        // global index of byte 0 of the window
    uint32_t rstride;                                      // = qcap * 16
    __device__ __forceinline__ uint8_t at(uint64_t gidx) const {
        const uint32_t off = (uint32_t)(gidx - wbase);
        return base[(off >> 4) * rstride + (off & 15u)];
    }
    // aligned dword at window byte offset o (o % 4 == 0); offsets past the staged pieces read other LDS
    // bytes (or 0 beyond the allocation): callers only use the bytes they know to be staged
    __device__ __forceinline__ uint32_t dword(uint32_t o) const {
        return *reinterpret_cast<const uint32_t *>(base + (o >> 4) * rstride + (o & 15u));
    }
    // byte at window offset o
    __device__ __forceinline__ uint32_t byte(uint32_t o) const { return base[(o >> 4) * rstride + (o & 15u)]; }
};

// The two whole-pattern Peq tables of the bit-vector verification in LDS (fz_device.h: fz_verify_lev_bits): [side][256]
// words of NW x 8 bytes, forward table first.
#define FZ_PEQ_BYTES(NW) (2u * 256u * (FZ_BITS_WIDTH(NW) / 8u))
template <int NW>
struct FzPeqLds {
    typedef typename FzBitsWord<NW>::T T;
    typedef __attribute__((address_space(3))) const T LdsT;
    uint32_t tabs;                                         // LDS byte address of the forward table
    // a table's handle = its LDS address: a word's address is one v_lshl_add_u32
    __device__ __forceinline__ uint32_t table(uint32_t side) const { return tabs + side * (256u * (FZ_BITS_WIDTH(NW) / 8u)); }
    __device__ __forceinline__ T at(uint32_t tab, uint32_t ch) const {
        return *(LdsT *)(uintptr_t)(tab + ch * (FZ_BITS_WIDTH(NW) / 8u));
    }
};

// N dwords of the byte string that starts at byte offset `off` of a dword-readable source: rd(o) = the aligned
// dword at byte offset o.  One v_alignbyte per dword brings the string to byte 0 of the result.
template <int N, class Rd>
__device__ __forceinline__ FzBytes<N> fz_load_bytes(Rd rd, uint32_t off) {
    const uint32_t a0 = off & ~3u, sh = off & 3u;
    uint32_t raw[N + 1];
#pragma unroll
    for (int q = 0; q <= N; ++q) raw[q] = rd(a0 + 4u * (uint32_t)q);
    FzBytes<N> b;
#pragma unroll
    for (int q = 0; q < N; ++q) b.r[q] = __builtin_amdgcn_alignbyte(raw[q + 1], raw[q], sh);
    return b;
}

// Start of the staged window of the hit (block starting at s, index idx) inside the segment that starts at sa:
// the dword-aligned buffer position at or below max(sa, idx - s - k).
__device__ __forceinline__ uint64_t fz_window_lo(const FzScanArgs &a, uint64_t idx, uint32_t s, uint64_t sa) {
    const uint64_t reach = (uint64_t)s + a.k;
    uint64_t wlo = idx - sa > reach ? idx - reach : sa;
    if (wlo < a.geom.buf_off) wlo = a.geom.buf_off;
    return wlo;
}
__device__ __forceinline__ uint64_t fz_window_base(const FzScanArgs &a, uint64_t wlo) {
    return a.geom.buf_off + ((wlo - a.geom.buf_off) & ~(uint64_t)3);
}

// Asynchronous 16-byte copy global -> LDS (global_load_lds_dwordx4): every active lane l copies 16 bytes from
// ITS address gsrc to LDS byte address lds_dst + 16 * l (lds_dst wave-uniform, goes through M0).  No VGPR is
// written; completion is tracked by vmcnt like any load.  hipcc does not count this statement in its own
// s_waitcnt bookkeeping: its vmcnt(N) waits then cover MORE than it intended (vmcnt(N) = "at most N still
// in flight", and loads retire in order), never less; the consumer of the LDS bytes waits vmcnt(0) itself.
__device__ __forceinline__ void fz_glds16(const uint8_t *gsrc, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

__device__ __forceinline__ unsigned long long fz_bcast64(unsigned long long v) {
    // (the builtin returns int: widen through uint32_t, or a low word with bit 31 set sign-extends into the high word)
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
           (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// _substitutions_only_ngrams_template.h:103-121 for the hits of a wave, four characters per step: the window's Hamming
// distance to the WHOLE pattern (the n-gram's own positions agree — the caller has confirmed the n-gram — and add nothing),
// text dwords brought to the pattern's alignment by v_alignbyte, nonzero bytes of the xor counted by one v_bcnt.  The loop is
// wave-uniform (m / 4 steps, left when no lane is within the budget any more): fz_verify_subs's per-lane skip over the
// n-gram and per-lane early return compile to ~90 scalar instructions per character and lane group on dense candidates
// (1 GiB DNA, m = 20, 4 substitutions: 1.9e9 SALU instructions).  -> dist = the Hamming distance where it is <= k.
__device__ __forceinline__ bool fz_verify_subs_wave(const FzDmaWindow &t, const uint8_t *pat_lds, uint32_t m, uint32_t k, uint32_t L,
                                                    uint32_t s, uint64_t idx, bool valid, FzRec &rec) {
    const uint32_t off = valid ? (uint32_t)(idx - s - t.wbase) : 0u;
    const uint32_t a0 = off & ~3u, sh = off & 3u;
    uint32_t prev = t.dword(a0), nd = 0;
    for (uint32_t q = 0; q < m; q += 4u) {
        const uint32_t next = t.dword(a0 + q + 4u);
        uint32_t d = __builtin_amdgcn_alignbyte(next, prev, sh) ^ *reinterpret_cast<const uint32_t *>(pat_lds + q);
        if (q + 4u > m) d &= (1u << (8u * (m - q))) - 1u;              // (uniform: the pattern's last, partial dword)
        const uint32_t nz = (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;   // bit 7 of every nonzero byte
        nd += (uint32_t)__popc(nz);
        prev = next;
        if ((q & 4u) && !__ballot(valid && nd <= k)) break;
    }
    rec.l = s; rec.r = m - s - L; rec.dist = nd; rec.aux = 0;
    return valid && nd <= k;
}

// ---------------------------------------------------------------------------------------------
// Wave-level verification of up to 64 candidates: each valid lane owns one (hit = block | idx), the segment it
// is verified in and a slot vl of the window area.
//  1. staged form (PREF = false): every lane fetches the <= m + 2k window bytes around its candidate into LDS
//     with independent aligned dword loads (slot vl < a.vlanes);
//     prefetched form (PREF = true, the fused in-memory scan): the window of queue entry vl is already in LDS —
//     fz_prefetch_windows requested it by LDS-DMA right after the tile that produced the hit, while its cache
//     lines were still in L2, and the scan went on meanwhile.  (Measured, round 2: the fetch at flush time, one
//     exposed HBM round trip per wave at the end of its life, cost 0.019 of the 0.226 ms of the headline scan;
//     the DP itself cost nothing measurable.)
//  2. the n-gram is confirmed exactly (the filter only compared a hash of its first min(L, 8) bytes), then the
//     reference's per-hit logic (fz_verify_lev / fz_verify_subs) runs out of LDS,
//  3. the wave appends its records with ONE global atomic.
// Returns the number of exactly-confirmed n-gram hits (wave-uniform, statistics).
//  BITS = 1 / 2 (prefetched form, Levenshtein): the two expansions run as bit-vector columns on 64 / 128-bit words
//  (fz_verify_lev_bits) with the Peq tables at `peq_tabs` in LDS, instead of the register band.
//  RAG (a batch of sequences, fz_device.h: ragged segments): the prefetched window was requested before the hit's sequence
//  was known, as that of an unsegmented search — it starts at or below the sequence's own clamp and holds every byte
//  the verification touches, so only its base is taken as the prefetch computed it (segment start 0).
template <int MAXK, bool PREF, int BITS = 0, bool RAG = false>
__device__ __forceinline__ uint32_t fz_wave_verify(const uint8_t *__restrict__ buf, const FzScanArgs &a,
                                                   const uint8_t *pat_lds, const FzWaveLds &w, uint32_t vl,
                                                   uint64_t hit, const FzSeg &sg, bool valid,
                                                   FzRec *__restrict__ recs, unsigned long long *__restrict__ counters,
                                                   const uint8_t *pref_win = nullptr, const uint8_t *peq_tabs = nullptr) {
    static_assert(BITS == 0 || PREF, "the bit-vector form verifies prefetched windows");     // (BITS = -1: Hamming count only)
    const uint32_t lane = fz_lane();
    const uint32_t g = fz_hit_block(hit);
    const uint64_t idx = fz_hit_index(hit);
    const uint32_t s = g * a.L;
    // window [wlo, whi) in global coordinates; every byte the verification touches lies inside it
    const uint64_t wlo = fz_window_lo(a, idx, s, (RAG && PREF) ? 0ull : sg.sa);
    const uint64_t wbase = fz_window_base(a, wlo);
    if constexpr (!PREF) {
        uint64_t whi = idx - s + a.m + a.k;
        const uint64_t lim = a.geom.buf_off + a.geom.buf_len;
        if (whi > lim) whi = lim;
        if (whi > sg.se) whi = sg.se;
        const uint32_t nd = valid ? (uint32_t)((whi - wbase + 3) >> 2) : 0u;
        const int64_t lbase = (int64_t)(wbase - a.geom.buf_off);
        // eight loads in flight per lane, then eight LDS stores (a load-store loop would pay the HBM/L2
        // round trip once per dword: 8 - 21 serial round trips per flush)
        for (uint32_t d0 = 0; d0 < a.win_dwords; d0 += 8) {
            uint32_t v[8];
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j)
                v[j] = (d0 + j < nd) ? *reinterpret_cast<const uint32_t *>(buf + lbase + (int64_t)(d0 + j) * 4) : 0u;
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j)
                if (d0 + j < nd) w.win[(d0 + j) * a.vlanes + vl] = v[j];
        }
        fz_wave_lds_sync();
    }
    FzRec rec;
    bool ok = false;
    auto run = [&](const auto &t) {
        auto prd = [&](uint32_t o) -> uint32_t { return *reinterpret_cast<const uint32_t *>(pat_lds + o); };
        if constexpr (PREF) {
            // exact n-gram test on registers: 8 bytes of text and pattern, masked to min(L, 8) (uniform), the
            // rest (L > 8) byte by byte
            const uint32_t off = (uint32_t)(idx - wbase);
            const FzBytes<2> tn = fz_load_bytes<2>([&](uint32_t o) { return t.dword(o); }, off);
            const FzBytes<2> pn = fz_load_bytes<2>(prd, s);
            const uint32_t m0 = a.L >= 4 ? 0xffffffffu : (1u << (8u * a.L)) - 1u;
            const uint32_t m1 = a.L >= 8 ? 0xffffffffu : a.L > 4 ? (1u << (8u * (a.L - 4u))) - 1u : 0u;
            if ((((tn.r[0] ^ pn.r[0]) & m0) | ((tn.r[1] ^ pn.r[1]) & m1)) != 0) valid = false;
            if (a.L > 8 && valid) {
                const uint8_t *ng = pat_lds + s;
                for (uint32_t b = 8; b < a.L; ++b)
                    if (ng[b] != t.at(idx + b)) { valid = false; break; }
            }
        } else {
            if (valid) {
                const uint8_t *ng = pat_lds + s;
                for (uint32_t b = 0; b < a.L; ++b)
                    if (ng[b] != t.at(idx + b)) { valid = false; break; }
            }
        }
        const uint32_t confirmed = (uint32_t)__popcll(__ballot(valid));
        if constexpr (BITS < 0) {                            // the substitutions-only form alone (fz_scan_kernel<..., 3>)
            ok = fz_verify_subs_wave(t, pat_lds, a.m, a.k, a.L, s, idx, valid, rec);
        } else if constexpr (BITS != 0) {
            // every lane takes part: the loop's control is wave-uniform (lanes without a candidate idle in it)
            const FzPeqLds<BITS> peq{(uint32_t)(uintptr_t)(FzLdsU8 *)peq_tabs};
            ok = fz_verify_lev_bits<BITS>(peq, [&](uint32_t o) -> uint32_t { return t.byte(o); }, wbase, sg.sa, sg.se, a.m, a.k,
                                          a.L, s, idx, valid, rec);
        } else if (a.mode == FZ_MODE_LEV) {
            FzLdsScores sc{w.scores + (PREF ? 0u : vl), a.vlanes};
            if (valid) ok = fz_verify_lev<MAXK>(sc, t, sg.sa, sg.se, pat_lds, a.m, a.k, a.L, s, idx, rec);
        } else if (valid) {
            ok = fz_verify_subs(t, pat_lds, a.m, a.k, a.L, s, idx, rec);
        }
        return confirmed;
    };
    uint32_t confirmed;
    if constexpr (PREF) {
        confirmed = run(FzDmaWindow{pref_win, wbase, a.qcap * 16u});      // piece 0 of the lane's queue entry
    } else {
        confirmed = run(FzLdsWindow{reinterpret_cast<const uint8_t *>(w.win + vl), wbase, a.vlanes * 4u});
    }
    const unsigned long long mask = __ballot(ok);
    if (mask) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&counters[1], (unsigned long long)__popcll(mask));
        base = fz_bcast64(base);
        if (ok) {
            rec.key = hit;
            rec.aux = sg.j;
            const unsigned long long slot = base + fz_rank(mask);
            if (slot < a.rec_cap) recs[slot] = rec;
        }
    }
    fz_wave_lds_sync();
    return confirmed;
}

// Exact test of one (local position, block) candidate against the buffer in HBM (emit mode).
__device__ __forceinline__ bool fz_confirm(const uint8_t *__restrict__ buf, const FzScanArgs &a, uint32_t blk,
                                           uint64_t local) {
    if ((fz_load_win(buf, (int64_t)local) & a.mask1) != a.A[blk]) return false;
    if (a.L > 4 && (fz_load_win(buf, (int64_t)local + a.d2) & a.mask2) != a.B[blk]) return false;
    if (a.L > 8) {                                         // (two loops under a uniform branch: see fz_copy_pattern)
        if (a.pat_g) {
            const uint8_t *pg = reinterpret_cast<const uint8_t *>(a.pat_g) + a.s[blk];
            for (uint32_t b = 8; b < a.L; ++b)
                if (buf[local + b] != pg[b]) return false;
        } else {
            for (uint32_t b = 8; b < a.L; ++b)
                if (buf[local + b] != a.pat[a.s[blk] + b]) return false;
        }
    }
    return true;
}

#define FZ_HDR_WORDS 128                                   // 64-bit counters in the result header
#define FZ_HDR_TICKET 3                                    // counters[3]: ticket shards that are complete (final launch)
#define FZ_HDR_SHARD0 96                                   // counters[96 .. 111]: workgroups that finished, by blockIdx % 16
#define FZ_TICKET_SHARDS 16u

// End of the final kernel of a search: the LAST workgroup to get here copies the counters into
// host-visible memory (a.host_hdr), so the host needs no D2H copy command after the kernel (the
// records themselves are then written straight to pinned host memory as well).  Every thread of
// the workgroup must call it.
// No agent-scope fence on purpose: on this multi-XCD part __threadfence() writes back the XCD's L2,
// and one per workgroup made the scan 1.7x slower.  It is not needed either: everything the last
// workgroup reads was produced by agent-scope atomics (performed memory-side), __syncthreads() makes
// each wave wait for its own outstanding atomics (s_waitcnt vmcnt(0)) before the ticket is taken,
// and the counters are read back with agent-scope atomic loads.
// `flag` is one LDS dword the workgroup no longer needs (no static __shared__ here: it would move the
// dynamic LDS base off 0 and cost the scan an address add per table lookup).
__device__ __forceinline__ void fz_finish_launch(const FzScanArgs &a, unsigned long long *__restrict__ counters,
                                                 volatile uint32_t *flag, uint32_t participants = 0) {
    if (!a.host_hdr) return;
    if (participants == 0) participants = gridDim.x;       // workgroups that take a ticket (all, unless the caller says fewer)
    __syncthreads();                                       // all waves' counter atomics are complete, LDS is free
    if (threadIdx.x == 0) {
        // Two-level ticket: 16 shard words, then one word for the shards' last arrivals.  One word only sustains ~90
        // atomics per microsecond chip-wide, and the workgroups of a short launch all finish together (1536 of them on a
        // 64 MiB scan: 10 us of its 42 us were this queue).
        const uint32_t nshard = participants < FZ_TICKET_SHARDS ? participants : FZ_TICKET_SHARDS;
        const uint32_t r = blockIdx.x % nshard;
        const unsigned long long members = (participants - r + nshard - 1u) / nshard;   // workgroups b < participants with b % nshard == r
        bool last = atomicAdd(&counters[FZ_HDR_SHARD0 + r], 1ull) == members - 1ull;
        if (last) last = atomicAdd(&counters[FZ_HDR_TICKET], 1ull) == (unsigned long long)nshard - 1ull;
        *flag = last ? 1u : 0u;
    }
    __syncthreads();
    if (*flag) {
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(a.host_hdr);
        for (uint32_t i = threadIdx.x; i < FZ_HDR_WORDS; i += blockDim.x) {
            dst[i] = __hip_atomic_load(&counters[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // ... and leaves the counters zeroed for the next search (no memset command on the stream)
            __hip_atomic_store(&counters[i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// A wave-uniform value the compiler does not recognise as such (it then keeps it in a VGPR and updates it with
// VALU ops): reading it through v_readfirstlane pins it to an SGPR; on values it already knows to be uniform the
// call folds away.
__device__ __forceinline__ uint32_t fz_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// Candidate code of the queue: tile-local byte offset (14 bits) | block (FZ_BLK_BITS bits) | tile iteration.
__device__ __forceinline__ uint32_t fz_code(uint32_t off, uint32_t blk, uint32_t titer) {
    return off | (blk << FZ_TILE_BITS) | (titer << (FZ_TILE_BITS + FZ_BLK_BITS));
}

// Queue entry -> (block of this launch, local byte position in the buffer).
__device__ __forceinline__ uint64_t fz_code_local(uint32_t code, uint32_t &blk) {
    blk = (code >> FZ_TILE_BITS) & (FZ_MAX_BLOCKS_PER_LAUNCH - 1u);
    // the workgroup's physical tile walk (first tile, stride) as the scan kernel left it in LDS.  A shard has fewer than
    // 2^31 tiles (enqueue_shard), so the walk is 32-bit arithmetic, and the negative stride of a reversed launch is its
    // two's complement: the sum wraps to the tile
    FzLdsU32 *walk = (FzLdsU32 *)(uintptr_t)FZ_WALK_LDS;
    const uint32_t tile = walk[0] + (code >> (FZ_TILE_BITS + FZ_BLK_BITS)) * walk[1];
    return (uint64_t)tile * FZ_TILE_BYTES + (code & (FZ_TILE_BYTES - 1u));
}

// Fused in-memory scan: request the sequence windows of the queue entries [qf, qn) — a.win_pieces LDS-DMA
// copies of 16 bytes per entry, lane = entry, destination = the entry's slot of the window area.  Called
// after every tile that queued something, i.e. while the lines are still in L2 (the re-fetch at flush time
// used to be 10 % extra HBM traffic, profiles/r01_pmc_summary.json), and nothing waits for the data before
// the flush.  Entries that the range check will drop are fetched as well (their address is inside the
// buffer; cheaper than testing here).
__device__ __forceinline__ void fz_prefetch_windows(const uint8_t *__restrict__ buf, const FzScanArgs &a,
                                                    const FzWaveLds &w, uint32_t qf, uint32_t qn) {
    const uint32_t lane = fz_lane();
    // The queue entries were stored by this wave: a wave's LDS operations are performed in issue order, so the
    // reads below see them; only the compiler must not reorder.  (fz_wave_lds_sync() would be wrong here: its
    // workgroup-scope release is an s_waitcnt vmcnt(0), i.e. a wait for the rows just requested for the next tile.)
    asm volatile("" ::: "memory");
    for (uint32_t e0 = qf; e0 < qn; e0 += 64u) {
        const uint32_t e = e0 + lane;
        if (e < qn) {
            uint32_t blk;
            const uint64_t idx = a.geom.buf_off + fz_code_local(w.queue[e], blk);
            const uint64_t wbase = fz_window_base(a, fz_window_lo(a, idx, (a.g0 + blk) * a.L, 0));
            const uint8_t *src = buf + (wbase - a.geom.buf_off);
            for (uint32_t c = 0; c < a.win_pieces; ++c)
                fz_glds16(src + 16u * c, (uint32_t)__builtin_amdgcn_readfirstlane((int)(w.win_lds + (c * a.qcap + e0) * 16u)));
        }
    }
}

// The same for the entries a tile has just queued — the common call, once per tile and wave (93 % of the tiles
// of the headline workload queue something) — with everything that is the same for all of them kept scalar:
// the tile's buffer position is wave-uniform, and from the second tile of the buffer on no window is clamped
// at the start of the sequence, so window start = tile base + ((offset - s - k) & ~3) is one 32-bit lane value
// next to a scalar base (global_load_lds with an SGPR base).  ~9 VALU per call instead of ~40 (64-bit
// multiply-adds, compares and selects per lane): 262 000 calls per GiB.  `tile_local` = tile * FZ_TILE_BYTES >= one tile.
__device__ __forceinline__ void fz_prefetch_tile(const uint8_t *__restrict__ buf, const FzScanArgs &a, const FzWaveLds &w,
                                                 uint32_t qf, uint32_t qn, uint64_t tile_local) {
    const uint32_t lane = fz_lane();
    asm volatile("" ::: "memory");                         // the queue stores of this wave are issued before the reads below
    constexpr uint32_t BIAS = 2048u;                       // > FZ_MAX_M + FZ_MAX_K: keeps the lane offset non-negative
    const uint8_t *sbase = buf + fz_bcast64(tile_local) - BIAS;
    const uint32_t c0 = a.g0 * a.L + a.k;
    for (uint32_t e0 = qf; e0 < qn; e0 += 64u) {
        const uint32_t e = e0 + lane;
        if (e < qn) {
            const uint32_t code = w.queue[e];
            const uint32_t reach = ((code >> FZ_TILE_BITS) & (FZ_MAX_BLOCKS_PER_LAUNCH - 1u)) * a.L + c0;           // (g0 + block) * L + k
            const uint32_t voff = (((code & (FZ_TILE_BYTES - 1u)) - reach) & ~3u) + BIAS;
            for (uint32_t c = 0; c < a.win_pieces; ++c) {
                const uint32_t lds_dst = fz_uniform(w.win_lds + (c * a.qcap + e0) * 16u);
                uint32_t keep;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(voff + 16u * c), "s"(sbase), "s"(lds_dst) : "memory");
            }
        }
    }
}

// Process queue entries [0, qn): range-check, then verify in place (FUSED) or confirm against HBM and
// bulk-append to the global hit list.  SEG: the sequence is a batch of file chunks (segments), a
// position may belong to two of them and is range-checked / verified once per segment; compiled
// separately because the in-memory search (one segment, the whole sequence) must not pay for it in
// registers.  FUSED && !SEG: the windows were prefetched (entry e -> slot e).  Returns the number of
// confirmed n-gram hits.
// Generic search, window table (fz_device.h: FzGenDedup): the scan enters every n-gram hit it lists — its window's slot
// (claimed by atomicCAS), the hit as a member of the window, and the window's leader = the hit of the smallest block
// (atomicMax on the inverted word) — so that when the automaton kernel starts, every hit knows whether it runs.
__device__ __forceinline__ void fz_gen_claim(const FzScanArgs &a, uint64_t hit, unsigned long long q) {
    if (q >= FZ_GEN_ORDER_MAX) return;
    const FzGenDedup dd(a.gen_dedup);
    const uint32_t blk = fz_hit_block(hit);
    const unsigned long long wk = fz_hit_index(hit) + a.k - (unsigned long long)blk * a.L + 1ull;
    uint32_t slot = (uint32_t)((wk * 0x9E3779B97F4A7C15ull) >> 40) & (FZ_GEN_DEDUP_SLOTS - 1u);
    uint32_t at = FZ_GEN_DEDUP_NONE;
    for (uint32_t probe = 0; probe < 32u; ++probe) {
        const unsigned long long old = atomicCAS(&dd.keys[slot], 0ull, wk);
        if (old == 0ull || old == wk) { at = slot; break; }
        slot = (slot + 1u) & (FZ_GEN_DEDUP_SLOTS - 1u);
    }
    if (at != FZ_GEN_DEDUP_NONE) {                            // (a crowded table or a full member list: the hit stays on its own)
        const uint32_t pos = atomicAdd(&dd.nmem[at], 1u);
        if (pos < FZ_GEN_DEDUP_MEMBERS) dd.mem[at * FZ_GEN_DEDUP_MEMBERS + pos] = (uint32_t)q;
        else at = FZ_GEN_DEDUP_NONE;
    }
    if (at != FZ_GEN_DEDUP_NONE) atomicMax(&dd.best[at], ~(((unsigned long long)blk << 32) | q));
    dd.wslot[q] = at;
}

template <int GW, bool RAG>
__device__ __forceinline__ uint32_t fz_flush_wf(const uint8_t *__restrict__ buf, const FzScanArgs &a, const uint8_t *lds0,
                                                const uint8_t *pat_lds, const FzWaveLds &w, const uint8_t *area, uint32_t per_wave,
                                                volatile uint32_t *fills, uint32_t wave, uint32_t qn, bool pooled,
                                                FzRec *__restrict__ recs, unsigned long long *__restrict__ counters);

// MAXK: the widest register band the verification carries (fz_expand_any); the lean instances pass 2.
template <bool FUSED, bool SEG, bool RAG, int MAXK = 4>
__device__ __forceinline__ uint32_t fz_queue_flush(const uint8_t *__restrict__ buf, const FzScanArgs &a,
                                                   const uint8_t *pat_lds, const FzWaveLds &w, uint32_t qn,
                                                   uint64_t *__restrict__ hits, FzRec *__restrict__ recs,
                                                   unsigned long long *__restrict__ counters) {
    constexpr bool PREF = FUSED && !SEG;
    const uint32_t lane = fz_lane();
    uint32_t confirmed = 0;
    if (PREF) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every prefetched window has landed in LDS
    fz_wave_lds_sync();
    const uint32_t width = (FUSED && !PREF) ? a.vlanes : 64u;  // candidates handled per pass
    const uint32_t ncand = (SEG && FUSED) ? fz_segment_candidates(a.geom) : 1u;
    for (uint32_t e0 = 0; e0 < qn; e0 += width) {
        for (uint32_t c = 0; c < ncand; ++c) {               // one inlined copy of the verification for both segments
            const uint32_t e = e0 + lane;
            bool valid = lane < width && e < qn;
            uint64_t hit = 0;
            uint64_t local = 0;
            uint32_t blk = 0;
            FzSeg sg;
            sg.sa = 0; sg.se = a.geom.n; sg.j = 0; sg.ok = 1;
            if (valid) {
                local = fz_code_local(w.queue[e], blk);
                const uint64_t idx = a.geom.buf_off + local;
                if (!SEG) {
                    if constexpr (RAG) sg = fz_segment_one<true>(a.geom, idx);
                    valid = fz_hit_in_range(a, blk, idx, sg);
                } else if (FUSED) {
                    sg = fz_segment(a.geom, idx, c);
                    valid = fz_hit_in_range(a, blk, idx, sg);
                } else {                                      // hit list: accepted by ANY segment (the verify kernel re-checks)
                    valid = false;
                    for (uint32_t cc = 0; cc < fz_segment_candidates(a.geom); ++cc)
                        valid = valid || fz_hit_in_range(a, blk, idx, fz_segment(a.geom, idx, cc));
                }
                hit = fz_hit_pack(a.g0 + blk, idx);
            }
            if (FUSED) {
                if (SEG && c && !__ballot(valid)) continue;
                confirmed += fz_wave_verify<MAXK, PREF, 0, RAG>(buf, a, pat_lds, w, lane, hit, sg, valid, recs, counters,
                                                     PREF ? reinterpret_cast<const uint8_t *>(w.win) + e * 16u : nullptr);
            } else {
                if (valid) valid = fz_confirm(buf, a, blk, local);
                const unsigned long long mask = __ballot(valid);
                if (mask) {
                    unsigned long long base = 0;
                    if (lane == 0) base = atomicAdd(&counters[0], (unsigned long long)__popcll(mask));
                    base = fz_bcast64(base);
                    const unsigned long long slot = base + fz_rank(mask);
                    if (valid && slot < a.hit_cap) {
                        hits[slot] = hit;
                        if (!SEG && a.gen_dedup) fz_gen_claim(a, hit, slot);
                    }
                }
            }
        }
    }
    fz_wave_lds_sync();
    return confirmed;
}

// The LAST flush of a workgroup of the fused in-memory scan, pooled: when all tiles are done every wave holds a
// partly filled queue (on the headline workload ~32 entries: verifying them per wave keeps half the lanes idle,
// and the scan is short of VALU issue slots, not of latency).  The four waves publish their fills, meet at one
// barrier and verify the concatenation of the four queues 64 entries at a time, pass p on wave p mod 4: a lane
// finds the wave that owns its entry by three compares and reads code and prefetched window out of that wave's
// area.  `area` = first wave's queue, `per_wave` = bytes per wave area, `fills` = four LDS dwords.
template <int MAXK, int BITS = 0, bool RAG = false>
__device__ __forceinline__ uint32_t fz_pooled_flush(const uint8_t *__restrict__ buf, const FzScanArgs &a,
                                                    const uint8_t *pat_lds, const uint8_t *area, uint32_t per_wave,
                                                    volatile uint32_t *fills, uint32_t wave, uint32_t qn,
                                                    FzRec *__restrict__ recs, unsigned long long *__restrict__ counters,
                                                    const uint8_t *peq_tabs = nullptr) {
    const uint32_t lane = fz_lane();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's prefetched windows have landed in LDS
    if (lane == 0) fills[wave] = qn;
    __syncthreads();
    const uint32_t n0 = fills[0], n1 = fills[1], n2 = fills[2], n3 = fills[3];
    const uint32_t total = n0 + n1 + n2 + n3;
    FzWaveLds none;
    none.queue = nullptr; none.win = nullptr; none.scores = nullptr; none.win_lds = 0;
    uint32_t confirmed = 0;
    for (uint32_t e0 = wave * 64u; e0 < total; e0 += FZ_WAVES_PER_BLOCK * 64u) {
        uint32_t li = e0 + lane, ow = 0;
        bool valid = li < total;
        if (li >= n0) { li -= n0; ow = 1; if (li >= n1) { li -= n1; ow = 2; if (li >= n2) { li -= n2; ow = 3; } } }
        const uint8_t *mine = area + ow * per_wave;
        uint64_t hit = 0;
        FzSeg sg;
        sg.sa = 0; sg.se = a.geom.n; sg.j = 0; sg.ok = 1;
        if (valid) {
            uint32_t blk;
            const uint64_t idx = a.geom.buf_off + fz_code_local(reinterpret_cast<const uint32_t *>(mine)[li], blk);
            if constexpr (RAG) sg = fz_segment_one<true>(a.geom, idx);
            valid = fz_hit_in_range(a, blk, idx, sg);
            hit = fz_hit_pack(a.g0 + blk, idx);
        }
        confirmed += fz_wave_verify<MAXK, true, BITS, RAG>(buf, a, pat_lds, none, lane, hit, sg, valid, recs, counters,
                                                      mine + a.qcap * 4u + li * 16u, peq_tabs);
    }
    return confirmed;
}

// Mid-scan flush of the fused bit-vector forms (in-memory Levenshtein searches, fz_scan_kernel<..., WFG = 1 / 2>; NW = 0:
// the register band / Hamming count under the same queue discipline, WFG = 3).  A pass
// costs the wave ~m - L + 2k columns whatever its number of candidates, so passes are FULL: the queue is worked off 64
// entries at a time, and what is left below 64 moves to the front of the queue — code and prefetched window pieces —
// and waits for the next tiles' entries (only a queue that holds fewer than 64 in the first place is verified as it is:
// the scan loop asks for that when it expects the next tile to overflow it).  `qn` -> the entries kept.
template <int NW, bool RAG>
__device__ __forceinline__ uint32_t fz_bits_flush(const uint8_t *__restrict__ buf, const FzScanArgs &a, const uint8_t *pat_lds,
                                                  const uint8_t *peq_tabs, const FzWaveLds &w, uint32_t &qn,
                                                  FzRec *__restrict__ recs, unsigned long long *__restrict__ counters) {
    const uint32_t lane = fz_lane();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // every prefetched window has landed in LDS
    fz_wave_lds_sync();
    const uint32_t end = qn >= 64u ? qn & ~63u : qn;
    uint32_t confirmed = 0;
    for (uint32_t e0 = 0; e0 < end; e0 += 64u) {
        const uint32_t e = e0 + lane;
        bool valid = e < end;
        uint64_t hit = 0;
        FzSeg sg;
        sg.sa = 0; sg.se = a.geom.n; sg.j = 0; sg.ok = 1;
        if (valid) {
            uint32_t blk;
            const uint64_t idx = a.geom.buf_off + fz_code_local(w.queue[e], blk);
            if constexpr (RAG) sg = fz_segment_one<true>(a.geom, idx);
            valid = fz_hit_in_range(a, blk, idx, sg);
            hit = fz_hit_pack(a.g0 + blk, idx);
        }
        confirmed += fz_wave_verify<4, true, NW, RAG>(buf, a, pat_lds, w, lane, hit, sg, valid, recs, counters,
                                                 reinterpret_cast<const uint8_t *>(w.win) + e * 16u, peq_tabs);
    }
    const uint32_t rem = qn - end;                          // < 64, and only behind at least one full pass
    if (lane < rem) {
        w.queue[lane] = w.queue[end + lane];
        uint8_t *wb = reinterpret_cast<uint8_t *>(w.win);
        for (uint32_t c = 0; c < a.win_pieces; ++c)
            *reinterpret_cast<uint4 *>(wb + (c * a.qcap + lane) * 16u) = *reinterpret_cast<const uint4 *>(wb + (c * a.qcap + end + lane) * 16u);
    }
    qn = rem;
    fz_wave_lds_sync();
    return confirmed;
}

// NWIN  : 1 -> hash = (masked dword at the offset) * K               (L <= 4, v_mul_lo_u32);
//         2 -> hash = low24(dword at offset + DH) * K + dword at offset (v_mad_u32_u24), DH = min(L, 8) - 3.
// FUSED : verify candidates inside this kernel (records out) or emit exact hits (hit list out).
// SEG   : the buffer is a batch of file chunks with per-chunk clamps (find_near_matches_in_file).
// SA    : the table slot comes from hash bits 2..6 as they are (one v_and per offset instead of v_lshrrev + v_and;
//         measured -7 % on the headline workload: the fused scan is bound by VALU issue, +/- one full-rate VALU op
//         per offset = +10 / -7 %).  Those bits only depend on window bytes 0 and DH, so the host can use this form
//         when the blocks of a launch differ there (fzhip.hip: choose_launch_blocks); the general form takes any
//         five hash bits.
// Each thread owns 16 consecutive byte offsets per row and reads 24 bytes (16 + 8 halo).
// Block test: slot = (hash >> lut_shift) & 31; lut[slot] holds the hash of the block that lives there
// (the host picks K and lut_shift so that different block hashes get different slots) or, for a free
// slot, a value that belongs to another slot, so hash ^ lut[slot] == 0 <=> the window hashes like
// some block.  32 slots of 4 bytes = one slot per LDS bank: lanes that read different slots never
// collide, lanes that read the same slot are served by one broadcast.
// Measured against per-block VALU compares (benchmarks/filter_variants.hip, v3 vs v14, 3 blocks,
// L2-resident data): 0.222 -> 0.175 ms per GiB, and no longer growing with the number of blocks.
// Fast hits are queued per wave ACROSS tiles and processed 64 at a time (full lanes, one latency
// chain per ~100 candidates instead of one per tile).  A tile denser than the queue is re-scanned
// by enumeration ("slow tile": correctness path for pathological inputs).
// Half-tile software pipeline: rows 0-1 of the NEXT tile are requested before rows 2-3 of this one are
// tested, so a wave always has two rows (3 KiB) of loads in flight while it computes, on the same 24 data
// VGPRs as "load a tile, test a tile" (measured: 0.236 -> 0.227 ms on the headline workload).
// What round 2 measured about this kernel (benchmarks/lab_*.sh, 1 GiB DNA, |p| = 20, k = 2):
//   * one VALU op less per offset (slot address by v_and only): no change -> the hot loop is not bound by
//     VALU issue; the scan without candidates takes 0.200 ms at 7, 6, 5 and 4 workgroups per CU alike;
//   * without verification 0.206 ms, with the window fetch but no DP 0.225 ms, complete 0.226 ms: what
//     candidates cost was the exposed fetch of their windows at the end of every wave's life -> prefetched
//     by LDS-DMA now (fz_prefetch_windows).
// 7 waves per SIMD (72 VGPRs): measured 2-3 % faster than the natural 79-VGPR / 6-wave allocation;
// 8 waves (64 VGPRs) spills 27 VGPRs in the verify path and is 50 % slower.
// RAG   : the buffer is a batch of sequences packed back to back (fz_batch_search): the in-memory forms, every candidate
//         range-checked and verified inside its own sequence (fz_device.h: ragged segments).  The ragged instances are
//         kernels of their own (fz_batch_scan_kernel) compiled from the same text (fz_kernel_bodies.inc, section 1), so
//         that the in-memory ones stay what they were, instruction for instruction.

template <int NWIN, int DH, bool FUSED, bool SEG, bool SA, int WFG = 0>
// (the bit-vector forms: 6 waves per SIMD = 80 VGPRs with one-word columns, 5 = 96 with two-word ones — their queues and Peq
//  tables leave LDS for at most that many workgroups per CU anyway, and the column loop keeps the next column's Peq word and
//  character in flight)
// (round 6, the equal-n-gram sets in the rare path: the file API's fused instances and the lane-per-cell forms, which sat at
//  exactly 72 VGPRs, take 6 waves as well — the former are bound by the host's copies, the latter serve patterns beyond 128
//  characters only)
#define FZ_SCAN_WAVES(WFG, FUSED, SEG) ((WFG) == 2 ? 5 : ((WFG) != 0 || ((FUSED) && (SEG))) ? 6 : 7)      // (WFG = 4: 6 as well)
__global__ __launch_bounds__(FZ_FILTER_THREADS)
__attribute__((amdgpu_waves_per_eu(FZ_SCAN_WAVES(WFG, FUSED, SEG), FZ_SCAN_WAVES(WFG, FUSED, SEG)))) void fz_scan_kernel(
    const uint8_t *__restrict__ buf, const FzScanArgs a, uint64_t ntiles,
    uint64_t *__restrict__ hits, FzRec *__restrict__ recs, unsigned long long *__restrict__ counters) {
    constexpr bool RAG = false, DUPH = true;
    constexpr int MAXK = 4;
#define FZ_KERNEL_BODY 1
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}

// The lean instances of the in-memory register-band / Hamming-count form (FUSED, !SEG, WFG = 0: the headline workload, the
// substitutions-only searches, Levenshtein budgets 1 and 2) — kernels of their own from the same text, like the ragged ones,
// so that every fz_scan_kernel instance stays what it was.  Compiled out of them (DUPH = false, MAXK = 2):
//   * the equal-n-gram slot sets of the rare path: the run-time test, the `while (__ballot(set))` loop in each of its 64
//     unrolled copies and the set bits of the table word.  The host only launches a lean instance when no two blocks of the
//     launch hash alike (fzhip.hip: scan_is_lean);
//   * the register bands for k = 3 and 4 (right and left expansion, mid-scan and pooled flush: eight DP loops) — k >= 3 is
//     never routed here.
// What that leaves the headline instance: profiles/r23_headline_lean.txt.
template <int NWIN, int DH, bool SA>
__global__ __launch_bounds__(FZ_FILTER_THREADS)
__attribute__((amdgpu_waves_per_eu(FZ_SCAN_WAVES(0, true, false), FZ_SCAN_WAVES(0, true, false)))) void fz_lean_scan_kernel(
    const uint8_t *__restrict__ buf, const FzScanArgs a, uint64_t ntiles,
    uint64_t *__restrict__ hits, FzRec *__restrict__ recs, unsigned long long *__restrict__ counters) {
    constexpr bool FUSED = true, SEG = false, RAG = false, DUPH = false;
    constexpr int WFG = 0, MAXK = 2;
#define FZ_KERNEL_BODY 1
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}

// The ragged instances (6 waves per SIMD: the per-candidate lookup lives in the flushes, next to the verification).
template <int NWIN, int DH, bool FUSED, bool SA, int WFG = 0>
__global__ __launch_bounds__(FZ_FILTER_THREADS)
__attribute__((amdgpu_waves_per_eu(FZ_SCAN_WAVES(WFG, true, true), FZ_SCAN_WAVES(WFG, true, true)))) void fz_batch_scan_kernel(
    const uint8_t *__restrict__ buf, const FzScanArgs a, uint64_t ntiles,
    uint64_t *__restrict__ hits, FzRec *__restrict__ recs, unsigned long long *__restrict__ counters) {
    constexpr bool SEG = false, RAG = true, DUPH = true;
    constexpr int MAXK = 4;
#define FZ_KERNEL_BODY 1
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}

// Verification of a hit list in HBM, one lane per candidate (parameter ranges whose LDS footprint does
// not fit beside the filter, substitutions with large budgets, Levenshtein budgets above 31).  One wave
// verifies 64 hits at a time.  Dynamic LDS: pattern + per-wave window/score areas.
__global__ __launch_bounds__(256) void fz_verify_kernel(const uint8_t *__restrict__ buf, const FzScanArgs a,
                                 const uint64_t *__restrict__ hits, FzRec *__restrict__ recs,
                                 unsigned long long *__restrict__ counters) {
    constexpr bool RAG = false;
#define FZ_KERNEL_BODY 2
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}
// ... of a batch of sequences (ragged segments)
__global__ __launch_bounds__(256) void fz_batch_verify_kernel(const uint8_t *__restrict__ buf, const FzScanArgs a,
                                 const uint64_t *__restrict__ hits, FzRec *__restrict__ recs,
                                 unsigned long long *__restrict__ counters) {
    constexpr bool RAG = true;
#define FZ_KERNEL_BODY 2
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}

// ---------------------------------------------------------------------------------------------
// Lane-per-DP-cell verification (the north star's wavefront form), for budgets 5 .. 31 where one
// lane per candidate is a long serial chain.  GW lanes own one candidate; lane gl holds the band
// cell D[i][i + gl - K] of the current row i (K = max_l_dist).  Row i + 1 needs
//   the diagonal  D[i][i+d]      = the lane's own cell,
//   the upper     D[i][i+1+d]    = the cell of lane gl + 1          (one DPP row shift),
//   the left      D[i+1][i+d]    = the NEW cell of lane gl - 1:  v[gl] = min_{e <= gl} (a[e] + gl - e),
//                                  a prefix-min over the lanes of a[e] - e (log2 GW DPP steps).
// Same table as fz_expand_band / c_expand_*: band K >= budget holds every cell <= budget, bottom row
// scanned for the LAST arg-min from the column-0 baseline (pyx:33-34, :67-69).
template <int GW>
__device__ __forceinline__ uint32_t fz_xl_shl1(uint32_t v, uint32_t fill, uint32_t gl) {
    if constexpr (GW == 16) {
        return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x101, 0xf, 0xf, false);   // row_shl:1
    } else {
        // lane l <- lane l + 1 across the wave (wave_shl:1; lane 63 <- fill), then the last lane of every group <- fill
        const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x130, 0xf, 0xf, false);
        return gl == (uint32_t)GW - 1u ? fill : o;
    }
}

template <int GW>
__device__ __forceinline__ uint32_t fz_xl_prefix_min(uint32_t v, uint32_t gl) {
    if constexpr (GW == 16) {
        // v = min(v, v of the lane n below) in one instruction each: a DPP source outside the row disables
        // the lane, and since destination and second source are the same register such a lane keeps v
        asm volatile("s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\ts_nop 1"
                     : "+v"(v));
    } else {
        // inside the 16-lane rows as above, then the last lane of row 0 / 2 into rows 1 / 3 (32-lane groups) and the last
        // lane of row 1 into rows 2 and 3 (the whole wave): lanes without a source keep their value
        v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
        v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
        v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
        v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
        v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
        if constexpr (GW == 64)
            v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    }
    return v;
}

// The rows of one bounded expansion for every group of the wave.  All arguments but gl are uniform inside a
// group.  sub(i) = lds[sub_addr + i * sub_step], win(j) = lds[win_addr + j * win_step] (bytes in LDS;
// reads one element outside either range land in this workgroup's LDS and only feed cells that are
// forced anyway).  -> the lane's cell of the bottom row, D[sublen][sublen + gl - K] (garbage above `budget`
// once every live group has run out of cells within its budget: nothing can pass then).
template <int GW>
__device__ __forceinline__ uint32_t fz_wf_rows(const uint8_t *lds, uint32_t gl, uint32_t K, int sub_addr, int sub_step,
                                               uint32_t sublen, int win_addr, int win_step, uint32_t winlen,
                                               uint32_t budget, bool valid) {
    constexpr uint32_t INF = 0x3fffu;
    const int d = (int)gl - (int)K;
    const bool act = valid && gl <= 2u * K;
    uint32_t jv = act ? (uint32_t)d : 0x7fff0000u;          // column j = i + d of this lane (row 0); "negative" = huge
    uint32_t cell = jv <= winlen ? jv : INF;                // row 0: D[0][j] = j
    if (!valid) { win_addr = sub_addr = 0; win_step = sub_step = 0; }
    int caddr = win_addr + win_step * d;                    // row i compares win(i + d - 1)
    if (!act) caddr = win_addr;
    int paddr = sub_addr;
    uint32_t chr = lds[caddr], pc = lds[paddr];
    const uint32_t bias = (uint32_t)GW - gl;
    for (uint32_t i = 1;; ++i) {
        const bool live = valid && i <= sublen;
        if (!__ballot(live)) break;
        caddr += win_step;
        paddr += sub_step;
        const uint32_t nchr = lds[caddr], npc = lds[paddr];   // next row's characters: their latency hides behind this row
        jv += 1u;
        const uint32_t up = fz_xl_shl1<GW>(cell, INF, gl);
        uint32_t v = min(cell + (chr != pc ? 1u : 0u), up + 1u);
        if (jv == 0u) v = i;                                  // column 0: D[i][0] = i
        const bool bad = jv > winlen;
        v = bad ? INF : v;
        v = fz_xl_prefix_min<GW>(v + bias, gl) - bias;
        v = bad ? INF : v;
        if (live) cell = v;
        chr = nchr;
        pc = npc;
        // row minima never decrease: once no live candidate has a cell within its budget, nothing can pass
        if ((i & 3u) == 0u && !__ballot(live && cell <= budget)) break;
    }
    return cell;
}

// Bottom row -> (best, last arg-min) over the columns 1 .. winlen from the column-0 baseline
// (pyx:33-34, :67-69); uniform inside the group.  winlen may be smaller than the one the rows ran with:
// a cell only depends on cells of smaller or equal columns.
template <int GW>
__device__ __forceinline__ bool fz_wf_pick(uint32_t cell, uint32_t gl, uint32_t K, uint32_t sublen, uint32_t winlen,
                                           uint32_t budget, bool valid, uint32_t &dist, uint32_t &consumed) {
    const int jb = (int)sublen + (int)gl - (int)K;
    const bool validj = valid && gl <= 2u * K && jb >= 1 && jb <= (int)winlen;
    uint32_t key = validj ? ((cell << 8) | (255u - gl)) : 0xffffffffu;     // min cell, then the LARGEST column
    key = fz_xl_prefix_min<GW>(key, gl);
    key = (uint32_t)__shfl((int)key, (int)((fz_lane() & ~((uint32_t)GW - 1u)) + (uint32_t)GW - 1u), 64);
    uint32_t best = sublen, arg = 0;
    if (key != 0xffffffffu && (key >> 8) <= sublen) {
        best = key >> 8;
        arg = (uint32_t)((int)sublen + (int)(255u - (key & 255u)) - (int)K);
    }
    dist = best;
    consumed = arg;
    return valid && best <= budget;
}

// The same verification inside the scan kernel (fz_scan_kernel<..., WF = true>, in-memory searches): queued candidates,
// 64 / GW at a time on GW lanes each, straight from the queue — no hit list, no second kernel and no gap between the two.
// One pass = one memory round trip (the candidates' windows into LDS), the exact n-gram test out of LDS (the scan's filter
// compared a hash), the two expansions, one atomic for the records of the pass.
// (Measured and not kept: right and left expansion of a candidate side by side on two lane groups, the left one with the
// full budget and the pick narrowed afterwards — the rows of a pass drop from max(right) + max(left) over its candidates
// to max(right, left), but a pass takes half the candidates: 0.2128 vs 0.2141 ms where candidates are rare (configs[3a]),
// 0.847 vs 0.605 ms where they are dense and leave after a few rows (1 GiB DNA, m = 40).)
// `have` / `code` are uniform inside a lane group.  Returns the number of confirmed, in-range n-gram hits of the pass.
template <int GW, bool RAG>
__device__ __forceinline__ uint32_t fz_wf_pass(const uint8_t *__restrict__ buf, const FzScanArgs &a, const uint8_t *lds0,
                                               const uint8_t *pat_lds, uint8_t *gwin, bool have, uint32_t code,
                                               FzRec *__restrict__ recs, unsigned long long *__restrict__ counters) {
    static_assert(GW < 64, "one ballot word holds several lane groups");
    const uint32_t lane = fz_lane();
    const uint32_t grp = lane / (uint32_t)GW, gl = lane % (uint32_t)GW;
    uint32_t blk = 0;
    const uint64_t local = fz_code_local(code, blk);
    const uint64_t idx = a.geom.buf_off + local;
    const uint32_t s = (a.g0 + blk) * a.L;
    FzSeg sg;
    sg.sa = 0; sg.se = a.geom.n; sg.j = 0; sg.ok = 1;
    if constexpr (RAG) sg = fz_segment_one<true>(a.geom, idx);
    bool valid = have && fz_hit_in_range(a, blk, idx, sg);
    if (!__ballot(valid)) return 0;
    // the candidate's window [wlo, whi), staged as plain bytes: byte g of the sequence at gwin[g - wbase]
    uint64_t whi = 0, wbase = 0;
    if (valid) {
        whi = idx - s + a.m + a.k;
        const uint64_t lim = a.geom.buf_off + a.geom.buf_len;
        if (whi > lim) whi = lim;
        if (whi > sg.se) whi = sg.se;
        wbase = fz_window_base(a, fz_window_lo(a, idx, s, sg.sa));
    }
    const uint32_t nd = valid ? (uint32_t)((whi - wbase + 3) >> 2) : 0u;
    const uint8_t *src = buf + (int64_t)(wbase - a.geom.buf_off);
    for (uint32_t d0 = 0; d0 < a.win_dwords; d0 += 4u * (uint32_t)GW) {       // four loads in flight per lane, then four stores
        uint32_t v[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t dd = d0 + j * (uint32_t)GW + gl;
            v[j] = dd < nd ? *reinterpret_cast<const uint32_t *>(src + (size_t)dd * 4) : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t dd = d0 + j * (uint32_t)GW + gl;
            if (dd < nd) reinterpret_cast<uint32_t *>(gwin)[dd] = v[j];
        }
    }
    fz_wave_lds_sync();
    // exact n-gram test: lane gl compares the bytes gl, gl + GW, ...
    bool differs = false;
    if (valid) {
        const uint8_t *tn = gwin + (uint32_t)(idx - wbase), *pn = pat_lds + s;
        for (uint32_t b = gl; b < a.L; b += (uint32_t)GW) differs = differs || tn[b] != pn[b];
    }
    const unsigned long long group_bits = (((1ull << GW) - 1ull) << (grp * (uint32_t)GW));
    if (__ballot(differs) & group_bits) valid = false;
    const unsigned long long vm = __ballot(valid && gl == 0);
    if (!vm) { fz_wave_lds_sync(); return 0; }
    const int prel = (int)(pat_lds - lds0), wrel = (int)(gwin - lds0);
    auto lds_of = [&](uint64_t gidx) -> int { return valid ? wrel + (int)(int64_t)(gidx - wbase) : 0; };
    // right: p[s+L:] vs t[idx+L : min(se, idx-s+m+k)]
    uint64_t rbeg = idx + a.L, rend = idx + a.m + a.k - s;
    if (rend > sg.se) rend = sg.se;
    if (rbeg > sg.se) rbeg = sg.se;
    if (rend < rbeg) rend = rbeg;
    const uint32_t rwin = (uint32_t)(rend - rbeg), rlen = a.m - s - a.L;
    uint32_t dR = 0, r = 0, dL = 0, l = 0;
    const uint32_t cellr = fz_wf_rows<GW>(lds0, gl, a.k, prel + (int)(s + a.L), 1, rlen, lds_of(rbeg), 1, rwin, a.k, valid);
    const bool ok1 = fz_wf_pick<GW>(cellr, gl, a.k, rlen, rwin, a.k, valid, dR, r);
    // left: reversed p[:s] vs reversed t[max(sa, idx-s-(k-dR)) : idx], budget k - dR
    const uint32_t bl = ok1 ? a.k - dR : 0u;
    const uint64_t want = (uint64_t)s + bl;
    const uint64_t lbeg = (idx - sg.sa > want) ? idx - want : sg.sa;
    const uint32_t lwin = ok1 ? (uint32_t)(idx - lbeg) : 0u;
    const uint32_t celll = fz_wf_rows<GW>(lds0, gl, a.k, prel + (int)s - 1, -1, s, lds_of(idx) - 1, -1, lwin, bl, ok1);
    const bool ok = fz_wf_pick<GW>(celll, gl, a.k, s, lwin, bl, ok1, dL, l) && gl == 0;
    const unsigned long long mask = __ballot(ok);
    if (mask) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&counters[1], (unsigned long long)__popcll(mask));
        base = fz_bcast64(base);
        const unsigned long long slot = base + fz_rank(mask);
        if (ok && slot < a.rec_cap) {
            FzRec rec;
            rec.key = fz_hit_pack(a.g0 + blk, idx); rec.l = l; rec.r = r; rec.dist = dL + dR; rec.aux = sg.j;
            recs[slot] = rec;
        }
    }
    fz_wave_lds_sync();
    return (uint32_t)__popcll(vm);
}

// The flush of the fused lane-per-cell form — ONE call site in the scan kernel (a second inlined copy of the pass costs the
// hot loop its registers).  In the middle of the scan (`pooled` = false: this wave's queue filled up) the wave works through
// its own queue.  At the end of the workgroup's life (`pooled` = true, every wave gets here exactly once) what the four waves
// still hold is pooled, as fz_pooled_flush does for the lane-per-candidate form, and dealt out 64 / GW candidates at a time,
// pass p to wave p mod 4: the n-gram hits of one near match sit a few bytes apart, i.e. in ONE wave's queue, and would take
// that wave several passes while the other three have none.
// `area` = first wave's area (queue first), `per_wave` = bytes per wave area, `fills` = four LDS dwords.
template <int GW, bool RAG>
__device__ __forceinline__ uint32_t fz_flush_wf(const uint8_t *__restrict__ buf, const FzScanArgs &a, const uint8_t *lds0,
                                                const uint8_t *pat_lds, const FzWaveLds &w, const uint8_t *area, uint32_t per_wave,
                                                volatile uint32_t *fills, uint32_t wave, uint32_t qn, bool pooled,
                                                FzRec *__restrict__ recs, unsigned long long *__restrict__ counters) {
    constexpr uint32_t NH = 64u / (uint32_t)GW;                         // candidates per pass
    const uint32_t lane = fz_lane();
    const uint32_t grp = lane / (uint32_t)GW;
    uint32_t n0 = qn, n1 = 0, n2 = 0, n3 = 0, first = 0, step = NH;
    const uint8_t *q0 = reinterpret_cast<const uint8_t *>(w.queue);
    if (pooled) {
        if (lane == 0) fills[wave] = qn;
        __syncthreads();
        n0 = fills[0]; n1 = fills[1]; n2 = fills[2]; n3 = fills[3];
        first = wave * NH;
        step = FZ_WAVES_PER_BLOCK * NH;
        q0 = area;
    } else {
        fz_wave_lds_sync();
    }
    const uint32_t total = n0 + n1 + n2 + n3;
    uint8_t *gwin = reinterpret_cast<uint8_t *>(w.win) + grp * (a.win_dwords * 4u + 16u);
    uint32_t confirmed = 0;
    // (Measured: a pass with the hits of one near match — different blocks, so max(right) + max(left) ~ 100 rows of a
    // 64-byte pattern — takes 17 - 23 us, ~400 cycles per row, next to six streaming waves per SIMD; s_setprio(3)
    // around the passes changed nothing: the rows wait for their own dependent instructions, not for issue slots.)
    for (uint32_t e0 = first; e0 < total; e0 += step) {
        uint32_t li = e0 + grp, ow = 0;
        const bool have = li < total;
        if (li >= n0) { li -= n0; ow = 1; if (li >= n1) { li -= n1; ow = 2; if (li >= n2) { li -= n2; ow = 3; } } }
        const uint32_t code = have ? reinterpret_cast<const uint32_t *>(q0 + ow * per_wave)[li] : 0u;
        confirmed += fz_wf_pass<GW, RAG>(buf, a, lds0, pat_lds, gwin, have, code, recs, counters);
    }
    return confirmed;
}

// Levenshtein verification of a hit list, GW lanes per hit (64 / GW hits per wave at a time): right
// expansion, then left with what the right one left of the budget (levenshtein_ngram.py:177-189).
// (Measured and dropped: right and left expansions of a hit side by side on two lane groups — half the
// rows per wave but twice the workgroups, 0.031 vs 0.029 ms: the rows are ~11 us of this kernel, the rest
// is launch, two dependent load round trips and the finish tickets.)
// Record slot = hit number (x candidate segment): no slot atomics — all waves of this kernel finish at
// about the same time, and 1400 atomics on one counter word took longer than the DP rows.  Slots of hits
// that did not verify carry FZ_REC_NONE; the host drops them.  Long hit lists (more than FZ_WF_COMPACT_MIN
// slots) append their records instead, one atomic per pass that verified something: a slot per hit of a
// dense list is megabytes of empty records for the host to copy and skip (2.4e6 hits of 1 GiB of DNA at
// m = 54, k = 8: 57 MB per search, 16 of the call's 19 ms).
// Dynamic LDS: pattern + per-wave window areas (one contiguous byte window per hit).
template <int GW>
__global__ __launch_bounds__(1024) void fz_verify_wf_kernel(const uint8_t *__restrict__ buf, const FzScanArgs a,
                                                            const uint64_t *__restrict__ hits, FzRec *__restrict__ recs,
                                                            unsigned long long *__restrict__ counters) {
    constexpr bool RAG = false;
#define FZ_KERNEL_BODY 3
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}
template <int GW>
__global__ __launch_bounds__(1024) void fz_batch_verify_wf_kernel(const uint8_t *__restrict__ buf, const FzScanArgs a,
                                                                  const uint64_t *__restrict__ hits, FzRec *__restrict__ recs,
                                                                  unsigned long long *__restrict__ counters) {
    constexpr bool RAG = true;
#define FZ_KERNEL_BODY 3
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}

// ---------------------------------------------------------------------------------------------
// fz_verify_big_kernel<CPL> — verification without size limits: ONE WAVE PER HIT, lane-per-DP-cell with CPL band
// cells per lane (2k + 1 <= 64 * CPL cells: budgets up to 1023), pattern and sequence read from HBM / L2 as they
// are (no LDS staging: subsequences up to FZ_MAX_M_ANY).  Used where the other verifications do not fit: patterns
// longer than the kernel-argument block, budgets above FZ_MAX_K, windows or score rings beyond LDS
// (levenshtein_ngram.py:159-198 has no limit on either).  Same table as fz_expand / c_expand_*
// (_levenshtein_ngrams.pyx:9-154): lane gl owns the cells x = gl * CPL + c of a row, cell x of row i is
// D[i][i + x - K]; the upper neighbour is cell x + 1 of the previous row (the next lane's first cell: one DPP wave
// shift), the left-neighbour recurrence v[x] = min_{e <= x} (a[e] + x - e) is a prefix-min of a[e] - e: sequential
// inside the lane, one exclusive wave scan (DPP row shifts + row broadcasts) across lanes.  Cells beyond 2K are
// computed as well (a wider band is still exact).  The 64 pattern characters and the 64 characters entering the
// band's right edge of the next 64 rows are fetched with one coalesced load each and handed out by v_readlane.
__device__ __forceinline__ uint32_t fz_dpp_wave_shl1(uint32_t v, uint32_t edge) {     // lane l <- lane l + 1; lane 63 <- edge
    return (uint32_t)__builtin_amdgcn_update_dpp((int)edge, (int)v, 0x130, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t fz_dpp_wave_shr1(uint32_t v, uint32_t edge) {     // lane l <- lane l - 1; lane 0 <- edge
    return (uint32_t)__builtin_amdgcn_update_dpp((int)edge, (int)v, 0x138, 0xf, 0xf, false);
}
// inclusive prefix-min over the 64 lanes (lanes without a source keep their value)
__device__ __forceinline__ uint32_t fz_wave_incl_min(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    return v;
}

// One bounded expansion by the whole wave; every argument is wave-uniform.  sub(i) = psub[i * sstep] (i < sublen),
// win(j) = pwin[j * wstep] (j < winlen), both in global memory.  -> (ok, dist, consumed) as fz_expand.
template <int CPL>
__device__ __forceinline__ bool fz_big_expand(const uint8_t *psub, int sstep, uint32_t sublen, const uint8_t *pwin, int wstep,
                                              uint32_t winlen, uint32_t K, uint32_t budget, uint32_t &dist, uint32_t &consumed) {
    if (sublen == 0) { dist = 0; consumed = 0; return true; }       // pyx:28-30
    constexpr uint32_t INF = 0x3fffffffu;
    constexpr uint32_t NX = 64u * (uint32_t)CPL;
    const uint32_t lane = fz_lane();
    const uint32_t x0 = lane * (uint32_t)CPL;
    uint32_t cell[CPL], chr[CPL];
    int jb = (int)x0 - (int)K;                                       // column of cell 0 of this lane in row i: jb + c (row 0 now)
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int j = jb + c;
        cell[c] = (j >= 0 && (uint32_t)j <= winlen) ? (uint32_t)j : INF;                       // row 0: D[0][j] = j
        chr[c] = (j >= 0 && (uint32_t)j < winlen) ? (uint32_t)pwin[(int64_t)j * wstep] : 0x100u;   // row 1 compares win[j]
    }
    uint32_t pvec = 0, wvec = 0;
    for (uint32_t i = 1; i <= sublen; ++i) {
        const uint32_t r = (i - 1u) & 63u;
        if (r == 0) {
            const uint32_t pi = i - 1u + lane;                                                // pattern characters of rows i .. i + 63
            pvec = pi < sublen ? (uint32_t)psub[(int64_t)pi * sstep] : 0u;
            const int64_t wj = (int64_t)(i + lane) + (int64_t)NX - 1 - (int64_t)K;           // right-edge character after row i + lane
            wvec = (wj >= 0 && wj < (int64_t)winlen) ? (uint32_t)pwin[wj * wstep] : 0x100u;
        }
        const uint32_t pc = (uint32_t)__builtin_amdgcn_readlane((int)pvec, (int)r);
        const uint32_t edge = (uint32_t)__builtin_amdgcn_readlane((int)wvec, (int)r);
        jb += 1;
        const uint32_t up_last = fz_dpp_wave_shl1(cell[0], INF);                             // D[i-1][..] of the next lane's first cell
        // a[c] = min(diag + cost, up + 1), forced at column 0 and outside the table; t[c] = running min of a[e] + (NX - e)
        uint32_t run = 0xffffffffu;
        uint32_t t[CPL];
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int j = jb + c;
            const uint32_t up = (c + 1 < CPL) ? cell[(c + 1 < CPL) ? c + 1 : 0] : up_last;
            uint32_t v = min(cell[c] + (chr[c] != pc ? 1u : 0u), up + 1u);
            if (j == 0) v = i;                                                               // D[i][0] = i
            if (j < 0 || (uint32_t)j > winlen) v = INF;
            run = min(run, v + (NX - (x0 + (uint32_t)c)));
            t[c] = run;
        }
        const uint32_t incl = fz_wave_incl_min(run);
        const uint32_t excl = fz_dpp_wave_shr1(incl, 0xffffffffu);
        uint32_t any_low = 0;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int j = jb + c;
            uint32_t v = min(excl, t[c]) - (NX - (x0 + (uint32_t)c));
            v = min(v, INF);
            if (j < 0 || (uint32_t)j > winlen) v = INF;
            cell[c] = v;
            any_low |= (v <= budget) ? 1u : 0u;
        }
        // next row's characters: every cell takes its right neighbour's
        const uint32_t in = fz_dpp_wave_shl1(chr[0], edge);
#pragma unroll
        for (int c = 0; c + 1 < CPL; ++c) chr[c] = chr[c + 1];
        chr[CPL - 1] = in;
        // row minima never decrease: once no cell is within the budget nothing can pass (pyx:61-65)
        if ((i & 3u) == 0u && !__ballot(any_low != 0u)) return false;
    }
    // bottom row: min over the columns 1 .. winlen, the LARGEST column among equals, from the column-0 baseline
    uint32_t key = 0xffffffffu;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int j = jb + c;
        if (j >= 1 && (uint32_t)j <= winlen) key = min(key, (min(cell[c], 0xfffffu) << 12) | (NX - 1u - (x0 + (uint32_t)c)));
    }
    key = fz_wave_incl_min(key);
    key = (uint32_t)__builtin_amdgcn_readlane((int)key, 63);
    uint32_t best = sublen, arg = 0;
    if (key != 0xffffffffu && (key >> 12) <= sublen) {
        best = key >> 12;
        arg = (uint32_t)((int)sublen + (int)(NX - 1u - (key & 0xfffu)) - (int)K);
    }
    dist = best;
    consumed = arg;
    return best <= budget;
}

template <int CPL>
__global__ __launch_bounds__(64) void fz_verify_big_kernel(const uint8_t *__restrict__ buf, const FzScanArgs a,
                                                           const uint64_t *__restrict__ hits, FzRec *__restrict__ recs,
                                                           unsigned long long *__restrict__ counters) {
    constexpr bool RAG = false;
#define FZ_KERNEL_BODY 4
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}
template <int CPL>
__global__ __launch_bounds__(64) void fz_batch_verify_big_kernel(const uint8_t *__restrict__ buf, const FzScanArgs a,
                                                                 const uint64_t *__restrict__ hits, FzRec *__restrict__ recs,
                                                                 unsigned long long *__restrict__ counters) {
    constexpr bool RAG = true;
#define FZ_KERNEL_BODY 4
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}

// ---------------------------------------------------------------------------------------------
// K4  fz_generic_kernel: the generic (mixed-limit) search's per-hit verification — the greedy
// candidate-set automaton of generic_search.py:57-177 run on the window
// seq[max(0, idx-s-k) : idx-s+m+k] of every exact n-gram hit (generic_search.py:222-237).
// One WAVE per hit: the candidate list lives in LDS and its 64-wide slices are advanced by the 64
// lanes; successor candidates and matches are written through wave prefix sums, so both lists keep
// exactly the reference's order (its emitted *list*, not just the set, is reproduced).  The
// character loop is inherently sequential; parallelism comes from hits x candidates.
#ifndef FZ_LP_PAIR
#define FZ_LP_PAIR 1                                       // the per-hit automaton steps two 64-candidate slices per trip
#endif
#ifndef FZ_GEN_MCAP
#define FZ_GEN_MCAP 128                                    // match-buffer entries per wave (1 KB: with 256-entry candidate lists
                                                           // 24 waves per CU are resident, every hit of configs[3b] at once)
#endif

// Inclusive prefix sum over the 64 lanes on DPP: four row shifts scan the 16-lane rows, row_bcast:15 / :31 carry
// the row totals across (6 VALU adds; the ds_bpermute form — six __shfl_up — paid six LDS round trips per call,
// and the automaton calls it once per 64 candidates per window character).
__device__ __forceinline__ uint32_t fz_wave_incl_scan(uint32_t v) {
    // update_dpp(old, src, ctrl, row_mask, bank_mask, bound_ctrl): lanes without a source keep `old` (0 here)
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2 and 3
    return v;
}

// KIND (FzLpKind) and HBM_LISTS are compile-time: the per-hit instance carries none of the tiled Levenshtein
// automaton's code, and with the lists in LDS their accesses are ds_ instructions instead of flat ones.
template <int KIND, bool HBM_LISTS>
__global__ __launch_bounds__(64) void fz_lp_kernel(const uint8_t *__restrict__ buf, const FzScanArgs a,
                                                   const uint64_t *__restrict__ hits, uint64_t n_items,
                                                   FzGenRec *__restrict__ recs,
                                                   unsigned long long *__restrict__ counters) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x;
    const uint32_t mpad = (a.m + 15u) & ~15u;
    const uint32_t wmax = a.m + 2u * a.k + a.lp_starts;
    const uint32_t wpad = (wmax + 15u) & ~15u;
    uint8_t *pat = smem;
    uint8_t *win = smem + mpad;
    // Candidate lists: LDS normally; for inputs whose candidate sets outgrow it (two-letter alphabets with
    // large budgets) per-workgroup lists in HBM.  One wave per workgroup, so the workgroup-scope fences
    // of fz_wave_lds_sync order its global accesses just as they order the LDS ones.
    FzGCand *cur = HBM_LISTS ? reinterpret_cast<FzGCand *>(a.cand_scratch) + (size_t)blockIdx.x * 2u * a.cand_cap
                             : reinterpret_cast<FzGCand *>(smem + mpad + wpad);
    FzGCand *nxt = cur + a.cand_cap;
    uint64_t *mbuf = reinterpret_cast<uint64_t *>(smem + mpad + wpad + (HBM_LISTS ? 0u : 2u * a.cand_cap * (uint32_t)sizeof(FzGCand)));
    fz_copy_pattern(pat, a, lane, 64u);
    fz_wave_lds_sync();
    auto patf = [&](uint32_t i) -> uint8_t { return pat[i]; };
    constexpr bool per_hit = KIND == FZ_LP_GENERIC_HIT;
    constexpr bool lev = KIND == FZ_LP_LEV_SEQ;

    unsigned long long nitems = n_items;
    if (per_hit) { nitems = counters[0]; if (nitems > a.hit_cap) nitems = a.hit_cap; }
    const uint32_t ncand = per_hit ? fz_segment_candidates(a.geom) : 1u;
    // device-side ordering (fz_gen_order_kernel / fz_gen_scatter_kernel below): every hit leaves its row count
    const bool order = per_hit && a.gen_order != 0;
    unsigned long long *order_first = reinterpret_cast<unsigned long long *>(a.gen_order);
    uint32_t *order_count = reinterpret_cast<uint32_t *>(order_first + FZ_GEN_ORDER_MAX);
    // window table (FzGenDedup, fz_device.h): hits that share a window run the automaton once
    const bool dedup = per_hit && a.gen_dedup != 0 && nitems <= FZ_GEN_ORDER_MAX && ncand == 1u;
    const FzGenDedup dd(a.gen_dedup);
    for (uint64_t qc = blockIdx.x; qc < nitems * ncand; qc += gridDim.x) {
        if ((a.flags & FZ_FLAG_ANY) && __hip_atomic_load(&counters[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) break;   // has_near_match_*
        const uint64_t q = qc / ncand;
        uint64_t key_base, w0, w1;
        uint32_t spawn_len, seg_j = 0;
        bool flush_end;
        if (per_hit) {
            const uint64_t hit = hits[q];
            const uint32_t s = fz_hit_block(hit) * a.L;
            const uint64_t idx = fz_hit_index(hit);
            const FzSeg sg = fz_segment(a.geom, idx, (uint32_t)(qc % ncand));
            if (!fz_hit_in_range_s(a, s, idx, sg)) {                   // wave-uniform: one hit per wave
                if (order && q < FZ_GEN_ORDER_MAX && lane == 0) { order_first[q] = 0; order_count[q] = 0; }
                continue;
            }
            if (dedup) {
                // the scan entered the hit into the window table: only the window's leader (smallest block) runs
                const uint32_t sl = dd.wslot[q];
                if (sl != FZ_GEN_DEDUP_NONE && dd.leader(sl) != (uint32_t)q) {
                    if (order && lane == 0) { order_first[q] = 0; order_count[q] = 0; }
                    continue;
                }
            }
            const uint64_t reach = (uint64_t)s + a.k;
            w0 = idx - sg.sa > reach ? idx - reach : sg.sa;            // generic_search.py:231
            w1 = idx - s + a.m + a.k;
            if (w1 > sg.se) w1 = sg.se;
            spawn_len = (uint32_t)(w1 - w0);
            flush_end = true;                                          // the window IS the sequence there
            key_base = hit;
            seg_j = sg.j;
        } else {
            w0 = a.geom.own_lo + q * a.lp_starts;
            const uint64_t own_end = a.geom.own_hi < a.geom.n ? a.geom.own_hi : a.geom.n;
            spawn_len = (uint32_t)((own_end - w0) < a.lp_starts ? (own_end - w0) : a.lp_starts);
            w1 = w0 + spawn_len + a.m + a.k;
            if (w1 > a.geom.n) w1 = a.geom.n;
            flush_end = w1 == a.geom.n;     // candidates alive at the true sequence end are flushed;
            key_base = w0;                  // elsewhere every candidate of this tile has died by w1
        }
        const uint32_t wlen = (uint32_t)(w1 - w0);
        for (uint32_t i = lane; i < wlen; i += 64u) win[i] = buf[(w0 - a.geom.buf_off) + i];
        fz_wave_lds_sync();

        uint32_t ncur = 0, mb = 0, mseq = 0;
        bool overflow = false;
        // FZ_FLAG_FOLD (fz_generic_ngrams_consolidated): what leaves the kernel is not the hit's matches but (hull, best
        // match) pairs — every match that overlaps the running hull of the hit's earlier matches is folded into it
        // (the group test of common.py:150-159; "best" = smallest distance, then longest, then smallest start: a total
        // order, so the fold order does not matter).  The matches of one hit nearly always overlap: ~1 pair per hit
        // instead of ~34 rows (configs[3b]: 6e3 pairs instead of 2.1e5 rows cross PCIe), and the host only merges hulls.
        const bool fold = per_hit && (a.flags & FZ_FLAG_FOLD);
        bool f_have = false;
        uint32_t f_lo = 0, f_hi = 0, f_k1 = 0, f_k2 = 0, f_pairs = 0;   // hull [lo, hi), best = (dist << 16 | 0xffff - len, start)
        auto emit_pair = [&]() {
            if (lane == 0) {
                // (measured: without this atomic — slot = hit number — the kernel takes the same 0.164 ms: the slot counter is
                //  not what the automaton waits for)
                // Window table: this hit stands for every hit of its window.  Their equal matches fall into one overlap group
                // (the smallest block — this hit's — is the one a consolidation keeps) EXCEPT zero-length matches, which
                // overlap nothing, not even their own copies (common.py:152-153): a pair with an empty hull is emitted once
                // per member of the window, under that member's key.
                const uint32_t sl = dedup ? dd.wslot[q] : FZ_GEN_DEDUP_NONE;
                uint32_t copies = 1u;
                if (sl != FZ_GEN_DEDUP_NONE && f_lo == f_hi) { copies = dd.nmem[sl]; copies = copies < FZ_GEN_DEDUP_MEMBERS ? copies : FZ_GEN_DEDUP_MEMBERS; }
                for (uint32_t cpy = 0; cpy < copies; ++cpy) {
                    const unsigned long long slot = atomicAdd(&counters[1], 1ull);
                    if (slot < a.rec_cap) {
                        const uint32_t len = 0xffffu - (f_k1 & 0xffffu);
                        FzGenRec r;
                        r.key = copies > 1u ? hits[dd.mem[sl * FZ_GEN_DEDUP_MEMBERS + cpy]] : key_base;
                        r.seq = f_pairs; r.se = f_k2 | ((f_k2 + len) << 16); r.dist = f_k1 >> 16; r.win = f_lo | (f_hi << 16);
                        recs[slot] = r;
                    }
                }
            }
            ++f_pairs;
            f_have = false;
        };
        auto wave_min = [&](uint32_t v) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)fz_wave_incl_min(v), 63); };
        auto fold_matches = [&]() {
            fz_wave_lds_sync();
            for (uint32_t e0 = 0; e0 < mb; e0 += 64u) {
                const bool have_row = e0 + lane < mb;
                const uint64_t v = have_row ? mbuf[e0 + lane] : 0ull;
                const uint32_t rs = (uint32_t)v & 0xffffu, re = ((uint32_t)v >> 16) & 0xffffu, rd = (uint32_t)(v >> 32) & 0xffffu;
                const uint32_t k1 = (rd << 16) | (0xffffu - (re - rs));
                unsigned long long pending = __ballot(have_row);
                while (pending) {
                    if (!f_have) {                                 // a new hull starts with the first row that is left
                        const uint32_t l0 = (uint32_t)__builtin_ctzll(pending);
                        f_lo = (uint32_t)__builtin_amdgcn_readlane((int)rs, (int)l0);
                        f_hi = (uint32_t)__builtin_amdgcn_readlane((int)re, (int)l0);
                        f_k1 = (uint32_t)__builtin_amdgcn_readlane((int)k1, (int)l0);
                        f_k2 = f_lo;
                        f_have = true;
                        pending &= pending - 1ull;
                        continue;
                    }
                    const bool mine = ((pending >> lane) & 1ull) && !(re <= f_lo || rs >= f_hi);
                    const unsigned long long ov = __ballot(mine);
                    if (!ov) { emit_pair(); continue; }            // nothing left overlaps this hull: it is complete for now
                    const uint32_t mlo = wave_min(mine ? rs : 0xffffffffu), mhi = ~wave_min(mine ? ~re : 0xffffffffu);
                    const uint32_t mk1 = wave_min(mine ? k1 : 0xffffffffu);
                    const uint32_t mk2 = wave_min((mine && k1 == mk1) ? rs : 0xffffffffu);
                    f_lo = mlo < f_lo ? mlo : f_lo;
                    f_hi = mhi > f_hi ? mhi : f_hi;
                    if (mk1 < f_k1 || (mk1 == f_k1 && mk2 < f_k2)) { f_k1 = mk1; f_k2 = mk2; }
                    pending &= ~ov;
                }
            }
            mseq += mb;
            mb = 0;
            fz_wave_lds_sync();
        };
        // match buffer entry: se (32) | dist (16) | step-in-window (16)
        auto flush_matches = [&]() {
            if (mb == 0) return;
            if (fold) { fold_matches(); return; }
            fz_wave_lds_sync();
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(&counters[1], (unsigned long long)mb);
            base = fz_bcast64(base);
            for (uint32_t e = lane; e < mb; e += 64u) {
                if (base + e < a.rec_cap) {
                    const uint64_t v = mbuf[e];
                    FzGenRec r;
                    r.key = per_hit ? key_base : key_base + (v >> 48);
                    r.seq = mseq + e; r.se = (uint32_t)v; r.dist = (uint32_t)(v >> 32) & 0xffffu; r.win = per_hit ? (order ? (uint32_t)q : seg_j) : (uint32_t)q;
                    recs[base + e] = r;
                }
            }
            mseq += mb;
            mb = 0;
            fz_wave_lds_sync();
        };
        for (uint32_t index = 0; index <= wlen && !overflow; ++index) {
            const bool last = index == wlen;                           // end-of-window flush pass
            if (last && !flush_end) break;
            uint8_t ch = 0;
            uint32_t nnext = 0;
            uint32_t fresh_at = 0xffffffffu;                           // list position of this character's fresh candidate
            if (!last) {
                ch = win[index];
                if (index < spawn_len) {
                    if (!lev) {                                        // generic: fresh candidate appended (py:80)
                      // (per-hit windows: only starts that can still reach the pattern's end, fz_gen_start_useful)
                      if (!per_hit || fz_gen_start_useful(index, wlen, a.m, a.max_dels, a.k)) {
                        if (ncur >= a.cand_cap) { overflow = true; break; }
                        // (start = index, everything else 0) never goes through the list: the lane that owns
                        // position ncur takes it from registers — no LDS store + wait per character
                        fresh_at = ncur;
                        ++ncur;
                      }
                    } else {                                           // Levenshtein: levenshtein.py:75-80
                        uint32_t f = 0xffffffffu;
                        const uint32_t lim = a.k + 1 < a.m ? a.k + 1 : a.m;
                        for (uint32_t i = 0; i < lim; ++i) if (pat[i] == ch) { f = i; break; }
                        if (f != 0xffffffffu) {
                            if (f + 1 == a.m) {                        // immediate match, emitted first
                                if (mb + 1 > FZ_GEN_MCAP) flush_matches();
                                if (lane == 0) mbuf[mb] = (uint64_t)(index | ((index + 1) << 16)) | ((uint64_t)f << 32) | ((uint64_t)index << 48);
                                ++mb;
                            } else {                                   // new candidate goes FIRST
                                if (lane == 0) { FzGCand c; c.start = (uint16_t)index; c.j = (uint16_t)(f + 1); c.l = (uint8_t)f; c.ns = c.ni = c.nd = 0; nxt[0] = c; }
                                nnext = 1;
                            }
                        }
                    }
                }
            }
            const bool more_seq = w0 + index + 1 < a.geom.n;   // tiled Levenshtein mode only
            // the outputs of one slice of 64 candidates go to the lists through wave prefix sums, in list order
            auto emit = [&](const FzGStep &st) -> bool {
                const uint32_t packed = (st.fa + st.fb + st.fc) | ((st.f1 + st.f2) << 16);
                const uint32_t incl = fz_wave_incl_scan(packed);
                const uint32_t tot = __builtin_amdgcn_readlane(incl, 63);
                const uint32_t excl = incl - packed;
                const uint32_t tot_s = tot & 0xffffu, tot_m = tot >> 16;
                if (nnext + tot_s > a.cand_cap) return false;
                if (mb + tot_m > FZ_GEN_MCAP) flush_matches();
                uint2 *nx = reinterpret_cast<uint2 *>(nxt) + nnext + (excl & 0xffffu);
                uint64_t *mp = mbuf + mb + (excl >> 16);
                const uint64_t stamp = (uint64_t)index << 48;
                {
                    if (st.fa) nx[0] = make_uint2(st.a0, st.a1);
                    if (st.fb) nx[st.fa] = make_uint2(st.b0, st.b1);
                    if (st.fc) nx[st.fa + st.fb] = make_uint2(st.c0, st.c1);
                    if (st.f1) mp[0] = (uint64_t)st.m1 | ((uint64_t)st.d1 << 32) | stamp;
                    if (st.f2) mp[st.f1] = (uint64_t)st.m2 | ((uint64_t)st.d2 << 32) | stamp;
                }
                nnext += tot_s;
                mb += tot_m;
                return true;
            };
            if (!last && !lev) {
                // the hot loop (its own copy of `emit`: no register shuffling where the two forms would join).  Every
                // lane steps — positions below cand_cap are readable, lanes past the list step an all-zero candidate
                // and have their five output flags cleared: no divergence
                auto load_step = [&](uint32_t c0, FzGStep &st) {
                    const bool valid = c0 + lane < ncur;
                    uint2 cw = reinterpret_cast<const uint2 *>(cur)[c0 + lane];
                    const bool fresh = c0 + lane == fresh_at;
                    cw.x = valid ? (fresh ? index : cw.x) : 0u;
                    cw.y = valid && !fresh ? cw.y : 0u;
                    fz_generic_step_packed(cw.x, cw.y, ch, index, a.m, patf, a.max_subs, a.max_ins, a.max_dels, a.k, st);
                    const uint32_t vm = valid ? 1u : 0u;
                    st.fa &= vm; st.fb &= vm; st.fc &= vm; st.f1 &= vm; st.f2 &= vm;
                };
                uint32_t c0 = 0;
#if FZ_LP_PAIR
                // Two slices of 64 candidates per trip while the list has more than one: their loads, steps and prefix
                // scans are independent chains the hardware can overlap (a hit's time is this dependent chain, character
                // after character, and the kernel takes as long as its slowest hits — the ones with long lists); only
                // the output offsets of the second slice wait for the first one's totals.  (Lists in LDS only: the
                // second slice may read up to 127 entries past the list, which there is still this wave's LDS.)
                if constexpr (!HBM_LISTS) {
                    for (; c0 + 64u < ncur && !overflow; c0 += 128u) {
                        FzGStep sa, sb;
                        load_step(c0, sa);
                        load_step(c0 + 64u, sb);
                        const uint32_t pa = (sa.fa + sa.fb + sa.fc) | ((sa.f1 + sa.f2) << 16);
                        const uint32_t pb = (sb.fa + sb.fb + sb.fc) | ((sb.f1 + sb.f2) << 16);
                        const uint32_t ia = fz_wave_incl_scan(pa), ib = fz_wave_incl_scan(pb);
                        const uint32_t ta = __builtin_amdgcn_readlane(ia, 63), tb = __builtin_amdgcn_readlane(ib, 63);
                        const uint32_t tot_s = (ta & 0xffffu) + (tb & 0xffffu), tot_m = (ta >> 16) + (tb >> 16);
                        if (nnext + tot_s > a.cand_cap) { overflow = true; break; }
                        if (tot_m > FZ_GEN_MCAP) {                 // more matches than the buffer holds at once: one slice at a time
                            if (!emit(sa) || !emit(sb)) overflow = true;
                            continue;
                        }
                        if (mb + tot_m > FZ_GEN_MCAP) flush_matches();
                        const uint32_t ea = ia - pa, eb = ib - pb + ta;
                        uint2 *nxa = reinterpret_cast<uint2 *>(nxt) + nnext + (ea & 0xffffu);
                        uint2 *nxb = reinterpret_cast<uint2 *>(nxt) + nnext + (eb & 0xffffu);
                        uint64_t *mpa = mbuf + mb + (ea >> 16), *mpb = mbuf + mb + (eb >> 16);
                        const uint64_t stamp = (uint64_t)index << 48;
                        if (sa.fa) nxa[0] = make_uint2(sa.a0, sa.a1);
                        if (sa.fb) nxa[sa.fa] = make_uint2(sa.b0, sa.b1);
                        if (sa.fc) nxa[sa.fa + sa.fb] = make_uint2(sa.c0, sa.c1);
                        if (sb.fa) nxb[0] = make_uint2(sb.a0, sb.a1);
                        if (sb.fb) nxb[sb.fa] = make_uint2(sb.b0, sb.b1);
                        if (sb.fc) nxb[sb.fa + sb.fb] = make_uint2(sb.c0, sb.c1);
                        if (sa.f1) mpa[0] = (uint64_t)sa.m1 | ((uint64_t)sa.d1 << 32) | stamp;
                        if (sa.f2) mpa[sa.f1] = (uint64_t)sa.m2 | ((uint64_t)sa.d2 << 32) | stamp;
                        if (sb.f1) mpb[0] = (uint64_t)sb.m1 | ((uint64_t)sb.d1 << 32) | stamp;
                        if (sb.f2) mpb[sb.f1] = (uint64_t)sb.m2 | ((uint64_t)sb.d2 << 32) | stamp;
                        nnext += tot_s;
                        mb += tot_m;
                    }
                }
#endif
                for (; c0 < ncur && !overflow; c0 += 64u) {
                    FzGStep st;
                    load_step(c0, st);
                    if (!emit(st)) { overflow = true; break; }
                }
            } else {
                for (uint32_t c0 = 0; c0 < ncur; c0 += 64u) {
                    FzGStep st;
                    fz_gstep_clear(st);
                    if (c0 + lane < ncur) {
                        const uint2 cw = reinterpret_cast<const uint2 *>(cur)[c0 + lane];
                        const FzGCand c = fz_gcand_of(cw.x, cw.y);
                        if (!last) {
                            // slot form (no scratch array); its skip loop has no lane-divergent exit — see fz_device.h for the
                            // hipcc miscompile of the `break` form that kept this out of the kernel in round 4.
                            fz_levlp_step_slots(cw.x, cw.y, ch, index, more_seq, a.m, patf, a.k, st);
                        } else {
                            uint32_t d;
                            const bool hit_end = lev ? fz_levlp_final(c, a.m, a.k, d) : fz_generic_final(c, a.m, a.max_dels, a.k, d);
                            if (hit_end) { st.f1 = 1; st.m1 = (uint32_t)c.start | (wlen << 16); st.d1 = d; }
                        }
                    }
                    if (!emit(st)) { overflow = true; break; }
                }
            }
            // the next character reads what this one stored: a wave's LDS operations are performed in issue order,
            // only the compiler must not reorder; lists in HBM need the real thing
            if (HBM_LISTS) fz_wave_lds_sync(); else asm volatile("" ::: "memory");
            FzGCand *tmp = cur; cur = nxt; nxt = tmp;
            ncur = nnext;
        }
        if (overflow) {
            if (lane == 0) atomicAdd(&counters[2], 1ull);              // host retries with bigger lists
        } else {
            flush_matches();
            if (fold && f_have) emit_pair();
        }
        if (order && q < FZ_GEN_ORDER_MAX && lane == 0) { order_first[q] = 0; order_count[q] = overflow ? 0u : mseq; }
        fz_wave_lds_sync();
    }
    // folded search whose pairs went straight into the host's staging buffer: the last workgroup publishes the counters
    // there as well (no D2H copy command behind the kernel) and leaves them zeroed for the next search
    fz_finish_launch(a, counters, reinterpret_cast<volatile uint32_t *>(smem));
}

// ---- the generic search's automaton, one WORKGROUP of four waves per n-gram hit (round 4) --------------------------
// fz_lp_kernel runs a hit on ONE wave: ~74 window characters one after the other, every character 2-3 slices of 64
// candidates, every slice a dependent chain of ~220 instructions and three LDS round trips — a hit's time is that chain
// (0.15 ms for BASELINE configs[3b], however few hits there are: the kernel lasts as long as its slowest hit, and with
// the window table a third of the waves is left, on a machine that is then mostly idle).  But the candidates of
// different START positions never interact: a candidate's successors keep its start, the list is grouped by start in
// ascending order (fresh candidates are appended, generic_search.py:80), and a match's place in the emission order is
// (window character, start, order among the matches of that start).  So the starts are dealt out to the four waves of
// a workgroup (start mod W, W = 2 or 4 — neighbouring starts carry the large trees of a true occurrence), every wave runs the whole
// window over its own quarter of the list with NO synchronisation, buffers its matches, and at the end the four sorted
// buffers are merged by rank (binary searches on (character, start): no ties across waves).  One slice per character
// instead of 2-3.  A hit whose wave outgrows its list quarter or its match buffer is counted in counters[FZ_HDR_GEN_FAIL]
// and the host runs the search again with fz_lp_kernel (which also keeps the lists-in-HBM form, the file API's segments
// and the tiled whole-sequence automata).
#define FZ_GH_MAX_WAVES 4u                                  // waves per hit: template parameter W in {2, 4}
#define FZ_GH_MCAP_W(W) ((W) == 1u ? 512u : 256u)           // matches a wave buffers for one hit (one wave per hit: the whole hit's)
#define FZ_HDR_GEN_FAIL 5                                   // counters[5]: hits fz_gen_hit_kernel could not finish
#define FZ_GH_CTL_BYTES 64u

__device__ __forceinline__ uint32_t fz_gh_lower_bound(const uint64_t *mb, uint32_t n, uint32_t key) {
    uint32_t lo = 0, hi = n;                                // first entry whose (character << 16 | start) is >= key
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint64_t v = mb[mid];
        const uint32_t kv = ((uint32_t)(v >> 48) << 16) | ((uint32_t)v & 0xffffu);
        if (kv < key) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// BITS (round 5; patterns of at most 64 characters, budgets of at most 32): the candidate step is fz_generic_step_bits —
// one 64-bit equality word per window character (a 256-entry table of the pattern in LDS, looked up once per window
// character when the window is staged), every flag a 0 / 1 word, the five outputs stored UNCONDITIONALLY (an absent output
// goes to a per-lane dummy slot: no exec-mask juggling around five ds_writes).  With fz_gen_start_useful a window's list
// rarely passes 64 candidates, so this form runs ONE wave per hit (W = 1: no rank merge, no cross-wave traffic).
#define FZ_GH_PT_BYTES 2048u
template <uint32_t W, bool BITS>
__global__ __launch_bounds__(64 * W) void fz_gen_hit_kernel(const uint8_t *__restrict__ buf, const FzScanArgs a,
                                                                      const uint64_t *__restrict__ hits, FzGenRec *__restrict__ recs,
                                                                      unsigned long long *__restrict__ counters) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    // (the wave number through v_readfirstlane: the compiler must know it is the same in every lane, or the list lengths
    //  that depend on it — and every loop over them — turn into per-lane values and exec-mask loops)
    const uint32_t wave = fz_uniform(tid >> 6);
    const uint32_t mpad = (a.m + 15u) & ~15u;
    const uint32_t wpad = (a.m + 2u * a.k + 15u) & ~15u;
    const uint32_t capw = fz_uniform(a.cand_cap);           // candidate slots per list of ONE wave
    uint8_t *pat = smem;
    uint8_t *win = smem + mpad;
    volatile uint32_t *ctl = reinterpret_cast<volatile uint32_t *>(smem + mpad + wpad);   // [0] run [1] fail [2..5] matches per wave [6,7] record base [8] stop
    FzGCand *lists = reinterpret_cast<FzGCand *>(smem + mpad + wpad + FZ_GH_CTL_BYTES);
    FzGCand *cur = lists + (size_t)wave * 2u * capw, *nxt = cur + capw;
    uint64_t *mball = reinterpret_cast<uint64_t *>(lists + (size_t)W * 2u * capw);
    constexpr uint32_t FZ_GH_MCAP = FZ_GH_MCAP_W(W);
    uint64_t *mbuf = mball + (size_t)wave * FZ_GH_MCAP;
    // BITS: equality words of the pattern by byte value, of the staged window by position, and the dummy slots
    unsigned long long *ptab = reinterpret_cast<unsigned long long *>(mball + (size_t)W * FZ_GH_MCAP);
    unsigned long long *pwin = ptab + 256;
    uint2 *dummy = reinterpret_cast<uint2 *>(pwin + wpad) + tid;
    fz_copy_pattern(pat, a, tid, 64u * W);
    if constexpr (BITS) {
        for (uint32_t i = tid; i < 256u; i += 64u * W) ptab[i] = 0ull;
        __syncthreads();
        for (uint32_t i = tid; i < a.m; i += 64u * W) atomicOr(&ptab[pat[i]], 1ull << i);
        __syncthreads();
    }
    auto patf = [&](uint32_t i) -> uint8_t { return pat[i]; };
    // (everything that is the same in all lanes goes through v_readfirstlane: values loaded from memory are per-lane values
    //  to the compiler, and list lengths, loop bounds and branch conditions derived from them would become vector registers
    //  and exec-mask loops — the first build of this kernel ran its slice loop that way)
    unsigned long long nitems = fz_bcast64(counters[0]);
    if (nitems > a.hit_cap) nitems = a.hit_cap;
    const bool order = a.gen_order != 0;
    unsigned long long *order_first = reinterpret_cast<unsigned long long *>(a.gen_order);
    uint32_t *order_count = reinterpret_cast<uint32_t *>(order_first + FZ_GEN_ORDER_MAX);
    const bool dedup = a.gen_dedup != 0 && nitems <= FZ_GEN_ORDER_MAX;
    const FzGenDedup dd(a.gen_dedup);
    const bool fold = (a.flags & FZ_FLAG_FOLD) != 0;
    for (uint64_t q = blockIdx.x; q < nitems; q += gridDim.x) {
        __syncthreads();                                    // the previous hit's LDS (window, lists, buffers, ctl) is free
        const uint64_t hit = fz_bcast64(hits[q]);
        const uint32_t s = fz_hit_block(hit) * a.L;
        const uint64_t idx = fz_hit_index(hit);
        const FzSeg sg = fz_segment(a.geom, idx, 0u);
        if (!fz_hit_in_range_s(a, s, idx, sg)) {             // the same for every thread
            if (order && q < FZ_GEN_ORDER_MAX && tid == 0) { order_first[q] = 0; order_count[q] = 0; }
            continue;
        }
        const uint64_t reach = (uint64_t)s + a.k;
        const uint64_t w0 = idx - sg.sa > reach ? idx - reach : sg.sa;               // generic_search.py:231
        uint64_t w1 = idx - s + a.m + a.k;
        if (w1 > sg.se) w1 = sg.se;
        const uint32_t wlen = (uint32_t)(w1 - w0);
        if (tid == 0) {
            uint32_t run = 1u, stop = 0u;
            if ((a.flags & FZ_FLAG_ANY) && __hip_atomic_load(&counters[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) { stop = 1u; run = 0u; }
            if (dedup && !stop) {                           // the window table (fz_device.h: FzGenDedup): only the window's leader runs
                const uint32_t sl = dd.wslot[q];
                if (sl != FZ_GEN_DEDUP_NONE && dd.leader(sl) != (uint32_t)q) {
                    run = 0u;
                    if (order) { order_first[q] = 0; order_count[q] = 0; }
                }
            }
            ctl[0] = run; ctl[1] = 0u; ctl[8] = stop;
        }
        for (uint32_t i = tid; i < wlen; i += 64u * W) {
            const uint8_t c = buf[(w0 - a.geom.buf_off) + i];
            win[i] = c;
            if constexpr (BITS) pwin[i] = ptab[c];
        }
        __syncthreads();
        if (fz_uniform(ctl[8])) break;                      // has_near_match_*: a record exists somewhere
        if (!fz_uniform(ctl[0])) continue;   // a hit of a smaller block runs this window

        // ---- this wave's quarter of the candidate list over the whole window; no synchronisation with the other waves ----
        uint32_t ncur = 0, mb = 0;
        uint32_t pw0l = 0, pw0h = 0, pw1l = 0, pw1h = 0;    // BITS: equality words of window positions lane and 64 + lane (m + 2k <= 128)
        if constexpr (BITS) {
            const unsigned long long e0 = lane < wlen ? pwin[lane] : 0ull, e1 = 64u + lane < wlen ? pwin[64u + lane] : 0ull;
            pw0l = (uint32_t)e0; pw0h = (uint32_t)(e0 >> 32); pw1l = (uint32_t)e1; pw1h = (uint32_t)(e1 >> 32);
        }
        bool fail = false;
        FzGCand *lc = cur, *ln = nxt;
        // end of the window (py:172-177): the survivors that reach the pattern's end by deletions
        auto final_flush = [&]() {
            for (uint32_t c0 = 0; c0 < ncur; c0 += 64u) {
                const bool valid = c0 + lane < ncur;
                const uint2 cw = reinterpret_cast<const uint2 *>(lc)[c0 + lane];
                const FzGCand c = fz_gcand_of(cw.x, cw.y);
                uint32_t d = 0;
                const bool hit_end = valid && fz_generic_final(c, a.m, a.max_dels, a.k, d);
                const unsigned long long mask = __ballot(hit_end);
                const uint32_t tot_m = (uint32_t)__popcll(mask);
                if (mb + tot_m > FZ_GH_MCAP) { fail = true; break; }
                if (hit_end) mbuf[mb + fz_rank(mask)] = (uint64_t)((uint32_t)c.start | (wlen << 16)) | ((uint64_t)d << 32) | ((uint64_t)wlen << 48);
                mb = fz_uniform(mb + tot_m);
            }
        };
        if constexpr (BITS) {
            // The window in two runs with straight-line bodies: characters whose start can still reach the pattern's end
            // (fz_gen_start_useful is monotone: index <= wlen + min(max_dels, max_l) - m) spawn, the others only step what is
            // alive and stop when nothing is.  Round 5's phase stamps (profiles/r05_lab_ab.txt) had shown ~740 of a character's
            // ~1 640 cycles OUTSIDE the trip — loop control: the one loop over "spawn? / last character? / failed? / which half of
            // the equality words?" compiled into a maze of ~15 scalar branches and SGPR-spill reloads per character.
            const uint32_t dlim = a.max_dels < a.k ? a.max_dels : a.k;
            const uint32_t n_spawn = wlen + dlim >= a.m ? (wlen + dlim - a.m + 1u < wlen ? wlen + dlim - a.m + 1u : wlen) : 0u;
            // one window character over this wave's list (the fresh candidate, if any, at list position fresh_at)
            auto one_char = [&](uint32_t index, uint32_t fresh_at) -> bool {
                // (the window's equality words live in two register pairs, lane = window position: v_readlane with the
                //  character's number instead of an LDS round trip at the head of every character's chain; both halves are
                //  read and one is selected — no branch)
                const uint32_t il = index & 63u;
                const uint32_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)pw0l, (int)il), h0 = (uint32_t)__builtin_amdgcn_readlane((int)pw0h, (int)il);
                const uint32_t l1 = (uint32_t)__builtin_amdgcn_readlane((int)pw1l, (int)il), h1 = (uint32_t)__builtin_amdgcn_readlane((int)pw1h, (int)il);
                const bool low = index < 64u;
                const unsigned long long peq = (unsigned long long)(low ? l0 : l1) | ((unsigned long long)(low ? h0 : h1) << 32);
                const uint64_t stamp = (uint64_t)index << 48;
                uint32_t nnext = 0;
                // One TRIP steps U slices of 64 candidates: their loads, steps and prefix scans are independent chains that the
                // hardware overlaps, one pass of offsets, 5 U unconditional stores.  With pruned starts nearly every character
                // is ONE slice: that case is a straight line.
                auto trip = [&](auto uc, uint32_t c0) -> bool {
                    constexpr uint32_t U = decltype(uc)::value;
                    FzGStep st[U];
                    uint32_t packed[U], incl[U], base[U];
#pragma unroll
                    for (uint32_t u = 0; u < U; ++u) {
                        const uint32_t at = c0 + 64u * u + lane;
                        const bool valid = at < ncur;
                        uint2 cw = reinterpret_cast<const uint2 *>(lc)[at];      // (past the list: still this workgroup's LDS)
                        const bool fresh = at == fresh_at;
                        cw.x = valid ? (fresh ? index : cw.x) : 0u;
                        cw.y = valid && !fresh ? cw.y : 0u;
                        fz_generic_step_bits(cw.x, cw.y, peq, index, a.m, a.max_subs, a.max_ins, a.max_dels, a.k, st[u]);
                        const uint32_t vm = valid ? 1u : 0u;
                        st[u].fa &= vm; st[u].fb &= vm; st[u].fc &= vm; st[u].f1 &= vm; st[u].f2 &= vm;
                        packed[u] = (st[u].fa + st[u].fb + st[u].fc) | ((st[u].f1 + st[u].f2) << 16);
                    }
#pragma unroll
                    for (uint32_t u = 0; u < U; ++u) incl[u] = fz_wave_incl_scan(packed[u]);
                    uint32_t tot = 0;
#pragma unroll
                    for (uint32_t u = 0; u < U; ++u) { base[u] = tot; tot += (uint32_t)__builtin_amdgcn_readlane((int)incl[u], 63); }
                    const uint32_t tot_s = tot & 0xffffu, tot_m = tot >> 16;
                    if (nnext + tot_s > capw || mb + tot_m > FZ_GH_MCAP) return false;
#pragma unroll
                    for (uint32_t u = 0; u < U; ++u) {
                        const uint32_t excl = incl[u] - packed[u] + base[u];
                        uint2 *nx = reinterpret_cast<uint2 *>(ln) + nnext + (excl & 0xffffu);
                        uint64_t *mp = mbuf + mb + (excl >> 16);
                        // five stores, none of them conditional: an absent output lands in this lane's dummy slot
                        uint2 *pa = st[u].fa ? nx : dummy;
                        uint2 *pb = st[u].fb ? nx + st[u].fa : dummy;
                        uint2 *pc = st[u].fc ? nx + st[u].fa + st[u].fb : dummy;
                        uint64_t *p1 = st[u].f1 ? mp : reinterpret_cast<uint64_t *>(dummy);
                        uint64_t *p2 = st[u].f2 ? mp + st[u].f1 : reinterpret_cast<uint64_t *>(dummy);
                        *pa = make_uint2(st[u].a0, st[u].a1);
                        *pb = make_uint2(st[u].b0, st[u].b1);
                        *pc = make_uint2(st[u].c0, st[u].c1);
                        *p1 = (uint64_t)st[u].m1 | ((uint64_t)st[u].d1 << 32) | stamp;
                        *p2 = (uint64_t)st[u].m2 | ((uint64_t)st[u].d2 << 32) | stamp;
                    }
                    nnext = fz_uniform(nnext + tot_s);
                    mb = fz_uniform(mb + tot_m);
                    return true;
                };
                bool ok = true;
                if (ncur <= 64u) {
                    ok = trip(std::integral_constant<uint32_t, 1>{}, 0u);
                } else {
                    for (uint32_t c0 = 0; c0 < ncur && ok;) {
                        if (ncur - c0 > 64u) { ok = trip(std::integral_constant<uint32_t, 2>{}, c0); c0 += 128u; }
                        else { ok = trip(std::integral_constant<uint32_t, 1>{}, c0); c0 += 64u; }
                    }
                }
                // the next character reads what this one stored: a wave's LDS operations are performed in issue order
                asm volatile("" ::: "memory");
                FzGCand *tmp = lc; lc = ln; ln = tmp;
                ncur = fz_uniform(nnext);
                return ok;
            };
            uint32_t index = 0;
            for (; index < n_spawn; ++index) {
                uint32_t fresh_at = 0xffffffffu;
                if ((index & (W - 1u)) == wave) {               // this start is ours: the fresh candidate (py:80), taken from registers
                    if (ncur >= capw) { fail = true; break; }
                    fresh_at = ncur;
                    ncur = fz_uniform(ncur + 1u);
                }
                if (ncur != 0u && !one_char(index, fresh_at)) { fail = true; break; }
            }
            if (!fail)
                for (; index < wlen && ncur != 0u; ++index)
                    if (!one_char(index, 0xffffffffu)) { fail = true; break; }
            if (!fail && ncur != 0u) final_flush();
        } else {
        for (uint32_t index = 0; index <= wlen && !fail; ++index) {
            uint32_t nnext = 0;
            // nothing alive and no start left that could still reach the pattern's end: the rest of the window emits nothing
            if (ncur == 0u && !fz_gen_start_useful(index, wlen, a.m, a.max_dels, a.k)) break;
            if (index < wlen) {
                const uint8_t ch = (uint8_t)fz_uniform(win[index]);
                uint32_t fresh_at = 0xffffffffu;
                // this start is ours: the fresh candidate (py:80), taken from registers — unless nothing that starts here can
                // reach the pattern's end inside the window (fz_gen_start_useful)
                if ((index & (W - 1u)) == wave && fz_gen_start_useful(index, wlen, a.m, a.max_dels, a.k)) {
                    if (ncur >= capw) { fail = true; break; }
                    fresh_at = ncur;
                    ncur = fz_uniform(ncur + 1u);
                }
                for (uint32_t c0 = 0; c0 < ncur; c0 += 64u) {
                    const bool valid = c0 + lane < ncur;
                    uint2 cw = reinterpret_cast<const uint2 *>(lc)[c0 + lane];      // (up to 63 slots past the list: still this workgroup's LDS)
                    const bool fresh = c0 + lane == fresh_at;
                    cw.x = valid ? (fresh ? index : cw.x) : 0u;
                    cw.y = valid && !fresh ? cw.y : 0u;
                    FzGStep st;
                    fz_generic_step_packed(cw.x, cw.y, ch, index, a.m, patf, a.max_subs, a.max_ins, a.max_dels, a.k, st);
                    const uint32_t vm = valid ? 1u : 0u;
                    st.fa &= vm; st.fb &= vm; st.fc &= vm; st.f1 &= vm; st.f2 &= vm;
                    const uint32_t packed = (st.fa + st.fb + st.fc) | ((st.f1 + st.f2) << 16);
                    const uint32_t incl = fz_wave_incl_scan(packed);
                    const uint32_t tot = __builtin_amdgcn_readlane(incl, 63);
                    const uint32_t excl = incl - packed;
                    const uint32_t tot_s = tot & 0xffffu, tot_m = tot >> 16;
                    if (nnext + tot_s > capw || mb + tot_m > FZ_GH_MCAP) { fail = true; break; }
                    uint2 *nx = reinterpret_cast<uint2 *>(ln) + nnext + (excl & 0xffffu);
                    uint64_t *mp = mbuf + mb + (excl >> 16);
                    const uint64_t stamp = (uint64_t)index << 48;
                    if (st.fa) nx[0] = make_uint2(st.a0, st.a1);
                    if (st.fb) nx[st.fa] = make_uint2(st.b0, st.b1);
                    if (st.fc) nx[st.fa + st.fb] = make_uint2(st.c0, st.c1);
                    if (st.f1) mp[0] = (uint64_t)st.m1 | ((uint64_t)st.d1 << 32) | stamp;
                    if (st.f2) mp[st.f1] = (uint64_t)st.m2 | ((uint64_t)st.d2 << 32) | stamp;
                    nnext = fz_uniform(nnext + tot_s);
                    mb = fz_uniform(mb + tot_m);
                }
            } else {
                final_flush();
            }
            // the next character reads what this one stored: a wave's LDS operations are performed in issue order
            asm volatile("" ::: "memory");
            FzGCand *tmp = lc; lc = ln; ln = tmp;
            ncur = fz_uniform(nnext);
        }
        }
        if (lane == 0) { ctl[2u + wave] = mb; if (fail) ctl[1] = 1u; }
        __syncthreads();
        if (fz_uniform(ctl[1])) {                           // outgrew a list quarter or a match buffer: the host re-runs with fz_lp_kernel
            if (tid == 0) atomicAdd(&counters[FZ_HDR_GEN_FAIL], 1ull);
            continue;
        }
        uint32_t mbw[W];
        uint32_t total = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; ++w) { mbw[w] = fz_uniform(ctl[2u + w]); total += mbw[w]; }
        if (order && q < FZ_GEN_ORDER_MAX && tid == 0) { order_first[q] = 0; order_count[q] = total; }
        if (total == 0) continue;
        if (fold) {
            // first stage of consolidate_overlapping_matches (common.py:150-159), as in fz_lp_kernel: every match that overlaps
            // the running hull is folded into it; the order of the matches does not matter (best = a total order), so wave 0
            // takes the four buffers one after the other
            if (wave == 0) {
                bool f_have = false;
                uint32_t f_lo = 0, f_hi = 0, f_k1 = 0, f_k2 = 0, f_pairs = 0;
                auto emit_pair = [&]() {
                    if (lane == 0) {
                        // (window table: a pair with an empty hull once per member of the window — see fz_lp_kernel)
                        const uint32_t sl = dedup ? dd.wslot[q] : FZ_GEN_DEDUP_NONE;
                        uint32_t copies = 1u;
                        if (sl != FZ_GEN_DEDUP_NONE && f_lo == f_hi) { copies = dd.nmem[sl]; copies = copies < FZ_GEN_DEDUP_MEMBERS ? copies : FZ_GEN_DEDUP_MEMBERS; }
                        for (uint32_t cpy = 0; cpy < copies; ++cpy) {
                            const unsigned long long slot = atomicAdd(&counters[1], 1ull);
                            if (slot < a.rec_cap) {
                                const uint32_t len = 0xffffu - (f_k1 & 0xffffu);
                                FzGenRec r;
                                r.key = copies > 1u ? hits[dd.mem[sl * FZ_GEN_DEDUP_MEMBERS + cpy]] : hit;
                                r.seq = f_pairs; r.se = f_k2 | ((f_k2 + len) << 16); r.dist = f_k1 >> 16; r.win = f_lo | (f_hi << 16);
                                recs[slot] = r;
                            }
                        }
                    }
                    ++f_pairs;
                    f_have = false;
                };
                auto wave_min = [&](uint32_t v) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)fz_wave_incl_min(v), 63); };
                for (uint32_t w = 0; w < W; ++w) {
                    const uint64_t *mbx = mball + (size_t)w * FZ_GH_MCAP;
                    const uint32_t nw = fz_uniform(ctl[2u + w]);
                    for (uint32_t e0 = 0; e0 < nw; e0 += 64u) {
                        const bool have_row = e0 + lane < nw;
                        const uint64_t v = have_row ? mbx[e0 + lane] : 0ull;
                        const uint32_t rs = (uint32_t)v & 0xffffu, re = ((uint32_t)v >> 16) & 0xffffu, rd = (uint32_t)(v >> 32) & 0xffffu;
                        const uint32_t k1 = (rd << 16) | (0xffffu - (re - rs));
                        unsigned long long pending = __ballot(have_row);
                        while (pending) {
                            if (!f_have) {
                                const uint32_t l0 = (uint32_t)__builtin_ctzll(pending);
                                f_lo = (uint32_t)__builtin_amdgcn_readlane((int)rs, (int)l0);
                                f_hi = (uint32_t)__builtin_amdgcn_readlane((int)re, (int)l0);
                                f_k1 = (uint32_t)__builtin_amdgcn_readlane((int)k1, (int)l0);
                                f_k2 = f_lo;
                                f_have = true;
                                pending &= pending - 1ull;
                                continue;
                            }
                            const bool mine = ((pending >> lane) & 1ull) && !(re <= f_lo || rs >= f_hi);
                            const unsigned long long ov = __ballot(mine);
                            if (!ov) { emit_pair(); continue; }
                            const uint32_t mlo = wave_min(mine ? rs : 0xffffffffu), mhi = ~wave_min(mine ? ~re : 0xffffffffu);
                            const uint32_t mk1 = wave_min(mine ? k1 : 0xffffffffu);
                            const uint32_t mk2 = wave_min((mine && k1 == mk1) ? rs : 0xffffffffu);
                            f_lo = mlo < f_lo ? mlo : f_lo;
                            f_hi = mhi > f_hi ? mhi : f_hi;
                            if (mk1 < f_k1 || (mk1 == f_k1 && mk2 < f_k2)) { f_k1 = mk1; f_k2 = mk2; }
                            pending &= ~ov;
                        }
                    }
                }
                if (f_have) emit_pair();
            }
            continue;
        }
        // the hit's records, contiguous and in emission order: record (base + rank), rank = the match's place among the four
        // sorted buffers (its own position + the entries of the other waves with a smaller (character, start))
        if (tid == 0) {
            const unsigned long long base = atomicAdd(&counters[1], (unsigned long long)total);
            ctl[6] = (uint32_t)base; ctl[7] = (uint32_t)(base >> 32);
        }
        __syncthreads();
        const unsigned long long base = (unsigned long long)ctl[6] | ((unsigned long long)ctl[7] << 32);
        for (uint32_t e = lane; e < mb; e += 64u) {
            const uint64_t v = mbuf[e];
            const uint32_t key = ((uint32_t)(v >> 48) << 16) | ((uint32_t)v & 0xffffu);
            uint32_t rank = e;
#pragma unroll
            for (uint32_t w = 0; w < W; ++w)
                if (w != wave) rank += fz_gh_lower_bound(mball + (size_t)w * FZ_GH_MCAP, mbw[w], key);
            if (base + rank < a.rec_cap) {
                FzGenRec r;
                r.key = hit; r.seq = rank; r.se = (uint32_t)v; r.dist = (uint32_t)(v >> 32) & 0xffffu; r.win = order ? (uint32_t)q : sg.j;
                recs[base + rank] = r;
            }
        }
    }
    // folded search whose pairs went straight into the host's staging buffer: the last workgroup publishes the counters
    __syncthreads();
    fz_finish_launch(a, counters, reinterpret_cast<volatile uint32_t *>(smem + mpad + wpad + 60u));
}

// Reference order of the generic search's rows (generic_search.py:221-237: blocks in order, the hits of a block by
// index, the matches of a hit in emission order) restored on the device.  A hit's first row = the rows of all hits
// with a smaller key (block << 56 | index).  Quadratic, tiled 256 x 64 over (hit, other hit) pairs with partial
// sums added atomically (6e3 hits = 2304 tiles); the host orders searches with more than FZ_GEN_ORDER_MAX hits.
__device__ __forceinline__ unsigned long long *counters_rw(const unsigned long long *c) { return const_cast<unsigned long long *>(c); }

__global__ __launch_bounds__(256) void fz_gen_order_kernel(const uint64_t *__restrict__ hits, const FzScanArgs a,
                                                           const unsigned long long *counters) {
    constexpr uint32_t TJ = 64;                                 // other hits per tile: the length of a thread's serial chain
    __shared__ uint64_t skey[TJ];
    __shared__ uint32_t scnt[TJ];
    const unsigned long long n = counters[0];
    if (n > a.hit_cap || n > FZ_GEN_ORDER_MAX || counters[2]) return;
    unsigned long long *first = reinterpret_cast<unsigned long long *>(a.gen_order);
    const uint32_t *count = reinterpret_cast<const uint32_t *>(first + FZ_GEN_ORDER_MAX);
    // rows of hit j: its own, or — window table — those of its window's leader (the hit of the smallest block)
    const bool dedup = a.gen_dedup != 0;
    const FzGenDedup dd(a.gen_dedup);
    auto rows_of = [&](uint32_t j) -> uint32_t {
        if (!dedup) return count[j];
        const uint32_t sl = dd.wslot[j];
        return count[sl == FZ_GEN_DEDUP_NONE ? j : dd.leader(sl)];
    };
    const uint32_t nti = ((uint32_t)n + 255u) / 256u, ntj = ((uint32_t)n + TJ - 1u) / TJ;
    for (uint32_t p = blockIdx.x; p < nti * ntj; p += gridDim.x) {
        const uint32_t i = (p / ntj) * 256u + threadIdx.x, j = (p % ntj) * TJ + threadIdx.x;
        __syncthreads();
        if (threadIdx.x < TJ) {
            skey[threadIdx.x] = j < n ? hits[j] : ~0ull;
            scnt[threadIdx.x] = j < n ? rows_of(j) : 0u;
        }
        __syncthreads();
        if (p % ntj == 0 && threadIdx.x < TJ) {                 // the search's row count: every hit once (tile column 0 of its row)
            uint32_t mine = 0;
            for (uint32_t ii = (p / ntj) * 256u + threadIdx.x; ii < (p / ntj) * 256u + 256u && ii < n; ii += TJ) mine += rows_of(ii);
            if (mine) atomicAdd(&counters_rw(counters)[FZ_HDR_GEN_ROWS], (unsigned long long)mine);
        }
        if (i < n) {
            const uint64_t me = hits[i];
            uint32_t sum = 0;                                   // <= TJ * rows of one hit
#pragma unroll 16
            for (uint32_t t = 0; t < TJ; ++t) sum += skey[t] < me ? scnt[t] : 0u;
            if (sum) atomicAdd(&first[i], (unsigned long long)sum);
        }
    }
}

// ... and every record goes to row (first row of its hit + emission number) as a finished fz_match.
__global__ __launch_bounds__(256) void fz_gen_scatter_kernel(const uint64_t *__restrict__ hits, const FzScanArgs a,
                                                             const FzGenRec *__restrict__ recs, FzOutRow *__restrict__ rows,
                                                             const unsigned long long *__restrict__ counters) {
    const unsigned long long n = counters[0], nr = counters[1];
    if (n > a.hit_cap || n > FZ_GEN_ORDER_MAX || counters[2] || nr > a.rec_cap) return;
    const unsigned long long *first = reinterpret_cast<const unsigned long long *>(a.gen_order);
    const bool dedup = a.gen_dedup != 0;
    const FzGenDedup dd(a.gen_dedup);
    for (unsigned long long r = (unsigned long long)blockIdx.x * 256u + threadIdx.x; r < nr; r += (unsigned long long)gridDim.x * 256u) {
        const FzGenRec rec = recs[r];
        const uint32_t sl = dedup ? dd.wslot[rec.win] : FZ_GEN_DEDUP_NONE;
        if (sl == FZ_GEN_DEDUP_NONE) {                          // a hit on its own
            const unsigned long long at = first[rec.win] + rec.seq;
            if (at < a.rows_cap) rows[at] = fz_gen_row(hits[rec.win], a.L, a.k, 0, rec.se, rec.dist);
            continue;
        }
        if (dd.leader(sl) != rec.win) continue;                 // ran before a hit of a smaller block arrived: that one's records count
        uint32_t nm = dd.nmem[sl];
        nm = nm < FZ_GEN_DEDUP_MEMBERS ? nm : FZ_GEN_DEDUP_MEMBERS;
        for (uint32_t i = 0; i < nm; ++i) {                     // the same match for every hit of the window (the leader is a member too)
            const uint32_t h = dd.mem[sl * FZ_GEN_DEDUP_MEMBERS + i];
            const unsigned long long at = first[h] + rec.seq;
            if (at < a.rows_cap) rows[at] = fz_gen_row(hits[h], a.L, a.k, 0, rec.se, rec.dist);
        }
    }
}

// (f)3  Substitutions-only without the n-gram filter (_find_near_matches_substitutions_lp,
// substitutions_only.py:82-136): every window with Hamming distance <= k.  One lane per start.
__global__ __launch_bounds__(256) void fz_hamming_kernel(const uint8_t *__restrict__ buf, const FzScanArgs a,
                                                         FzRec *__restrict__ recs,
                                                         unsigned long long *__restrict__ counters) {
    __shared__ uint8_t pat_s[FZ_MAX_M];
    const bool in_lds = a.m <= FZ_MAX_M;                               // longer patterns are read from HBM (uniform address: one broadcast load)
    if (in_lds) for (uint32_t i = threadIdx.x; i < a.m; i += blockDim.x) pat_s[i] = a.pat[i];
    __syncthreads();
    const uint8_t *pat_g = reinterpret_cast<const uint8_t *>(a.pat_g);
    const uint64_t lo = a.geom.own_lo;
    uint64_t hi = a.geom.own_hi;                                       // starts i with i + m <= n
    if (a.geom.n < a.m) hi = lo;
    else if (hi > a.geom.n - a.m + 1) hi = a.geom.n - a.m + 1;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t span = hi > lo ? hi - lo : 0;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < span; base += stride) {
        if ((a.flags & FZ_FLAG_ANY) && __hip_atomic_load(&counters[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) break;   // has_near_match_*
        const uint64_t i = lo + base + threadIdx.x;
        bool ok = base + threadIdx.x < span;
        uint32_t d = 0;
        if (ok) {
            const uint8_t *t = buf + (i - a.geom.buf_off);
            if (in_lds) { for (uint32_t q = 0; q < a.m && d <= a.k; ++q) d += (pat_s[q] != t[q]) ? 1u : 0u; }
            else { for (uint32_t q = 0; q < a.m && d <= a.k; ++q) d += (pat_g[q] != t[q]) ? 1u : 0u; }
            ok = d <= a.k;
        }
        const unsigned long long mask = __ballot(ok);
        if (mask) {
            unsigned long long slot0 = 0;
            if (fz_lane() == 0) slot0 = atomicAdd(&counters[1], (unsigned long long)__popcll(mask));
            slot0 = fz_bcast64(slot0);
            if (ok) {
                const unsigned long long slot = slot0 + fz_rank(mask);
                if (slot < a.rec_cap) { FzRec r; r.key = i; r.l = 0; r.r = 0; r.dist = d; r.aux = 0; recs[slot] = r; }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Multi-pattern search (fz_device.h: the fz_mp_* table).  Two kernels per group of patterns, whatever their number:
//
//   fz_mp_filter_kernel  one streaming pass in fz_scan_kernel's layout (16 KiB tiles, a 16-byte load + 8-byte halo per lane
//       and row).  Per byte offset: the window hash (two v_alignbyte, one v_mad_u32_u24), one LDS dword of the signature, one
//       bit test.  With hundreds of n-grams "some lane fired" is the common case, not the rare one, so survivors do not go
//       through a wave-uniform branch per group of offsets and a queue of positions to re-check: every offset of a row has
//       its own ballot, a fired offset looks its full hash up in the slot table (the signature's false positives end here)
//       and the run of block-table entries it names is compacted by ballot / mbcnt into the wave's queue of finished hits
//       (entry << 48 | global index).  A full queue is appended to a hit list in HBM with ONE atomic; the workgroups spread
//       over FZ_MP_LISTS lists with counters a cache line apart (a single counter word sustains ~90 atomics/us chip-wide:
//       5e7 hits per GiB in queues of 256 would spend 2 ms on one word).
//       LDS: 12 KiB of table + 4 x 2 KiB of queues = 20 KiB per workgroup, 8 workgroups per CU.
//   fz_mp_verify_kernel  the hit lists, one candidate per lane, 64 at a time, as fz_verify_kernel does for one pattern — the
//       acceptance range of the block (fz_block_range + ownership), the window staged in LDS, the exact n-gram test, then
//       fz_verify_lev (right, then left, last arg-min) — against the LANE's pattern: bytes and length come from the group's
//       pattern table in LDS, the block's start from its block-table entry.  Records carry the pattern id in `aux`.
#define FZ_MP_LISTS 16u
#define FZ_MP_QCAP 256u                                    // hits a wave queues before it appends them
#define FZ_MP_CTR_WORDS 512u                               // 64-bit counters of a group launch:
#define FZ_MP_CTR_RECS 1u                                  //   [1] records, [8 .. 71] confirmed-hit tallies,
#define FZ_MP_CTR_LIST(l) (128u + 16u * (l))               //   [128 + 16 l] hits appended to list l (128 bytes apart)
#define FZ_MP_FILTER_LDS (FZ_MP_FILTER_WORDS * 4u + FZ_WAVES_PER_BLOCK * FZ_MP_QCAP * 8u)
#define FZ_MP_RING_SLOTS (2u * FZ_MP_MAX_K + 2u)           // score ring of fz_expand (budgets above FZ_REG_BAND_MAX only)

__host__ __device__ inline uint32_t fz_mp_verify_wave_bytes(uint32_t win_dwords) { return win_dwords * 256u + FZ_MP_RING_SLOTS * 128u; }
__host__ __device__ inline uint32_t fz_mp_verify_lds(uint32_t win_dwords) {
    return FZ_MP_VERIFY_WORDS * 4u + FZ_WAVES_PER_BLOCK * fz_mp_verify_wave_bytes(win_dwords);
}

template <int DH>
__global__ __launch_bounds__(FZ_FILTER_THREADS) void fz_mp_filter_kernel(const uint8_t *__restrict__ buf, const FzMpArgs a, uint64_t ntiles,
                                                                         const uint32_t *__restrict__ desc, uint64_t *__restrict__ hits,
                                                                         unsigned long long *__restrict__ counters) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t *sig = reinterpret_cast<uint32_t *>(smem);
    const uint32_t *slots = sig + FZ_MP_DESC_SLOTS;
    for (uint32_t i = threadIdx.x; i < FZ_MP_FILTER_WORDS; i += FZ_FILTER_THREADS) sig[i] = desc[i];
    __syncthreads();
    const uint32_t wave = fz_uniform(threadIdx.x >> 6);
    const uint32_t lane = fz_lane();
    const uint32_t lane_off = threadIdx.x * 16u;
    uint64_t *queue = reinterpret_cast<uint64_t *>(smem + FZ_MP_FILTER_WORDS * 4u) + wave * FZ_MP_QCAP;
    const uint32_t list = blockIdx.x % FZ_MP_LISTS;
    uint64_t *lhits = hits + (uint64_t)list * a.hit_cap;
    unsigned long long *lctr = counters + FZ_MP_CTR_LIST(list);
    const uint64_t data_end = a.geom.buf_off + a.geom.buf_len;
    uint32_t qn = 0;                                       // wave-uniform queue fill

    auto flush = [&]() {
        fz_wave_lds_sync();
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(lctr, (unsigned long long)qn);
        base = fz_bcast64(base);
        for (uint32_t i = lane; i < qn; i += 64u)
            if (base + i < a.hit_cap) lhits[base + i] = queue[i];      // (an overflowing list: the counter tells, the host re-runs)
        qn = 0;
        fz_wave_lds_sync();
    };

    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint8_t *tsrc = buf + fz_bcast64(tile * (uint64_t)FZ_TILE_BYTES);
        uint4 v[FZ_FILTER_ROWS];
        uint2 hl[FZ_FILTER_ROWS];
#pragma unroll
        for (int r = 0; r < FZ_FILTER_ROWS; ++r) {
            v[r] = *reinterpret_cast<const uint4 *>(tsrc + r * FZ_ROW_BYTES + lane_off);
            hl[r] = *reinterpret_cast<const uint2 *>(tsrc + r * FZ_ROW_BYTES + lane_off + 16);
        }
        const uint64_t gtile = a.geom.buf_off + tile * (uint64_t)FZ_TILE_BYTES + lane_off;
#pragma unroll
        for (int r = 0; r < FZ_FILTER_ROWS; ++r) {
            const uint32_t w[7] = {v[r].x, v[r].y, v[r].z, v[r].w, hl[r].x, hl[r].y, 0u};
            uint32_t hv[16];
            uint32_t fired = 0;
#pragma unroll
            for (int o = 0; o < 16; ++o) {
                hv[o] = __umul24(FZ_WIN(w, o + DH), FZ_MP_HASH_K) + FZ_WIN(w, o);
                const uint32_t t = fz_mp_sig_bit(hv[o]);
                fired |= ((sig[t >> 5] >> (t & 31u)) & 1u) << o;
            }
            if (!__ballot(fired != 0u)) continue;
#pragma unroll
            for (int o = 0; o < 16; ++o) {
                const bool f = ((fired >> o) & 1u) != 0u;
                if (!__ballot(f)) continue;
                const uint64_t gidx = gtile + (uint64_t)(r * FZ_ROW_BYTES + o);
                uint32_t e = 0;
                if (f && gidx >= a.geom.own_lo && gidx < a.geom.own_hi && gidx + a.L <= data_end) e = fz_mp_lookup(slots, hv[o]);
                uint32_t first = e & 0xffffu, cnt = e >> 16;
                for (;;) {
                    const unsigned long long mk = __ballot(cnt != 0u);
                    if (!mk) break;
                    if (qn + 64u > FZ_MP_QCAP) flush();
                    if (cnt != 0u) queue[qn + fz_rank(mk)] = fz_hit_pack(first, gidx);
                    qn += (uint32_t)__popcll(mk);
                    if (cnt != 0u) { ++first; --cnt; }
                }
            }
        }
    }
    if (qn) flush();
}

__global__ __launch_bounds__(FZ_FILTER_THREADS) void fz_mp_verify_kernel(const uint8_t *__restrict__ buf, const FzMpArgs a,
                                                                         const uint32_t *__restrict__ desc, const uint64_t *__restrict__ hits,
                                                                         FzRec *__restrict__ recs, unsigned long long *__restrict__ counters) {
    constexpr bool RAG = false;
#define FZ_KERNEL_BODY 5
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}
// The same text over a batch (fz_batch_search_multi): the candidate's own sequence — one fz_segment_ragged lookup per lane,
// after the entry checks and before anything is staged — takes the place of [0, n) in the block's range, the window's clamps
// and fz_verify_lev (fz_device.h: fz_mp_rag_accept).  A kernel of its own, so fz_mp_verify_kernel's code does not move.
__global__ __launch_bounds__(FZ_FILTER_THREADS) void fz_mp_batch_verify_kernel(const uint8_t *__restrict__ buf, const FzMpArgs a,
                                                                               const uint32_t *__restrict__ desc, const uint64_t *__restrict__ hits,
                                                                               FzRec *__restrict__ recs, unsigned long long *__restrict__ counters) {
    constexpr bool RAG = true;
#define FZ_KERNEL_BODY 5
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}

// fz_mp_verify_kernel's counterpart for substitutions-only groups (fz_subs_ngrams_multi): same launch shape, hit lists,
// counters and records; per candidate the reference's _substitutions_only_ngrams_template.h:97-121 against the LANE's pattern.
//   * the block's hit range is fz_block_range(FZ_MODE_SUBS): the window [idx - s, idx - s + m) lies inside [0, n) — no clamps,
//     no +-k reach, so the window is staged whole or the candidate is dropped, and there is no score ring: a wave's LDS is
//     win_dwords x 256 bytes with win_dwords = (longest m + 3) / 4 + 1;
//   * window dword d of lane l sits at win[d * 64 + l]: a ds_read_b32 banks by dword address mod 32 within each 32-lane
//     half, so the lanes of a half read 32 different banks — no conflicts, whatever the lanes' alignments;
//   * the pattern table is TRANSPOSED on its way into LDS: dword j of pattern i at pat4[j * 64 + i].  The descriptor's rows
//     are 128 bytes = 32 dwords apart, which would put dword j of EVERY pattern on bank j: up to 32-way when every lane of a
//     half holds another pattern.  Transposed, the bank is i mod 32: lanes of one pattern broadcast, lanes of different
//     patterns conflict two-way at the most (patterns i and i + 32 in one half);
//   * exact n-gram test (fz_mp_block_equal), then the mismatches outside the block (fz_mp_verify_subs), both a dword per
//     step and wave-uniform in their trip counts.
struct FzLdsColumn {
    const uint32_t *base;                                  // the lane's dword 0; consecutive dwords are 64 apart
    __device__ __forceinline__ uint32_t dword(uint32_t j) const { return base[j * 64u]; }
};

__host__ __device__ inline uint32_t fz_mp_verify_subs_lds(uint32_t win_dwords) {
    return FZ_MP_VERIFY_WORDS * 4u + FZ_WAVES_PER_BLOCK * win_dwords * 256u;
}

__global__ __launch_bounds__(FZ_FILTER_THREADS) void fz_mp_verify_subs_kernel(const uint8_t *__restrict__ buf, const FzMpArgs a,
                                                                              const uint32_t *__restrict__ desc, const uint64_t *__restrict__ hits,
                                                                              FzRec *__restrict__ recs, unsigned long long *__restrict__ counters) {
    constexpr bool RAG = false;
#define FZ_KERNEL_BODY 6
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}
// ... and over a batch: the window [idx - s, idx - s + m) lies inside the candidate's own sequence (fz_mp_rag_accept).  The
// dword-granular staging may bring up to 3 bytes of a neighbouring sequence or of the padding along; fz_mp_block_equal and
// fz_mp_verify_subs mask them.
__global__ __launch_bounds__(FZ_FILTER_THREADS) void fz_mp_batch_verify_subs_kernel(const uint8_t *__restrict__ buf, const FzMpArgs a,
                                                                                    const uint32_t *__restrict__ desc, const uint64_t *__restrict__ hits,
                                                                                    FzRec *__restrict__ recs, unsigned long long *__restrict__ counters) {
    constexpr bool RAG = true;
#define FZ_KERNEL_BODY 6
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}

// fz_mp_verify_subs_kernel's counterpart for groups with symbol classes (fz_subs_ngrams_multi_cls; fz_device.h: the class
// descriptor): same launch shape, hit lists, counters, records, staging and acceptance.  Kernels of their own, so the
// substitutions kernels' code does not move.  What differs per candidate:
//   * the mask rows ride into LDS transposed exactly as the pattern rows do (dword j of pattern i at msk4[j * 64 + i]) and
//     tmask follows as 256 bytes; a workgroup's tables are FZ_MP_CLS_VERIFY_WORDS dwords (17.5 KiB) in front of the windows;
//   * the block test is class-exact (fz_mp_block_match_cls) and the count is the class mismatches outside the block
//     (fz_mp_verify_cls): the dword xor as before, and one tmask byte read for a differing byte at a class position — the
//     lanes' addresses are data-dependent there, as a table lookup's are, and plain positions never reach it.
__host__ __device__ inline uint32_t fz_mp_verify_cls_lds(uint32_t win_dwords) {
    return FZ_MP_CLS_VERIFY_WORDS * 4u + FZ_WAVES_PER_BLOCK * win_dwords * 256u;
}

__global__ __launch_bounds__(FZ_FILTER_THREADS) void fz_mp_verify_cls_kernel(const uint8_t *__restrict__ buf, const FzMpArgs a,
                                                                             const uint32_t *__restrict__ desc, const uint64_t *__restrict__ hits,
                                                                             FzRec *__restrict__ recs, unsigned long long *__restrict__ counters) {
    constexpr bool RAG = false;
#define FZ_KERNEL_BODY 7
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}
// ... and over a batch (fz_batch_search_multi_cls, fz_batch_assign_cls).  The bytes of a neighbouring sequence or of the
// padding that the dword-granular staging brings along lie outside the byte masks of both tests, and the masks cover the
// class lookup too: such a byte is neither compared nor looked up.
__global__ __launch_bounds__(FZ_FILTER_THREADS) void fz_mp_batch_verify_cls_kernel(const uint8_t *__restrict__ buf, const FzMpArgs a,
                                                                                   const uint32_t *__restrict__ desc, const uint64_t *__restrict__ hits,
                                                                                   FzRec *__restrict__ recs, unsigned long long *__restrict__ counters) {
    constexpr bool RAG = true;
#define FZ_KERNEL_BODY 7
#include "fz_kernel_bodies.inc"
#undef FZ_KERNEL_BODY
}

// ---------------------------------------------------------------------------------------------
// Best-pattern assignment (fz_batch_assign; fz_device.h: fz_assign_*).  Behind a verification launch the records are in HBM
// and the answer a demultiplexer wants is a minimum per sequence over them:
//
//   fz_assign_reduce_kernel  one record per lane, grid-strided: its sequence (the ragged lookup the verification ran), its two
//       keys, then an unsigned atomic minimum on lo[seq] (u64) and on hi[seq] (u32), device scope, no return value.  Before
//       each atomic the lane reads the entry with a relaxed device-scope load and skips the atomic when the entry is already
//       <= its key: the tables only ever decrease, so a stale value can cost a superfluous atomic, never a wrong skip.  Records
//       that concentrate in one sequence (one long read, periodic reads) would otherwise serialise on one word at the ~90
//       atomics/us a single word sustains.  No LDS.
//   fz_assign_finish_kernel  one lane per sequence: the two entries decoded into the 16-byte output row.
#define FZ_ASSIGN_THREADS 256u

__global__ __launch_bounds__(FZ_ASSIGN_THREADS) void fz_assign_reduce_kernel(const FzRec *__restrict__ recs, uint64_t n_recs, uint32_t L,
                                                                             FzRagged rag, uint64_t n, const FzAssignPat *__restrict__ pat,
                                                                             uint32_t npat, uint32_t k, unsigned long long *__restrict__ lo,
                                                                             uint32_t *__restrict__ hi) {
    const uint64_t stride = (uint64_t)gridDim.x * FZ_ASSIGN_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * FZ_ASSIGN_THREADS + threadIdx.x; i < n_recs; i += stride) {
        const FzRec r = recs[i];
        uint32_t seq, khi;
        uint64_t klo;
        if (!fz_assign_keys(rag, n, r, L, pat, npat, k, seq, klo, khi)) continue;
        if (__hip_atomic_load(&lo[seq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > klo)
            (void)__hip_atomic_fetch_min(&lo[seq], (unsigned long long)klo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_load(&hi[seq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > khi)
            (void)__hip_atomic_fetch_min(&hi[seq], khi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(FZ_ASSIGN_THREADS) void fz_assign_finish_kernel(const unsigned long long *__restrict__ lo,
                                                                             const uint32_t *__restrict__ hi, uint64_t n_seqs,
                                                                             const uint32_t *__restrict__ pm, uint32_t k,
                                                                             FzAssignRow *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * FZ_ASSIGN_THREADS;
    for (uint64_t j = (uint64_t)blockIdx.x * FZ_ASSIGN_THREADS + threadIdx.x; j < n_seqs; j += stride)
        out[j] = fz_assign_row(lo[j], hi[j], pm, k);
}

// ---------------------------------------------------------------------------------------------
// Records (fz_batch_upload_records; fz_device.h: fz_rec_*): a text of lines is split into a batch where it lies, in HBM.
// Every step is a launch of its own on the context's stream and the launch boundaries are the only ordering between
// workgroups: nothing here waits for another workgroup inside a launch.
//
//   fz_rec_count_kernel        one workgroup per 16 KiB tile: newlines of the tile (16-byte loads, popcount of the byte mask)
//   fz_rec_scan_reduce_kernel  sum of FZ_RSCAN_ITEMS u64 per workgroup                  } exclusive scan of u64, any length:
//   fz_rec_scan_down_kernel    exclusive scan inside the workgroup + the scanned sum     } reduce, scan the sums, add back
//   fz_rec_lines_kernel        every newline's position at its global rank (tile base + rank inside the tile)
//   fz_rec_measure_kernel      one lane per record: start and length of its sequence, the FASTQ checks, the longest length
//   fz_rec_gather_kernel       packed[] by 16-byte pieces of the DESTINATION: a piece inside one sequence is one unaligned
//                              16-byte load and one aligned 16-byte store, whatever the sequence's length or alignment; a
//                              piece across a sequence end (1 in 9 for 150-byte reads) goes byte by byte
#define FZ_REC_THREADS 256u

// Exclusive scan of one value per thread over the FZ_REC_THREADS threads of a workgroup; total = the workgroup's sum.
__device__ __forceinline__ uint64_t fz_rec_block_scan(uint64_t v, uint64_t *wsum, uint64_t &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    uint64_t base = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < FZ_REC_THREADS / 64u; ++w) {
        const uint64_t s = wsum[w];
        if (w < wave) base += s;
        total += s;
    }
    __syncthreads();                                       // wsum is free for the next call
    return base + inc - v;
}

__device__ __forceinline__ uint32_t fz_rec_nl_count(const uint4 &v) {
    return (uint32_t)(__builtin_popcount(fz_rec_nl_mask(v.x)) + __builtin_popcount(fz_rec_nl_mask(v.y)) +
                      __builtin_popcount(fz_rec_nl_mask(v.z)) + __builtin_popcount(fz_rec_nl_mask(v.w)));
}

// raw: whole tiles (the bytes behind the text are zero).  counts[t] = newlines of tile t.
__global__ __launch_bounds__(FZ_REC_THREADS) void fz_rec_count_kernel(const uint8_t *__restrict__ raw, uint64_t ntiles,
                                                                      uint64_t *__restrict__ counts) {
    __shared__ uint32_t acc;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        if (threadIdx.x == 0) acc = 0;
        __syncthreads();
        const uint4 *src = reinterpret_cast<const uint4 *>(raw + t * (uint64_t)FZ_TILE_BYTES);
        uint32_t c = 0;
#pragma unroll
        for (uint32_t q = 0; q < FZ_TILE_BYTES / 16u / FZ_REC_THREADS; ++q) c += fz_rec_nl_count(src[q * FZ_REC_THREADS + threadIdx.x]);
#pragma unroll
        for (uint32_t d = 32; d; d >>= 1) c += __shfl_xor(c, d, 64);
        if ((threadIdx.x & 63u) == 0) atomicAdd(&acc, c);
        __syncthreads();
        if (threadIdx.x == 0) counts[t] = acc;
        __syncthreads();
    }
}

__global__ __launch_bounds__(FZ_RSCAN_THREADS) void fz_rec_scan_reduce_kernel(const uint64_t *__restrict__ in, uint64_t n,
                                                                             uint64_t *__restrict__ sums) {
    __shared__ uint64_t wsum[FZ_RSCAN_THREADS / 64u];
    const uint64_t nb = (n + FZ_RSCAN_ITEMS - 1u) / FZ_RSCAN_ITEMS;
    for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint64_t i0 = b * FZ_RSCAN_ITEMS + threadIdx.x * FZ_RSCAN_PER_THREAD;
        uint64_t s = 0;
#pragma unroll
        for (uint32_t q = 0; q < FZ_RSCAN_PER_THREAD; ++q) s += i0 + q < n ? in[i0 + q] : 0;
        uint64_t total;
        (void)fz_rec_block_scan(s, wsum, total);
        if (threadIdx.x == 0) sums[b] = total;
    }
}

// In place.  sums: the workgroups' sums after their own exclusive scan (null: one workgroup, nothing to add).
__global__ __launch_bounds__(FZ_RSCAN_THREADS) void fz_rec_scan_down_kernel(uint64_t *__restrict__ data, uint64_t n,
                                                                           const uint64_t *__restrict__ sums) {
    __shared__ uint64_t wsum[FZ_RSCAN_THREADS / 64u];
    const uint64_t nb = (n + FZ_RSCAN_ITEMS - 1u) / FZ_RSCAN_ITEMS;
    for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint64_t i0 = b * FZ_RSCAN_ITEMS + threadIdx.x * FZ_RSCAN_PER_THREAD;
        uint64_t x0 = i0 < n ? data[i0] : 0, x1 = i0 + 1u < n ? data[i0 + 1u] : 0, x2 = i0 + 2u < n ? data[i0 + 2u] : 0,
                 x3 = i0 + 3u < n ? data[i0 + 3u] : 0;
        static_assert(FZ_RSCAN_PER_THREAD == 4u, "four items per thread");
        uint64_t total;
        uint64_t run = fz_rec_block_scan(x0 + x1 + x2 + x3, wsum, total) + (sums ? sums[b] : 0);
        if (i0 < n) data[i0] = run;
        run += x0;
        if (i0 + 1u < n) data[i0 + 1u] = run;
        run += x1;
        if (i0 + 2u < n) data[i0 + 2u] = run;
        run += x2;
        if (i0 + 3u < n) data[i0 + 3u] = run;
    }
}

__device__ __forceinline__ void fz_rec_emit_word(uint32_t w, uint64_t pos, uint64_t *__restrict__ nl, uint64_t &at) {
    uint32_t m = fz_rec_nl_mask(w);
    while (m) {
        nl[at++] = pos + ((uint32_t)__builtin_ctz(m) >> 3);
        m &= m - 1u;
    }
}

// tile_base[t] = newlines in front of tile t (the exclusive scan of fz_rec_count_kernel's counts).  The pieces of a tile
// are taken in the order of the count kernel's loads (piece q * 256 + thread), which is the order of their positions.
__global__ __launch_bounds__(FZ_REC_THREADS) void fz_rec_lines_kernel(const uint8_t *__restrict__ raw, uint64_t ntiles,
                                                                      const uint64_t *__restrict__ tile_base, uint64_t *__restrict__ nl) {
    __shared__ uint64_t wsum[FZ_REC_THREADS / 64u];
    constexpr uint32_t Q = FZ_TILE_BYTES / 16u / FZ_REC_THREADS;
    static_assert(Q == 4u, "four 16-bit counters in one scanned word (a counter holds at most 16 * 256 * 4)");
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t tpos = t * (uint64_t)FZ_TILE_BYTES;
        const uint4 *src = reinterpret_cast<const uint4 *>(raw + tpos);
        const uint4 v0 = src[threadIdx.x], v1 = src[FZ_REC_THREADS + threadIdx.x], v2 = src[2u * FZ_REC_THREADS + threadIdx.x],
                    v3 = src[3u * FZ_REC_THREADS + threadIdx.x];
        const uint64_t mine = (uint64_t)fz_rec_nl_count(v0) | ((uint64_t)fz_rec_nl_count(v1) << 16) | ((uint64_t)fz_rec_nl_count(v2) << 32) |
                              ((uint64_t)fz_rec_nl_count(v3) << 48);
        uint64_t total;
        const uint64_t ex = fz_rec_block_scan(mine, wsum, total);
        if (total == 0) continue;                          // (uniform over the workgroup)
        const uint64_t base = tile_base[t];
        const uint64_t t0 = total & 0xffffu, t1 = (total >> 16) & 0xffffu, t2 = (total >> 32) & 0xffffu;
        uint64_t at;
        uint64_t pos = tpos + (uint64_t)threadIdx.x * 16u;
        at = base + (ex & 0xffffu);
        fz_rec_emit_word(v0.x, pos, nl, at); fz_rec_emit_word(v0.y, pos + 4u, nl, at);
        fz_rec_emit_word(v0.z, pos + 8u, nl, at); fz_rec_emit_word(v0.w, pos + 12u, nl, at);
        pos += FZ_REC_THREADS * 16u;
        at = base + t0 + ((ex >> 16) & 0xffffu);
        fz_rec_emit_word(v1.x, pos, nl, at); fz_rec_emit_word(v1.y, pos + 4u, nl, at);
        fz_rec_emit_word(v1.z, pos + 8u, nl, at); fz_rec_emit_word(v1.w, pos + 12u, nl, at);
        pos += FZ_REC_THREADS * 16u;
        at = base + t0 + t1 + ((ex >> 32) & 0xffffu);
        fz_rec_emit_word(v2.x, pos, nl, at); fz_rec_emit_word(v2.y, pos + 4u, nl, at);
        fz_rec_emit_word(v2.z, pos + 8u, nl, at); fz_rec_emit_word(v2.w, pos + 12u, nl, at);
        pos += FZ_REC_THREADS * 16u;
        at = base + t0 + t1 + t2 + ((ex >> 48) & 0xffffu);
        fz_rec_emit_word(v3.x, pos, nl, at); fz_rec_emit_word(v3.y, pos + 4u, nl, at);
        fz_rec_emit_word(v3.z, pos + 8u, nl, at); fz_rec_emit_word(v3.w, pos + 12u, nl, at);
    }
}

// lens has n_seqs + 1 entries (the last one 0: its exclusive scan is the sequences' starts in packed[] and, one entry on,
// their ends).  info[0] = the smallest error key (starts at FZ_REC_NO_ERROR), info[1] = the longest sequence (starts at 0).
__global__ __launch_bounds__(FZ_REC_THREADS) void fz_rec_measure_kernel(const uint8_t *__restrict__ raw, uint64_t n,
                                                                        const uint64_t *__restrict__ nl, uint64_t n_nl, uint64_t n_lines,
                                                                        uint32_t period, uint32_t phase, uint32_t flags, uint64_t n_seqs,
                                                                        uint64_t *__restrict__ starts, uint64_t *__restrict__ lens,
                                                                        unsigned long long *__restrict__ info) {
    const uint64_t stride = (uint64_t)gridDim.x * FZ_REC_THREADS;
    unsigned long long longest = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * FZ_REC_THREADS + threadIdx.x; r < n_seqs; r += stride) {
        const FzRecOut o = fz_rec_measure(raw, n, nl, n_nl, n_lines, period, phase, flags, r);
        starts[r] = o.start;
        lens[r] = o.len;
        longest = o.len > longest ? o.len : longest;
        if (o.reason != FZ_REC_OK) (void)atomicMin(&info[0], (unsigned long long)fz_rec_err_key(r, o.reason));
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        const unsigned long long o = __shfl_xor(longest, d, 64);
        longest = o > longest ? o : longest;
    }
    if ((threadIdx.x & 63u) == 0 && longest > __hip_atomic_load(&info[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        (void)atomicMax(&info[1], longest);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        lens[n_seqs] = 0;
        const uint64_t key = fz_rec_count_key(n_lines, period, flags);
        if (key != FZ_REC_NO_ERROR) (void)atomicMin(&info[0], (unsigned long long)key);
    }
}

// at[j] = where sequence j starts in packed[] (n_seqs + 1 entries: at[j + 1] = its end, at[n_seqs] = total > 0).
__global__ __launch_bounds__(FZ_REC_THREADS) void fz_rec_gather_kernel(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ starts,
                                                                       const uint64_t *__restrict__ at, uint64_t n_seqs, uint64_t total,
                                                                       uint8_t *__restrict__ packed) {
    __shared__ uint64_t bound[2];
    const uint64_t *ends = at + 1;
    const uint64_t ntiles = (total + FZ_TILE_BYTES - 1u) / FZ_TILE_BYTES;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t p0 = t * (uint64_t)FZ_TILE_BYTES;
        const uint64_t p1 = p0 + FZ_TILE_BYTES < total ? p0 + FZ_TILE_BYTES : total;
        if (threadIdx.x < 2u) {                            // the sequences of the tile's first and last byte
            const uint64_t target = threadIdx.x ? p1 - 1u : p0;
            uint64_t lo = 0, hi = n_seqs - 1u;
            while (lo < hi) {                              // first j with ends[j] > target (target < total = ends[n_seqs - 1])
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (ends[mid] > target) hi = mid; else lo = mid + 1u;
            }
            bound[threadIdx.x] = lo;
        }
        __syncthreads();
        const uint64_t jlo = bound[0], jhi = bound[1];
        for (uint32_t q = 0; q < FZ_TILE_BYTES / 16u / FZ_REC_THREADS; ++q) {
            uint64_t p = p0 + (uint64_t)(q * FZ_REC_THREADS + threadIdx.x) * 16u;
            if (p >= p1) continue;
            uint64_t lo = jlo, hi = jhi;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (ends[mid] > p) hi = mid; else lo = mid + 1u;
            }
            uint64_t j = lo;
            if (p + 16u <= ends[j]) {                      // the piece lies inside sequence j
                uint4 v;
                __builtin_memcpy(&v, raw + starts[j] + (p - at[j]), 16);
                *reinterpret_cast<uint4 *>(packed + p) = v;
            } else {
                const uint64_t pe = p + 16u < total ? p + 16u : total;
                for (; p < pe; ++p) {
                    while (ends[j] <= p) ++j;              // (p < total: such a j exists)
                    packed[p] = raw[starts[j] + (p - at[j])];
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// FASTA (fz_batch_upload_fasta; fz_device.h: fz_fa_*): behind the records path's newline count, scan and line table,
//   fz_fa_heads_kernel         one lane per line.  First pass: flag[i] = line i starts with '>' (n_lines + 1 entries, the
//                              last one 0); its exclusive scan is rank[]: line i belongs to record rank[i + 1] - 1, and
//                              rank[n_lines] = the records.  Second pass (head != null): head[rank[i]] = i for every header
//                              line, head[n_seqs] = n_lines
//   fz_fa_measure_kernel       one lane per record, from its first and last sequence line only: the row of the index, the
//                              length for the scan, the longest length, the verdict on the last line
//   fz_fa_check_kernel         one lane per line: a sequence line against its record's linebases / linewidth
//   fz_fa_gather_kernel        packed[] by 16-byte pieces of the DESTINATION, the newlines left behind
// As above the launch boundaries are the only ordering between workgroups.
__global__ __launch_bounds__(FZ_REC_THREADS) void fz_fa_heads_kernel(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ nl,
                                                                     uint64_t n_lines, uint64_t *__restrict__ flag,
                                                                     uint64_t *__restrict__ head) {
    const uint64_t stride = (uint64_t)gridDim.x * FZ_REC_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * FZ_REC_THREADS + threadIdx.x; i <= n_lines; i += stride) {
        if (!head) flag[i] = i < n_lines ? fz_fa_is_head(raw, nl, i) : 0u;
        else if (i == n_lines || flag[i + 1] != flag[i]) head[flag[i]] = i;
    }
}

// info as fz_rec_measure_kernel's.  starts[r] = the row's offset (fz_batch_tables), lens: n_seqs + 1 entries, the last one 0.
__global__ __launch_bounds__(FZ_REC_THREADS) void fz_fa_measure_kernel(const uint8_t *__restrict__ raw, uint64_t n,
                                                                       const uint64_t *__restrict__ nl, uint64_t n_nl,
                                                                       const uint64_t *__restrict__ head, uint64_t n_seqs,
                                                                       FzFaRow *__restrict__ rows, uint64_t *__restrict__ starts,
                                                                       uint64_t *__restrict__ lens, unsigned long long *__restrict__ info) {
    const uint64_t stride = (uint64_t)gridDim.x * FZ_REC_THREADS;
    unsigned long long longest = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * FZ_REC_THREADS + threadIdx.x; r < n_seqs; r += stride) {
        const FzFaOut o = fz_fa_measure(raw, n, nl, n_nl, head, r);
        rows[r] = o.row;
        starts[r] = o.row.offset;
        lens[r] = o.row.length;
        longest = o.row.length > longest ? o.row.length : longest;
        if (o.reason != FZ_REC_OK) (void)atomicMin(&info[0], (unsigned long long)fz_rec_err_key(r, o.reason));
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        const unsigned long long o = __shfl_xor(longest, d, 64);
        longest = o > longest ? o : longest;
    }
    if ((threadIdx.x & 63u) == 0 && longest > __hip_atomic_load(&info[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        (void)atomicMax(&info[1], longest);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        lens[n_seqs] = 0;
        const uint64_t key = fz_fa_text_key(raw, n);
        if (key != FZ_REC_NO_ERROR) (void)atomicMin(&info[0], (unsigned long long)key);
    }
}

// rank[] = the scanned flags, head[] and rows[] as above.  Lines in front of the first header belong to no record (the
// text's own error, fz_fa_text_key, is smaller than any of theirs).
__global__ __launch_bounds__(FZ_REC_THREADS) void fz_fa_check_kernel(const uint8_t *__restrict__ raw, uint64_t n,
                                                                     const uint64_t *__restrict__ nl, uint64_t n_nl, uint64_t n_lines,
                                                                     const uint64_t *__restrict__ rank, const uint64_t *__restrict__ head,
                                                                     const FzFaRow *__restrict__ rows, unsigned long long *__restrict__ info) {
    const uint64_t stride = (uint64_t)gridDim.x * FZ_REC_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * FZ_REC_THREADS + threadIdx.x; i < n_lines; i += stride) {
        const uint64_t c = rank[i + 1];
        if (c == 0 || head[c - 1u] == i) continue;         // no record yet; a header line
        const uint64_t r = c - 1u;
        const uint32_t why = fz_fa_line_check(raw, n, nl, n_nl, i, i + 1u == head[r + 1u], rows[r].linebases, rows[r].linewidth);
        if (why == FZ_REC_OK) continue;
        const unsigned long long key = fz_rec_err_key(r, why);
        if (key < __hip_atomic_load(&info[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) (void)atomicMin(&info[0], key);
    }
}

__device__ __forceinline__ uint4 fz_fa_upper16(uint4 v) {
    v.x = fz_fa_upper4(v.x); v.y = fz_fa_upper4(v.y); v.z = fz_fa_upper4(v.z); v.w = fz_fa_upper4(v.w);
    return v;
}

// Bytes 0 .. room - 1 of a, the others of b (0 < room < 16).
__device__ __forceinline__ uint32_t fz_fa_merge4(uint32_t a, uint32_t b, uint32_t room, uint32_t first) {
    const uint32_t k = room > first ? room - first : 0u;
    const uint32_t m = k >= 4u ? 0xffffffffu : (1u << (8u * k)) - 1u;
    return (a & m) | (b & ~m);
}

// at[j] = where record j starts in packed[] (n_seqs + 1 entries, at[n_seqs] = total > 0); rows[j]: its offset, linebases
// and linewidth in the text.  Base q of record j lies at fz_fa_src(rows[j], q).  A piece inside one record:
//   - inside one line: one unaligned 16-byte load, one aligned 16-byte store;
//   - across a line end, linebases >= 16 (3 pieces in 15 of 60-column lines): the piece holds `room` bytes of this line and
//     16 - room of the next one, which starts linewidth - linebases behind this line's end.  Two unaligned 16-byte loads,
//     at src and at src + (linewidth - linebases): byte i of the first is the piece's byte i for i < room, byte i of the
//     second for i >= room (the second load is shifted by the terminator's width), merged by a byte mask;
//   - linebases < 16 (a piece may hold three lines), a piece across a record's end, the last piece: byte by byte.
// The over-read guard: neither slack behind the buffer nor a byte path near its end is needed, because every 16-byte load
// covers only bytes between the source positions of the piece's first and last base (src <= load, load + 16 <= the last
// base's position + 1 <= n): the one-line load reads exactly the 16 bases; of the two merged loads the first ends in front
// of the second's end, and the second ends with the piece's last base.  (raw is whole tiles besides.)
__global__ __launch_bounds__(FZ_REC_THREADS) void fz_fa_gather_kernel(const uint8_t *__restrict__ raw, const FzFaRow *__restrict__ rows,
                                                                      const uint64_t *__restrict__ at, uint64_t n_seqs, uint64_t total,
                                                                      uint32_t flags, uint8_t *__restrict__ packed) {
    __shared__ uint64_t bound[2];
    const uint64_t *ends = at + 1;
    const uint64_t ntiles = (total + FZ_TILE_BYTES - 1u) / FZ_TILE_BYTES;
    const bool upper = (flags & FZ_FA_UPPER) != 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t p0 = t * (uint64_t)FZ_TILE_BYTES;
        const uint64_t p1 = p0 + FZ_TILE_BYTES < total ? p0 + FZ_TILE_BYTES : total;
        if (threadIdx.x < 2u) {                            // the records of the tile's first and last byte
            const uint64_t target = threadIdx.x ? p1 - 1u : p0;
            uint64_t lo = 0, hi = n_seqs - 1u;
            while (lo < hi) {                              // first j with ends[j] > target (target < total = ends[n_seqs - 1])
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (ends[mid] > target) hi = mid; else lo = mid + 1u;
            }
            bound[threadIdx.x] = lo;
        }
        __syncthreads();
        const uint64_t jlo = bound[0], jhi = bound[1];
        for (uint32_t q = 0; q < FZ_TILE_BYTES / 16u / FZ_REC_THREADS; ++q) {
            uint64_t p = p0 + (uint64_t)(q * FZ_REC_THREADS + threadIdx.x) * 16u;
            if (p >= p1) continue;
            uint64_t lo = jlo, hi = jhi;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (ends[mid] > p) hi = mid; else lo = mid + 1u;
            }
            uint64_t j = lo;
            if (p + 16u <= ends[j]) {                      // the piece lies inside record j
                const uint64_t off = rows[j].offset, lb = rows[j].linebases, lw = rows[j].linewidth, b = p - at[j];
                const uint64_t src = fz_fa_src(off, lb, lw, b), room = lb - fz_fa_col(lb, b);
                if (room >= 16u || lb >= 16u) {
                    uint4 v;
                    __builtin_memcpy(&v, raw + src, 16);
                    if (room < 16u) {
                        uint4 w;
                        __builtin_memcpy(&w, raw + src + (lw - lb), 16);
                        const uint32_t rm = (uint32_t)room;
                        v.x = fz_fa_merge4(v.x, w.x, rm, 0u); v.y = fz_fa_merge4(v.y, w.y, rm, 4u);
                        v.z = fz_fa_merge4(v.z, w.z, rm, 8u); v.w = fz_fa_merge4(v.w, w.w, rm, 12u);
                    }
                    *reinterpret_cast<uint4 *>(packed + p) = upper ? fz_fa_upper16(v) : v;
                    continue;
                }
            }
            const uint64_t pe = p + 16u < total ? p + 16u : total;
            for (; p < pe; ++p) {
                while (ends[j] <= p) ++j;                  // (p < total: such a j exists; records without bases are passed)
                const uint32_t c = raw[fz_fa_src(rows[j].offset, rows[j].linebases, rows[j].linewidth, p - at[j])];
                packed[p] = (uint8_t)(upper ? fz_fa_upper4(c) : c);
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// Derived batches (fz_batch_derive; fz_device.h: fz_derive_*): a batch made from a batch, without leaving the device.
//   fz_derive_measure_kernel   one lane per output: its source sequence from index[], the cut from starts[] / ends[] (null:
//                              the defaults), checked against the parent's scanned length table; src[] and the lengths for
//                              the records path's scan, the longest length, the smallest bad (item, reason)
//   fz_derive_gather_kernel    packed[] by 16-byte pieces of the DESTINATION, as fz_rec_gather_kernel (which IS the instance
//                              that neither reverses nor translates, launched over the parent's packed bytes)
// info as fz_rec_measure_kernel's.  offs = the parent's d_ends_base (not read when n_src == 0).
__global__ __launch_bounds__(FZ_REC_THREADS) void fz_derive_measure_kernel(const uint64_t *__restrict__ offs, uint64_t n_src,
                                                                           const uint32_t *__restrict__ index,
                                                                           const uint64_t *__restrict__ starts,
                                                                           const uint64_t *__restrict__ ends, uint64_t n_out,
                                                                           uint64_t *__restrict__ src, uint64_t *__restrict__ lens,
                                                                           unsigned long long *__restrict__ info) {
    const uint64_t stride = (uint64_t)gridDim.x * FZ_REC_THREADS;
    unsigned long long longest = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * FZ_REC_THREADS + threadIdx.x; j < n_out; j += stride) {
        const FzDrvItem o = fz_derive_item(offs, n_src, index, starts, ends, j);
        src[j] = o.src;
        lens[j] = o.len;
        longest = o.len > longest ? o.len : longest;
        if (o.reason != FZ_REC_OK) (void)atomicMin(&info[0], (unsigned long long)fz_rec_err_key(j, o.reason));
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        const unsigned long long o = __shfl_xor(longest, d, 64);
        longest = o > longest ? o : longest;
    }
    if ((threadIdx.x & 63u) == 0 && longest > __hip_atomic_load(&info[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        (void)atomicMax(&info[1], longest);
    if (blockIdx.x == 0 && threadIdx.x == 0) lens[n_out] = 0;
}

// at[j] = where output j starts in packed[] (n_seqs + 1 entries, at[n_seqs] = total > 0), src[j] = its lowest byte in raw,
// the parent's packed bytes.  A piece inside one output is one unaligned 16-byte load and one aligned 16-byte store: REV
// takes the 16 bytes that END where the piece's first byte comes from (fz_derive_piece_lo) and turns them round in registers
// (fz_derive_rev16); XLAT sends every byte through the table, which the workgroup holds in LDS as 64 dwords.  With 32 banks
// table bytes c and c ^ 0x80 share a bank, so two lanes that read such a pair may cost a second LDS cycle; lanes that read
// the same dword are one broadcast.  (Not measured with counters.)  A piece across an output's end goes byte by byte
// (fz_derive_byte_src).
// The over-read guard is the address rule's: every load covers exactly the source bytes of the piece's own output bytes,
// which lie inside [src[j], src[j] + len) — parent sequences lie back to back, and a neighbour's bytes are never loaded.
template <bool REV, bool XLAT>
__global__ __launch_bounds__(FZ_REC_THREADS) void fz_derive_gather_kernel(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ src,
                                                                          const uint64_t *__restrict__ at, uint64_t n_seqs, uint64_t total,
                                                                          const uint32_t *__restrict__ table, uint8_t *__restrict__ packed) {
    __shared__ uint64_t bound[2];
    __shared__ uint32_t xl[64];
    const uint8_t *xb = reinterpret_cast<const uint8_t *>(xl);
    const uint64_t *ends = at + 1;
    const uint64_t ntiles = (total + FZ_TILE_BYTES - 1u) / FZ_TILE_BYTES;
    if (XLAT && threadIdx.x < 64u) xl[threadIdx.x] = table[threadIdx.x];   // (the first tile's barrier orders it)
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t p0 = t * (uint64_t)FZ_TILE_BYTES;
        const uint64_t p1 = p0 + FZ_TILE_BYTES < total ? p0 + FZ_TILE_BYTES : total;
        if (threadIdx.x < 2u) {                            // the outputs of the tile's first and last byte
            const uint64_t target = threadIdx.x ? p1 - 1u : p0;
            uint64_t lo = 0, hi = n_seqs - 1u;
            while (lo < hi) {                              // first j with ends[j] > target (target < total = ends[n_seqs - 1])
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (ends[mid] > target) hi = mid; else lo = mid + 1u;
            }
            bound[threadIdx.x] = lo;
        }
        __syncthreads();
        const uint64_t jlo = bound[0], jhi = bound[1];
        for (uint32_t q = 0; q < FZ_TILE_BYTES / 16u / FZ_REC_THREADS; ++q) {
            uint64_t p = p0 + (uint64_t)(q * FZ_REC_THREADS + threadIdx.x) * 16u;
            if (p >= p1) continue;
            uint64_t lo = jlo, hi = jhi;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (ends[mid] > p) hi = mid; else lo = mid + 1u;
            }
            uint64_t j = lo;
            if (p + 16u <= ends[j]) {                      // the piece lies inside output j
                uint4 v;
                __builtin_memcpy(&v, raw + fz_derive_piece_lo(src[j], ends[j] - at[j], p - at[j], 16u, REV), 16);
                if (REV) fz_derive_rev16(v.x, v.y, v.z, v.w);
                if (XLAT) { v.x = fz_derive_xlat4(xb, v.x); v.y = fz_derive_xlat4(xb, v.y); v.z = fz_derive_xlat4(xb, v.z); v.w = fz_derive_xlat4(xb, v.w); }
                *reinterpret_cast<uint4 *>(packed + p) = v;
            } else {
                const uint64_t pe = p + 16u < total ? p + 16u : total;
                for (; p < pe; ++p) {
                    while (ends[j] <= p) ++j;              // (p < total: such a j exists; empty outputs are passed)
                    const uint8_t c = raw[fz_derive_byte_src(src[j], ends[j] - at[j], p - at[j], REV)];
                    packed[p] = XLAT ? xb[c] : c;
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// Formatted text (fz_batch_format; fz_device.h: fz_format_*): C batches become one text of records, without leaving the device.
//   fz_format_measure_kernel   one lane per record: the lengths of its sequences from the columns' scanned length tables,
//                              the literals' total, the pair of columns checked for equal length; the record lengths for
//                              the records path's scan, the longest record, the smallest bad (record, reason)
//   fz_format_gather_kernel    text[] by 16-byte pieces of the DESTINATION, as fz_derive_gather_kernel
// info as fz_rec_measure_kernel's.  desc lies in device memory.
__global__ __launch_bounds__(FZ_REC_THREADS) void fz_format_measure_kernel(const FzFmtDesc *__restrict__ desc, uint64_t n,
                                                                           uint64_t *__restrict__ lens,
                                                                           unsigned long long *__restrict__ info) {
    const uint64_t stride = (uint64_t)gridDim.x * FZ_REC_THREADS;
    unsigned long long longest = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * FZ_REC_THREADS + threadIdx.x; j < n; j += stride) {
        const FzFmtRec o = fz_format_record(*desc, j);
        lens[j] = o.len;
        longest = o.len > longest ? o.len : longest;
        if (o.reason != FZ_REC_OK) (void)atomicMin(&info[0], (unsigned long long)fz_rec_err_key(j, o.reason));
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        const unsigned long long o = __shfl_xor(longest, d, 64);
        longest = o > longest ? o : longest;
    }
    if ((threadIdx.x & 63u) == 0 && longest > __hip_atomic_load(&info[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        (void)atomicMax(&info[1], longest);
    if (blockIdx.x == 0 && threadIdx.x == 0) lens[n] = 0;
}

// at[j] = where record j starts in text[] (n + 1 entries, at[n] = total > 0).  The descriptor, its literals included, is
// copied into LDS once per workgroup.  Every piece finds its record by the search over at[] and its segment by the walk
// (fz_format_seek).  A piece inside one column segment is one unaligned 16-byte load from that column's packed bytes and
// one aligned 16-byte store; every other piece — across a segment or record seam, in a literal, the text's last partial one
// — goes byte by byte under a cursor that moves on from segment to segment (fz_format_settle, fz_format_byte_src).
// The over-read guard is the address rule's: a 16-byte load covers exactly the source bytes of the piece's own output
// bytes, which lie inside sequence j of the column (fz_format_run), never a neighbouring sequence or padding.  text is
// allocated in whole tiles; the aligned stores end at or in front of `total` besides.
__global__ __launch_bounds__(FZ_REC_THREADS) void fz_format_gather_kernel(const FzFmtDesc *__restrict__ desc,
                                                                          const uint64_t *__restrict__ at, uint64_t n, uint64_t total,
                                                                          uint8_t *__restrict__ text) {
    __shared__ uint64_t bound[2];
    __shared__ FzFmtDesc sd;
    static_assert(sizeof(FzFmtDesc) % 4u == 0, "the descriptor is copied by dwords");
    {
        const uint32_t *g = reinterpret_cast<const uint32_t *>(desc);
        uint32_t *s = reinterpret_cast<uint32_t *>(&sd);
        for (uint32_t i = threadIdx.x; i < sizeof(FzFmtDesc) / 4u; i += FZ_REC_THREADS) s[i] = g[i];   // (the first tile's barrier orders it)
    }
    const uint64_t *ends = at + 1;
    const uint64_t ntiles = (total + FZ_TILE_BYTES - 1u) / FZ_TILE_BYTES;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t p0 = t * (uint64_t)FZ_TILE_BYTES;
        const uint64_t p1 = p0 + FZ_TILE_BYTES < total ? p0 + FZ_TILE_BYTES : total;
        if (threadIdx.x < 2u) {                            // the records of the tile's first and last byte
            const uint64_t target = threadIdx.x ? p1 - 1u : p0;
            uint64_t lo = 0, hi = n - 1u;
            while (lo < hi) {                              // first j with ends[j] > target (target < total = ends[n - 1])
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (ends[mid] > target) hi = mid; else lo = mid + 1u;
            }
            bound[threadIdx.x] = lo;
        }
        __syncthreads();
        const uint64_t jlo = bound[0], jhi = bound[1];
        for (uint32_t q = 0; q < FZ_TILE_BYTES / 16u / FZ_REC_THREADS; ++q) {
            uint64_t p = p0 + (uint64_t)(q * FZ_REC_THREADS + threadIdx.x) * 16u;
            if (p >= p1) continue;
            uint64_t lo = jlo, hi = jhi;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (ends[mid] > p) hi = mid; else lo = mid + 1u;
            }
            uint64_t j = lo;
            FzFmtCur g = fz_format_seek(sd, j, p - at[j]);
            if (fz_format_run(g, 16u)) {                   // the piece lies inside one sequence of one column
                uint4 v;
                __builtin_memcpy(&v, sd.col[g.seg >> 1].bytes + fz_format_run_lo(sd, j, g), 16);
                *reinterpret_cast<uint4 *>(text + p) = v;
            } else {
                const uint64_t pe = p + 16u < total ? p + 16u : total;
                for (; p < pe; ++p) {
                    fz_format_settle(sd, j, g);            // (p < total: a byte follows)
                    text[p] = *fz_format_byte_src(sd, j, g);
                    ++g.off;
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// End overlaps (fz_batch_end_overlaps; fz_device.h: fz_overlap_*): a prefix of a pattern at the end of every read of a batch.
// Nothing is filtered and nothing is streamed: a launch looks at the last fz_overlap_tail bytes of every read only.
//
//   fz_overlap_kernel<MODE>  one lane per read, a workgroup per 256 reads, grid-strided so that a workgroup's tables serve
//       many reads.  LDS: the launch's patterns — lengths, 64-byte rows, and for Levenshtein the forward and the reversed Peq
//       table of every pattern (2 x 256 x 8 B, built here from the row: thread t owns word t of both tables) — then per wave
//       the window, win_dwords x 256 B in the lane-transposed layout of the verification kernels (dword d of lane l at
//       win[d * 64 + l]: 32 banks per half wave, no conflicts at any alignment).  The read's extent comes from ends[]; its
//       tail is staged a dword at a time (fz_overlap_stage: every dword starts in front of buf_len), the patterns of the
//       launch are walked in a wave-uniform loop with the best key in registers (fz_overlap_lane), and a lane with an answer
//       does ONE device-scope atomic maximum without return value on table[read].  table is zeroed by a memset in front of the
//       first launch (0: none); later chunks of the list are further launches over the same table.
//   fz_overlap_finish_kernel  one lane per read: the key decoded into the 8-byte output row.
struct FzOvlArgs {
    FzRagged rag;
    uint64_t buf_len;
    const uint32_t *rows;                                  // the call's patterns: FZ_OVL_ROW_BYTES each, zeros behind a pattern
    const uint32_t *pm;                                    // ... and their lengths
    uint32_t p0, npat;                                     // the patterns of this launch
    uint32_t k, o;
    uint32_t tmax, win_dwords;                             // the longest tail of the launch's patterns, and the window for it
};

__host__ __device__ inline uint32_t fz_overlap_tables_lds(uint32_t mode, uint32_t npat) {
    return fz_overlap_chunk(mode) * (4u + FZ_OVL_ROW_BYTES) + (mode == FZ_MODE_LEV ? npat * 4096u : 0u);
}
__host__ __device__ inline uint32_t fz_overlap_lds(uint32_t mode, uint32_t npat, uint32_t win_dwords) {
    return fz_overlap_tables_lds(mode, npat) + FZ_WAVES_PER_BLOCK * win_dwords * 256u;
}

template <uint32_t MODE>
__global__ __launch_bounds__(FZ_FILTER_THREADS) void fz_overlap_kernel(const uint8_t *__restrict__ buf, const FzOvlArgs a,
                                                                       unsigned long long *__restrict__ table) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr uint32_t CH = MODE == FZ_MODE_LEV ? FZ_OVL_CHUNK_LEV : FZ_OVL_CHUNK_SUBS, RD = FZ_OVL_ROW_BYTES / 4u;
    uint32_t *pm = reinterpret_cast<uint32_t *>(smem);
    uint32_t *rows = pm + CH;
    uint64_t *peq = reinterpret_cast<uint64_t *>(rows + CH * RD);
    for (uint32_t i = threadIdx.x; i < a.npat; i += FZ_FILTER_THREADS) pm[i] = a.pm[a.p0 + i];
    for (uint32_t i = threadIdx.x; i < a.npat * RD; i += FZ_FILTER_THREADS) rows[i] = a.rows[a.p0 * RD + i];
    __syncthreads();
    if constexpr (MODE == FZ_MODE_LEV) {
        for (uint32_t i = threadIdx.x; i < a.npat * 512u; i += FZ_FILTER_THREADS)
            peq[i] = fz_overlap_peq_word(reinterpret_cast<const uint8_t *>(rows + (i >> 9) * RD), pm[i >> 9], i & 255u, (i >> 8) & 1u);
        __syncthreads();
    }
    const uint32_t lane = fz_lane();
    uint32_t *win = reinterpret_cast<uint32_t *>(smem + fz_overlap_tables_lds(MODE, a.npat)) + (threadIdx.x >> 6) * a.win_dwords * 64u + lane;
    const FzOvlTabs tb{pm, rows, peq};
    const uint64_t n_seqs = a.rag.n_seqs, groups = (n_seqs + FZ_FILTER_THREADS - 1u) / FZ_FILTER_THREADS;
    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const uint64_t j = g * FZ_FILTER_THREADS + threadIdx.x;
        const bool have = j < n_seqs;
        const uint64_t sa = have && j ? a.rag.ends[j - 1u] : 0ull, se = have ? a.rag.ends[j] : 0ull;   // (no read: an empty one)
        const FzOvlStage st = fz_overlap_stage(sa, se, a.tmax, a.buf_len);
        fz_overlap_stage_copy(buf, st, a.win_dwords, win, 64u);
        fz_wave_lds_sync();
        const uint64_t key = fz_overlap_lane<MODE>(tb, win, 64u, st, (uint32_t)(se - sa), a.p0, a.npat, a.k, a.o);
        if (key) (void)__hip_atomic_fetch_max(&table[j], (unsigned long long)key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        fz_wave_lds_sync();
    }
}

__global__ __launch_bounds__(FZ_ASSIGN_THREADS) void fz_overlap_finish_kernel(const unsigned long long *__restrict__ table,
                                                                              const uint64_t *__restrict__ ends, uint64_t n_seqs,
                                                                              FzOverlapRow *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * FZ_ASSIGN_THREADS;
    for (uint64_t j = (uint64_t)blockIdx.x * FZ_ASSIGN_THREADS + threadIdx.x; j < n_seqs; j += stride)
        out[j] = fz_overlap_row(table[j], (uint32_t)(ends[j] - (j ? ends[j - 1u] : 0ull)));
}

// ---------------------------------------------------------------------------------------------
// Score cuts (fz_batch_score_cuts; fz_device.h: fz_cuts_*): per read where the running sum of a score table, taken from its
// 3' end and / or its 5' end, peaks — quality trimming and poly-A trimming are two tables.
//
//   fz_cuts_kernel  one lane per read, a workgroup per 256 reads, grid-strided.  LDS: the table of each requested side,
//       256 x int16 (512 B; thread t brings entry t), then per wave ONE window of FZ_CUT_PIECE_DWORDS x 256 B in the
//       lane-transposed layout of the overlap and verification kernels (dword d of lane l at win[d * 64 + l]: 32 banks per
//       half wave, no conflicts at any alignment) — 17 KiB per workgroup.  The read's extent comes from ends[].  Per side the
//       read is walked in pieces (fz_cuts_piece: from its end for 3', its start for 5'); the piece loop is wave-uniform, it
//       runs while a ballot says some lane is live, and a finished lane stages nothing (fz_stage_copy<false>: no load, no
//       LDS store).  Every dword loaded starts in front of buf_len (fz_stage_range).  The lane writes its own 8-byte row: no
//       atomics, no finish kernel, no memset.
struct FzCutArgs {
    FzRagged rag;
    uint64_t buf_len;
    const int16_t *w;                                      // the call's tables: side s (0: 3', 1: 5') at w + 256 s
    uint32_t sides, walk, flags;                           // bit s of sides: side s is asked for (fz_cuts_row); of walk: its table
                                                           // has a positive score, so it is walked (the others cut nothing)
    uint32_t num, den;
    int32_t wmax3, wmax5;                                  // the largest score of each table
};

// One side of one read: the wave-uniform piece loop -> the number of bytes that side cuts.
__device__ __forceinline__ uint32_t fz_cuts_side(const uint8_t *__restrict__ buf, const FzCutArgs &a, uint32_t side, int32_t wmax,
                                                 const int16_t *tab, uint32_t *win, uint64_t sa, uint64_t se, uint32_t n) {
    const FzCutRule r = fz_cuts_rule(side, a.flags, a.num, a.den, wmax, 1u);
    FzCutState c = fz_cuts_begin(n, r);
    while (FZ_WAVE_BALLOT(c.live)) {
        const FzOvlStage st = fz_cuts_piece(c, sa, se, side, a.buf_len);
        fz_stage_copy<false>(buf, st, FZ_CUT_PIECE_DWORDS, win, 64u);
        fz_wave_lds_sync();
        fz_cuts_lane(c, tab, win, 64u, st, n, side, r);
        fz_wave_lds_sync();
    }
    return c.trim;
}

__global__ __launch_bounds__(FZ_FILTER_THREADS) void fz_cuts_kernel(const uint8_t *__restrict__ buf, const FzCutArgs a,
                                                                    FzCutRow *__restrict__ out) {
    static_assert(FZ_FILTER_THREADS == 256, "thread t brings table entry t");
    __shared__ int16_t tab[2][256];
    __shared__ uint32_t wins[FZ_WAVES_PER_BLOCK * FZ_CUT_PIECE_DWORDS * 64u];
    for (uint32_t side = 0; side < 2u; ++side)
        if ((a.walk >> side) & 1u) tab[side][threadIdx.x] = a.w[side * 256u + threadIdx.x];
    __syncthreads();
    uint32_t *win = wins + (threadIdx.x >> 6) * FZ_CUT_PIECE_DWORDS * 64u + fz_lane();
    const uint64_t n_seqs = a.rag.n_seqs, groups = (n_seqs + FZ_FILTER_THREADS - 1u) / FZ_FILTER_THREADS;
    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const uint64_t j = g * FZ_FILTER_THREADS + threadIdx.x;
        const bool have = j < n_seqs;
        const uint64_t sa = have && j ? a.rag.ends[j - 1u] : 0ull, se = have ? a.rag.ends[j] : 0ull;   // (no read: an empty one)
        const uint32_t n = (uint32_t)(se - sa);
        const uint32_t trim3 = (a.walk & 1u) ? fz_cuts_side(buf, a, 0u, a.wmax3, tab[0], win, sa, se, n) : 0u;   // (wave-uniform)
        const uint32_t trim5 = (a.walk & 2u) ? fz_cuts_side(buf, a, 1u, a.wmax5, tab[1], win, sa, se, n) : 0u;
        if (have) out[j] = fz_cuts_row(n, trim3, trim5, a.sides);
    }
}
