// fz_device.h — per-candidate verification logic shared by the HIP kernels (fz_kernels.h).
//
// Everything here is FZ_HD (__host__ __device__) so that tests/ can also compile the very same
// functions with g++ and run them lane-by-lane against the oracle in the CPU-only container
// (tests/host_emul.cpp).  The product only ever runs them on the GPU.
//
// Reference semantics (file:line into /root/reference/src/fuzzysearch/), see SURVEY.md App. A:
//   fz_expand           <- c_expand_short / c_expand_long       _levenshtein_ngrams.pyx:9-154
//   fz_verify_lev       <- body of the hit loop                 levenshtein_ngram.py:177-198
//   fz_verify_subs      <- mismatch counting around a hit       _substitutions_only_ngrams_template.h:103-121
//                          + count_differences_with_maximum     common.py:119-142 / substitutions_only.py:266-278
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FZ_HD __host__ __device__ __forceinline__
#else
#define FZ_HD inline
#endif

// "does any lane of the wave want this?" — wave-uniform on the device (a scalar branch), the caller's own flag
// in host code (tests/host_emul.cpp drives one candidate at a time)
#if defined(__HIP_DEVICE_COMPILE__)
#define FZ_WAVE_ANY(x) (__ballot((x) != 0) != 0ull)
#define FZ_WAVE_BALLOT(x) __ballot((x) != 0)
#else
#define FZ_WAVE_ANY(x) ((x) != 0)
#define FZ_WAVE_BALLOT(x) ((x) ? 1ull : 0ull)
#endif

#define FZ_MAX_BLOCKS_PER_LAUNCH 16    // n-gram blocks tested by one filter launch (round 6: 8 -> 16; a pattern of 9 .. 16 blocks is ONE pass)
#define FZ_BLK_BITS 4                  // log2(FZ_MAX_BLOCKS_PER_LAUNCH): bits of the block number in a queue code
#define FZ_MAX_REGIONS 8               // regions of a scan grid (FzScanArgs.reg_*)
#define FZ_MAX_M 1024                  // pattern bytes carried in the kernel argument block (longer patterns: FzScanArgs.pat_g)
#define FZ_MAX_K 255                   // largest budget of the LDS-ring verification and of the candidate automata (8-bit counters)
#define FZ_MAX_M_ANY 65535u            // longest subsequence any path accepts (16-bit window-relative coordinates)
#define FZ_MAX_K_ANY 1023u             // largest Levenshtein / substitution budget (fz_verify_big_kernel: 2k + 1 <= 64 lanes x 32 cells)

// What fz_lp_kernel iterates over.
enum FzLpKind : uint32_t {
    FZ_LP_GENERIC_HIT = 0,   // generic automaton on the window around every n-gram hit (generic_search.py:198-237)
    FZ_LP_GENERIC_SEQ = 1,   // generic automaton over the whole sequence (generic_search.py:57-177), tiled by start
    FZ_LP_LEV_SEQ = 2,       // Levenshtein automaton over the whole sequence (levenshtein.py:52-148), tiled by start
};

enum FzMode : uint32_t { FZ_MODE_EXACT = 0, FZ_MODE_LEV = 1, FZ_MODE_SUBS = 2, FZ_MODE_GENERIC = 3 };

// Geometry of the resident (shard of the) sequence.  All match arithmetic is in GLOBAL
// coordinates; `buf` holds global bytes [buf_off, buf_off + buf_len).
//
// Segments (find_near_matches_in_file, __init__.py:129-200): the reference searches a file chunk by
// chunk, every chunk as an INDEPENDENT sequence (window clamps use the chunk's own ends), so the
// result depends on the chunk geometry.  A whole batch of chunks is resident at
// once here and every chunk is a "segment" with its own clamps:
//     segment j = [seg_org + j*S - pre, seg_org + (j+1)*S + post)  clipped to  [seg_org, n)
// binary files (:129-171): S = chunk_size - keep, pre = 0, post = keep;
// text files   (:174-200): S = chunk_size,        pre = keep, post = 0     (keep = m - 1 + extra).
// seg_stride == 0: one segment, the whole sequence [0, n).  With pre, post <= S / 2 a position lies in
// at most two segments: its core segment (idx - seg_org) / S and the neighbour the extension
// reaches into.  A launch owns the segments [seg_j0, seg_j1).
struct FzGeom {
    uint64_t n;         // global sequence length (every clamp of App. A uses this)
    uint64_t buf_off;   // global index of buf[0]
    uint64_t buf_len;   // valid bytes in buf (the allocation is zero-padded on both sides)
    uint64_t own_lo;    // this shard owns n-gram hits with own_lo <= idx < own_hi
    uint64_t own_hi;
    uint64_t seg_stride;   // S; 0 = unsegmented
    uint64_t seg_org;      // global index where segment 0's core starts
    uint64_t seg_j0, seg_j1;   // segments owned by this launch
    uint32_t seg_pre, seg_post;
};

// One segment's bounds [sa, se).
struct FzSeg { uint64_t sa, se; uint32_t j; uint32_t ok; };

// Candidate segment number c (0 or 1) of position idx; ok = 0 if there is no such segment in this launch.
FZ_HD FzSeg fz_segment(const FzGeom &g, uint64_t idx, uint32_t c) {
    FzSeg r;
    r.j = 0;
    if (g.seg_stride == 0) { r.sa = 0; r.se = g.n; r.ok = c == 0 ? 1u : 0u; return r; }
    r.sa = r.se = 0; r.ok = 0;
    if (idx < g.seg_org) return r;
    uint64_t j = (idx - g.seg_org) / g.seg_stride;
    if (c == 1) {
        if (g.seg_post) { if (j == 0) return r; --j; }       // the previous segment's extension reaches here
        else if (g.seg_pre) ++j;                              // the next segment starts `pre` bytes early
        else return r;
    }
    if (j < g.seg_j0 || j >= g.seg_j1) return r;
    const uint64_t core = g.seg_org + j * g.seg_stride;
    r.sa = (core - g.seg_org >= g.seg_pre) ? core - g.seg_pre : g.seg_org;
    r.se = core + g.seg_stride + g.seg_post;
    if (r.se > g.n) r.se = g.n;
    r.j = (uint32_t)j;
    r.ok = (idx >= r.sa && idx < r.se) ? 1u : 0u;
    return r;
}
FZ_HD uint32_t fz_segment_candidates(const FzGeom &g) { return (g.seg_stride && (g.seg_pre || g.seg_post)) ? 2u : 1u; }

// Ragged segments (fz_batch_upload: one pattern, many sequences): the buffer holds n_seqs sequences packed back to back,
// no separators, no padding; sequence j = [j ? ends[j-1] : 0, ends[j]) with ends[] the cumulative end offsets (u64,
// non-decreasing; equal neighbours = an empty sequence).  A position lies in exactly ONE sequence:
//     j = the first j with ends[j] > idx.
// The binary search is bounded by a second table built at upload, first[t] = the first j with ends[j] > t * 16 KiB (the
// sequence that holds the first byte of tile t; n_seqs past the end), ntiles + 1 entries: the sequence of a position in
// tile t is one of first[t] .. first[t+1] — one step where sequences are longer than a tile, ~7 for 150-byte reads.
// To the host's planning and to every clamp that is not per sequence a batch is ONE in-memory sequence (seg_stride = 0,
// n = total bytes); the segment fields of FzGeom, unused in that form, carry the tables, and only the ragged kernel
// instances (fz_kernels.h: RAG) read them:
//     seg_org = device address of ends[],  seg_j0 = device address of first[],  seg_j1 = n_seqs.
#define FZ_RAG_TILE_BITS 14            // = FZ_TILE_BITS (fz_kernels.h): the granule of first[]
struct FzRagged { const uint64_t *ends; const uint32_t *first; uint64_t n_seqs; };

FZ_HD FzRagged fz_ragged(const FzGeom &g) {
    FzRagged r;
    r.ends = reinterpret_cast<const uint64_t *>(g.seg_org);
    r.first = reinterpret_cast<const uint32_t *>(g.seg_j0);
    r.n_seqs = g.seg_j1;
    return r;
}

// first[] of an offset table: `ntiles` + 1 entries.
FZ_HD void fz_ragged_first(const uint64_t *ends, uint64_t n_seqs, uint64_t ntiles, uint32_t *first) {
    uint64_t j = 0;
    for (uint64_t t = 0; t <= ntiles; ++t) {
        while (j < n_seqs && ends[j] <= (t << FZ_RAG_TILE_BITS)) ++j;
        first[t] = (uint32_t)j;
    }
}

// The sequence of position idx (idx < n = ends[n_seqs - 1], else ok = 0).
FZ_HD FzSeg fz_segment_ragged(const FzRagged &t, uint64_t n, uint64_t idx) {
    FzSeg r;
    r.sa = r.se = 0; r.j = 0; r.ok = 0;
    if (idx >= n || t.n_seqs == 0) return r;
    const uint64_t tile = idx >> FZ_RAG_TILE_BITS;
    uint32_t lo = t.first[tile], hi = t.first[tile + 1];   // (n_seqs < 2^32)
    if (hi >= t.n_seqs) hi = (uint32_t)t.n_seqs - 1u;
    while (lo < hi) {                                      // first j in [lo, hi] with ends[j] > idx
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (t.ends[mid] > idx) hi = mid; else lo = mid + 1u;
    }
    r.sa = lo ? t.ends[lo - 1] : 0;
    r.se = t.ends[lo];
    r.j = lo;
    r.ok = 1;
    return r;
}

// fz_segment / fz_segment_candidates of a kernel instance: strided (or unsegmented) by the geometry, or (RAG) ragged.
template <bool RAG>
FZ_HD uint32_t fz_segment_candidates_of(const FzGeom &g) { return RAG ? 1u : fz_segment_candidates(g); }
template <bool RAG>
FZ_HD FzSeg fz_segment_of(const FzGeom &g, uint64_t idx, uint32_t c) {
    if constexpr (RAG) {
        return fz_segment_ragged(fz_ragged(g), g.n, idx);
    } else {
        return fz_segment(g, idx, c);
    }
}

// The segment a kernel instance verifies a position in when it does not go through fz_segment's strided candidates:
// the whole sequence, or (RAG) the position's own sequence of a batch.
template <bool RAG>
FZ_HD FzSeg fz_segment_one(const FzGeom &g, uint64_t idx) {
    if constexpr (RAG) {
        return fz_segment_ragged(fz_ragged(g), g.n, idx);
    } else {
        FzSeg r;
        r.sa = 0; r.se = g.n; r.j = 0; r.ok = 1;
        return r;
    }
}

// One scan launch: up to FZ_MAX_BLOCKS_PER_LAUNCH n-gram blocks of length L.  A hit of block b at global index idx is
// accepted for the segment [sa, se) iff
//     sa + lo_rel[b] <= idx  &&  idx + L <= se - hi_sub[b]  &&  abs_lo <= idx  &&  idx + L <= abs_hi
//     &&  own_lo <= idx < own_hi
// (levenshtein_ngram.py:171-176: lo_rel = max(0, s - k), hi_sub = max(0, m - s - L - k);
//  _substitutions_only_ngrams_template.h:97-101: lo_rel = s, hi_sub = m - s - L;
//  search_exact.py:70-71: abs_lo / abs_hi = the clamped start / end index).
struct FzScanArgs {
    FzGeom   geom;
    uint32_t mode;                              // FzMode: what happens to confirmed hits
    uint32_t m, k;                              // pattern length, edit / substitution budget
    uint32_t L;                                 // n-gram length
    uint32_t nblk;                              // real blocks in this launch
    uint32_t g0;                                // global block index of block 0 of this launch
    uint32_t d2;                                // byte offset of the 2nd exact-compare window
    uint32_t mask1;                             // mask of the 1st window ((1 << 8L) - 1 when L < 4)
    uint32_t mask2;                             // mask of the 2nd window (n-gram bytes d2 .. d2+3)
    uint32_t fused;                             // 1: verify inside the scan kernel, 0: emit hits
    uint32_t band_w;                            // rolling score slots per lane (2k + 2)
    uint32_t win_dwords;                        // window dwords staged per lane ((m + 2k + 6) / 4 + 1)
    uint32_t vlanes;                            // lanes of a wave that verify at once (64, 32 or 16): LDS vs lane use
    uint32_t max_subs, max_ins, max_dels;       // generic search limits (k = max_l_dist there)
    uint32_t cand_cap;                          // automaton kernels: candidate slots per list
    uint64_t cand_scratch;                      // 0: both lists in LDS; else device address of per-wave lists in HBM
                                                // (2 * cand_cap slots per workgroup; pathological inputs only)
    uint32_t lp_kind;                           // FzLpKind of fz_lp_kernel
    uint32_t lp_starts;                         // tiled modes: start positions owned by one window
    uint32_t hash_k;                            // odd multiplier of the window hash (24 bits when L > 4)
    uint32_t lut_shift;                         // table slot of a hash h = (h >> lut_shift) & 31
    uint32_t gw;                                // wavefront verification: lanes per candidate (16, 32 or 64)
    uint32_t qcap;                              // fused in-memory scan: queue entries (= prefetched windows) per wave
    uint32_t win_pieces;                        // ... and 16-byte pieces per window (LDS-DMA granule)
    uint32_t flags;                             // tuning knobs (0 in production)
    uint32_t H[FZ_MAX_BLOCKS_PER_LAUNCH];       // fast-path hash of each block's n-gram
    uint32_t A[FZ_MAX_BLOCKS_PER_LAUNCH];       // 1st window value per block (little endian)
    uint32_t B[FZ_MAX_BLOCKS_PER_LAUNCH];       // 2nd window value per block
    uint32_t lo_rel[FZ_MAX_BLOCKS_PER_LAUNCH];  // accepted hit range of a block, relative to the segment ends
    uint32_t hi_sub[FZ_MAX_BLOCKS_PER_LAUNCH];
    uint32_t s[FZ_MAX_BLOCKS_PER_LAUNCH];       // ngram_start of each block inside the pattern
    uint64_t abs_lo, abs_hi;                    // absolute index range (exact search with start / end index)
    uint64_t hit_cap;                           // capacity of the hit list
    uint64_t rec_cap;                           // capacity of the record list
    uint64_t gen_order;                         // generic search, one shard, no segments: device address of the ordering
                                                // area (FZ_GEN_ORDER_MAX x {u64 first row, u32 row count}); 0: the host orders
    uint64_t gen_dedup;                         // generic search: device address of the window table (FzGenDedup layout below);
                                                // 0: every n-gram hit runs the automaton on its own
    uint64_t rows_cap;                          // generic search ordered on the device: rows the row buffer holds
    uint64_t host_hdr;                          // device-visible address of the host copy of the counters
                                                // (0: none); the last workgroup of the launch fills it
    uint64_t pat_g;                             // m > FZ_MAX_M: device address of the pattern (pat[] unused); else 0
    uint8_t  pat[FZ_MAX_M];                     // whole pattern (m <= FZ_MAX_M)
    // Scan grid in regions (nreg = 0: one region, every workgroup strides over all tiles): workgroups [reg_wg0[r],
    // reg_wg0[r] + reg_nwg[r]) stride over the tiles [reg_tile0[r], reg_end[r]) — the last resident round of a launch gets
    // fewer and fewer tiles per workgroup so that the machine does not drain one long workgroup life at a time
    uint32_t nreg;
    uint32_t reg_wg0[FZ_MAX_REGIONS], reg_nwg[FZ_MAX_REGIONS];
    uint64_t reg_tile0[FZ_MAX_REGIONS], reg_end[FZ_MAX_REGIONS];
};

// The tile walk of one scan workgroup.  Logical: first, first + stride, .. below limit — what the regions above say.
// Physical: the tile whose bytes a step of the walk reads — the logical tile, or (a reversed launch, FZ_FLAG_REVERSE)
// its mirror ntiles - 1 - logical, so that the workgroups that start first read the END of the buffer first: the next
// scan of a resident sequence starts where the last one ended, while those lines are still in the Infinity Cache.
// Everything that orders the work (regions, shares, taper, the limit tests) stays logical; only addresses and
// positions are physical.  The scan kernel and the host twin (fz_debug_scan_walk) both go through these functions.
struct FzWalk {
    uint64_t first, limit;   // logical
    uint32_t stride;
    uint64_t phys_first;     // physical tile of iteration 0
    int32_t phys_stride;     // ... and the step to the next iteration's (negative when reversed)
};
FZ_HD uint64_t fz_walk_phys(uint64_t ntiles, uint64_t logical, bool rev) { return rev ? ntiles - 1u - logical : logical; }
FZ_HD FzWalk fz_scan_walk(uint32_t nreg, const uint32_t *reg_wg0, const uint32_t *reg_nwg, const uint64_t *reg_tile0,
                          const uint64_t *reg_end, uint32_t grid, uint64_t ntiles, uint32_t wg, bool rev) {
    uint32_t wg0 = 0, stride = grid;
    uint64_t tile0 = 0, limit = ntiles;
#pragma unroll
    for (uint32_t r = 0; r < FZ_MAX_REGIONS; ++r)
        if (r < nreg && wg >= reg_wg0[r]) { wg0 = reg_wg0[r]; stride = reg_nwg[r]; tile0 = reg_tile0[r]; limit = reg_end[r]; }
    FzWalk w;
    w.first = tile0 + (wg - wg0);
    w.limit = limit;
    w.stride = stride;
    w.phys_first = fz_walk_phys(ntiles, w.first, rev);
    w.phys_stride = rev ? -(int32_t)stride : (int32_t)stride;
    return w;
}
// Physical tile of iteration `iter` of the walk; ~0 when the walk has no such iteration.
FZ_HD uint64_t fz_walk_tile(const FzWalk &w, uint32_t iter) {
    if (w.first + (uint64_t)iter * w.stride >= w.limit) return ~0ull;
    return (uint64_t)((int64_t)w.phys_first + (int64_t)iter * (int64_t)w.phys_stride);
}

// A hit: (block g << FZ_IDX_BITS) | global idx (48-bit index: sequences below 256 TiB; 16-bit block number).
// A record: what verification produced for one hit.
#define FZ_IDX_BITS 48
#define FZ_MAX_BLOCKS 65535u           // n-gram blocks of one search (block numbers must fit the key's upper 16 bits)
struct FzRec {
    uint64_t key;        // (g << FZ_IDX_BITS) | idx  -> sorting by key restores the reference's order
    uint32_t l;          // bytes consumed to the left of idx   (start = idx - l)
    uint32_t r;          // bytes consumed right of the n-gram  (end   = idx + L + r)
    uint32_t dist;
    uint32_t aux;        // segment number (file API), else 0
};

#define FZ_REC_NONE 0xffffffffu        // FzRec.dist of a slot whose hit did not verify (slot-per-hit kernels)

FZ_HD uint64_t fz_hit_pack(uint32_t g, uint64_t idx) { return ((uint64_t)g << FZ_IDX_BITS) | idx; }
FZ_HD uint32_t fz_hit_block(uint64_t h) { return (uint32_t)(h >> FZ_IDX_BITS); }
FZ_HD uint64_t fz_hit_index(uint64_t h) { return h & ((1ull << FZ_IDX_BITS) - 1ull); }

// Hash of the first min(L, 8) bytes of an n-gram window as the filter's fast path computes it:
//   L > 4:  x  = bytes [0, 4)                  (little-endian dword)
//           yh = low 24 bits of the dword at byte min(L, 8) - 3, i.e. bytes [min(L,8)-3, min(L,8))
//           h  = yh * K + x                    (one v_mad_u32_u24; K < 2^24)
//   L <= 4: h  = (x & mask) * K                (K odd: a bijection of the masked dword)
// Collisions only cost a visit to the exact re-check.
// Six bits of h, (h >> lut_shift) & 63, select the slot of the block-hash table; the host picks K and
// lut_shift per launch so that different block hashes use different slots.
FZ_HD uint32_t fz_hash_windows(uint32_t x, uint32_t yh, uint32_t k) { return (yh & 0xffffffu) * (k & 0xffffffu) + x; }
FZ_HD uint32_t fz_hash_short(uint32_t x_masked, uint32_t k) { return x_masked * k; }

// ---------------------------------------------------------------------------------------------
// Bounded edit-distance expansion == c_expand_short == c_expand_long (SURVEY.md trap 2):
//   D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (sub[i-1] != win[j-1]), D[i][j-1]+1, D[i-1][j]+1)
//   best = len(sub), arg = 0;  for j = 1..len(win): if D[len(sub)][j] <= best: best, arg = D[..][j], j
//   -> (best, arg) if best <= budget else none.
// Evaluated column by column like the reference, but only on the diagonal band |i - j| <= budget:
// a cell outside the band is > budget, and cells > budget can never produce a cell <= budget, so
// the banded result is exact for every outcome that passes `best <= budget` (App. A.1: 0/100000).
// The band of one column is kept in a ring of W = 2*budget + 2 slots per lane (row i lives in slot
// i mod W; LDS on the GPU): Sc.get(slot) / Sc.set(slot, v).
// `sub(i)` / `win(j)` return element i / j of the (possibly reversed) piece and window.
template <class Sc, class SubF, class WinF>
FZ_HD bool fz_expand(Sc &sc, SubF sub, uint32_t sublen, WinF win, uint32_t winlen, uint32_t budget,
                     uint32_t &dist, uint32_t &consumed) {
    if (sublen == 0) { dist = 0; consumed = 0; return true; }       // pyx:28-30
    const uint32_t big = budget + 1;                                // "more than the budget"
    const uint32_t W = 2 * budget + 2;
    uint32_t best = sublen, arg = 0;
    // column 0: D[i][0] = i.  Only rows 1..budget can matter (D[i][0] > budget otherwise).
    {
        uint32_t rows = budget < sublen ? budget : sublen;
        for (uint32_t i = 1; i <= rows; ++i) sc.set(i, i);          // i < W, slot = i
    }
    // columns beyond sublen + budget cannot hold a bottom-row value <= budget
    uint32_t jmax = winlen;
    if (jmax > sublen + budget) jmax = sublen + budget;
    uint32_t i0 = 1, slot0 = 1;                                     // first band row and its slot
    for (uint32_t j = 1; j <= jmax; ++j) {
        const uint8_t ch = win(j - 1);
        // rows in band for this column: i in [max(1, j - budget), min(sublen, j + budget)]
        if (j > budget + 1) { ++i0; slot0 = (slot0 + 1 == W) ? 0 : slot0 + 1; }
        uint32_t i1 = j + budget; if (i1 > sublen) i1 = sublen;
        if (i0 > i1) break;                                         // band left the table (j - budget > sublen)
        uint32_t a, c;
        if (i0 == 1) { a = j - 1; c = j; }                          // D[0][j-1], D[0][j]  (pyx:49-50)
        else { a = sc.get(slot0 == 0 ? W - 1 : slot0 - 1); c = big; }  // D[i0-1][j-1] in band; D[i0-1][j] out
        uint32_t slot = slot0;
        uint32_t cmin = c;                                          // min over this column's band (+ D[0][j])
        for (uint32_t i = i0; i <= i1; ++i) {
            // left neighbour D[i][j-1]: out of band when i - (j-1) > budget -> treat as > budget
            uint32_t b = (i + 1 > j + budget) ? big : sc.get(slot);
            uint32_t v = a + (ch != sub(i - 1) ? 1u : 0u);          // pyx:54-58
            if (b + 1 < v) v = b + 1;
            if (c + 1 < v) v = c + 1;
            sc.set(slot, v);
            c = v;
            a = b;
            if (v < cmin) cmin = v;
            slot = (slot + 1 == W) ? 0 : slot + 1;
        }
        if (i1 == sublen && c <= best) { best = c; arg = j; }       // '<=' -> LAST arg-min (pyx:67-69)
        // column minima never decrease: once every cell is over budget no later column can pass
        // (the reference bails the same way, pyx:61-65)
        if (cmin > budget) break;
    }
    if (best <= budget) { dist = best; consumed = arg; return true; }
    return false;
}

// Register-resident variant of fz_expand for small budgets (K = the search's max_l_dist, <= FZ_REG_BAND_MAX):
// the same DP table, evaluated row by row on the band |j - i| <= K with the 2K+1 cells of a row and
// the 2K+1 window characters they are compared with held in statically indexed registers (the
// loops over the band offset d are fully unrolled) — no LDS round trip per cell, which made the
// ring version latency-bound (~300 cycles per cell).  Same result: the table does not depend on
// the evaluation order, the band K >= budget contains every cell <= budget, the bottom row is
// scanned in ascending j with '<=' (last arg-min) from the column-0 baseline, and a row whose
// minimum exceeds the budget ends the search (row minima never decrease).
#define FZ_REG_BAND_MAX 8
template <int K, class SubF, class WinF>
FZ_HD bool fz_expand_band(SubF sub, uint32_t sublen, WinF win, uint32_t winlen, uint32_t budget,
                          uint32_t &dist, uint32_t &consumed) {
    if (sublen == 0) { dist = 0; consumed = 0; return true; }
    constexpr uint32_t INF = 0x3fffffffu;
    constexpr int W = 2 * K + 1;
    uint32_t cell[W];            // row i: cell[d + K] = D[i][i + d]
    uint32_t chr[W];             // row i: chr[d + K] = win[i + d - 1], the character of column j = i + d
#pragma unroll
    for (int x = 0; x < W; ++x) {
        const int d = x - K;
        cell[x] = (d >= 0 && (uint32_t)d <= winlen) ? (uint32_t)d : INF;      // row 0: D[0][j] = j
        chr[x] = (d >= 0 && (uint32_t)d < winlen) ? (uint32_t)win((uint32_t)d) : 0x100u;   // row 1 compares win[d]
    }
    for (uint32_t i = 1; i <= sublen; ++i) {
        const uint32_t pc = sub(i - 1);
        uint32_t left = INF, rowmin = INF;
#pragma unroll
        for (int x = 0; x < W; ++x) {
            const int d = x - K;
            const int64_t j = (int64_t)i + d;
            const uint32_t diag = cell[x];
            const uint32_t up = (x + 1 < W) ? cell[x + 1] : INF;
            uint32_t v = diag + (chr[x] != pc ? 1u : 0u);
            if (up + 1 < v) v = up + 1;
            if (left + 1 < v) v = left + 1;
            if (j == 0) v = i;                                               // column 0: D[i][0] = i
            if (j < 0 || j > (int64_t)winlen) v = INF;
            cell[x] = v;
            left = v;
            if (v < rowmin) rowmin = v;
        }
        if (rowmin > budget) return false;
#pragma unroll
        for (int x = 0; x + 1 < W; ++x) chr[x] = chr[x + 1];
        const uint32_t nj = i + K;                                           // next row's rightmost column - 1
        chr[W - 1] = nj < winlen ? (uint32_t)win(nj) : 0x100u;
    }
    uint32_t best = sublen, arg = 0;                                         // column-0 baseline (pyx:33-34)
#pragma unroll
    for (int x = 0; x < W; ++x) {
        const int64_t j = (int64_t)sublen + (x - K);
        if (j >= 1 && j <= (int64_t)winlen && cell[x] <= best) { best = cell[x]; arg = (uint32_t)j; }
    }
    if (best <= budget) { dist = best; consumed = arg; return true; }
    return false;
}

// A byte string held in N registers: byte q of the string = byte (q & 3) of r[q >> 2].
// (Round 2 also measured the whole band DP on such registers — four rows per loop trip, every character a static
// byte of a register, dwords streamed a trip ahead: the rows of a flush took 6 300 instead of 11 500 cycles of
// latency but twice the wave instructions, and the fused scan is bound by VALU issue: 0.231 -> 0.235 ms.  Not kept;
// commit a3442c1^..HEAD~ has it with its host test.)
template <int N>
struct FzBytes {
    uint32_t r[N];
    FZ_HD uint32_t at(int q) const { return (r[q >> 2] >> (8 * (q & 3))) & 0xffu; }
};

// Budget-dispatched expansion: register band for k <= MAXK (<= FZ_REG_BAND_MAX), LDS ring otherwise.
// MAXK is a compile-time cap so that a kernel only pays (in VGPRs) for the band widths it may run:
// the fused scan kernel uses 4 (keeps it at <= 64 VGPRs), its lean instances 2 (fz_kernels.h: fz_lean_scan_kernel, only
// routed to with k <= 2), the stand-alone verify kernel 8.
template <int MAXK, class Sc, class SubF, class WinF>
FZ_HD bool fz_expand_any(Sc &sc, uint32_t k, SubF sub, uint32_t sublen, WinF win, uint32_t winlen, uint32_t budget,
                         uint32_t &dist, uint32_t &consumed) {
    if (k == 1) return fz_expand_band<1>(sub, sublen, win, winlen, budget, dist, consumed);
    if (k == 2) return fz_expand_band<2>(sub, sublen, win, winlen, budget, dist, consumed);
    if constexpr (MAXK >= 3) {
        if (k == 3) return fz_expand_band<3>(sub, sublen, win, winlen, budget, dist, consumed);
    }
    if constexpr (MAXK >= 4) {
        if (k == 4) return fz_expand_band<4>(sub, sublen, win, winlen, budget, dist, consumed);
    }
    if constexpr (MAXK >= 8) {
        if (k == 5) return fz_expand_band<5>(sub, sublen, win, winlen, budget, dist, consumed);
        if (k == 6) return fz_expand_band<6>(sub, sublen, win, winlen, budget, dist, consumed);
        if (k == 7) return fz_expand_band<7>(sub, sublen, win, winlen, budget, dist, consumed);
        if (k == 8) return fz_expand_band<8>(sub, sublen, win, winlen, budget, dist, consumed);
    }
    return fz_expand(sc, sub, sublen, win, winlen, budget, dist, consumed);
}

// Accepted hit range of the block starting at pattern offset s, relative to the ends of the sequence /
// segment: sa + lo_rel <= idx and idx + L <= se - hi_sub.
FZ_HD void fz_block_range(uint32_t mode, uint32_t m, uint32_t k, uint32_t L, uint32_t s, uint32_t &lo_rel, uint32_t &hi_sub) {
    if (mode == FZ_MODE_SUBS) { lo_rel = s; hi_sub = m - s - L; }                  // template.h:97-101
    else if (mode == FZ_MODE_EXACT) { lo_rel = 0; hi_sub = 0; }
    else {                                                                         // levenshtein_ngram.py:171-176
        lo_rel = s > k ? s - k : 0;
        hi_sub = m - s - L > k ? m - s - L - k : 0;
    }
}

// Index-range test of a candidate against one segment (block's accepted hit range, absolute range,
// shard ownership) — the `for index in search_exact(ngram, sequence, start, end)` bounds of
// levenshtein_ngram.py:171-176 / generic_search.py:221-228 / _substitutions_only_ngrams_template.h:97-101.
FZ_HD bool fz_hit_in_range(const FzScanArgs &a, uint32_t blk, uint64_t idx, const FzSeg &sg) {
    if (!sg.ok || blk >= a.nblk) return false;
    if (idx < sg.sa + a.lo_rel[blk]) return false;
    if (sg.se < a.hi_sub[blk] || idx + a.L > sg.se - a.hi_sub[blk]) return false;
    if (idx < a.abs_lo || idx + a.L > a.abs_hi) return false;
    return idx >= a.geom.own_lo && idx < a.geom.own_hi;
}

// The same test for a hit of ANY block of the search (kernels that run after the scan launches).
FZ_HD bool fz_hit_in_range_s(const FzScanArgs &a, uint32_t s, uint64_t idx, const FzSeg &sg) {
    if (!sg.ok) return false;
    uint32_t lo_rel, hi_sub;
    fz_block_range(a.mode, a.m, a.k, a.L, s, lo_rel, hi_sub);
    if (idx < sg.sa + lo_rel) return false;
    if (sg.se < hi_sub || idx + a.L > sg.se - hi_sub) return false;
    if (idx < a.abs_lo || idx + a.L > a.abs_hi) return false;
    return idx >= a.geom.own_lo && idx < a.geom.own_hi;
}

// levenshtein_ngram.py:177-198 for one hit (block starting at s in the pattern, hit at idx) inside the
// sequence / segment [sa, se) (sa = 0, se = n for an in-memory search).
// `t.at(g)` returns the sequence byte at GLOBAL index g; only indices inside
// [max(sa, idx-s-k), min(se, idx-s+m+k)) are ever requested.
template <int MAXK, class Sc, class Seq>
FZ_HD bool fz_verify_lev(Sc &sc, const Seq &t, uint64_t sa, uint64_t se, const uint8_t *p, uint32_t m,
                         uint32_t k, uint32_t L, uint32_t s, uint64_t idx, FzRec &rec) {
    // right: p[s+L:] vs t[idx+L : min(se, idx-s+m+k)]      (idx >= sa+s-k guarantees idx-s+m+k >= sa)
    const uint32_t rlen = m - s - L;
    uint64_t rbeg = idx + L;
    uint64_t rend = idx + m + k - s; if (rend > se) rend = se;
    if (rbeg > se) rbeg = se;
    if (rend < rbeg) rend = rbeg;
    uint32_t dR = 0, r = 0;
    {
        const uint8_t *ps = p + s + L;
        auto sub = [&](uint32_t i) -> uint8_t { return ps[i]; };
        auto win = [&](uint32_t j) -> uint8_t { return t.at(rbeg + j); };
        if (!fz_expand_any<MAXK>(sc, k, sub, rlen, win, (uint32_t)(rend - rbeg), k, dR, r)) return false;
    }
    // left: reversed p[:s] vs reversed t[max(sa, idx-s-(k-dR)) : idx], budget k - dR
    const uint32_t bl = k - dR;
    uint64_t want = (uint64_t)s + bl;
    uint64_t lbeg = (idx - sa > want) ? (idx - want) : sa;
    uint32_t dL = 0, l = 0;
    {
        auto sub = [&](uint32_t i) -> uint8_t { return p[s - 1 - i]; };
        auto win = [&](uint32_t j) -> uint8_t { return t.at(idx - 1 - j); };
        if (!fz_expand_any<MAXK>(sc, k, sub, s, win, (uint32_t)(idx - lbeg), bl, dL, l)) return false;
    }
    rec.l = l; rec.r = r; rec.dist = dL + dR; rec.aux = 0;
    return true;
}

// ---------------------------------------------------------------------------------------------
// Bit-vector expansion — the same table as fz_expand (c_expand_short / c_expand_long, _levenshtein_ngrams.pyx:9-154),
// evaluated one COLUMN (= one sequence character) at a time by the column recurrence of Myers (1999) in Hyyrö's (2001)
// form: a column of the table is held as its vertical differences, two bit vectors over the piece's rows
//     VP bit i: D[i+1][j] - D[i][j] = +1        VN bit i: D[i+1][j] - D[i][j] = -1
// and one step takes the column j-1 to the column j with ~15 word operations, whatever the budget — no band, no cell
// outside it, every cell exact.  The piece's last row is the TOP bit of the vector, so the score D[m'][j] follows from the
// sign bits of the horizontal differences; the reference's `D[0][j] = j` boundary (the window is matched from its first
// character: prefix distance, not the search-anywhere form) is the 1 shifted into the horizontal +1 vector.
// One candidate per LANE; a piece of up to 64 rows is one 64-bit word (NW = 1), up to 128 rows two (NW = 2), up to 32 rows
// half a word (NW = 4 names the 32-bit form: half the vector instructions per column for patterns up to 32 characters).
//
// Both pieces of a hit come out of TWO tables per search, not two per n-gram block: with the whole pattern laid down top-
// aligned, position q at bit q + (64 NW - m) of the forward table Peq[c] and at bit 64 NW - 1 - q of the reversed one,
//     the right piece p[s+L:]         (rows i = q - s - L)  occupies the top  m - s - L  bits of the forward table,
//     the left piece  reversed(p[:s]) (rows i = s - 1 - q)  occupies the top  s          bits of the reversed table
// for EVERY block start s: a piece is selected by masking Eq with its top bits (`hm`), never by a shift.  The rows below
// a piece then hold Eq = 0, VP = 0, VN = 0, stay that way under the recurrence (their horizontal +1 bits are all set, which
// is exactly the boundary's +1 entering the piece's first row) and feed no carry into it.
template <int NW> struct FzBitsWord;
template <> struct FzBitsWord<1> { typedef uint64_t T; };
template <> struct FzBitsWord<2> { typedef unsigned __int128 T; };
template <> struct FzBitsWord<4> { typedef uint32_t T; };
#define FZ_BITS_WIDTH(NW) ((NW) == 4 ? 32u : 64u * (uint32_t)(NW))   // bits of a column vector = longest pattern of the form
#define FZ_BITS_MAX_M(NW) FZ_BITS_WIDTH(NW)

template <int NW> FZ_HD uint32_t fz_bits_fwd_bit(uint32_t m, uint32_t q) { return q + (FZ_BITS_WIDTH(NW) - m); }
template <int NW> FZ_HD uint32_t fz_bits_rev_bit(uint32_t, uint32_t q) { return FZ_BITS_WIDTH(NW) - 1u - q; }

template <int NW>
struct FzBitsCol {
    typename FzBitsWord<NW>::T vp, vn;
};

// a | ~x
template <class T> FZ_HD T fz_or_not(T a, T x) { return a | ~x; }

// Column j-1 -> column j.  `eq`: the piece's rows whose character equals the column's (masked to the piece).
// -> D[m'][j] - D[m'][j-1] (-1, 0 or +1).
template <int NW>
FZ_HD int32_t fz_bits_column(FzBitsCol<NW> &c, typename FzBitsWord<NW>::T eq) {
    typedef typename FzBitsWord<NW>::T T;
    constexpr int TOP = (int)FZ_BITS_WIDTH(NW) - 1;
    const T d0 = (((eq & c.vp) + c.vp) ^ c.vp) | eq | c.vn;     // rows whose diagonal difference is 0
    T hp = fz_or_not<T>(c.vn, d0 | c.vp);                       // horizontal +1
    T hn = c.vp & d0;                                           // horizontal -1
    const int32_t delta = (int32_t)(uint32_t)(uint64_t)(hp >> TOP) - (int32_t)(uint32_t)(uint64_t)(hn >> TOP);
    hp = (hp << 1) | (T)1;                                      // D[0][j] - D[0][j-1] = +1
    hn = hn << 1;
    c.vp = fz_or_not<T>(hn, d0 | hp);
    c.vn = hp & d0;
    return delta;
}

#if defined(__HIP_DEVICE_COMPILE__)
// The one- and two-word columns on the GPU, written on their 32-bit words (only the addition is a wide operation): gfx950
// has a three-input bit operation (v_bitop3_b32) and a funnel shift (v_alignbit_b32), which the compiler only forms from
// 32-bit operands — 36 vector instructions per one-word column instead of 41, 58 instead of 70 per two-word one.  Same
// function, bit for bit (the host model runs the generic one; tests/test_gpu_bits_verify.py holds these against the oracle).
template <int NW>
__device__ __forceinline__ int32_t fz_bits_column_words(FzBitsCol<NW> &c, typename FzBitsWord<NW>::T eq) {
    typedef typename FzBitsWord<NW>::T T;
    constexpr int NH = 2 * NW;                                   // 32-bit words of a vector
    const T sum = (eq & c.vp) + c.vp;
    uint32_t d0[NH], hp[NH], hn[NH];
#pragma unroll
    for (int w = 0; w < NH; ++w) {
        const uint32_t vpw = (uint32_t)(c.vp >> (32 * w)), vnw = (uint32_t)(c.vn >> (32 * w)), eqw = (uint32_t)(eq >> (32 * w));
        d0[w] = (((uint32_t)(sum >> (32 * w)) ^ vpw) | eqw) | vnw;
        hp[w] = vnw | ~(d0[w] | vpw);
        hn[w] = vpw & d0[w];
    }
    const int32_t delta = (int32_t)(hp[NH - 1] >> 31) - (int32_t)(hn[NH - 1] >> 31);
    T nvp = 0, nvn = 0;
#pragma unroll
    for (int w = 0; w < NH; ++w) {
        const uint32_t hps = (hp[w] << 1) | (w ? hp[w ? w - 1 : 0] >> 31 : 1u);      // D[0][j] - D[0][j-1] = +1 enters word 0
        const uint32_t hns = (hn[w] << 1) | (w ? hn[w ? w - 1 : 0] >> 31 : 0u);
        nvp |= (T)(hns | ~(d0[w] | hps)) << (32 * w);
        nvn |= (T)(hps & d0[w]) << (32 * w);
    }
    c.vp = nvp;
    c.vn = nvn;
    return delta;
}
template <> FZ_HD int32_t fz_bits_column<1>(FzBitsCol<1> &c, uint64_t eq) { return fz_bits_column_words<1>(c, eq); }
template <> FZ_HD int32_t fz_bits_column<2>(FzBitsCol<2> &c, unsigned __int128 eq) { return fz_bits_column_words<2>(c, eq); }
#endif

// One expansion on its own (tests, and the statement of what the two-phase loop below computes per side):
// peq(c) = the piece's rows that hold character c, bit i = row i + 1 at bit 64 NW - sublen + i.
template <int NW, class PeqF, class WinF>
FZ_HD bool fz_expand_bits(PeqF peq, uint32_t sublen, WinF win, uint32_t winlen, uint32_t budget,
                          uint32_t &dist, uint32_t &consumed) {
    typedef typename FzBitsWord<NW>::T T;
    if (sublen == 0) { dist = 0; consumed = 0; return true; }       // pyx:28-30
    const T hm = ~(T)0 << (FZ_BITS_WIDTH(NW) - sublen);
    FzBitsCol<NW> c;
    c.vp = hm; c.vn = 0;                                             // column 0: D[i][0] = i
    uint32_t score = sublen, best = sublen, arg = 0;                 // pyx:33-34
    for (uint32_t j = 1; j <= winlen; ++j) {
        score += (uint32_t)fz_bits_column<NW>(c, peq(win(j - 1)) & hm);
        if (score <= best) { best = score; arg = j; }                // '<=' -> LAST arg-min (pyx:67-69)
    }
    if (best <= budget) { dist = best; consumed = arg; return true; }
    return false;
}

// levenshtein_ngram.py:177-198 for one hit by the bit-vector recurrence: right expansion with budget k, then the left one
// with what is left of it, as ONE loop in which every lane walks through its own two expansions — a lane's right piece has
// m - s - L rows and its left one s, so the lanes of a wave differ in both but hardly in the sum (~ m - L + 2k columns):
// run one after the other the wave would pay max(right) + max(left) columns, this way it pays max(right + left).
//   peq.table(side)    -> handle of the forward (0) / reversed (1) table,   peq.at(handle, c) -> its word for character c
//   txt(o)             -> sequence byte at global index wbase + o.  The loop requests a column's Peq word one column
//                         ahead and its character two ahead (on the GPU both are LDS reads: their latency then hides behind
//                         the ~40 instructions of a column), so txt is also asked for up to TWO positions past the end of
//                         an expansion's window (either side); what it returns there is never used.
// `valid` = false: the lane has no candidate (it still takes part in the wave-uniform loop control).
template <int NW, class PeqT, class TxtF>
FZ_HD bool fz_verify_lev_bits(const PeqT &peq, TxtF txt, uint64_t wbase, uint64_t sa, uint64_t se, uint32_t m, uint32_t k,
                              uint32_t L, uint32_t s, uint64_t idx, bool valid, FzRec &rec) {
    typedef typename FzBitsWord<NW>::T T;
    constexpr uint32_t NB = FZ_BITS_WIDTH(NW);
    FzBitsCol<NW> col;
    T hm = 0;
    uint32_t rem = 0, wl = 0, score = 0, key = 0, budget = k, dR = 0, r = 0;
    // start an expansion of a piece of `rows` rows over `cols` window characters: column 0 is D[i][0] = i, the running
    // minimum starts at the column-0 baseline (best = rows, arg = 0: pyx:33-34).  key = (score << 8) | columns left: the
    // minimum over the columns prefers, among equal scores, the LATER column ('<=': last arg-min, pyx:67-69).
    auto start = [&](uint32_t rows, uint32_t cols) {
        hm = rows ? ~(T)0 << (NB - rows) : (T)0;
        col.vp = hm; col.vn = 0;
        score = rows;
        wl = rows ? cols : 0u;                                       // an empty piece expands to (0, 0) (pyx:28-30)
        rem = wl;
        key = (rows << 8) | wl;
    };
    // right: p[s+L:] vs t[idx+L : min(se, idx-s+m+k)]
    uint64_t rbeg = idx + L, rend = idx + m + k - s;
    if (rend > se) rend = se;
    if (rbeg > se) rbeg = se;
    if (rend < rbeg) rend = rbeg;
    start(m - s - L, (uint32_t)(rend - rbeg));
    uint32_t phase = valid ? 0u : 2u;                                // 0 right, 1 left, 2 done
    if (!valid) rem = 0;
    uint32_t pos = (uint32_t)(rbeg - wbase), dir = 1u;
    uint32_t tab = peq.table(0);
    uint32_t chn = 0;                                                // character of the column after the next one
    T eqn = 0;                                                       // Peq word of the next column
    // (the reads of an expansion's first two characters are made whether it has columns or not: txt tolerates them)
    auto prime = [&]() {
        eqn = peq.at(tab, txt(pos));
        chn = txt(pos + dir);
        pos += 2u * dir;
    };
    if (valid) prime();
    bool ok = false;
    uint32_t res_l = 0, res_dist = 0;
    // what the left expansion will be, as far as it does not depend on the right one's outcome
    const T hm_left = s ? ~(T)0 << (NB - s) : (T)0;
    const uint32_t pos_left = (uint32_t)(idx - wbase) - 1u;
    const uint64_t room_left = idx - sa;                             // sequence bytes to the left of the hit
    // Loop control on wave masks (the host model is a wave of one lane): `live` = lanes that still have an expansion to
    // finish.  A column costs ~36 vector instructions; what is added per column for control is one compare and scalar work.
    unsigned long long live = FZ_WAVE_BALLOT(phase < 2u);
    while (live) {
        if (FZ_WAVE_BALLOT(rem == 0u) & live) {                     // some lane's expansion has seen its last column
            if (rem == 0u && phase < 2u) {
                // ONE divergent region with selects inside it, and one WAVE-UNIFORM branch around the left expansion's start
                // (nested divergent branches cost this block more in exec-mask bookkeeping than its arithmetic; most of a
                // wave's ~40 turn events per pass only end lanes — a failed right side, a finished left one — and skip it)
                const uint32_t best = key >> 8, arg = wl - (key & 255u);
                const bool pass = best <= budget;
                const bool to_left = pass && phase == 0u, finish = pass && phase == 1u;
                res_l = finish ? arg : res_l;
                res_dist = finish ? dR + best : res_dist;
                ok = ok || finish;
                phase = to_left ? 1u : 2u;
                if (FZ_WAVE_ANY(to_left)) {
                    // left: reversed p[:s] vs reversed t[max(sa, idx-s-(k-dR)) : idx], budget k - dR
                    dR = to_left ? best : dR;
                    r = to_left ? arg : r;
                    budget = to_left ? k - best : budget;
                    const uint64_t want = (uint64_t)s + budget;
                    const uint32_t lcols = (uint32_t)(room_left > want ? want : room_left);
                    hm = hm_left;
                    col.vp = hm_left; col.vn = 0;
                    score = s;
                    wl = (to_left && s) ? lcols : 0u;                // (an empty piece expands to (0, 0))
                    rem = wl;
                    key = (s << 8) | wl;
                    pos = pos_left; dir = ~0u;
                    tab = peq.table(1);
                    prime();
                }
            }
            live = FZ_WAVE_BALLOT(phase < 2u);
        }
        const uint32_t act = rem != 0u ? 1u : 0u;                    // (rem != 0 only in phases 0 and 1)
        if (act) {
            const T eq = eqn & hm;
            eqn = peq.at(tab, chn);
            chn = txt(pos);
            pos += dir;
            score += (uint32_t)fz_bits_column<NW>(col, eq);
            const uint32_t cand = (score << 8) | (rem - 1u);
            if (cand < key) key = cand;
        }
        rem -= act;
    }
    rec.l = res_l; rec.r = r; rec.dist = res_dist; rec.aux = 0;
    return ok;
}

// _substitutions_only_ngrams_template.h:103-121 for one hit h of the block starting at s:
// window start i = h - s; accept iff Hamming(p, t[i:i+m]) <= k.  The caller guarantees
// s <= h and h - s + m <= n (the block's hit range).  dist = min(Hamming, k+1) (common.py:119-142
// as called from substitutions_only.py:270-274) which, for an accepted window, is the Hamming
// distance itself.
template <class Seq>
FZ_HD bool fz_verify_subs(const Seq &t, const uint8_t *p, uint32_t m, uint32_t k, uint32_t L,
                          uint32_t s, uint64_t h, FzRec &rec) {
    const uint64_t i0 = h - s;
    uint32_t nd = 0;
    for (uint32_t q = 0; q < m; ++q) {
        if (q == s) { q += L - 1; continue; }                       // the n-gram itself matched
        nd += (p[q] != t.at(i0 + q)) ? 1u : 0u;
        if (nd > k) return false;
    }
    rec.l = s; rec.r = m - s - L; rec.dist = nd; rec.aux = 0;
    return true;
}

// ---------------------------------------------------------------------------------------------
// Generic search: the greedy candidate-set automaton of
// _find_near_matches_generic_linear_programming (generic_search.py:57-177, _generic_search.pyx:61-233;
// SURVEY.md trap 6 / App. A.3 — NOT a DP).  One candidate, one window character -> up to three
// successor candidates and up to two matches, in the reference's order.  Coordinates are relative
// to the window (<= m + 2k bytes), so 16 bits suffice.
struct FzGCand {
    uint16_t start, j;                 // window-relative start, next pattern index (subseq_index)
    uint8_t l, ns, ni, nd;             // l_dist, n_subs, n_ins, n_dels
};

struct FzGOut {
    FzGCand succ[3];
    uint32_t nsucc;
    uint32_t mstart[2], mend[2], mdist[2];
    uint32_t nmatch;
};

// Appends with compile-time indices only: a dynamically indexed member array would move the whole
// struct to scratch memory on the GPU (78 scratch accesses in the automaton kernel's inner loop).
FZ_HD void fz_gout_succ(FzGOut &o, const FzGCand &x) {
    if (o.nsucc == 0) o.succ[0] = x;
    else if (o.nsucc == 1) o.succ[1] = x;
    else o.succ[2] = x;
    ++o.nsucc;
}
FZ_HD void fz_gout_match(FzGOut &o, uint32_t start, uint32_t end, uint32_t dist) {
    if (o.nmatch == 0) { o.mstart[0] = start; o.mend[0] = end; o.mdist[0] = dist; }
    else { o.mstart[1] = start; o.mend[1] = end; o.mdist[1] = dist; }
    ++o.nmatch;
}

template <class PatF>
FZ_HD void fz_generic_step(const FzGCand &c, uint8_t ch, uint32_t index, uint32_t m, PatF pat,
                           uint32_t max_subs, uint32_t max_ins, uint32_t max_dels, uint32_t max_l, FzGOut &o) {
    o.nsucc = 0; o.nmatch = 0;
    auto match = [&](uint32_t end, uint32_t dist) { fz_gout_match(o, c.start, end, dist); };
    if (ch == pat(c.j)) {                                              // py:85-94
        if (c.j + 1u == m) match(index + 1, c.l);
        else { FzGCand x = c; x.j = (uint16_t)(c.j + 1); fz_gout_succ(o, x); }
        return;
    }
    if (c.l == max_l) return;                                          // py:101-102
    if (c.ni < max_ins) {                                              // py:104-109: skip a sequence char
        FzGCand x = c; x.ni++; x.l++; fz_gout_succ(o, x);
    }
    if (c.j + 1u < m) {                                                // py:111-128
        if (c.ns < max_subs) {
            FzGCand x = c; x.ns++; x.j++; x.l++; fz_gout_succ(o, x);
        } else if (c.nd < max_dels && c.ni < max_ins) {
            FzGCand x = c; x.ni++; x.nd++; x.j++; x.l++; fz_gout_succ(o, x);
        }
    } else if (c.ns < max_subs || (c.nd < max_dels && c.ni < max_ins)) {   // py:129-138
        match(index + 1, c.l + 1u);
    }
    uint32_t lim = max_dels - c.nd;                                    // py:141-165: skip pattern chars
    if (max_l - c.l < lim) lim = max_l - c.l;
    for (uint32_t sk = 1; sk <= lim; ++sk) {
        if (c.j + sk == m) { match(index, c.l + sk); break; }
        if (pat(c.j + sk) == ch) {
            if (c.j + sk + 1u == m) match(index, c.l + sk);
            else {
                FzGCand x = c; x.nd = (uint8_t)(c.nd + sk); x.j = (uint16_t)(c.j + 1u + sk); x.l = (uint8_t)(c.l + sk);
                fz_gout_succ(o, x);
            }
            break;
        }
    }
}

// The same step on the candidate as it lies in memory — dword 0 = start | j << 16, dword 1 = l | ns << 8 | ni << 16 |
// nd << 24 (FzGCand, little endian) — with the outputs in fixed slots: successor A (advance, or skip a sequence
// character), B (substitution, or insertion + deletion), C (skip pattern characters), match 1 (at index + 1) and
// match 2 (at index), which is the reference's order.  Field updates are additions on the packed words, there are no
// arrays to select into: the kernel's hot form (the struct form above costs ~3x the instructions on the GPU and
// stays as the host-tested statement of the reference; tests/test_device_logic_host.py holds the two together).
struct FzGStep {
    uint32_t a0, a1, b0, b1, c0, c1;
    uint32_t fa, fb, fc;               // 0 / 1: successor present
    uint32_t m1, d1, f1, m2, d2, f2;   // matches: start | end << 16, distance, present
};

FZ_HD void fz_gstep_clear(FzGStep &o) {
    o.a0 = o.a1 = o.b0 = o.b1 = o.c0 = o.c1 = 0; o.fa = o.fb = o.fc = 0;
    o.m1 = o.d1 = o.f1 = o.m2 = o.d2 = o.f2 = 0;
}

// Written without lane-divergent control flow: flags are 0 / 1 words combined with & | ^, the pattern-skip loop
// runs a wave-uniform number of rounds (the profile of the branchy form showed the automaton's waves neither
// executing vector instructions nor waiting for memory for two thirds of their time: exec-mask bookkeeping
// and ~100 branches per 64 candidates).
template <class PatF>
FZ_HD void fz_generic_step_packed(uint32_t w0, uint32_t w1, uint8_t ch, uint32_t index, uint32_t m, PatF pat,
                                  uint32_t max_subs, uint32_t max_ins, uint32_t max_dels, uint32_t max_l, FzGStep &o) {
    // conditions as bools combined with & | ! (never && ||): lane masks in scalar registers on the GPU, where the
    // vector ALU is this kernel's busiest unit
    const uint32_t start = w0 & 0xffffu, j = w0 >> 16;
    const uint32_t l = w1 & 0xffu, ns = (w1 >> 8) & 0xffu, ni = (w1 >> 16) & 0xffu, nd = w1 >> 24;
    // the pattern characters of the first two skip rounds are requested together with pattern[j]: three
    // independent reads instead of a chain of dependent ones (the kernel takes as long as its slowest hit, and a
    // hit's time is this chain, character after character)
    const uint32_t j1 = j + 1u < m ? j + 1u : m - 1u, j2 = j + 2u < m ? j + 2u : m - 1u;
    const uint8_t pj = pat(j);
    const uint8_t p1 = max_dels >= 1u ? pat(j1) : (uint8_t)0, p2 = max_dels >= 2u ? pat(j2) : (uint8_t)0;
    const bool adv = pj == ch;                                         // py:85-94
    const bool at_end = j + 1u == m;
    const bool live = !adv & (l != max_l);                             // py:101-102
    const bool can_ins = ni < max_ins, can_sub = ns < max_subs;
    const bool second = live & (can_sub | ((nd < max_dels) & can_ins));
    o.fa = ((adv & !at_end) | (live & can_ins)) ? 1u : 0u;             // py:104-109
    o.a0 = adv ? w0 + 0x10000u : w0;
    o.a1 = adv ? w1 : w1 + 0x00010001u;                                // ni++, l++
    o.fb = (second & !at_end) ? 1u : 0u;                               // py:111-128
    o.b0 = w0 + 0x10000u;
    o.b1 = w1 + (can_sub ? 0x00000101u : 0x01010001u);                 // ns++, l++  |  ni++, nd++, l++
    o.f1 = ((adv | second) & at_end) ? 1u : 0u;                        // py:86-88, py:129-138
    o.m1 = start | ((index + 1u) << 16);
    o.d1 = adv ? l : l + 1u;
    // py:141-165: the first sk in 1..lim with j + sk == m or pattern[j + sk] == ch
    uint32_t lim = max_dels - nd;
    lim = max_l - l < lim ? max_l - l : lim;
    lim = live ? lim : 0u;
    uint32_t fsk = 0;
    if (max_dels >= 1u) fsk = ((1u <= lim) & ((j + 1u >= m) | (p1 == ch))) ? 1u : 0u;
    if (max_dels >= 2u) fsk = ((2u <= lim) & (fsk == 0u) & ((j + 2u >= m) | (p2 == ch))) ? 2u : fsk;
    for (uint32_t sk = 3; sk <= max_dels; ++sk) {
        const bool open = (sk <= lim) & (fsk == 0u);
        if (!FZ_WAVE_ANY(open ? 1u : 0u)) break;
        const uint32_t pos = j + sk;
        const bool hit = (pos >= m) | (pat(pos < m ? pos : m - 1u) == ch);
        fsk = (open & hit) ? sk : fsk;
    }
    const bool found = fsk != 0u;
    const bool to_end = j + fsk + 1u >= m;                             // ran off the pattern, or matched its last char
    o.f2 = (found & to_end) ? 1u : 0u;
    o.m2 = start | (index << 16);
    o.d2 = l + fsk;
    o.fc = (found & !to_end) ? 1u : 0u;
    o.c0 = w0 + ((1u + fsk) << 16);
    o.c1 = w1 + ((fsk << 24) | fsk);
}

// The same step again for patterns of at most 64 characters and budgets of at most 32 (round 5): the comparisons
// pattern[j] == ch, pattern[j + 1] == ch, ... are bits of ONE 64-bit word per sequence character — peq, bit i set iff
// pattern[i] == ch (a 256-entry table per pattern, one look-up per window character, the same for every candidate) — and
// the skip search of py:141-165 ("the first sk with j + sk == m or pattern[j + sk] == ch") is one find-first-set on
// (peq with a sentinel bit at m) >> (j + 1).  Every flag is a 0 / 1 WORD computed with integer arithmetic — no
// comparison results in scalar registers, no lane-mask algebra on the scalar unit, no pattern reads from LDS, no loop:
// fz_gen_hit_kernel's time is the dependent instruction chain of this step, once per window character (round 4 measured
// ~2 300 cycles per character for the form above: ~150 instructions of which every second hops between the vector and
// the scalar unit).  Same outputs as fz_generic_step_packed, bit for bit (tests/host_emul.cpp holds them together).
FZ_HD uint32_t fz_b_lt(uint32_t a, uint32_t b) { return (a - b) >> 31; }                  // a < b for values below 2^31
FZ_HD uint32_t fz_b_eq(uint32_t a, uint32_t b) { return ((a ^ b) - 1u) >> 31; }           // a == b (a ^ b below 2^31)

FZ_HD void fz_generic_step_bits(uint32_t w0, uint32_t w1, uint64_t peq, uint32_t index, uint32_t m,
                                uint32_t max_subs, uint32_t max_ins, uint32_t max_dels, uint32_t max_l, FzGStep &o) {
    const uint32_t start = w0 & 0xffffu, j = w0 >> 16;
    const uint32_t l = w1 & 0xffu, ns = (w1 >> 8) & 0xffu, ni = (w1 >> 16) & 0xffu, nd = w1 >> 24;
    const uint64_t skipw = (peq >> 1) | (1ull << (m - 1u));             // bit (j + sk - 1): j + sk == m or pattern[j + sk] == ch
    const uint32_t adv = (uint32_t)(peq >> j) & 1u;                     // py:85-94
    const uint32_t skips = (uint32_t)(skipw >> j);                      // bit sk - 1 for sk = 1 .. 32
    const uint32_t nadv = adv ^ 1u;
    const uint32_t at_end = fz_b_eq(j + 1u, m), not_end = at_end ^ 1u;
    const uint32_t live = nadv & (fz_b_eq(l, max_l) ^ 1u);              // py:101-102
    const uint32_t can_ins = fz_b_lt(ni, max_ins), can_sub = fz_b_lt(ns, max_subs);
    const uint32_t second = live & (can_sub | (fz_b_lt(nd, max_dels) & can_ins));
    o.fa = (adv & not_end) | (live & can_ins);                          // py:104-109
    o.a0 = w0 + (adv << 16);
    o.a1 = w1 + nadv * 0x00010001u;                                     // ni++, l++
    o.fb = second & not_end;                                            // py:111-128
    o.b0 = w0 + 0x10000u;
    o.b1 = w1 + 0x01010001u - can_sub * (0x01010001u - 0x00000101u);    // ns++, l++  |  ni++, nd++, l++
    o.f1 = (adv | second) & at_end;                                     // py:86-88, py:129-138
    o.m1 = start | ((index + 1u) << 16);
    o.d1 = l + nadv;
    uint32_t lim = max_dels - nd;                                       // py:141-165
    const uint32_t lim2 = max_l - l;
    lim = lim2 < lim ? lim2 : lim;
    lim *= live;
    uint32_t fsk = (uint32_t)__builtin_ffs((int)skips);                 // 0: no such sk among the first 32
    fsk *= fz_b_lt(fsk, lim + 1u);                                      // beyond the budget: none
    const uint32_t found = fz_b_lt(0u, fsk);
    const uint32_t to_end = fz_b_lt(m, j + fsk + 2u);                   // j + fsk + 1 >= m: ran off the pattern, or matched its last char
    o.f2 = found & to_end;
    o.m2 = start | (index << 16);
    o.d2 = l + fsk;
    o.fc = found & (to_end ^ 1u);
    o.c0 = w0 + ((1u + fsk) << 16);
    o.c1 = w1 + ((fsk << 24) | fsk);
}

FZ_HD void fz_gcand_words(const FzGCand &c, uint32_t &w0, uint32_t &w1) {
    w0 = (uint32_t)c.start | ((uint32_t)c.j << 16);
    w1 = (uint32_t)c.l | ((uint32_t)c.ns << 8) | ((uint32_t)c.ni << 16) | ((uint32_t)c.nd << 24);
}
FZ_HD FzGCand fz_gcand_of(uint32_t w0, uint32_t w1) {
    FzGCand c;
    c.start = (uint16_t)w0; c.j = (uint16_t)(w0 >> 16);
    c.l = (uint8_t)w1; c.ns = (uint8_t)(w1 >> 8); c.ni = (uint8_t)(w1 >> 16); c.nd = (uint8_t)(w1 >> 24);
    return c;
}
// struct form -> slot form (the tiled Levenshtein automaton and the end-of-window flush: not hot)
FZ_HD void fz_gstep_from_out(const FzGOut &g, FzGStep &o) {
    fz_gstep_clear(o);
    if (g.nsucc > 0) { o.fa = 1; fz_gcand_words(g.succ[0], o.a0, o.a1); }
    if (g.nsucc > 1) { o.fb = 1; fz_gcand_words(g.succ[1], o.b0, o.b1); }
    if (g.nsucc > 2) { o.fc = 1; fz_gcand_words(g.succ[2], o.c0, o.c1); }
    if (g.nmatch > 0) { o.f1 = 1; o.m1 = g.mstart[0] | (g.mend[0] << 16); o.d1 = g.mdist[0]; }
    if (g.nmatch > 1) { o.f2 = 1; o.m2 = g.mstart[1] | (g.mend[1] << 16); o.d2 = g.mdist[1]; }
}

// find_near_matches_levenshtein_linear_programming (levenshtein.py:52-148): one candidate, one
// sequence character.  `more_seq` is the reference's `index + 1 < len(sequence)` (global).
template <class PatF>
FZ_HD void fz_levlp_step(const FzGCand &c, uint8_t ch, uint32_t index, bool more_seq, uint32_t m, PatF pat,
                         uint32_t k, FzGOut &o) {
    o.nsucc = 0; o.nmatch = 0;
    auto match = [&](uint32_t end, uint32_t dist) { fz_gout_match(o, c.start, end, dist); };
    if (pat(c.j) == ch) {                                              // :84-92
        if (c.j + 1u == m) match(index + 1, c.l);
        else { FzGCand x = c; x.j = (uint16_t)(c.j + 1); fz_gout_succ(o, x); }
        return;
    }
    if (c.l == k) return;                                              // :99-100
    { FzGCand x = c; x.l++; fz_gout_succ(o, x); }                   // :103 skip a sequence char
    if (more_seq && c.j + 1u < m) {                                    // :105-111 skip both
        FzGCand x = c; x.l++; x.j++; fz_gout_succ(o, x);
    }
    for (uint32_t sk = 1; sk <= k - c.l; ++sk) {                       // :114-137 skip pattern chars
        if (c.j + sk == m) { match(index + 1, c.l + sk); break; }
        if (pat(c.j + sk) == ch) {
            if (c.j + sk + 1u == m) match(index + 1, c.l + sk);
            else { FzGCand x = c; x.l = (uint8_t)(c.l + sk); x.j = (uint16_t)(c.j + 1u + sk); fz_gout_succ(o, x); }
            break;
        }
    }
}

// The same step with its outputs in the fixed slots of FzGStep (what fz_lp_kernel stores through wave prefix sums):
// successors in list order a (:103), b (:105-111), c (:114-137), at most one match.  No arrays: the struct form's
// succ[] was indexed dynamically and lived in scratch memory (20 bytes per lane in the tiled Levenshtein automaton).
//
// The pattern-skip loop (:114-137) is written WITHOUT a lane-divergent exit: every lane runs the same rounds and keeps
// the first sk that ends its search in `fsk`; the loop leaves on a wave-uniform condition only (as the generic step
// above does).  Round 4 had the reference's shape here — `for (sk ..) { if (hit) { ..; break; } }` — and hipcc
// (ROCm 7.2.0, gfx950, -O2 / -O3, inlined into fz_lp_kernel) miscompiled it: the VGPR holding successor a's first word
// (live across the loop) was reused for the temporary j + sk + 1 of the inner test and restored on ONE side of the
// branch that follows, so lanes whose skip ended on the last pattern character stored the successor (start = m, j = 0)
// instead of (start, j): one lost match per ~25 and ghost matches at tile offset + m.  Root-caused in round 5 (ISA in
// profiles/r05_levlp_miscompile.txt; -O1, noinline or this loop shape compile correctly; extra wave syncs change
// nothing — it never was a race).  benchmarks/lab_build.sh x -DFZ_LAB_ONLY -DFZ_LEVLP_BREAKLOOP (applies benchmarks/lab_patches/) + benchmarks/repro_lp.py
// rebuilds and shows the miscompiled form.
template <class PatF>
FZ_HD void fz_levlp_step_slots(uint32_t w0, uint32_t w1, uint8_t ch, uint32_t index, bool more_seq, uint32_t m, PatF pat,
                               uint32_t k, FzGStep &o) {
    fz_gstep_clear(o);
    const uint32_t start = w0 & 0xffffu, j = w0 >> 16, l = w1 & 0xffu;
    if (pat(j) == ch) {                                                // :84-92
        if (j + 1u == m) { o.f1 = 1; o.m1 = start | ((index + 1u) << 16); o.d1 = l; }
        else { o.fa = 1; o.a0 = w0 + 0x10000u; o.a1 = w1; }
        return;
    }
    if (l == k) return;                                                // :99-100
    o.fa = 1; o.a0 = w0; o.a1 = w1 + 1u;                               // :103 skip a sequence char (l++)
    if (more_seq && j + 1u < m) { o.fb = 1; o.b0 = w0 + 0x10000u; o.b1 = w1 + 1u; }   // :105-111 skip both
    uint32_t fsk = 0;                                                  // :114-137: the first sk in 1..k-l with j + sk == m or pattern[j + sk] == ch
    for (uint32_t sk = 1; sk <= k; ++sk) {
        const bool open = (sk <= k - l) & (fsk == 0u);
        if (!FZ_WAVE_ANY(open ? 1u : 0u)) break;                       // wave-uniform: no lane is still looking
        const uint32_t pos = j + sk;
        const bool hit = (pos >= m) | (pat(pos < m ? pos : m - 1u) == ch);
        fsk = (open & hit) ? sk : fsk;
    }
    if (fsk != 0u) {
        if (j + fsk + 1u >= m) { o.f1 = 1; o.m1 = start | ((index + 1u) << 16); o.d1 = l + fsk; }   // ran off the pattern, or matched its last char
        else { o.fc = 1; o.c0 = w0 + ((1u + fsk) << 16); o.c1 = w1 + fsk; }
    }
}

// levenshtein.py:144-148
FZ_HD bool fz_levlp_final(const FzGCand &c, uint32_t m, uint32_t k, uint32_t &dist) {
    dist = c.l + m - c.j;
    return dist <= k;
}

// Which window positions need a fresh candidate at all (round 5).  The automaton of a hit runs over the window
// [idx - s - k, idx - s + m + k) (generic_search.py:229-231) and the reference spawns a candidate at EVERY window character
// (py:80).  A candidate that starts at `index` consumes at most wlen - index characters; j advances by at most one per
// consumed character plus the pattern characters it deletes (nd <= max_dels, and nd <= l <= max_l), and every way of
// emitting a match — the last pattern character consumed (py:86-88, 129-138), skipping to the pattern's end (py:141-165),
// the end-of-window flush (py:172-177) — needs j + remaining deletions >= m.  So a start with
//     index + m > wlen + min(max_dels, max_l)
// can never emit anything, and since candidates of different starts never interact (successors keep their start, the list
// only grows by appending) leaving it out changes neither the matches nor their order.  BASELINE configs[3b] (m = 64,
// k = 5, max_dels = 2): 13 of a window's 74 characters spawn.
FZ_HD bool fz_gen_start_useful(uint32_t index, uint32_t wlen, uint32_t m, uint32_t max_dels, uint32_t max_l) {
    const uint32_t d = max_dels < max_l ? max_dels : max_l;
    return index + m <= wlen + d;
}

// End-of-window flush of one surviving candidate (py:172-177): -> true and dist if it matches.
FZ_HD bool fz_generic_final(const FzGCand &c, uint32_t m, uint32_t max_dels, uint32_t max_l, uint32_t &dist) {
    const uint32_t sk = m - c.j;
    if (c.nd + sk <= max_dels && c.l + sk <= max_l) { dist = c.l + sk; return true; }
    return false;
}

// Record of the generic search: one emitted match of the automaton run on the window of hit `key`.
struct FzGenRec {
    uint64_t key;        // per-hit mode: (block << FZ_IDX_BITS) | idx of the n-gram hit; tiled modes: global step index
    uint32_t seq;        // emission number within the work item (hit window / tile)
    uint32_t se;         // window-relative start | end << 16
    uint32_t dist;
    uint32_t win;        // tiled modes: window (tile) number; per-hit mode: segment number, or (no segments) the
                         // hit's slot in the hit list
};

// Window table of the generic search (round 4).  The automaton's input is the window [idx - s - k, idx - s + m + k) of
// an n-gram hit (generic_search.py:229-231): it depends on idx - s only, and the hits that the different n-gram blocks of
// ONE occurrence produce share it (a planted copy with e edits is found by up to G - e blocks: BASELINE configs[3b] has
// 3x as many hits as distinct windows).  The reference runs its automaton once per hit and emits the same matches each
// time; here the scan enters every hit it lists into a table of windows (fz_gen_claim: the window's slot by atomicCAS, the
// hit as a member, the window's LEADER = its hit of the smallest block by atomicMax on the inverted (block, slot) word),
// and the automaton kernel runs the leaders only:
//   ordered form: fz_gen_order_kernel counts the leader's rows for every member and fz_gen_scatter_kernel writes every row
//     of the leader once per member, with the member's block number;
//   folded / flag-only form: the other hits emit nothing (a consolidation of equal matches keeps the smallest block).
// Layout at FzScanArgs.gen_dedup: u64 keys[T] (idx + k - s + 1; 0 = free), u64 best[T] (~((block << 32) | hit-list slot),
// maximum = smallest block), u32 nmem[T], u32 mem[T][FZ_GEN_DEDUP_MEMBERS], u32 wslot[FZ_GEN_ORDER_MAX] (table slot of
// every hit, or FZ_GEN_DEDUP_NONE: the hit keeps its own rows).  keys, best and nmem must be zero when a search starts.
#define FZ_GEN_DEDUP_SLOTS 32768u
#define FZ_GEN_DEDUP_MEMBERS 7u
#define FZ_GEN_DEDUP_NONE 0xffffffffu
#define FZ_GEN_DEDUP_ZERO_BYTES ((size_t)FZ_GEN_DEDUP_SLOTS * 20u)
#define FZ_GEN_DEDUP_BYTES ((size_t)FZ_GEN_DEDUP_SLOTS * (8u + 8u + 4u + 4u * FZ_GEN_DEDUP_MEMBERS) + (size_t)16384u * 4u)
#define FZ_HDR_GEN_ROWS 4                              // counters[4]: rows of the ordered generic search (hits x their window's matches)

struct FzGenDedup {
    unsigned long long *keys, *best;
    uint32_t *nmem, *mem, *wslot;
    FZ_HD explicit FzGenDedup(uint64_t base) {
        keys = reinterpret_cast<unsigned long long *>(base);
        best = keys + FZ_GEN_DEDUP_SLOTS;
        nmem = reinterpret_cast<uint32_t *>(best + FZ_GEN_DEDUP_SLOTS);
        mem = nmem + FZ_GEN_DEDUP_SLOTS;
        wslot = mem + (size_t)FZ_GEN_DEDUP_SLOTS * FZ_GEN_DEDUP_MEMBERS;
    }
    FZ_HD uint32_t leader(uint32_t slot) const { return (uint32_t)~best[slot]; }     // hit-list slot of the smallest block's hit
};

// The generic search's records are ordered on the device when one shard without segments produced at most this
// many n-gram hits (fz_gen_order_kernel is quadratic in the hit count: 6e3 hits = 10 us); the host orders the rest.
#define FZ_GEN_ORDER_MAX 16384u

// One raw match as the C-ABI returns it (fz_match of include/fzhip.h; fzhip.hip asserts the layout).
struct FzOutRow { int64_t start, end; int32_t dist, block; };

// generic_search.py:229-237: the match `se` (window-relative start | end << 16) of the automaton run on the window
// of n-gram hit `key`, in sequence coordinates.  `sa` = start of the hit's segment (0 without segments).
FZ_HD FzOutRow fz_gen_row(uint64_t key, uint32_t L, uint32_t k, uint64_t sa, uint32_t se, uint32_t dist) {
    const uint64_t idx = fz_hit_index(key);
    const uint32_t blk = fz_hit_block(key);
    const uint64_t reach = (uint64_t)blk * L + k;
    const uint64_t w0 = idx - sa > reach ? idx - reach : sa;
    FzOutRow r;
    r.start = (int64_t)(w0 + (se & 0xffffu));
    r.end = (int64_t)(w0 + (se >> 16));
    r.dist = (int32_t)dist;
    r.block = (int32_t)blk;
    return r;
}

// Plain byte accessor over a resident buffer in GLOBAL coordinates (host emulation / tests).
struct FzSeqView {
    const uint8_t *buf;
    uint64_t buf_off;
    FZ_HD uint8_t at(uint64_t gidx) const { return buf[gidx - buf_off]; }
};

// ---------------------------------------------------------------------------------------------
// Multi-pattern search (fz_lev_ngrams_multi): ONE pass over the sequence tests every byte offset against the n-gram
// blocks of a GROUP of patterns that share the n-gram length L (fz_kernels.h: fz_mp_filter_kernel / fz_mp_verify_kernel).
//
// Batched domain of a pattern (everything else takes the single-pattern route inside the same call):
//     1 <= k <= FZ_MP_MAX_K,   m <= FZ_MP_MAX_M,   L = m / (k + 1) >= FZ_MP_MIN_L
// A group holds at most FZ_MP_MAX_PATS patterns with together at most FZ_MP_MAX_BLOCKS blocks.
//
// The filter's table, built per group on the host (fz_mp_build) and copied to LDS by every workgroup:
//   sig    a signature of 2^16 bits (8 KiB): bit fz_mp_sig_bit(h) is set for the hash h of every block's n-gram.  One LDS
//          dword read per byte offset; a random dword of 2048 spreads over the 64 banks like any random lookup (the scan
//          kernel's one-slot-per-bank table cannot hold 256 n-grams).
//   slots  FZ_MP_SLOTS open-addressed {hash, first entry | count << 16} pairs (linear probing, load <= 1/2): an offset whose
//          signature bit is set looks its full 32-bit hash up here; equal hashes (equal n-grams of several patterns or
//          blocks, or a true 32-bit collision) share one slot and name a RUN of entries.
//   ent    the group's block table, sorted by hash: pattern id | block number << 8 | block start s << 16.
// h covers the first min(L, 8) bytes of the window exactly as fz_hash_windows does (x = bytes [0, 4), yh = the three bytes
// that end at byte min(L, 8)), so the filter may over-report (a hash is no comparison) and never misses: every occurrence
// of a block's n-gram has that block's hash, its signature bit is set and its slot is found.  The verify kernel confirms the
// n-gram exactly.
#define FZ_MP_MAX_PATS 64u
#define FZ_MP_MAX_BLOCKS 256u
#define FZ_MP_MAX_M 128u
#define FZ_MP_MAX_K 8u
#define FZ_MP_MIN_L 4u
#define FZ_MP_SIG_BITS 16u
#define FZ_MP_SIG_WORDS (1u << (FZ_MP_SIG_BITS - 5u))
#define FZ_MP_SLOTS 512u
#define FZ_MP_HASH_K 0x9e3779u                   // odd 24-bit multiplier of the window hash (one v_mad_u32_u24 per offset)
// descriptor in HBM, in dwords: what the filter copies, then what the verification copies
#define FZ_MP_DESC_SLOTS FZ_MP_SIG_WORDS
#define FZ_MP_DESC_ENT (FZ_MP_DESC_SLOTS + 2u * FZ_MP_SLOTS)
#define FZ_MP_DESC_M (FZ_MP_DESC_ENT + FZ_MP_MAX_BLOCKS)
#define FZ_MP_DESC_PAT (FZ_MP_DESC_M + FZ_MP_MAX_PATS)
#define FZ_MP_DESC_WORDS (FZ_MP_DESC_PAT + FZ_MP_MAX_PATS * FZ_MP_MAX_M / 4u)
#define FZ_MP_FILTER_WORDS FZ_MP_DESC_ENT        // sig + slots
#define FZ_MP_VERIFY_WORDS (FZ_MP_DESC_WORDS - FZ_MP_DESC_ENT)

FZ_HD uint32_t fz_mp_dh(uint32_t L) { return (L < 8u ? L : 8u) - 3u; }           // byte offset of the hash's second window
FZ_HD uint32_t fz_mp_hash(uint32_t x, uint32_t yh) { return fz_hash_windows(x, yh, FZ_MP_HASH_K); }
FZ_HD uint32_t fz_mp_sig_bit(uint32_t h) { return (h ^ (h >> 16)) & ((1u << FZ_MP_SIG_BITS) - 1u); }
FZ_HD uint32_t fz_mp_slot(uint32_t h) { return (h * 0x9e3779b1u) >> 23; }        // 9 bits: FZ_MP_SLOTS
FZ_HD uint32_t fz_mp_entry(uint32_t pid, uint32_t g, uint32_t s) { return pid | (g << 8) | (s << 16); }

// The hash of the window that starts at w (at least min(L, 8) readable bytes).
FZ_HD uint32_t fz_mp_hash_bytes(const uint8_t *w, uint32_t L) {
    const uint32_t dh = fz_mp_dh(L);
    const uint32_t x = (uint32_t)w[0] | ((uint32_t)w[1] << 8) | ((uint32_t)w[2] << 16) | ((uint32_t)w[3] << 24);
    const uint32_t yh = (uint32_t)w[dh] | ((uint32_t)w[dh + 1] << 8) | ((uint32_t)w[dh + 2] << 16);
    return fz_mp_hash(x, yh);
}

FZ_HD bool fz_mp_sig_test(const uint32_t *sig, uint32_t h) {
    const uint32_t t = fz_mp_sig_bit(h);
    return ((sig[t >> 5] >> (t & 31u)) & 1u) != 0;
}

// -> first entry | count << 16 of the run of entries whose hash is h; 0: none.
FZ_HD uint32_t fz_mp_lookup(const uint32_t *slots, uint32_t h) {
    uint32_t s = fz_mp_slot(h);
    for (;;) {
        const uint32_t e = slots[2u * s + 1u];
        if ((e >> 16) == 0u) return 0u;                                          // an empty slot ends the probe
        if (slots[2u * s] == h) return e;
        s = (s + 1u) & (FZ_MP_SLOTS - 1u);
    }
}

// Host: the descriptor of a group.  pat[i] / m[i] = pattern i (npat <= FZ_MP_MAX_PATS, each inside the batched domain for
// this k and L); desc = FZ_MP_DESC_WORDS dwords.  -> number of entries (blocks), 0 when they exceed FZ_MP_MAX_BLOCKS.
inline uint32_t fz_mp_build(uint32_t *desc, const uint8_t *const *pat, const uint32_t *m, uint32_t npat, uint32_t L) {
    for (uint32_t i = 0; i < FZ_MP_DESC_WORDS; ++i) desc[i] = 0u;
    uint32_t hs[FZ_MP_MAX_BLOCKS], es[FZ_MP_MAX_BLOCKS], n = 0;
    for (uint32_t i = 0; i < npat; ++i) {
        uint32_t g = 0;
        for (uint32_t s = 0; s + L <= m[i]; s += L, ++g) {
            if (n == FZ_MP_MAX_BLOCKS) return 0u;
            hs[n] = fz_mp_hash_bytes(pat[i] + s, L);
            es[n] = fz_mp_entry(i, g, s);
            ++n;
        }
        desc[FZ_MP_DESC_M + i] = m[i];
        uint8_t *dst = reinterpret_cast<uint8_t *>(desc + FZ_MP_DESC_PAT) + i * FZ_MP_MAX_M;
        for (uint32_t q = 0; q < m[i]; ++q) dst[q] = pat[i][q];
    }
    for (uint32_t i = 1; i < n; ++i) {                                           // insertion sort by hash: runs of equal hashes
        const uint32_t h = hs[i], e = es[i];
        uint32_t j = i;
        for (; j > 0 && hs[j - 1] > h; --j) { hs[j] = hs[j - 1]; es[j] = es[j - 1]; }
        hs[j] = h; es[j] = e;
    }
    uint32_t *slots = desc + FZ_MP_DESC_SLOTS;
    for (uint32_t i = 0; i < n;) {
        uint32_t j = i;
        while (j < n && hs[j] == hs[i]) ++j;
        const uint32_t t = fz_mp_sig_bit(hs[i]);
        desc[t >> 5] |= 1u << (t & 31u);
        uint32_t s = fz_mp_slot(hs[i]);
        while ((slots[2u * s + 1u] >> 16) != 0u) s = (s + 1u) & (FZ_MP_SLOTS - 1u);
        slots[2u * s] = hs[i];
        slots[2u * s + 1u] = i | ((j - i) << 16);
        i = j;
    }
    for (uint32_t i = 0; i < n; ++i) desc[FZ_MP_DESC_ENT + i] = es[i];
    return n;
}

// Arguments of the two multi-pattern kernels.
struct FzMpArgs {
    FzGeom   geom;
    uint32_t k, L;
    uint32_t win_dwords;                         // window dwords staged per lane ((longest m + 2k + 6) / 4 + 1; substitutions
                                                 // only: (longest m + 3) / 4 + 1 — no reach beyond the window)
    uint32_t nent;                               // entries of the block table
    uint64_t hit_cap;                            // capacity of EACH of the FZ_MP_LISTS hit lists
    uint64_t rec_cap;
};

// ---------------------------------------------------------------------------------------------
// Multi-pattern search, substitutions only (fz_subs_ngrams_multi; fz_kernels.h: fz_mp_verify_subs_kernel).  The per-candidate
// part works a dword at a time on two dword-readable sources:
//   t.dword(j)   dword j of the candidate's staged window; the window [i0, i0 + m) starts `sh` (0 .. 3) bytes into dword 0
//   p4[j * ps]   dword j of the candidate's pattern (the descriptor's row: dword-aligned, bytes behind m are zero)
// Each step brings two window dwords to the pattern's alignment, xors, reduces the xor to one bit per differing byte and
// keeps the bytes a mask names.

// Bytes b of the dword at pattern offset q (q % 4 == 0) with lo <= q + b < hi, as a mask of whole bytes.
FZ_HD uint32_t fz_dword_bytes_in(uint32_t q, uint32_t lo, uint32_t hi) {
    const uint32_t b0 = lo > q ? lo - q : 0u;
    const uint32_t b1 = hi > q ? (hi - q < 4u ? hi - q : 4u) : 0u;
    if (b0 >= b1) return 0u;                                                     // (b0 < b1 <= 4: b0 <= 3)
    const uint32_t upto = b1 == 4u ? 0xffffffffu : (1u << (8u * b1)) - 1u;
    return upto & ~((1u << (8u * b0)) - 1u);
}

// Bit 7 of every byte in which the window dword (hi:lo shifted right by sh bytes) differs from the pattern dword.
FZ_HD uint32_t fz_dword_diff(uint32_t lo, uint32_t hi, uint32_t sh, uint32_t pat) {
    const uint32_t d = (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * sh)) ^ pat;
    return (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;
}

// The exact n-gram test: does the window equal the pattern on [s, s + L)?  (The filter reports hashes, not comparisons.)
// Every lane walks the dwords that hold ITS block: (L + 6) / 4 + 1 steps at the most, the same number for the wave.
template <class Win>
FZ_HD bool fz_mp_block_equal(const Win &t, uint32_t sh, const uint32_t *p4, uint32_t ps, uint32_t L, uint32_t s) {
    const uint32_t q0 = s & ~3u;
    uint32_t prev = t.dword(q0 >> 2), bad = 0;
    for (uint32_t q = q0; q < s + L; q += 4u) {
        const uint32_t next = t.dword((q >> 2) + 1u);
        bad |= fz_dword_diff(prev, next, sh, p4[(q >> 2) * ps]) & fz_dword_bytes_in(q, s, s + L);
        prev = next;
    }
    return bad == 0u;
}

// fz_verify_subs for a candidate of a group (same rec.l = s, rec.r = m - s - L, rec.dist): the mismatches of the window
// against the pattern OUTSIDE the block [s, s + L), accepted when they are <= k.  The loop runs over the dwords of the
// group's longest pattern m_max (wave-uniform; a shorter pattern's bytes behind m are masked out) and is left, every other
// dword, once no lane of the wave is within its budget — as fz_verify_subs_wave does for one pattern.
template <class Win>
FZ_HD bool fz_mp_verify_subs(const Win &t, uint32_t sh, const uint32_t *p4, uint32_t ps, uint32_t m, uint32_t m_max, uint32_t k,
                             uint32_t L, uint32_t s, bool valid, FzRec &rec) {
    uint32_t prev = t.dword(0u), nd = 0;
    for (uint32_t q = 0; q < m_max; q += 4u) {
        const uint32_t next = t.dword((q >> 2) + 1u);
        const uint32_t keep = fz_dword_bytes_in(q, 0u, s) | fz_dword_bytes_in(q, s + L, m);
        nd += (uint32_t)__builtin_popcount(fz_dword_diff(prev, next, sh, p4[(q >> 2) * ps]) & keep);
        prev = next;
        if ((q & 4u) && !FZ_WAVE_BALLOT(valid && nd <= k)) break;
    }
    rec.l = s; rec.r = m - s - L; rec.dist = nd; rec.aux = 0;
    return valid && nd <= k;
}

// ---------------------------------------------------------------------------------------------
// Symbol classes on the substitutions-only multi-pattern pass (fz_subs_ngrams_multi_cls; fz_kernels.h:
// fz_mp_verify_cls_kernel).  Two 256-byte tables define them:
//   tmask[t]   the one-hot bit of text byte t among the (at most 8) base symbols, 0 when t is no base symbol
//   pmask[c]   the set of pattern byte c as a mask over those bits, 0 for a plain byte
// Pattern byte c matches text byte t iff t == c or (tmask[t] & pmask[c]) != 0: text bytes are never classes.
//
// The filter and its table layout are unchanged: a block contributes one entry per DISTINCT hash over the spellings of the
// bytes the filter hashes (fz_mp_hash_bytes: [0, 4) and [dh, dh + 3) of the first min(L, 8) bytes).  A window within k class
// mismatches has a block with none (pigeonhole, as before); that block's text is one of its spellings, so its hash is in the
// table.  Class bytes the hash does not cover — block offset 8 and beyond, byte 4 of an L >= 8 block, bytes behind the last
// block — cost no entry.  Equal hashes of two spellings of ONE block give one entry, so a text position never reports the
// same (block, index) twice.
//
// The class descriptor = the plain descriptor, then one mask byte per pattern position in rows of FZ_MP_MAX_M (bytes behind
// m are zero, like the pattern rows), then tmask.
#define FZ_MP_CLS_DESC_MASK FZ_MP_DESC_WORDS
#define FZ_MP_CLS_DESC_TMASK (FZ_MP_CLS_DESC_MASK + FZ_MP_MAX_PATS * FZ_MP_MAX_M / 4u)
#define FZ_MP_CLS_DESC_WORDS (FZ_MP_CLS_DESC_TMASK + 256u / 4u)
#define FZ_MP_CLS_VERIFY_WORDS (FZ_MP_CLS_DESC_WORDS - FZ_MP_DESC_ENT)
#define FZ_MP_CLS_MAX_BASE 8u

FZ_HD bool fz_cls_match(uint8_t c, uint8_t t, const uint8_t *pmask, const uint8_t *tmask) { return t == c || (tmask[t] & pmask[c]) != 0; }

// Is byte b of a block's first H = min(L, 8) bytes part of the window hash?
FZ_HD bool fz_mp_hashed_byte(uint32_t L, uint32_t b) { return b < 4u || b >= fz_mp_dh(L); }

// Host: the distinct hashes over the spellings of one block (w = its first byte, L >= FZ_MP_MIN_L) in ascending order.
// -> their number; cap + 1 as soon as there are more than cap (hs holds cap + 1 values).
inline uint32_t fz_mp_cls_block_hashes(const uint8_t *w, uint32_t L, const uint8_t *pmask, const uint8_t *tmask, uint32_t *hs, uint32_t cap) {
    const uint32_t H = L < 8u ? L : 8u;
    uint8_t alt[8][FZ_MP_CLS_MAX_BASE + 1u];                                     // what each byte may be spelled as
    uint32_t nalt[8], at[8];
    uint8_t cur[8];
    for (uint32_t b = 0; b < H; ++b) {
        alt[b][0] = w[b];
        nalt[b] = 1u;
        if (pmask[w[b]] && fz_mp_hashed_byte(L, b))
            for (uint32_t t = 0; t < 256u; ++t)
                if (t != w[b] && (tmask[t] & pmask[w[b]]) && nalt[b] <= FZ_MP_CLS_MAX_BASE) alt[b][nalt[b]++] = (uint8_t)t;
        at[b] = 0u;
        cur[b] = w[b];
    }
    uint32_t n = 0;
    for (;;) {
        const uint32_t h = fz_mp_hash_bytes(cur, L);
        uint32_t lo = 0;
        while (lo < n && hs[lo] < h) ++lo;
        if (lo == n || hs[lo] != h) {
            for (uint32_t j = n; j > lo; --j) hs[j] = hs[j - 1];
            hs[lo] = h;
            if (++n > cap) return n;
        }
        uint32_t b = 0;                                                          // the next spelling
        for (; b < H; ++b) {
            if (++at[b] < nalt[b]) { cur[b] = alt[b][at[b]]; break; }
            at[b] = 0u;
            cur[b] = alt[b][0];
        }
        if (b == H) return n;
    }
}

// Host: the table entries of one pattern of n-gram length L: the sum over its blocks.  -> FZ_MP_MAX_BLOCKS + 1 when more.
inline uint32_t fz_mp_cls_entries(const uint8_t *p, uint32_t m, uint32_t L, const uint8_t *pmask, const uint8_t *tmask) {
    uint32_t hs[FZ_MP_MAX_BLOCKS + 1u], total = 0;
    for (uint32_t s = 0; s + L <= m; s += L) {
        total += fz_mp_cls_block_hashes(p + s, L, pmask, tmask, hs, FZ_MP_MAX_BLOCKS - total);
        if (total > FZ_MP_MAX_BLOCKS) return FZ_MP_MAX_BLOCKS + 1u;
    }
    return total;
}

// Host: fz_mp_build for a class group.  desc = FZ_MP_CLS_DESC_WORDS dwords.  -> number of entries, 0 when they exceed
// FZ_MP_MAX_BLOCKS (then the distinct hashes, at most as many, also stay within half of FZ_MP_SLOTS).
inline uint32_t fz_mp_build_cls(uint32_t *desc, const uint8_t *const *pat, const uint32_t *m, uint32_t npat, uint32_t L, const uint8_t *pmask,
                                const uint8_t *tmask) {
    static_assert(2u * FZ_MP_MAX_BLOCKS <= FZ_MP_SLOTS, "a full block table keeps the slot table's load within 1/2");
    for (uint32_t i = 0; i < FZ_MP_CLS_DESC_WORDS; ++i) desc[i] = 0u;
    uint32_t hs[FZ_MP_MAX_BLOCKS], es[FZ_MP_MAX_BLOCKS], one[FZ_MP_MAX_BLOCKS + 1u], n = 0;
    for (uint32_t i = 0; i < npat; ++i) {
        uint32_t g = 0;
        for (uint32_t s = 0; s + L <= m[i]; s += L, ++g) {
            const uint32_t c = fz_mp_cls_block_hashes(pat[i] + s, L, pmask, tmask, one, FZ_MP_MAX_BLOCKS - n);
            if (n + c > FZ_MP_MAX_BLOCKS) return 0u;
            for (uint32_t j = 0; j < c; ++j) { hs[n] = one[j]; es[n] = fz_mp_entry(i, g, s); ++n; }
        }
        desc[FZ_MP_DESC_M + i] = m[i];
        uint8_t *dst = reinterpret_cast<uint8_t *>(desc + FZ_MP_DESC_PAT) + i * FZ_MP_MAX_M;
        uint8_t *msk = reinterpret_cast<uint8_t *>(desc + FZ_MP_CLS_DESC_MASK) + i * FZ_MP_MAX_M;
        for (uint32_t q = 0; q < m[i]; ++q) { dst[q] = pat[i][q]; msk[q] = pmask[pat[i][q]]; }
    }
    uint8_t *tm = reinterpret_cast<uint8_t *>(desc + FZ_MP_CLS_DESC_TMASK);
    for (uint32_t t = 0; t < 256u; ++t) tm[t] = tmask[t];
    for (uint32_t i = 1; i < n; ++i) {                                           // insertion sort by hash: runs of equal hashes
        const uint32_t h = hs[i], e = es[i];
        uint32_t j = i;
        for (; j > 0 && hs[j - 1] > h; --j) { hs[j] = hs[j - 1]; es[j] = es[j - 1]; }
        hs[j] = h; es[j] = e;
    }
    uint32_t *slots = desc + FZ_MP_DESC_SLOTS;
    for (uint32_t i = 0; i < n;) {
        uint32_t j = i;
        while (j < n && hs[j] == hs[i]) ++j;
        const uint32_t t = fz_mp_sig_bit(hs[i]);
        desc[t >> 5] |= 1u << (t & 31u);
        uint32_t s = fz_mp_slot(hs[i]);
        while ((slots[2u * s + 1u] >> 16) != 0u) s = (s + 1u) & (FZ_MP_SLOTS - 1u);
        slots[2u * s] = hs[i];
        slots[2u * s + 1u] = i | ((j - i) << 16);
        i = j;
    }
    for (uint32_t i = 0; i < n; ++i) desc[FZ_MP_DESC_ENT + i] = es[i];
    return n;
}

// Bit 7 of every byte of `keep` in which the window dword does not CLASS-match the pattern dword: fz_dword_diff, and a
// differing byte whose mask byte (k4: the pattern's mask dword) is non-zero is taken back when the text byte's bit is in it.
// Plain positions cost what they cost before; a class position pays one tmask lookup, and only where the bytes differ.
// Bytes outside `keep` — another sequence's, the padding's, the pattern's zeros behind m — are never looked up nor counted.
FZ_HD uint32_t fz_dword_diff_cls(uint32_t lo, uint32_t hi, uint32_t sh, uint32_t pat, uint32_t k4, uint32_t keep, const uint8_t *tmask) {
    const uint32_t w = (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * sh));
    const uint32_t x = w ^ pat;
    uint32_t d = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u & keep;
    const uint32_t cls = (((k4 & 0x7f7f7f7fu) + 0x7f7f7f7fu) | k4) & d;           // differing bytes at class positions
    if (cls) {
        for (uint32_t b = 0; b < 4u; ++b)
            if (((cls >> (8u * b + 7u)) & 1u) && (tmask[(w >> (8u * b)) & 0xffu] & (k4 >> (8u * b)) & 0xffu)) d &= ~(0x80u << (8u * b));
    }
    return d;
}

// fz_mp_block_equal with classes: does the window class-match the pattern on [s, s + L)?  k4 = the pattern's mask row, laid
// out as p4 (same stride).
template <class Win>
FZ_HD bool fz_mp_block_match_cls(const Win &t, uint32_t sh, const uint32_t *p4, const uint32_t *k4, uint32_t ps, const uint8_t *tmask, uint32_t L,
                                 uint32_t s) {
    const uint32_t q0 = s & ~3u;
    uint32_t prev = t.dword(q0 >> 2), bad = 0;
    for (uint32_t q = q0; q < s + L; q += 4u) {
        const uint32_t next = t.dword((q >> 2) + 1u);
        bad |= fz_dword_diff_cls(prev, next, sh, p4[(q >> 2) * ps], k4[(q >> 2) * ps], fz_dword_bytes_in(q, s, s + L), tmask);
        prev = next;
    }
    return bad == 0u;
}

// fz_mp_verify_subs with classes: the class mismatches outside the block, accepted when they are <= k.
template <class Win>
FZ_HD bool fz_mp_verify_cls(const Win &t, uint32_t sh, const uint32_t *p4, const uint32_t *k4, uint32_t ps, const uint8_t *tmask, uint32_t m,
                            uint32_t m_max, uint32_t k, uint32_t L, uint32_t s, bool valid, FzRec &rec) {
    uint32_t prev = t.dword(0u), nd = 0;
    for (uint32_t q = 0; q < m_max; q += 4u) {
        const uint32_t next = t.dword((q >> 2) + 1u);
        const uint32_t keep = fz_dword_bytes_in(q, 0u, s) | fz_dword_bytes_in(q, s + L, m);
        nd += (uint32_t)__builtin_popcount(fz_dword_diff_cls(prev, next, sh, p4[(q >> 2) * ps], k4[(q >> 2) * ps], keep, tmask));
        prev = next;
        if ((q & 4u) && !FZ_WAVE_BALLOT(valid && nd <= k)) break;
    }
    rec.l = s; rec.r = m - s - L; rec.dist = nd; rec.aux = 0;
    return valid && nd <= k;
}

// ---------------------------------------------------------------------------------------------
// Multi-pattern search over a batch (fz_batch_search_multi; fz_kernels.h: fz_mp_batch_verify_kernel /
// fz_mp_batch_verify_subs_kernel).  The filter streams the packed bytes as one sequence and may report n-grams that straddle
// a seam; a candidate is accepted inside ITS sequence sg = fz_segment_ragged(idx) only — the block's hit range
// (fz_block_range) against [sg.sa, sg.se) as fz_hit_in_range has it, ownership, residency — and its window is
//     Levenshtein     [max(idx - s - k, sg.sa), min(idx - s + m + k, sg.se))   clipped to the buffer,
//     substitutions   [idx - s, idx - s + m), whole, inside the sequence by the range test.
// A sequence shorter than the n-gram, the pattern or the window (or an empty one, which holds no position) needs no case of
// its own: the range test rejects its candidates.
struct FzMpRagCand { uint64_t wlo, whi; };       // the bytes the candidate's verification may read (a rejected one: none)

FZ_HD bool fz_mp_rag_accept(uint32_t mode, const FzGeom &g, const FzSeg &sg, uint32_t m, uint32_t k, uint32_t L, uint32_t s,
                            uint64_t idx, FzMpRagCand &c) {
    c.wlo = c.whi = g.buf_off;
    uint32_t lo_rel, hi_sub;
    fz_block_range(mode, m, k, L, s, lo_rel, hi_sub);
    if (!sg.ok || idx < sg.sa + lo_rel) return false;
    if (sg.se < hi_sub || idx + L > sg.se - hi_sub) return false;
    if (idx < g.own_lo || idx >= g.own_hi) return false;
    const uint64_t data_end = g.buf_off + g.buf_len;
    if (mode == FZ_MODE_SUBS) {                            // lo_rel = s, hi_sub = m - s - L: the window's two ends
        if (idx - lo_rel < g.buf_off || idx + L + hi_sub > data_end) return false;
        c.wlo = idx - s;
        c.whi = c.wlo + m;
        return true;
    }
    if (idx < g.buf_off || idx + L > data_end) return false;
    const uint64_t reach = (uint64_t)s + k;
    uint64_t wlo = idx > reach ? idx - reach : 0ull;
    if (wlo < sg.sa) wlo = sg.sa;
    if (wlo < g.buf_off) wlo = g.buf_off;
    uint64_t whi = idx + m + k - s;                        // (idx + k >= sa + s: no wrap)
    if (whi > sg.se) whi = sg.se;
    if (whi > data_end) whi = data_end;
    c.wlo = wlo;
    c.whi = whi;
    return true;
}

// ---------------------------------------------------------------------------------------------
// Best-pattern assignment per sequence (fz_batch_assign; fz_kernels.h: fz_assign_reduce_kernel / fz_assign_finish_kernel).
// Every record of a verification launch becomes two keys, and the answer for a sequence is an unsigned minimum over its
// records' keys — two atomics per record that improves its sequence, no per-pattern state:
//     lo = dist << 56 | pattern << 40 | start_local << 8 | (m + k - len)     min: (dist, lowest pattern, smallest start, longest)
//     hi = dist << 16 | (0xffff - pattern)                                   min: (dist, HIGHEST pattern)
// `tied` = the pattern of hi differs from the pattern of lo: some other list position reaches the same distance.  (m - k <=
// len <= m + k, so the last field is 0 .. 2k.)  The bit fields give the domain: k <= FZ_ASSIGN_MAX_K (the all-ones initial
// value is no key), at most FZ_ASSIGN_MAX_PATS patterns, every sequence shorter than 2^32 bytes.
#define FZ_ASSIGN_MAX_K 127u
#define FZ_ASSIGN_MAX_PATS 65535u
#define FZ_ASSIGN_NONE_LO 0xffffffffffffffffull
#define FZ_ASSIGN_NONE_HI 0xffffffffu

FZ_HD uint64_t fz_assign_key(uint32_t dist, uint32_t pattern, uint32_t start_local, uint32_t len, uint32_t m, uint32_t k) {
    return ((uint64_t)dist << 56) | ((uint64_t)pattern << 40) | ((uint64_t)start_local << 8) | (uint64_t)((m + k - len) & 0xffu);
}
FZ_HD uint32_t fz_assign_key_hi(uint32_t dist, uint32_t pattern) { return (dist << 16) | (0xffffu - pattern); }

FZ_HD uint32_t fz_assign_key_dist(uint64_t key) { return (uint32_t)(key >> 56); }
FZ_HD uint32_t fz_assign_key_pattern(uint64_t key) { return (uint32_t)(key >> 40) & 0xffffu; }
FZ_HD uint32_t fz_assign_key_start(uint64_t key) { return (uint32_t)(key >> 8); }
FZ_HD uint32_t fz_assign_key_len(uint64_t key, uint32_t m, uint32_t k) { return m + k - (uint32_t)(key & 0xffu); }
FZ_HD uint32_t fz_assign_hi_dist(uint32_t hi) { return hi >> 16; }
FZ_HD uint32_t fz_assign_hi_pattern(uint32_t hi) { return 0xffffu - (hi & 0xffffu); }

// aux of a record -> {the pattern's position in the caller's list, its length}: 64 entries for a group, one entry (aux
// ignored) for a pattern searched on its own.
struct FzAssignPat { uint32_t pattern, m; };

// One output row (= fz_assign of include/fzhip.h): pattern = -1 and the rest 0 where nothing matched.
struct FzAssignRow { int32_t pattern; uint16_t dist, tied; uint32_t start, end; };

// What one record asks of its sequence's table entries: -> false when it does not count (no match, beyond the budget,
// outside every sequence).  start = idx - l, len = l + L + r, in the coordinates of the sequence that holds idx.
FZ_HD bool fz_assign_keys(const FzRagged &t, uint64_t n, const FzRec &r, uint32_t L, const FzAssignPat *pat, uint32_t npat, uint32_t k,
                          uint32_t &seq, uint64_t &lo, uint32_t &hi) {
    if (r.dist == FZ_REC_NONE || r.dist > k) return false;
    const uint64_t idx = fz_hit_index(r.key);
    const FzSeg sg = fz_segment_ragged(t, n, idx);
    if (!sg.ok || idx < sg.sa + r.l) return false;
    const FzAssignPat p = pat[npat > 1u ? (r.aux < npat ? r.aux : 0u) : 0u];
    seq = sg.j;
    lo = fz_assign_key(r.dist, p.pattern, (uint32_t)(idx - r.l - sg.sa), r.l + L + r.r, p.m, k);
    hi = fz_assign_key_hi(r.dist, p.pattern);
    return true;
}

// A sequence's two table entries -> its output row.  pm = the lengths of the caller's patterns (the key holds m + k - len).
FZ_HD FzAssignRow fz_assign_row(uint64_t lo, uint32_t hi, const uint32_t *pm, uint32_t k) {
    FzAssignRow o;
    o.pattern = -1; o.dist = 0; o.tied = 0; o.start = 0; o.end = 0;
    if (lo == FZ_ASSIGN_NONE_LO) return o;
    const uint32_t p = fz_assign_key_pattern(lo);
    o.pattern = (int32_t)p;
    o.dist = (uint16_t)fz_assign_key_dist(lo);
    o.tied = fz_assign_hi_pattern(hi) != p ? 1u : 0u;
    o.start = fz_assign_key_start(lo);
    o.end = o.start + fz_assign_key_len(lo, pm[p], k);
    return o;
}

// ---------------------------------------------------------------------------------------------
// Records (fz_batch_upload_records; fz_kernels.h: fz_rec_*_kernel): a text of lines becomes a batch on the device.
// A line ends at a '\n' or, the last one, at the end of the text; one '\r' in front of that end is not content.  The
// line table nl[] holds the positions of the n_nl newlines in ascending order; the text has n_nl lines, plus one when its
// last byte is no newline.  Record r is the lines r * period .. r * period + period - 1 and its sequence is line
// r * period + phase.  With FZ_REC_FASTQ_CHECKS (period 4, phase 1) a record is checked, and the smallest error key
// (record << 8 | reason) of the text is the one reported:
//     1 the line count is no multiple of 4 (record = n_lines / 4)      2 line 0 does not start with '@'
//     3 line 2 does not start with '+'                                  4 line 3 is not as long as line 1
#define FZ_REC_CHECKS 1u               // = FZ_REC_FASTQ_CHECKS (include/fzhip.h)
#define FZ_REC_OK 0u
#define FZ_REC_E_COUNT 1u
#define FZ_REC_E_AT 2u
#define FZ_REC_E_PLUS 3u
#define FZ_REC_E_QUAL 4u
#define FZ_REC_NO_ERROR 0xffffffffffffffffull

// 0x80 in every byte of w that is a '\n' (exact: no borrow crosses a byte), so popcount = the newlines of the word.
FZ_HD uint32_t fz_rec_nl_mask(uint32_t w) {
    const uint32_t x = w ^ 0x0a0a0a0au;
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

FZ_HD uint64_t fz_rec_n_lines(const uint8_t *text, uint64_t n, uint64_t n_nl) { return n_nl + ((n && text[n - 1] != '\n') ? 1u : 0u); }

// rank -> line: the content [start, end) of line i (i < fz_rec_n_lines), the '\r' in front of its end left out.
struct FzRecLine { uint64_t start, end; };
FZ_HD FzRecLine fz_rec_line(const uint8_t *text, uint64_t n, const uint64_t *nl, uint64_t n_nl, uint64_t i) {
    FzRecLine l;
    l.start = i ? nl[i - 1] + 1u : 0u;
    l.end = i < n_nl ? nl[i] : n;
    if (l.end > l.start && text[l.end - 1] == '\r') --l.end;
    return l;
}

FZ_HD uint64_t fz_rec_err_key(uint64_t record, uint32_t reason) { return (record << 8) | reason; }
FZ_HD uint64_t fz_rec_err_record(uint64_t key) { return key >> 8; }
FZ_HD uint32_t fz_rec_err_reason(uint64_t key) { return (uint32_t)(key & 0xffu); }

// How many sequences a text of n_lines lines holds: the records whose sequence line exists.
FZ_HD uint64_t fz_rec_n_seqs(uint64_t n_lines, uint32_t period, uint32_t phase) {
    return n_lines > phase ? (n_lines - phase + period - 1u) / period : 0u;
}

// record -> (start, len, verdict).  A record whose check lines do not all exist is not checked (FZ_REC_E_COUNT is the
// text's, not a record's: fz_rec_count_key).
struct FzRecOut { uint64_t start, len; uint32_t reason; };
FZ_HD FzRecOut fz_rec_measure(const uint8_t *text, uint64_t n, const uint64_t *nl, uint64_t n_nl, uint64_t n_lines, uint32_t period,
                              uint32_t phase, uint32_t flags, uint64_t r) {
    FzRecOut o;
    const uint64_t l0 = r * period;
    const FzRecLine s = fz_rec_line(text, n, nl, n_nl, l0 + phase);
    o.start = s.start; o.len = s.end - s.start; o.reason = FZ_REC_OK;
    if ((flags & FZ_REC_CHECKS) && l0 + 3u < n_lines) {
        const FzRecLine h = fz_rec_line(text, n, nl, n_nl, l0);
        const FzRecLine p = fz_rec_line(text, n, nl, n_nl, l0 + 2u);
        const FzRecLine q = fz_rec_line(text, n, nl, n_nl, l0 + 3u);
        if (h.end == h.start || text[h.start] != '@') o.reason = FZ_REC_E_AT;
        else if (p.end == p.start || text[p.start] != '+') o.reason = FZ_REC_E_PLUS;
        else if (q.end - q.start != o.len) o.reason = FZ_REC_E_QUAL;
    }
    return o;
}

// The text's own error key (FZ_REC_NO_ERROR: none).
FZ_HD uint64_t fz_rec_count_key(uint64_t n_lines, uint32_t period, uint32_t flags) {
    return ((flags & FZ_REC_CHECKS) && n_lines % period) ? fz_rec_err_key(n_lines / period, FZ_REC_E_COUNT) : FZ_REC_NO_ERROR;
}

// Exclusive scan of u64 in workgroups of FZ_RSCAN_ITEMS items: reduce per workgroup, scan the sums (the same scan, a
// level up), add them back.  fz_rscan_levels: the workgroup counts of the levels above `n` items, top last; -> their number.
#define FZ_RSCAN_THREADS 256u
#define FZ_RSCAN_PER_THREAD 4u
#define FZ_RSCAN_ITEMS (FZ_RSCAN_THREADS * FZ_RSCAN_PER_THREAD)
#define FZ_RSCAN_MAX_LEVELS 8
FZ_HD int fz_rscan_levels(uint64_t n, uint64_t *blocks) {
    int l = 0;
    while (n > FZ_RSCAN_ITEMS && l < FZ_RSCAN_MAX_LEVELS) {
        n = (n + FZ_RSCAN_ITEMS - 1u) / FZ_RSCAN_ITEMS;
        blocks[l++] = n;
    }
    return l;
}

// ---------------------------------------------------------------------------------------------
// FASTA (fz_batch_upload_fasta; fz_kernels.h: fz_fa_*_kernel): the rule of `samtools faidx`.  Lines are the records path's
// (nl[], fz_rec_line; trailing empty lines dropped first).  A line whose first byte is '>' is a header and opens a record;
// every other line is a sequence line of the record the nearest header above it opened.  Per record: linebases = the
// content length of its first sequence line, linewidth = the distance from that line's first byte to the next line's
// first byte (to the end of the text when there is none), offset = the position of its first base; all three 0 for a
// record without sequence lines, whose offset is the position behind the header line.  The smallest error key
// (record << 8 | reason, fz_rec_err_key) is the one reported; the reasons follow the FASTQ ones:
//     5 the text does not start with '>' (record 0)            6 an empty sequence line
//     7 a sequence line that is not the record's last differs from linebases / linewidth, or the last is longer than linebases
// head[r] = the line of record r's header (head[n_seqs] = n_lines), rank[i] = the headers in front of line i.
#define FZ_FA_UPPER 1u                 // = FZ_FA_UPPER (include/fzhip.h)
#define FZ_FA_E_START 5u
#define FZ_FA_E_EMPTY 6u
#define FZ_FA_E_WIDTH 7u

struct FzFaRow { uint64_t header_start, header_len, length, offset, linebases, linewidth; };   // = fz_fasta_row

// Where line i ends with its terminator: the first byte of line i + 1, or the end of the text.
FZ_HD uint64_t fz_fa_line_next(uint64_t n, const uint64_t *nl, uint64_t n_nl, uint64_t i) { return i < n_nl ? nl[i] + 1u : n; }

FZ_HD uint64_t fz_fa_is_head(const uint8_t *text, const uint64_t *nl, uint64_t i) { return text[i ? nl[i - 1] + 1u : 0u] == '>' ? 1u : 0u; }

// The text's own error key (FZ_REC_NO_ERROR: none).
FZ_HD uint64_t fz_fa_text_key(const uint8_t *text, uint64_t n) {
    return (n && text[0] != '>') ? fz_rec_err_key(0, FZ_FA_E_START) : FZ_REC_NO_ERROR;
}

// record -> its row and the verdict on its last sequence line, from its first and last sequence line only.
struct FzFaOut { FzFaRow row; uint32_t reason; };
FZ_HD FzFaOut fz_fa_measure(const uint8_t *text, uint64_t n, const uint64_t *nl, uint64_t n_nl, const uint64_t *head, uint64_t r) {
    FzFaOut o;
    const uint64_t h = head[r], lines = head[r + 1] - h - 1u;
    const FzRecLine hl = fz_rec_line(text, n, nl, n_nl, h);
    o.row.header_start = hl.start + 1u;
    o.row.header_len = hl.end - hl.start - 1u;
    o.reason = FZ_REC_OK;
    if (lines == 0) {
        o.row.length = 0; o.row.offset = fz_fa_line_next(n, nl, n_nl, h); o.row.linebases = 0; o.row.linewidth = 0;
        return o;
    }
    const FzRecLine f = fz_rec_line(text, n, nl, n_nl, h + 1u);
    const FzRecLine l = fz_rec_line(text, n, nl, n_nl, h + lines);
    o.row.offset = f.start;
    o.row.linebases = f.end - f.start;
    o.row.linewidth = fz_fa_line_next(n, nl, n_nl, h + 1u) - f.start;
    o.row.length = (lines - 1u) * o.row.linebases + (l.end - l.start);
    if (l.end - l.start > o.row.linebases) o.reason = FZ_FA_E_WIDTH;
    return o;
}

// Sequence line i of a record with (linebases, linewidth); last: it is the record's last line.
FZ_HD uint32_t fz_fa_line_check(const uint8_t *text, uint64_t n, const uint64_t *nl, uint64_t n_nl, uint64_t i, bool last,
                                uint64_t linebases, uint64_t linewidth) {
    const FzRecLine l = fz_rec_line(text, n, nl, n_nl, i);
    const uint64_t len = l.end - l.start;
    if (len == 0) return FZ_FA_E_EMPTY;
    if (last) return len > linebases ? FZ_FA_E_WIDTH : FZ_REC_OK;
    return (len != linebases || fz_fa_line_next(n, nl, n_nl, i) - l.start != linewidth) ? FZ_FA_E_WIDTH : FZ_REC_OK;
}

// Base q of a record -> its position in the text (linebases > 0: the record has bases).
FZ_HD uint64_t fz_fa_src(uint64_t offset, uint64_t linebases, uint64_t linewidth, uint64_t q) {
    if ((q | linebases) >> 32) return offset + (q / linebases) * linewidth + q % linebases;
    const uint32_t q32 = (uint32_t)q, lb32 = (uint32_t)linebases;
    return offset + (uint64_t)(q32 / lb32) * linewidth + q32 % lb32;
}

// ... and its column in its line (the same quotient: one division serves both).
FZ_HD uint64_t fz_fa_col(uint64_t linebases, uint64_t q) {
    if ((q | linebases) >> 32) return q % linebases;
    return (uint32_t)q % (uint32_t)linebases;
}

// bytes.upper() of four bytes at once: bit 5 cleared in every byte of 'a' .. 'z' (no carry crosses a byte: the operands
// are 7-bit), every other byte, those above 0x7f included, as it is.
FZ_HD uint32_t fz_fa_upper4(uint32_t w) {
    const uint32_t x = w & 0x7f7f7f7fu;
    const uint32_t ge_a = x + 0x1f1f1f1fu, gt_z = x + 0x05050505u;
    return w ^ ((ge_a & ~gt_z & ~w & 0x80808080u) >> 2);
}

// ---------------------------------------------------------------------------------------------
// Derived batches (fz_batch_derive; fz_kernels.h: fz_derive_*_kernel): a batch is made from a batch where it lies.
//     out[j] = X(parent[i_j][a_j : b_j]),  i_j = index[j] (null: j),  a_j = starts[j] (null: 0),  b_j = ends[j] (null: the
//     length of parent sequence i_j),  X = byte by byte through a 256-byte table (null: identity), then reversed (REV).
// offs = the parent's scanned length table (n_src + 1 entries, the first 0; not read when n_src == 0).  An item is bad when
// i_j >= n_src (1), a_j > b_j (2) or b_j > the parent sequence's length (3); the smallest error key (j << 8 | reason,
// fz_rec_err_key) is the one reported.  A bad item has no bytes.
#define FZ_DRV_REVERSE 1u              // = FZ_DERIVE_REVERSE (include/fzhip.h)
#define FZ_DRV_E_INDEX 1u
#define FZ_DRV_E_ORDER 2u
#define FZ_DRV_E_END 3u

// item -> (src: its lowest byte in the parent's packed bytes, len, verdict)
struct FzDrvItem { uint64_t src, len; uint32_t reason; };
FZ_HD FzDrvItem fz_derive_item(const uint64_t *offs, uint64_t n_src, const uint32_t *index, const uint64_t *starts, const uint64_t *ends,
                               uint64_t j) {
    FzDrvItem o;
    o.src = 0; o.len = 0; o.reason = FZ_REC_OK;
    const uint64_t i = index ? index[j] : j;
    if (i >= n_src) { o.reason = FZ_DRV_E_INDEX; return o; }
    const uint64_t lo = offs[i], n = offs[i + 1u] - lo;
    const uint64_t a = starts ? starts[j] : 0u, b = ends ? ends[j] : n;
    if (a > b) { o.reason = FZ_DRV_E_ORDER; return o; }
    if (b > n) { o.reason = FZ_DRV_E_END; return o; }
    o.src = lo + a; o.len = b - a;
    return o;
}

// The gather's address rule.  Output bytes [o, o + cnt) of an item (src, len), o + cnt <= len, are the cnt source bytes that
// start at fz_derive_piece_lo: in ascending order, or (rev) in descending order: output byte o + q is source byte
// lo + cnt - 1 - q.  Every one of them lies in [src, src + len).  fz_derive_byte_src: the source of output byte o alone.
FZ_HD uint64_t fz_derive_piece_lo(uint64_t src, uint64_t len, uint64_t o, uint32_t cnt, bool rev) {
    return rev ? src + len - o - cnt : src + o;
}
FZ_HD uint64_t fz_derive_byte_src(uint64_t src, uint64_t len, uint64_t o, bool rev) { return rev ? src + len - 1u - o : src + o; }

// Sixteen bytes in four little-endian dwords, their order reversed: the bytes swapped inside every dword, the dwords swapped.
FZ_HD void fz_derive_rev16(uint32_t &x, uint32_t &y, uint32_t &z, uint32_t &w) {
    const uint32_t a = __builtin_bswap32(w), b = __builtin_bswap32(z), c = __builtin_bswap32(y), d = __builtin_bswap32(x);
    x = a; y = b; z = c; w = d;
}

// Four bytes through the table.
FZ_HD uint32_t fz_derive_xlat4(const uint8_t *table, uint32_t v) {
    return (uint32_t)table[v & 0xffu] | ((uint32_t)table[(v >> 8) & 0xffu] << 8) | ((uint32_t)table[(v >> 16) & 0xffu] << 16) |
           ((uint32_t)table[v >> 24] << 24);
}

// ---------------------------------------------------------------------------------------------
// Formatted text (fz_batch_format; fz_kernels.h: fz_format_*_kernel): C batches of n sequences each become one text,
//     text = join over j < n of  lit[0] + col[0][j] + lit[1] + col[1][j] + ... + col[C - 1][j] + lit[C]
// A record is 2C + 1 segments: segment 2c is literal c, segment 2c + 1 is sequence j of column c.  The descriptor holds, per
// column, its packed bytes and its scanned length table (n + 1 entries, the first 0; not read when n == 0), and the
// literals back to back with their offsets.  It is the same struct on the device (device pointers, a copy in LDS per
// workgroup) and in the host twins (host pointers).  A record is bad when the two columns named for the check differ in
// length in it (1); the smallest error key (j << 8 | reason, fz_rec_err_key) is the one reported.
#define FZ_FMT_MAX_COLS 8u             // = FZ_FORMAT_MAX_COLUMNS (include/fzhip.h)
#define FZ_FMT_MAX_LIT 255u            // = FZ_FORMAT_MAX_LITERAL
#define FZ_FMT_NO_CHECK 0xffffffffu    // = FZ_FORMAT_NO_CHECK
#define FZ_FMT_E_EQUAL 1u
#define FZ_FMT_LIT_BYTES 2304u         // (FZ_FMT_MAX_COLS + 1) * FZ_FMT_MAX_LIT, rounded up to whole dwords

struct FzFmtCol { const uint8_t *bytes; const uint64_t *offs; };
struct FzFmtDesc {
    FzFmtCol col[FZ_FMT_MAX_COLS];
    uint32_t lit_off[FZ_FMT_MAX_COLS + 2u];               // literal c = lits[lit_off[c] .. lit_off[c + 1]); lit_off[C + 1] = their total
    uint32_t n_cols, equal_a, equal_b, pad_;
    uint8_t lits[FZ_FMT_LIT_BYTES];
};

FZ_HD uint64_t fz_format_col_len(const FzFmtDesc &d, uint32_t c, uint64_t j) { return d.col[c].offs[j + 1u] - d.col[c].offs[j]; }

// record -> (its length in the text, verdict)
struct FzFmtRec { uint64_t len; uint32_t reason; };
FZ_HD FzFmtRec fz_format_record(const FzFmtDesc &d, uint64_t j) {
    FzFmtRec o;
    o.len = d.lit_off[d.n_cols + 1u];
    for (uint32_t c = 0; c < d.n_cols; ++c) o.len += fz_format_col_len(d, c, j);
    o.reason = FZ_REC_OK;
    if (d.equal_a != FZ_FMT_NO_CHECK && d.equal_b != FZ_FMT_NO_CHECK && fz_format_col_len(d, d.equal_a, j) != fz_format_col_len(d, d.equal_b, j))
        o.reason = FZ_FMT_E_EQUAL;
    return o;
}

// The gather's address rule.  A cursor names one byte of record j: segment seg (0 .. 2C), byte off of its len.
struct FzFmtCur { uint32_t seg; uint64_t off, len; };
FZ_HD uint64_t fz_format_seg_len(const FzFmtDesc &d, uint64_t j, uint32_t seg) {
    return (seg & 1u) ? fz_format_col_len(d, seg >> 1, j) : (uint64_t)(d.lit_off[(seg >> 1) + 1u] - d.lit_off[seg >> 1]);
}

// Byte o of record j (o < the record's length) -> its cursor: at most 2C + 1 segments are walked.
FZ_HD FzFmtCur fz_format_seek(const FzFmtDesc &d, uint64_t j, uint64_t o) {
    FzFmtCur g;
    g.seg = 0; g.off = o; g.len = fz_format_seg_len(d, j, 0);
    while (g.off >= g.len && g.seg < 2u * d.n_cols) {
        g.off -= g.len;
        ++g.seg;
        g.len = fz_format_seg_len(d, j, g.seg);
    }
    return g;
}

// A cursor that may stand behind its segment's last byte -> the next byte of the text: empty segments and empty records
// are passed (the caller knows that a byte follows: its position lies in front of the text's end).
FZ_HD void fz_format_settle(const FzFmtDesc &d, uint64_t &j, FzFmtCur &g) {
    while (g.off >= g.len) {
        g.off = 0;
        if (g.seg == 2u * d.n_cols) { g.seg = 0; ++j; } else ++g.seg;
        g.len = fz_format_seg_len(d, j, g.seg);
    }
}

// Whether the cnt bytes from the cursor on are one run of column bytes, and where that run starts in the column's packed
// bytes: every one of them lies inside sequence j of the column.
FZ_HD bool fz_format_run(const FzFmtCur &g, uint32_t cnt) { return (g.seg & 1u) && g.off + cnt <= g.len; }
FZ_HD uint64_t fz_format_run_lo(const FzFmtDesc &d, uint64_t j, const FzFmtCur &g) { return d.col[g.seg >> 1].offs[j] + g.off; }

// The source of the one byte under the cursor: in a column's packed bytes, or in the descriptor's literals.
FZ_HD const uint8_t *fz_format_byte_src(const FzFmtDesc &d, uint64_t j, const FzFmtCur &g) {
    return (g.seg & 1u) ? d.col[g.seg >> 1].bytes + fz_format_run_lo(d, j, g) : d.lits + d.lit_off[g.seg >> 1] + g.off;
}

// ---------------------------------------------------------------------------------------------
// End overlaps (fz_batch_end_overlaps; fz_kernels.h: fz_overlap_kernel): a PREFIX of a pattern at the END of a read, the
// adapter that a read runs into and breaks off in.  Per read r (n bytes), pattern p (m bytes), budget k and smallest
// overlap o, over the strictly partial prefix lengths o <= i <= m - 1 with the scaled budget k_i = k * i / m:
//   Levenshtein     E(i) = min over a of ed(p[:i], r[a:]),  j(i) = the longest suffix of r at that distance
//   substitutions   E(i) = Hamming(p[:i], r[n - i:]) for i <= n,  j(i) = i
// i qualifies when E(i) <= k_i; the pattern answers with the i of the most matched characters i - E(i), then the smaller
// E(i); the read answers with the pattern of the largest i - d, then the smaller d, then the lower list position.  That order
// is the order of ONE unsigned key, so a read's answer is a maximum (0: none):
//   key = (i - d) << 40 | (255 - d) << 32 | (65535 - pattern) << 16 | j
#define FZ_OVL_MAX_M 64u               // one 64-bit column vector
#define FZ_OVL_MAX_K 16u
#define FZ_OVL_MAX_PATS 65534u         // 0xffff in a row's pattern field = none
#define FZ_OVL_ROW_BYTES 64u           // a pattern's row in the call's table: its bytes, zeros behind them
#define FZ_OVL_CHUNK_LEV 8u            // patterns per launch: two Peq tables of 2 KiB each per pattern in LDS
#define FZ_OVL_CHUNK_SUBS 64u          // ... the rows alone

struct FzOverlapRow { uint32_t start; uint16_t pattern; uint8_t overlap, dist; };   // = fz_overlap

FZ_HD uint32_t fz_overlap_chunk(uint32_t mode) { return mode == FZ_MODE_LEV ? FZ_OVL_CHUNK_LEV : FZ_OVL_CHUNK_SUBS; }
// The bytes at a read's end that a pattern can reach: its longest partial prefix and what that prefix may insert.
FZ_HD uint32_t fz_overlap_tail(uint32_t mode, uint32_t m, uint32_t k) {
    return m ? (m - 1u) + (mode == FZ_MODE_LEV ? k * (m - 1u) / m : 0u) : 0u;
}
// Dwords of a staged tail of up to tmax bytes: up to 3 bytes in front of it, and one dword behind the last for the
// two-dword steps of the substitutions form.
FZ_HD uint32_t fz_overlap_win_dwords(uint32_t tmax) { return (tmax + 6u) / 4u + 1u; }

FZ_HD uint64_t fz_overlap_key(uint32_t score, uint32_t d, uint32_t pattern, uint32_t j) {
    return ((uint64_t)score << 40) | ((uint64_t)(255u - d) << 32) | ((uint64_t)(65535u - pattern) << 16) | j;
}
// (n = the read's length)
FZ_HD FzOverlapRow fz_overlap_row(uint64_t key, uint32_t n) {
    FzOverlapRow r;
    r.start = n; r.pattern = 0xffffu; r.overlap = 0; r.dist = 0;
    if (key) {
        const uint32_t d = 255u - ((uint32_t)(key >> 32) & 0xffu);
        r.start = n - ((uint32_t)key & 0xffffu);
        r.pattern = (uint16_t)(65535u - ((uint32_t)(key >> 16) & 0xffffu));
        r.overlap = (uint8_t)((uint32_t)(key >> 40) + d);
        r.dist = (uint8_t)d;
    }
    return r;
}

// Word c of a pattern's Peq table in the top-aligned layout of fz_bits_column: position q at bit q + 64 - m of the forward
// table (side 0), at bit 63 - q of the reversed one (side 1).
FZ_HD uint64_t fz_overlap_peq_word(const uint8_t *p, uint32_t m, uint32_t c, uint32_t side) {
    uint64_t w = 0;
    for (uint32_t q = 0; q < m; ++q)
        if (p[q] == c) w |= 1ull << (side ? 63u - q : q + 64u - m);
    return w;
}

// fz_bits_column in the SEARCH form, D[0][j] = 0: the occurrence may start at any column.  The piece is the rows under `hm`
// (any run of bits of the top-aligned layout; eq is masked to it).  Nothing enters its first row: the horizontal vectors are
// masked to the piece before the shift and 0 is shifted in.  Rows above the piece are further rows that never match, rows
// below it keep hp = hn = 0 and add nothing to the sum's carry; neither feeds into the piece.
FZ_HD void fz_bits_column_search(FzBitsCol<1> &c, uint64_t eq, uint64_t hm) {
    const uint64_t d0 = (((eq & c.vp) + c.vp) ^ c.vp) | eq | c.vn;
    const uint64_t hp = (fz_or_not<uint64_t>(c.vn, d0 | c.vp) & hm) << 1;
    const uint64_t hn = ((c.vp & d0) & hm) << 1;
    c.vp = fz_or_not<uint64_t>(hn, d0 | hp);
    c.vn = hp & d0;
}

// Where a read's tail lies once it is staged a dword at a time: the last ts = min(n, tmax) bytes of [sa, se) start `sh`
// bytes into dword 0 of the window, which is dword wbase / 4 of the buffer; nd dwords hold them.  Every dword loaded starts
// in front of buf_len, so a load ends inside the padding behind the data at the latest.  The up to 3 bytes in front of the
// tail and behind the read's end belong to a neighbour or to the padding: the accessors below never hand them out.
struct FzOvlStage { uint64_t wbase; uint32_t sh, ts, nd; };
// ... of any run of bytes [wlo, whi) of the buffer (fz_cuts_piece stages a read piece by piece through it)
FZ_HD FzOvlStage fz_stage_range(uint64_t wlo, uint64_t whi, uint64_t buf_len) {
    FzOvlStage s;
    s.ts = (uint32_t)(whi - wlo);
    s.wbase = wlo & ~(uint64_t)3;
    s.sh = (uint32_t)(wlo - s.wbase);
    s.nd = s.ts ? (uint32_t)((whi - s.wbase + 3u) >> 2) : 0u;
    const uint64_t resident = buf_len > s.wbase ? (buf_len - s.wbase + 3u) >> 2 : 0u;
    if (s.nd > resident) s.nd = (uint32_t)resident;
    return s;
}
FZ_HD FzOvlStage fz_overlap_stage(uint64_t sa, uint64_t se, uint32_t tmax, uint64_t buf_len) {
    const uint64_t n = se - sa;
    return fz_stage_range(se - (n < tmax ? n : tmax), se, buf_len);
}
FZ_HD uint32_t fz_overlap_load_dword(const uint8_t *buf, uint64_t off) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t *>(buf + off);
#else
    uint32_t v;
    __builtin_memcpy(&v, buf + off, 4);
    return v;
#endif
}
// The window of one lane: dword d at win[d * stride] (the lane-transposed layout of the verification kernels: stride 64).
// FILL: the dwords of the window behind the staged ones are zeroed; without it only the nd staged dwords are written, and a
// lane with nothing to stage (nd = 0) touches neither the buffer nor the window.
template <bool FILL>
FZ_HD void fz_stage_copy(const uint8_t *buf, const FzOvlStage &s, uint32_t win_dwords, uint32_t *win, uint32_t stride) {
    const uint32_t nw = FILL || win_dwords < s.nd ? win_dwords : s.nd;
    for (uint32_t d0 = 0; d0 < nw; d0 += 4u) {             // (four loads in flight, then their stores)
        uint32_t x[4];
        for (uint32_t j = 0; j < 4u; ++j) x[j] = d0 + j < s.nd ? fz_overlap_load_dword(buf, s.wbase + 4u * (d0 + j)) : 0u;
        for (uint32_t j = 0; j < 4u; ++j)
            if (d0 + j < nw) win[(d0 + j) * stride] = x[j];
    }
}
FZ_HD void fz_overlap_stage_copy(const uint8_t *buf, const FzOvlStage &s, uint32_t win_dwords, uint32_t *win, uint32_t stride) {
    fz_stage_copy<true>(buf, s, win_dwords, win, stride);
}
struct FzOvlWindow {
    const uint32_t *win;
    uint32_t stride;
    uint32_t off;                                          // window byte offset of tail byte 0
    FZ_HD uint32_t dword(uint32_t j) const { return win[j * stride]; }
    FZ_HD uint32_t at(uint32_t t) const { return (win[((off + t) >> 2) * stride] >> (8u * ((off + t) & 3u))) & 0xffu; }
};

// The call's tables for the patterns of one launch (LDS on the device): lengths, rows, and (Levenshtein) the Peq tables,
// word c of side s of pattern i at peq[(2 i + s) * 256 + c].
struct FzOvlTabs { const uint32_t *pm; const uint32_t *rows; const uint64_t *peq; };
FZ_HD void fz_overlap_budget_step(uint32_t &acc, uint32_t &ki, uint32_t k, uint32_t m) {   // ki = k * i / m, from i - 1 to i (k < m)
    acc += k;
    if (acc >= m) { acc -= m; ++ki; }
}

// One pattern against one read's tail, Levenshtein: T = min(n, fz_overlap_tail) bytes behind w.  A forward search-form pass
// over rows p[:m-1] leaves D[i] = E(i) (exact wherever E(i) <= k_i: a longer suffix costs more than k_i) in the running sum
// of the vertical deltas; the best (i, d) then takes fz_expand_bits over the reversed tail with the reversed table, whose top
// i bits are p[:i] reversed: its last arg-min is j(i).  No lane of the wave qualifies: the second pass is skipped.
FZ_HD uint64_t fz_overlap_lev(const uint64_t *fwd, const uint64_t *rev, const FzOvlWindow &w, uint32_t T, uint32_t m, uint32_t k,
                              uint32_t o, uint32_t pattern) {
    const uint32_t rows = m - 1u;
    if (!rows || o > rows) return 0ull;                    // (wave-uniform; rows = 0 would shift by 64 below)
    const uint64_t hm = (~0ull << (64u - m)) & ~(1ull << 63);
    FzBitsCol<1> c;
    c.vp = hm; c.vn = 0;                                   // column 0: the empty suffix, D[i] = i
    for (uint32_t t = 0; t < T; ++t) fz_bits_column_search(c, fwd[w.at(t)] & hm, hm);
    uint32_t D = 0, acc = 0, ki = 0, best = 0;
    for (uint32_t i = 1; i <= rows; ++i) {
        const uint32_t bit = 63u - m + i;
        D += (uint32_t)(c.vp >> bit) & 1u;
        D -= (uint32_t)(c.vn >> bit) & 1u;
        fz_overlap_budget_step(acc, ki, k, m);
        const uint32_t key = ((i - D) << 8) | (255u - D);  // (wraps where D > i: impossible, D <= i)
        if (i >= o && D <= ki && key > best) best = key;
    }
    if (!FZ_WAVE_BALLOT(best != 0u)) return 0ull;
    if (!best) return 0ull;
    const uint32_t d = 255u - (best & 0xffu), i = (best >> 8) + d;
    const uint32_t winlen = T < i + d ? T : i + d;          // (j(i) <= i + d)
    uint32_t dist = 0, consumed = 0;
    const bool ok = fz_expand_bits<1>([&](uint32_t ch) { return rev[ch]; }, i, [&](uint32_t j) { return w.at(T - 1u - j); }, winlen, d,
                                      dist, consumed);
    return ok && dist == d ? fz_overlap_key(i - d, d, pattern, consumed) : 0ull;
}

// ... substitutions only: per i the window r[n - i:] against the row's dwords, two window dwords brought to the row's
// alignment per step (fz_dword_diff), the bytes of p[:i] kept (fz_dword_bytes_in), left once over k_i.  `end` = window byte
// offset of the read's end; every byte compared lies in [end - i, end) with i <= n: inside the read.
FZ_HD uint64_t fz_overlap_subs(const uint32_t *p4, const FzOvlWindow &w, uint32_t end, uint32_t n, uint32_t m, uint32_t k, uint32_t o,
                               uint32_t pattern) {
    const uint32_t imax = n < m - 1u ? n : m - 1u;
    uint32_t acc = 0, ki = 0, best = 0;
    for (uint32_t i = 1; i <= imax; ++i) {
        fz_overlap_budget_step(acc, ki, k, m);
        if (i < o) continue;
        const uint32_t ws = end - i, d0 = ws >> 2, sh = ws & 3u;
        uint32_t prev = w.dword(d0), nd = 0;
        for (uint32_t q = 0; q < i && nd <= ki; q += 4u) {
            const uint32_t next = w.dword(d0 + (q >> 2) + 1u);
            nd += (uint32_t)__builtin_popcount(fz_dword_diff(prev, next, sh, p4[q >> 2]) & fz_dword_bytes_in(q, 0u, i));
            prev = next;
        }
        const uint32_t key = ((i - nd) << 8) | (255u - nd);
        if (nd <= ki && key > best) best = key;
    }
    if (!best) return 0ull;
    const uint32_t d = 255u - (best & 0xffu), i = (best >> 8) + d;
    return fz_overlap_key(i - d, d, pattern, i);
}

// One read against the npat patterns p0 .. of a launch: the lane's part of fz_overlap_kernel behind the staging.  The loop
// over the patterns is wave-uniform; the best key stays in registers.
template <uint32_t MODE>
FZ_HD uint64_t fz_overlap_lane(const FzOvlTabs &tb, const uint32_t *win, uint32_t stride, const FzOvlStage &s, uint32_t n, uint32_t p0,
                               uint32_t npat, uint32_t k, uint32_t o) {
    uint64_t best = 0;
    for (uint32_t pi = 0; pi < npat; ++pi) {
        const uint32_t m = tb.pm[pi];
        uint32_t T = fz_overlap_tail(MODE, m, k);
        if (T > s.ts) T = s.ts;                            // = min(n, the pattern's tail): ts = min(n, the launch's longest)
        uint64_t key;
        if (MODE == FZ_MODE_LEV) {
            const FzOvlWindow w{win, stride, s.sh + (s.ts - T)};
            key = fz_overlap_lev(tb.peq + (2u * pi) * 256u, tb.peq + (2u * pi + 1u) * 256u, w, T, m, k, o, p0 + pi);
        } else {
            const FzOvlWindow w{win, stride, s.sh};
            key = fz_overlap_subs(tb.rows + pi * (FZ_OVL_ROW_BYTES / 4u), w, s.sh + s.ts, n, m, k, o, p0 + pi);
        }
        if (key > best) best = key;
    }
    return best;
}

// ---------------------------------------------------------------------------------------------
// Score cuts (fz_batch_score_cuts; fz_kernels.h: fz_cuts_kernel): where the running sum of a table of scores, taken from a
// read's end, peaks.  Per read r of n bytes, a table w of 256 signed scores, a flag `stop` and an optional miss rate
// num / den (a miss: a byte with w < 0):
//   cut3(r):  s = best = miss = 0; cut = n
//             for i = n - 1 down to 0:  s += w[r[i]]; miss += w[r[i]] < 0
//                                       if stop and s < 0: break
//                                       if s > best and (no rate or miss * den <= num * (n - i)): best = s; cut = i
//   cut5(r) = n - cut3(reversed r)
// (strict: of equal peaks the one nearest the end wins).  Quality trimming at cutoff q is w[b] = q - (b - base) with stop,
// poly-A trimming w['A'] = 1, -2 elsewhere, no stop, rate 1 / 5.  A lane keeps the number of bytes it has walked from its
// end (3') or its start (5') and `trim` = that number at the peak, so one text serves both sides: cut3 = n - trim, cut5 =
// trim.  The sums are 32-bit: the call refuses batches with max_seq_len * max|w| >= 2^31.
#ifndef FZ_CUT_STOP3                   // (include/fzhip.h states the same three)
#define FZ_CUT_STOP3 1u                // fz_batch_score_cuts' flags: the 3' side stops at the first negative sum
#define FZ_CUT_STOP5 2u                // ... the 5' side
#define FZ_CUT_RATE 4u                 // the miss rate is in force on the sides that do not stop
#endif
#define FZ_CUT_PIECE_DWORDS 16u        // a read is walked in pieces of 16 dwords of the buffer: 4 KiB of window per wave

struct FzCutRow { uint32_t start, end; };                  // = fz_cut
// One side's rule.  wmax = the table's largest score; bounded: a lane also ends where no later sum can pass its peak.
struct FzCutRule { int32_t wmax; uint32_t stop, rate, num, den, bounded; };
struct FzCutState { int32_t s, best; uint32_t trim, miss, walked, live; };

FZ_HD FzCutRule fz_cuts_rule(uint32_t side, uint32_t flags, uint32_t num, uint32_t den, int32_t wmax, uint32_t bounded) {
    FzCutRule r;
    r.wmax = wmax;
    r.stop = (flags >> side) & 1u;
    r.rate = (flags & FZ_CUT_RATE) && !r.stop ? 1u : 0u;
    r.num = num; r.den = den; r.bounded = bounded;
    return r;
}
// A lane is finished when its read is used up, when `stop` fired (fz_cuts_step), or when s + remaining * wmax <= best: every
// later sum is at most that, and only a sum ABOVE best moves the cut, so the test is exact.  (remaining * wmax < 2^31 by the
// call's refusal, and |s| <= walked * max|w|: the 32-bit sum cannot wrap.)
FZ_HD void fz_cuts_check(FzCutState &c, uint32_t n, const FzCutRule &r) {
    const bool done = c.walked >= n || (r.bounded && c.s + (int32_t)(n - c.walked) * r.wmax <= c.best);
    c.live = done ? 0u : c.live;
}
FZ_HD FzCutState fz_cuts_begin(uint32_t n, const FzCutRule &r) {
    FzCutState c;
    c.s = c.best = 0; c.trim = c.miss = c.walked = 0u; c.live = 1u;
    fz_cuts_check(c, n, r);
    return c;
}
// One byte's score into a lane that is live and `on` (the byte is the piece's own); every field moves by a select, so the
// state stays in registers whatever is inlined around it.
FZ_HD void fz_cuts_step(FzCutState &c, int32_t wv, const FzCutRule &r, bool on) {
    const bool go = on && c.live;
    c.s += go ? wv : 0;
    c.miss += go && wv < 0 ? 1u : 0u;
    c.walked += go ? 1u : 0u;
    const bool dead = go && r.stop && c.s < 0;
    bool within = true;
    if (r.rate) within = (uint64_t)c.miss * r.den <= (uint64_t)r.num * c.walked;   // (uniform)
    const bool take = go && !dead && c.s > c.best && within;
    c.best = take ? c.s : c.best;
    c.trim = take ? c.walked : c.trim;
    c.live = dead ? 0u : c.live;
}
// The next piece of the read [sa, se) for a lane that has walked c.walked bytes from its end (dir 0) or its start (dir 1):
// the bytes up to the next multiple of FZ_CUT_PIECE_DWORDS dwords of the BUFFER, so that every piece but the first fills its
// window whole and none needs more than FZ_CUT_PIECE_DWORDS dwords at any alignment.  A finished lane: the empty piece, nd = 0.
FZ_HD FzOvlStage fz_cuts_piece(const FzCutState &c, uint64_t sa, uint64_t se, uint32_t dir, uint64_t buf_len) {
    const uint64_t span = 4u * FZ_CUT_PIECE_DWORDS;
    uint64_t lo = sa, hi = sa;
    if (c.live && dir) {
        lo = sa + c.walked;
        hi = (lo & ~(uint64_t)3) + span;
        if (hi > se) hi = se;
    } else if (c.live) {
        hi = se - c.walked;
        const uint64_t top = ((hi - 1u) & ~(uint64_t)3) + 4u;   // (live: walked < n, so hi > sa >= 0)
        lo = top > span ? top - span : 0u;
        if (lo < sa) lo = sa;
    }
    return fz_stage_range(lo, hi, buf_len);
}
// One staged piece through one lane: its bytes in the order of the walk, a dword of the window at a time.  Only window bytes
// [sh, sh + ts) are scored: what else the dwords hold is a neighbour's, the padding's, or this read's outside the piece.
FZ_HD void fz_cuts_lane(FzCutState &c, const int16_t *w, const uint32_t *win, uint32_t stride, const FzOvlStage &st, uint32_t n,
                        uint32_t dir, const FzCutRule &r) {
    const uint32_t lo = st.sh, hi = st.sh + st.ts;
    for (uint32_t u = 0; u < st.nd && c.live; ++u) {
        const uint32_t d = dir ? u : st.nd - 1u - u;
        const uint32_t x = win[d * stride];
        for (uint32_t v = 0; v < 4u; ++v) {
            const uint32_t b = dir ? v : 3u - v, o = 4u * d + b;
            fz_cuts_step(c, (int32_t)w[(x >> (8u * b)) & 0xffu], r, o >= lo && o < hi);
        }
        fz_cuts_check(c, n, r);
    }
}
// sides: bit 0 the 3' side was asked for, bit 1 the 5' side.  Both asked for and nothing left between them: the empty read.
FZ_HD FzCutRow fz_cuts_row(uint32_t n, uint32_t trim3, uint32_t trim5, uint32_t sides) {
    FzCutRow row;
    row.start = (sides & 2u) ? trim5 : 0u;
    row.end = (sides & 1u) ? n - trim3 : n;
    if (sides == 3u && row.start >= row.end) row.start = row.end = 0u;
    return row;
}
