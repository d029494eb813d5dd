/* fzhip.h — C-ABI of libfzhip.so, the MI355X (gfx950) fuzzy substring search engine.
 *
 * This is the drop-in boundary for the hot path of taleinat/fuzzysearch 0.8.1.
 * The reference's native hooks are per-candidate CPython functions (GIL held, `y*` buffers):
 *
 *   search_exact_byteslike(sub, seq, start, end) -> list[int]        src/fuzzysearch/_common.c:5-112
 *   count_differences_with_maximum_byteslike(a, b, max) -> int       src/fuzzysearch/_common.c:115-173
 *   substitutions_only_find_near_matches_ngrams_byteslike(sub, seq, k) -> list[int]
 *                                   src/fuzzysearch/_substitutions_only_ngrams_template.h:10-138
 *   c_expand_short / c_expand_long(sub, seq, k) -> (dist, n) | (None, None)
 *                                   src/fuzzysearch/_levenshtein_ngrams.pyx:9-75, :78-154
 *   c_find_near_matches_generic_linear_programming(sub, seq, params) -> list[Match]
 *                                   src/fuzzysearch/_generic_search.pyx:25-233
 *
 * That granularity (one call per n-gram hit) cannot feed a GPU, so the replacement boundary sits
 * one level up, at the whole-search functions that *drive* those hooks:
 *
 *   fz_search_exact    <->  search_exact()                          search_exact.py:59-77
 *   fz_lev_ngrams      <->  find_near_matches_levenshtein_ngrams()  levenshtein_ngram.py:159-198
 *   fz_subs_ngrams     <->  substitutions_only_find_near_matches_ngrams_byteslike + the Match
 *                           construction of substitutions_only.py:258-278
 *   fz_generic_ngrams  <->  find_near_matches_generic_ngrams()      generic_search.py:198-237
 *   fz_consolidate     <->  consolidate_overlapping_matches()       common.py:185-189
 *   fz_group_best      <->  [get_best_match_in_group(g) for g in group_matches(ms)]
 *                                                                   substitutions_only.py:279-282
 *
 * Conventions: plain pointers and sizes only (no torch / Python types).  Every function returns
 * FZ_OK (0) or a negative FZ_E* code; fz_last_error() gives the text for the calling thread.
 * Inputs are borrowed for the duration of the call.  Outputs (`fz_match**`, `uint64_t**`) are
 * allocated by the library and released with fz_free().  A fz_ctx is not internally locked: use one
 * per host thread.  All device work happens on the ctx's own HIP streams; calls return after the
 * results are on the host.
 *
 * Error behaviour mirrors the reference: empty subsequence / n-gram length 0 -> FZ_EINVAL (the
 * reference raises ValueError: levenshtein_ngram.py:164-165, _common.c:50-53).
 */
#ifndef FZHIP_H
#define FZHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FZ_ABI_VERSION 1

#define FZ_OK          0
#define FZ_EINVAL     -1   /* invalid argument (maps to ValueError in the Python layer)     */
#define FZ_ENOMEM     -2   /* host or device allocation failed (MemoryError)               */
#define FZ_EDEVICE    -3   /* HIP runtime error / no usable gfx950 device (RuntimeError)   */
#define FZ_EUNSUPPORTED -4 /* parameters outside what the kernels support (m, k limits)    */
#define FZ_EHALO      -5   /* shard halo too small for this pattern (m + k bytes needed)   */
#define FZ_ETIMEOUT   -6   /* a collective did not complete within FZ_COMM_TIMEOUT_MS (a rank never arrived): the
                            * communicator is unusable from then on; searches without the collective still work  */

typedef struct fz_ctx fz_ctx;
typedef struct fz_seq fz_seq;

/* Raw-stream record.  `block` = n-gram block index g = ngram_start / ngram_len (the outer loop
 * variable of levenshtein_ngram.py:171); -1 where it does not apply.  Field order start, end,
 * dist matches fuzzysearch.Match (common.py:15-20). */
typedef struct {
    int64_t start, end;
    int32_t dist;
    int32_t block;
} fz_match;

typedef struct {
    uint64_t bytes_scanned;    /* sequence bytes streamed by the filter kernel(s), last call  */
    uint64_t ngram_hits;       /* exact n-gram hits handed to verification, last call        */
    uint64_t raw_matches;      /* raw-stream records produced, last call                     */
    double   filter_ms;        /* hipEvent span of the filter kernel(s), last call           */
    double   verify_ms;        /* hipEvent span of the verify kernel(s), last call           */
    double   device_ms;        /* hipEvent span first launch -> results on host, last call   */
    uint32_t filter_launches;  /* number of filter kernel launches in the last call          */
    uint32_t n_devices;
    uint32_t verify_form;      /* how the last call's n-gram hits were verified (FZ_FORM_*)   */
    uint32_t reserved_;
} fz_stats_t;

/* fz_stats_t.verify_form: chosen from the search's arguments alone (pattern, budget, sequence kind) */
#define FZ_FORM_NONE        0u   /* no verification (exact search, automaton searches)                          */
#define FZ_FORM_FUSED_BAND  1u   /* inside the scan: register band / Hamming count, one candidate per lane     */
#define FZ_FORM_FUSED_CELLS 2u   /* inside the scan: lane-per-DP-cell, 16 or 32 lanes per candidate            */
#define FZ_FORM_FUSED_BITS1 3u   /* inside the scan: bit-vector columns on one 64-bit word, candidate per lane */
#define FZ_FORM_FUSED_BITS2 4u   /* ... on two 64-bit words (patterns of 65 .. 128 characters)                 */
#define FZ_FORM_KERNEL      5u   /* a verification kernel of its own behind a hit list                         */
#define FZ_FORM_FUSED_BITS32 6u  /* inside the scan: bit-vector columns on one 32-bit word (patterns <= 32)     */

int         fz_abi_version(void);
const char *fz_last_error(void);
int         fz_device_count(int *n);

/* device_ids == NULL / n_devices == 0 -> device 0 only.  Requires gfx950.
 * fz_destroy also frees the sequences of the ctx that were not released (their handles die with it). */
int  fz_create(const int *device_ids, int n_devices, fz_ctx **out);
void fz_destroy(fz_ctx *ctx);

/* Make a sequence resident in HBM.  With several devices in the ctx it is split into contiguous
 * shards, each with a halo, and every later search runs on all devices concurrently
 * (SURVEY.md §8(e)). */
int  fz_seq_upload(fz_ctx *ctx, const uint8_t *host, uint64_t n, fz_seq **out);

/* One-process-per-GPU form (torchrun / RCCL jobs): this process holds bytes
 * [buf_global_off, buf_global_off + buf_len) of a global sequence of global_n bytes and OWNS the
 * n-gram hits whose index lies in [own_lo, own_hi).  The buffer must extend (m + k) bytes past
 * the owned range on both sides (clamped to the global sequence) for every later query, else the
 * query returns FZ_EHALO.  Results are in GLOBAL coordinates. */
int  fz_seq_upload_shard(fz_ctx *ctx, const uint8_t *host_buf, uint64_t buf_len,
                         uint64_t buf_global_off, uint64_t own_lo, uint64_t own_hi,
                         uint64_t global_n, fz_seq **out);
/* Several-devices-in-one-process form of the same thing, without a host copy of the whole sequence (32 GiB over
 * 8 GPUs is built shard by shard): fz_seq_new creates an empty sequence of global_n bytes, fz_seq_add_shard uploads
 * one shard — same meaning of the ranges as fz_seq_upload_shard — to device number dev_index OF THE CTX (one shard
 * per device; host_buf is borrowed for the call).  Every later search runs on all shards concurrently and the host
 * merges their streams (__init__.py:129-171 is the reference's only analogue: chunks with overlap). */
int  fz_seq_new(fz_ctx *ctx, uint64_t global_n, fz_seq **out);
int  fz_seq_add_shard(fz_seq *seq, int dev_index, const uint8_t *host_buf, uint64_t buf_len, uint64_t buf_global_off,
                      uint64_t own_lo, uint64_t own_hi);
uint64_t fz_seq_len(const fz_seq *seq);       /* global length */
void fz_seq_release(fz_seq *seq);

/* All (overlapping) occurrences of p in seq[lo:hi], ascending.  lo/hi are clamped like
 * search_exact.py:70-71; pass hi = UINT64_MAX for "to the end". */
int fz_search_exact(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m,
                    uint64_t lo, uint64_t hi, uint64_t **idx, uint64_t *n);

/* Raw, un-consolidated match stream of find_near_matches_levenshtein_ngrams, in the reference's
 * emission order (block ascending, then hit index ascending).  Requires m / (k+1) >= 1. */
int fz_lev_ngrams(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k,
                  fz_match **out, uint64_t *n);

/* The same search split in two so that the host (and other streams: a collective, a copy) can work
 * while the scan runs: _begin launches it and returns, _end waits and delivers exactly what
 * fz_lev_ngrams would.  Up to TWO searches may be in flight per ctx (a two-deep pipeline: the scan
 * of search i + 1 runs while the host orders and consumes the records of search i; every device has
 * two pinned result slots); _end always delivers the OLDEST one.  `p` is copied, `seq` must stay
 * alive; every other search call on the ctx fails with FZ_EINVAL until every _begin has had its _end. */
int fz_lev_ngrams_begin(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k);
int fz_lev_ngrams_end(fz_ctx *ctx, fz_match **out, uint64_t *n);       /* = fz_search_end */
/* The same two-deep pipeline for the other n-gram searches; fz_search_end delivers the OLDEST search in flight, whatever
 * its kind, exactly as the synchronous call would (fz_subs_ngrams / fz_generic_ngrams, or — consolidated != 0 —
 * fz_generic_ngrams_consolidated).  Substitutions-only searches share the Levenshtein searches' result slots and may
 * be mixed with them.  A generic search keeps its hit list and records on the device until it is collected, so two of
 * them run on two LANES (a second set of per-device buffers and a second stream, created on first use): the scan of
 * the younger search runs next to the automaton kernel of the older one.  Generic searches cannot be in flight
 * together with the other kinds (FZ_EINVAL). */
int fz_subs_ngrams_begin(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k);
int fz_generic_ngrams_begin(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m,
                            uint32_t max_subs, uint32_t max_ins, uint32_t max_dels, uint32_t max_l, int consolidated);
int fz_search_end(fz_ctx *ctx, fz_match **out, uint64_t *n);

/* Raw stream of the substitutions-only n-gram search: (i, i+m, min(Hamming, k+1), block) in the
 * reference's discovery order, cross-block duplicates preserved. */
int fz_subs_ngrams(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k,
                   fz_match **out, uint64_t *n);

/* Raw stream of find_near_matches_generic_ngrams (the greedy candidate-set automaton run on the
 * window around every n-gram hit), reference emission order: blocks in order, the hits of a block by index,
 * the matches of a hit as the automaton emits them, duplicates included.  The rows are ordered on the
 * device (one shard, at most 16 384 hits) or by the host; the bytes returned are the same either way. */
int fz_generic_ngrams(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m,
                      uint32_t max_subs, uint32_t max_ins, uint32_t max_dels, uint32_t max_l,
                      fz_match **out, uint64_t *n);

/* find_near_matches_generic_ngrams + consolidate_overlapping_matches in one call (what GenericSearch.search followed by
 * GenericSearch.consolidate_matches computes: generic_search.py:198-237, :256-273, common.py:185-189) — the same rows
 * as fz_consolidate(fz_generic_ngrams(...)).  The first stage of the consolidation runs on the device: the automaton
 * kernel folds the matches of every n-gram hit into (hull, best match) pairs, a few thousand pairs cross PCIe instead
 * of every raw match (BASELINE configs[3b]: 6e3 instead of 2.1e5 rows), the host merges overlapping hulls.  In-memory
 * sequences only (no file segments). */
int fz_generic_ngrams_consolidated(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m,
                                   uint32_t max_subs, uint32_t max_ins, uint32_t max_dels, uint32_t max_l,
                                   fz_match **out, uint64_t *n);

/* Search + the reduction the reference's strategy class applies to its result, in one call (round 4: find_near_matches
 * on a resident sequence paid a second C-ABI call and an array round trip through Python for it):
 *   fz_lev_ngrams_consolidated = fz_consolidate(fz_lev_ngrams(...))   LevenshteinSearch.search + consolidate_matches,
 *                                                                      levenshtein.py:151-164, common.py:185-189
 *   fz_subs_ngrams_best        = fz_group_best(fz_subs_ngrams(...))   what find_near_matches_substitutions_ngrams returns
 *                                                                      for bytes-like input, substitutions_only.py:258-282
 * (in a communicator: collective like the searches they start with). */
int fz_lev_ngrams_consolidated(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n);
int fz_subs_ngrams_best(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n);

/* n_pats Levenshtein n-gram searches with one budget k over one resident sequence, in as few passes over it as the
 * patterns allow.  pats = the patterns back to back, offs[i] .. offs[i+1] the bytes of pattern i (offs has n_pats + 1
 * entries).  *out = the raw streams of all patterns one after the other, (*out_offs)[i] .. (*out_offs)[i+1] the rows of
 * pattern i: byte for byte what fz_lev_ngrams(ctx, seq, pats + offs[i], offs[i+1] - offs[i], k, ...) returns, `block`
 * included.  Both outputs are released with fz_free.  Any pattern the single call refuses (empty, length <= k, beyond
 * the limits, halo too small) fails the whole call with that call's code and message before anything is searched.
 *
 * Planning is a function of the arguments alone.  The batched route takes the patterns with
 *     1 <= k <= 8,   m <= 128,   L = m / (k + 1) >= 4:
 * they are grouped by L in input order, a group holding at most 64 patterns with together at most 256 n-gram blocks
 * (the next pattern of that L that would exceed either starts a new group).  A group is ONE pass over the sequence: one
 * filter launch that tests every byte offset against all blocks of the group and appends the survivors to hit lists, and
 * one verification launch over those lists, per shard and whatever the number of patterns.  A group of one pattern and
 * every pattern outside the domain run through fz_lev_ngrams inside the same call.
 * Sequences of several shards: the group kernels run on every shard (global coordinates, ownership and halo as in the
 * single search) and the host orders every pattern's records of all shards together.  A context in a communicator
 * searches collectively: there the call is a loop over the collective fz_lev_ngrams, pattern by pattern, on every rank.
 * The call is synchronous; with a _begin outstanding it answers FZ_EINVAL.
 * fz_stats afterwards: filter_launches / bytes_scanned = filter launches of the whole call and the bytes they streamed,
 * ngram_hits = exactly confirmed hits, raw_matches = rows, all summed over the patterns; verify_form = FZ_FORM_KERNEL
 * when at least one group ran batched. */
int fz_lev_ngrams_multi(fz_ctx *ctx, fz_seq *seq, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats,
                        uint32_t k, fz_match **out, uint64_t **out_offs);
/* The same with every pattern's slice consolidated: slice i = what fz_lev_ngrams_consolidated returns for pattern i. */
int fz_lev_ngrams_multi_consolidated(fz_ctx *ctx, fz_seq *seq, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats,
                                     uint32_t k, fz_match **out, uint64_t **out_offs);
/* Test hook, no device needed: group_of[i] = the pass pattern i rides in (0 .. *n_groups - 1), or 0xffffffff when it
 * takes the single-pattern route. */
int fz_debug_multi_plan(const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                        uint32_t *group_of, uint32_t *n_groups);

/* The same for n_pats substitutions-only n-gram searches (k substitutions, no insertions or deletions): slice i of *out
 * = byte for byte what fz_subs_ngrams(ctx, seq, pats + offs[i], offs[i+1] - offs[i], k, ...) returns.  Same domain, same
 * grouping, same filter launch; the verification launch counts mismatches around the confirmed n-gram instead of running
 * the edit-distance expansion, and the planner's cost rule has constants of its own for it (measured).
 * Every pattern passes fz_subs_ngrams' checks first (the first one's error is the call's); patterns outside a group run
 * through fz_subs_ngrams inside the call; collective contexts and strided sequences loop.  fz_stats as above. */
int fz_subs_ngrams_multi(fz_ctx *ctx, fz_seq *seq, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats,
                         uint32_t k, fz_match **out, uint64_t **out_offs);
/* ... with every pattern's slice reduced by fz_group_best: slice i = what fz_subs_ngrams_best returns for pattern i. */
int fz_subs_ngrams_multi_best(fz_ctx *ctx, fz_seq *seq, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats,
                              uint32_t k, fz_match **out, uint64_t **out_offs);
/* fz_debug_multi_plan for either mode: 1 = Levenshtein (what fz_debug_multi_plan answers), 2 = substitutions only. */
int fz_debug_multi_plan_mode(uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                             uint32_t *group_of, uint32_t *n_groups);

/* One pattern, many sequences, one pass.  fz_batch_upload makes n_seqs sequences resident, packed back to back without
 * separators: sequence j = bytes[offs[j] .. offs[j+1]) (offs has n_seqs + 1 entries, offs[0] == 0, non-decreasing; equal
 * neighbours = an empty sequence).  n_seqs < 2^32.  Next to the bytes two tables go to the device: the cumulative end
 * offsets (u64 per sequence) and, per 16 KiB tile, the first sequence that touches it (u32), which bounds the search for
 * a position's sequence.  Single-device, non-collective contexts (else FZ_EUNSUPPORTED).  The handle is a batch handle:
 * fz_batch_search and fz_batch_search_multi take it, every other search function answers FZ_EINVAL for it (and those two
 * answer FZ_EINVAL for a plain sequence); fz_seq_len = the packed length; fz_seq_release / fz_destroy free bytes and tables. */
int fz_batch_upload(fz_ctx *ctx, const uint8_t *bytes, const uint64_t *offs, uint64_t n_seqs, fz_seq **out);

/* mode: FZ_MODE_EXACT / _LEV / _SUBS = 0 / 1 / 2 (k = 0 / max_l_dist / max_substitutions).
 * Every sequence is searched as a sequence of its own — window clamps and accepted n-gram ranges use its own ends, and
 * nothing that needs bytes of two sequences is found — in ONE pass over the packed bytes: the same filter launches as the
 * unsegmented search of the pattern over those bytes, whatever n_seqs is, and the same verification form (a function of
 * the arguments alone); a candidate additionally pays the lookup of its sequence.
 * Rows are in the LOCAL coordinates of their sequence, ordered by sequence; within one sequence they are byte for byte
 * what the single call returns for that sequence alone: fz_search_exact as (i, i + m, 0, -1), fz_lev_ngrams,
 * fz_subs_ngrams; with reduced != 0 what fz_lev_ngrams_consolidated / fz_subs_ngrams_best return for it (exact rows are
 * not reduced).  (*seq_of)[r] = sequence of row r.  Both outputs are released with fz_free.
 * The pattern is refused as the single calls refuse it, with their codes, before anything is searched.
 * fz_stats afterwards as for any search (raw_matches = rows before the reduction). */
int fz_batch_search(fz_ctx *ctx, fz_seq *batch, uint32_t mode, const uint8_t *p, uint32_t m, uint32_t k,
                    int reduced, fz_match **out, uint32_t **seq_of, uint64_t *n);

/* Many patterns, many sequences: fz_batch_search for every pattern of a list (packed as fz_lev_ngrams_multi takes them;
 * mode FZ_MODE_LEV or FZ_MODE_SUBS, one budget k) in as few passes over the packed bytes as the patterns allow.  The rows of
 * pattern i are (*out)[(*out_offs)[i] .. (*out_offs)[i+1]) with their sequences at the same positions of *seq_of; that slice
 * is byte for byte what fz_batch_search(ctx, batch, mode, pats + offs[i], m_i, k, reduced, ...) returns.  out_offs has
 * n_pats + 1 entries (n_pats = 0: the single entry 0); an empty batch gives empty slices.  All three outputs are released
 * with fz_free.
 * The patterns are planned as fz_debug_multi_plan_mode reports (same domain, groups and cost rule as fz_lev_ngrams_multi /
 * fz_subs_ngrams_multi): a group is one filter launch plus one verification launch that looks every candidate's sequence up
 * and verifies it inside that sequence alone; the patterns outside every group run, inside the same call, the code of
 * fz_batch_search.  Every pattern passes the single call's checks before anything is searched: the first refusal is the
 * call's, with its code.  FZ_EINVAL for a plain sequence handle, a search of the context still in flight or a file stream
 * in flight; FZ_EUNSUPPORTED for contexts of several devices or in a communicator.
 * fz_stats afterwards: the sums over the call; verify_form = FZ_FORM_KERNEL when a group rode a pass. */
int fz_batch_search_multi(fz_ctx *ctx, fz_seq *batch, uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats,
                          uint32_t k, int reduced, fz_match **out, uint32_t **seq_of, uint64_t **out_offs);

/* Best-pattern assignment: one answer per sequence instead of P x S row lists (demultiplexing reads against a barcode
 * list, adapter and primer panels, guide counting).  Row j of *out (n_seqs rows, released with fz_free):
 *   pattern  the lowest index among the patterns whose smallest distance in sequence j is the smallest of all; -1 when no
 *            pattern matches (then every other field is 0)
 *   dist     that distance
 *   tied     1 when at least one OTHER list position reaches the same dist in this sequence (a pattern listed twice ties
 *            with itself), else 0: every other pattern is at least one edit worse or absent
 *   start, end   local coordinates of one occurrence of `pattern` at `dist`: among that pattern's rows at that distance in
 *            that sequence — the rows of fz_batch_search(..., reduced = 0) — the one with the smallest start, then the
 *            largest end.  (pattern, dist and tied are also what the reduced rows give: a consolidation group keeps its
 *            minimum distance.  Only the position is defined on the raw stream: overlap groups are not a device-side notion.)
 * Nothing is ordered and no record is copied to the host: behind every verification launch one more kernel folds the
 * records, where they lie, into two tables of n_seqs entries by atomic minimum (fz_assign_reduce_kernel), and the tables
 * are decoded into the rows that are copied back (fz_assign_finish_kernel).
 * Checks, planning (fz_debug_multi_plan_mode answers for this call too), launches and fz_stats as fz_batch_search_multi;
 * raw_matches = records folded, verify_ms includes the fold.  Patterns outside every group are searched one by one as
 * fz_batch_search does and their rows go through the same fold.  In addition FZ_EUNSUPPORTED, before anything is searched,
 * for k > 127, more than 65 535 patterns, or a sequence of 2^32 bytes or more: the tables' keys have no room for them.
 * n_pats = 0, an empty batch and a batch of empty sequences give n_seqs rows of -1 and launch nothing. */
typedef struct {
    int32_t  pattern;
    uint16_t dist;
    uint16_t tied;
    uint32_t start, end;
} fz_assign;

int fz_batch_assign(fz_ctx *ctx, fz_seq *batch, uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats,
                    uint32_t k, fz_assign **out);

/* Test hook, no device needed: the fold of fz_batch_assign on the host, through the very functions the two kernels run
 * (fz_device.h: fz_assign_keys, fz_assign_row).  offs = the batch's n_seqs + 1 offsets; recs = n records of 24 bytes
 * {u64 key (low 48 bits: global index of the n-gram hit), u32 l, u32 r, u32 dist, u32 aux} with start = index - l and
 * end = index + L + r; pat_table = n_table pairs {u32 pattern index, u32 m} indexed by aux (one pair: aux ignored);
 * pat_m = the lengths of the n_pats patterns.  out = n_seqs rows. */
int fz_debug_assign_fold(const uint64_t *offs, uint64_t n_seqs, const void *recs, uint64_t n, uint32_t L,
                         const uint32_t *pat_table, uint32_t n_table, const uint32_t *pat_m, uint32_t n_pats, uint32_t k,
                         fz_assign *out);

/* End overlaps: the strictly partial PREFIX of a pattern at the END of every sequence of a batch (a read that runs into its
 * adapter and breaks off: "3' adapter, partial occurrences allowed").  Per sequence r of n bytes, pattern p of m bytes,
 * budget k and min_overlap o, over the prefix lengths o <= i <= m - 1, each with the scaled budget k_i = k * i / m:
 *   FZ_MODE_LEV   E(i) = min over a in [0, n] of ed(p[:i], r[a:]), j(i) = the largest j with ed(p[:i], r[n-j:]) == E(i)
 *                 (i may exceed n: a short sequence can hold a prefix with deletions)
 *   FZ_MODE_SUBS  E(i) = Hamming(p[:i], r[n-i:]) for i <= n, j(i) = i
 * A length qualifies when E(i) <= k_i.  A pattern answers with the i of the most matched bytes i - E(i), then the smaller
 * E(i); the sequence answers with the pattern of the largest i - d, then the smaller d, then the lower list position (a
 * pattern listed twice answers with its first).  Row j of *out (n_seqs rows, released with fz_free):
 *   pattern, overlap = i, dist = d, start = n - j(i);  none: pattern = 0xffff, overlap = dist = 0, start = n
 * so `start` is a cut position as it stands.  Whole occurrences, also those that end at the sequence's end, are
 * fz_batch_search's to find.
 * On the device (fz_kernels.h: fz_overlap_kernel): one lane per sequence reads its last m - 1 + k_(m-1) bytes only; the list
 * is cut into launches of 8 (FZ_MODE_LEV) or 64 (FZ_MODE_SUBS) patterns that fold into one table of a 64-bit key per
 * sequence by atomic maximum; a finish kernel decodes it and ONE copy of n_seqs * 8 bytes brings the rows back.
 * Domain: 1 <= m <= 64, k <= 16, k < m, at most 65 534 patterns, sequences shorter than 2^32 bytes.  Refusals, before anything
 * is launched: FZ_EUNSUPPORTED for anything outside the domain (the pattern is named), another mode, a plain sequence
 * handle, a context of several devices or in a communicator; FZ_EINVAL for min_overlap == 0, an empty pattern, a search
 * of the context still in flight.  No patterns or an empty batch: rows of none, or no rows.
 * fz_stats afterwards: filter_launches = the launches of the list, verify_ms = device_ms = their span with the finish kernel. */
typedef struct {
    uint32_t start;
    uint16_t pattern;
    uint8_t  overlap, dist;
} fz_overlap;

int fz_batch_end_overlaps(fz_ctx *ctx, fz_seq *batch, uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats,
                          uint32_t k, uint32_t min_overlap, fz_overlap **out);
/* Test hook, no device needed: the same call on the host, through the very functions the kernels' lanes run (fz_device.h:
 * fz_overlap_stage, fz_overlap_lane, fz_overlap_row) and with the same refusals.  bytes = the packed sequences, ends = their
 * n_seqs cumulative end offsets; out = n_seqs rows. */
int fz_debug_end_overlaps(uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                          uint32_t min_overlap, const uint8_t *bytes, const uint64_t *ends, uint64_t n_seqs, fz_overlap *out);
/* ms4 = {tables to the device, kernels (0 for a context that does not time them), rows to the host, the whole call} of
 * the context's last fz_batch_end_overlaps, in milliseconds. */
int fz_debug_overlap_ms(fz_ctx *ctx, double *ms4);

/* Score cuts: per sequence of a batch where the running sum of a table of scores, taken from its end, peaks — the cut
 * position of quality trimming (the running-sum rule of BWA) and of poly-A trimming, which are two tables.  Per sequence r
 * of n bytes, a table w of 256 signed scores, a flag `stop` and an optional miss rate num / den (a miss: a byte with w < 0):
 *   cut3(r):  s = best = miss = 0; cut = n
 *             for i = n - 1 down to 0:  s += w[r[i]]; miss += (w[r[i]] < 0)
 *                                       if stop and s < 0: break
 *                                       if s > best and (no rate or miss * den <= num * (n - i)): best = s; cut = i
 *   cut5(r) = n - cut3(reversed r)
 * The comparison is strict: of equal peaks the one nearest the end wins.  w3 / w5: the table of the 3' / the 5' side, NULL =
 * that side is not asked for.  flags: FZ_CUT_STOP3, FZ_CUT_STOP5 = that side stops; FZ_CUT_RATE = rate_num / rate_den is in
 * force on the sides that do not stop.  Row j of *out (n_seqs rows, released with fz_free): start = cut5 (0 when the 5' side
 * is not asked for), end = cut3 (n when the 3' side is not); both sides asked for and start >= end: both 0, the empty
 * sequence.  Quality trimming at cutoff q: w[b] = q - (b - base), stop.  Poly-A: w['A'] = 1, every other byte -2, no stop,
 * rate 1 / 5.
 * On the device (fz_kernels.h: fz_cuts_kernel): one lane per sequence walks it in pieces of 64 bytes from the asked end,
 * with 32-bit sums, and leaves it when the sequence is used up, when `stop` fired, or when s + remaining * wmax <= best
 * (wmax = the table's largest score: no later sum can pass the peak; exact).  The lane writes its row, ONE copy of
 * n_seqs * 8 bytes brings the rows back.  A table without a positive score cuts nothing: no side with one, and nothing is
 * launched.
 * Refusals, before anything is launched: FZ_EUNSUPPORTED for a plain sequence handle, a context of several devices or in a
 * communicator, and a batch with max_seq_len * max|w| >= 2^31 (both numbers are named: the sums are 32-bit); FZ_EINVAL for
 * both tables NULL, flags outside the three, rate_den == 0 with FZ_CUT_RATE, a search of the context still in flight.
 * fz_stats afterwards: filter_launches = 1 or 0, verify_ms = device_ms = the kernel's span. */
#define FZ_CUT_STOP3 1u
#define FZ_CUT_STOP5 2u
#define FZ_CUT_RATE 4u

typedef struct {
    uint32_t start, end;
} fz_cut;

int fz_batch_score_cuts(fz_ctx *ctx, fz_seq *batch, const int16_t *w3, const int16_t *w5, uint32_t flags,
                        uint32_t rate_num, uint32_t rate_den, fz_cut **out);
/* Test hook, no device needed: the same call on the host, through the very functions the kernel's lanes run (fz_device.h:
 * fz_cuts_piece, fz_stage_copy, fz_cuts_lane, fz_cuts_row) and with the same refusals.  bytes = the packed sequences, ends =
 * their n_seqs cumulative end offsets; out = n_seqs rows. */
int fz_debug_score_cuts(const int16_t *w3, const int16_t *w5, uint32_t flags, uint32_t rate_num, uint32_t rate_den,
                        const uint8_t *bytes, const uint64_t *ends, uint64_t n_seqs, fz_cut *out);
/* ms4 = {tables to the device, kernel (0 for a context that does not time it), rows to the host, the whole call} of the
 * context's last fz_batch_score_cuts, in milliseconds. */
int fz_debug_cuts_ms(fz_ctx *ctx, double *ms4);

/* Symbol classes (IUPAC patterns) on the substitutions-only multi-pattern pass.  Two tables of 256 bytes define them:
 *   tmask[t]  the one-hot bit of text byte t among the base symbols (at most 8), 0 when t is no base symbol
 *   pmask[c]  the set of pattern byte c as a mask over those bits, 0 for a plain byte
 * Pattern byte c matches text byte t iff t == c or (tmask[t] & pmask[c]) != 0; text bytes are never classes.  The class
 * distance of a pattern and a window of its length is the number of positions that do not match; the class forms below are
 * the named calls with that distance in the place of the Hamming distance: every window within k appears once in the raw
 * stream of every n-gram block it class-matches, rows (start, end, dist, block) in the order of the plain calls.
 * Every pattern rides a pass, a list of one included: the cost rule is not consulted and there is no single-pattern route.
 * So every pattern must be inside the batched domain (1 <= k <= 8, m <= 128, m / (k + 1) >= 4), and its n-gram blocks must
 * fit the filter's table: a block contributes one entry per distinct hash over the spellings of the bytes the filter hashes
 * (bytes 0 .. 3 and the last three of its first min(L, 8) bytes; class bytes elsewhere are free), a group holds 64 patterns
 * and 256 entries, and a pattern that needs more than 256 on its own is refused.  FZ_EUNSUPPORTED names the pattern in both
 * cases, before anything is searched; so do collective contexts and strided sequences.  FZ_EINVAL for a tmask entry of more
 * than one bit or a bit used twice.  All other checks, shards and halos (m bytes), outputs and fz_stats as for the plain call. */
int fz_subs_ngrams_multi_cls(fz_ctx *ctx, fz_seq *seq, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                             const uint8_t *pmask, const uint8_t *tmask, fz_match **out, uint64_t **out_offs);
/* ... with every pattern's slice reduced by fz_group_best (the best match of every overlap group). */
int fz_subs_ngrams_multi_best_cls(fz_ctx *ctx, fz_seq *seq, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats,
                                  uint32_t k, const uint8_t *pmask, const uint8_t *tmask, fz_match **out, uint64_t **out_offs);
/* fz_batch_search_multi in substitutions mode, with classes. */
int fz_batch_search_multi_cls(fz_ctx *ctx, fz_seq *batch, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats,
                              uint32_t k, const uint8_t *pmask, const uint8_t *tmask, int reduced, fz_match **out,
                              uint32_t **seq_of, uint64_t **out_offs);
/* fz_batch_assign in substitutions mode, with classes: the same fold over the class forms' records. */
int fz_batch_assign_cls(fz_ctx *ctx, fz_seq *batch, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                        const uint8_t *pmask, const uint8_t *tmask, fz_assign **out);
/* Test hook, no device needed: the plan of a class call.  group_of[i] = the pass pattern i rides in (never 0xffffffff);
 * pat_entries[i] (optional, n_pats values) = the table entries of pattern i; group_entries[g] (optional, room for n_pats
 * values) = the entries of group g.  The class calls' refusals, with their codes. */
int fz_debug_multi_plan_cls(const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k, const uint8_t *pmask,
                            const uint8_t *tmask, uint32_t *group_of, uint32_t *n_groups, uint32_t *pat_entries,
                            uint32_t *group_entries);

/* Test hook, no device needed: the sequence of position idx of a batch with the offsets `offs` — the lookup the kernels
 * run (fz_device.h: fz_segment_ragged, the per-tile bound included), on the host.  *j = its number, [*sa, *se) its bytes.
 * FZ_EINVAL for idx >= offs[n_seqs].  The tables are built on the first call for an offset array and kept for the next
 * calls with the same array (same address, length and total). */
int fz_debug_batch_segment(const uint64_t *offs, uint64_t n_seqs, uint64_t idx, uint64_t *j, uint64_t *sa, uint64_t *se);

/* Records: a text of lines (a FASTQ file, a file with one read per line) becomes a batch on the device.  The text is
 * copied to the device once and split there (fz_kernels.h: fz_rec_*_kernel): newlines are counted per 16 KiB tile, the
 * counts scanned, every newline's position written at its rank, one lane per record measures its sequence, the lengths
 * are scanned and the sequences gathered into a buffer laid out as fz_batch_upload's.  No per-sequence work on the host.
 *   Lines: a line ends at '\n' or, the last one, at the end of the text (an empty text has no lines); one '\r' in front of
 *   that end is not content.  Record r = lines r * lines_per_record .. + lines_per_record - 1, its sequence = line
 *   r * lines_per_record + sequence_line (sequence_line < lines_per_record), empty lines included.
 *   FZ_REC_FASTQ_CHECKS (lines_per_record = 4, sequence_line = 1 only): trailing empty lines are dropped first, then the
 *   smallest (record, reason) is an error: 1 the line count is no multiple of 4 (record = lines / 4), 2 line 0 does not
 *   start with '@', 3 line 2 does not start with '+', 4 line 3 is not as long as line 1.  Then the call answers FZ_EINVAL
 *   with *out = NULL, info->bad_record / bad_reason filled in and nothing left allocated.  (bad_reason = 0: no error.)
 *   Multi-line FASTQ and compressed input are not understood; FASTA is fz_batch_upload_fasta's.
 * The handle is a batch handle like fz_batch_upload's (same refusals: several devices or a communicator, a search in
 * flight, a text of 2^48 bytes or more, 2^32 sequences or more); fz_batch_search, _multi and _assign cannot tell them apart. */
#define FZ_REC_FASTQ_CHECKS 1u
typedef struct {
    uint64_t n_lines, n_seqs, packed_bytes, bad_record;
    uint32_t bad_reason;
} fz_records_info;

int fz_batch_upload_records(fz_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t lines_per_record, uint32_t sequence_line,
                            uint32_t flags, fz_seq **out, fz_records_info *info);

/* The tables of a batch handle, n_seqs entries each (either may be NULL): src_starts[j] = offset of sequence j's first byte
 * in the text it was cut from (a handle of fz_batch_upload: offs[j]; of fz_batch_derive: its lowest source byte in the parent's
 * packed bytes), ends[j] = its end in the packed bytes. */
int fz_batch_tables(const fz_seq *batch, uint64_t *src_starts, uint64_t *ends);

/* Test hooks.  fz_debug_batch_bytes: the packed bytes of a batch handle back from the device (cap >= fz_seq_len).
 * fz_debug_records_split: no device — the split of fz_batch_upload_records on the host through the functions its kernels
 * run (fz_device.h: fz_rec_line, fz_rec_measure, fz_rec_err_key); *src_starts, *ends (n_seqs entries) and *packed are
 * released with fz_free and are NULL after an error, which is reported as above.
 * fz_debug_scan_items: the items one workgroup of the device scan handles (its seams).  fz_debug_records_ms: device and host
 * spans of the context's last fz_batch_upload_records, milliseconds: {H2D copy, the kernels, the D2H of ends[], whole call}. */
int fz_debug_batch_bytes(fz_seq *batch, uint8_t *out, uint64_t cap);
int fz_debug_records_split(const uint8_t *text, uint64_t n, uint32_t lines_per_record, uint32_t sequence_line, uint32_t flags,
                           uint64_t **src_starts, uint64_t **ends, uint8_t **packed, fz_records_info *info);
uint32_t fz_debug_scan_items(void);
int fz_debug_records_ms(fz_ctx *ctx, double *ms4);

/* FASTA: the contigs of a FASTA text become a batch on the device, by the rule of `samtools faidx`.  Lines are those of
 * fz_batch_upload_records, trailing empty lines dropped first.  A line whose first byte is '>' is a header and opens a
 * record; every other line is a sequence line of the record the nearest header above it opened; a record's sequence is the
 * concatenation of its sequence lines' contents (none: an empty contig).  Per record: linebases = the content length of its
 * first sequence line, linewidth = the distance from that line's first byte to the next line's first byte (to the end of the
 * text when no line follows), offset = the position of its first base; all 0 for an empty contig, whose offset is the
 * position behind the header line.  header_start / header_len: the header line's content without the '>'.
 *   The smallest (record, reason) is an error, reported as fz_batch_upload_records reports the FASTQ ones (FZ_EINVAL, *out =
 *   NULL, info->bad_record / bad_reason, nothing left allocated), with the reasons behind the FASTQ ones: 5 the text is not
 *   empty and does not start with '>' (record 0), 6 an empty sequence line inside a record, 7 a sequence line that is not
 *   the record's last has a content length or width other than linebases / linewidth, or the last one is longer than
 *   linebases.  ';' comment lines, blank lines between records and compressed input are not understood.
 *   Sequence bytes pass through untouched; FZ_FA_UPPER clears bit 5 of every byte in 'a' .. 'z' as they are gathered.
 * On the device (fz_kernels.h: fz_fa_*_kernel): behind the newline table of the records path one lane per line flags the
 * headers, the scan of the flags gives every line its record, one lane per record measures it from its first and last
 * sequence line, one lane per line checks it, the lengths are scanned and the bases gathered without their newlines.
 * Refusals, the handle, fz_batch_tables (src_starts[j] = offset of record j) and fz_debug_records_ms as fz_batch_upload_records.
 * fz_batch_fasta_index: the n_seqs rows of such a handle, copied from the device on demand (FZ_EINVAL for any other handle). */
#define FZ_FA_UPPER 1u
typedef struct {
    uint64_t header_start, header_len, length, offset, linebases, linewidth;
} fz_fasta_row;

int fz_batch_upload_fasta(fz_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t flags, fz_seq **out, fz_records_info *info);
int fz_batch_fasta_index(const fz_seq *batch, fz_fasta_row *rows);
/* Test hooks, no device: the split of fz_batch_upload_fasta on the host through the functions its kernels run (fz_device.h:
 * fz_fa_measure, fz_fa_line_check, fz_fa_src, fz_fa_upper4); *rows, *ends (n_seqs entries) and *packed are released with
 * fz_free and are NULL after an error.  fz_debug_fasta_upper4: the gather's fold of four bytes.  fz_debug_fasta_src: the
 * position in the text of base q of a record with that offset, linebases and linewidth (linebases = 0: offset). */
int fz_debug_fasta_split(const uint8_t *text, uint64_t n, uint32_t flags, fz_fasta_row **rows, uint64_t **ends, uint8_t **packed,
                         fz_records_info *info);
uint32_t fz_debug_fasta_upper4(uint32_t w);
uint64_t fz_debug_fasta_src(uint64_t offset, uint64_t linebases, uint64_t linewidth, uint64_t q);

/* Derived batches: a batch made from a batch where it lies, in device memory.  The rule:
 *     out[j] = X(batch[i_j][a_j : b_j])   for j < n_out
 *     i_j = index[j] (index NULL: j, and n_out must be the batch's number of sequences), a_j = starts[j] (NULL: 0),
 *     b_j = ends[j] (NULL: the length of sequence i_j); starts / ends are per OUTPUT and local to sequence i_j;
 *     X = every byte through the 256-byte table `translate` (NULL: as it is), then, with FZ_DERIVE_REVERSE, the bytes in
 *     reverse order.
 *   index may repeat and need not ascend, so the derived batch may be larger than its parent; empty outputs are sequences.
 *   An item is bad when i_j is no sequence of the batch (reason 1), a_j > b_j (2) or b_j > the length of sequence i_j (3).  The
 *   smallest bad j is an error: FZ_EINVAL, *out = NULL, info->bad_item / bad_reason filled in, nothing left allocated.
 * On the device (fz_kernels.h: fz_derive_*_kernel): the given tables are uploaded, one lane per output measures and checks
 * it, the lengths are scanned as fz_batch_upload_records scans them, and the bytes are gathered from the batch's packed bytes
 * by 16-byte pieces of the destination.  No text crosses PCIe; ends[] of the new handle comes back.
 * `batch`: a live batch handle of this context (fz_batch_upload, _records, _fasta or fz_batch_derive), which stays as it is
 * and may be released before the derived one.  Refusals as the uploads': several devices or a communicator, a search in
 * flight, n_out of 2^32 or more, a packed length of 2^48 bytes or more (FZ_EUNSUPPORTED).  The handle is a batch handle like
 * any other; its fz_batch_tables src_starts[j] is the offset of output j's lowest source byte in the PARENT's packed bytes. */
#define FZ_DERIVE_REVERSE 1u
typedef struct {
    uint64_t n_out, packed_bytes, longest, bad_item;
    uint32_t bad_reason;
} fz_derive_info;

int fz_batch_derive(fz_ctx *ctx, fz_seq *batch, const uint32_t *index, const uint64_t *starts, const uint64_t *ends, uint64_t n_out,
                    uint32_t flags, const uint8_t *translate, fz_seq **out, fz_derive_info *info);
/* Test hooks.  fz_debug_derive_plan: no device; the measure step and the scan on the host through the function the kernel
 * runs (fz_device.h: fz_derive_item).  offs = the parent's n_src + 1 offsets; src[] (n_out entries) and at[] (n_out + 1: the
 * outputs' starts in the packed bytes, the total last) are the caller's; the verdict as above, in *info.
 * fz_debug_derive_ms: device and host spans of the context's last fz_batch_derive, milliseconds: {the tables' H2D copies,
 * measure + scan, the gather (hipEvents on the stream), the D2H of ends[] (host clock, started once the gather has finished),
 * whole call}.  With timing off (fz_set_timing) the first four are 0 and the call does not wait for the gather on its own. */
int fz_debug_derive_plan(const uint64_t *offs, uint64_t n_src, const uint32_t *index, const uint64_t *starts, const uint64_t *ends,
                         uint64_t n_out, uint64_t *src, uint64_t *at, fz_derive_info *info);
int fz_debug_derive_ms(fz_ctx *ctx, double *ms5);

/* Several lines of every record: fz_batch_upload_records for n_kept lines of each record from ONE copy of the text and ONE
 * line table.  lines[i] < lines_per_record names the line of handle outs[i]; 1 <= n_kept <= lines_per_record, a repeated
 * entry is FZ_EINVAL.  Measure, scan and gather run once per kept line with the kernels of fz_batch_upload_records; every
 * kept line gets a batch handle of its own, all with the same number of sequences: the records in which every kept line
 * exists.  With FZ_REC_FASTQ_CHECKS (lines_per_record = 4; any lines) trailing empty lines are dropped first and the FASTQ
 * verdict is computed once, by the measure at line 1 whether or not line 1 is kept, and reported exactly as
 * fz_batch_upload_records reports it; the other lines are measured without checks over the trimmed text.  On any error
 * every handle already made is released and all outs[] are NULL.  *info is filled for line lines[0].  Refusals as
 * fz_batch_upload_records.  fz_debug_records_ms afterwards: {H2D copy, the kernels of all lines, the D2H of all ends[], whole call}. */
int fz_batch_upload_records_lines(fz_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t lines_per_record, const uint32_t *lines,
                                  uint32_t n_kept, uint32_t flags, fz_seq **outs, fz_records_info *info);

/* Formatted text: batches become the text of a file, assembled in device memory.  The rule:
 *     text = join over j < n of  lit[0] + col[0][j] + lit[1] + col[1][j] + ... + col[C - 1][j] + lit[C]
 *   columns: C live batch handles of this context (1 <= C <= FZ_FORMAT_MAX_COLUMNS) with n sequences each; a column may
 *   appear twice; they stay as they are.  literals: the C + 1 byte strings back to back, literal_lens: their lengths, each
 *   at most FZ_FORMAT_MAX_LITERAL.  equal_a / equal_b: two columns whose sequences must be of one length in every record
 *   (FASTQ: bases and qualities), or FZ_FORMAT_NO_CHECK for either.  A record in which they differ is bad (reason 1); the
 *   smallest bad record is an error: FZ_EINVAL, info->bad_record / bad_reason filled in, nothing written to `out`, nothing
 *   left allocated.  The text's length, sum(fz_seq_len(col)) + n * sum(literal_lens), is known before anything runs: `out`
 *   is the caller's buffer of `cap` bytes, and a cap smaller than the text is FZ_EINVAL.
 * On the device (fz_kernels.h: fz_format_*_kernel): one lane per record measures and checks it, the lengths are scanned as
 * fz_batch_upload_records scans them, the text is gathered by 16-byte pieces of the destination from the columns' packed
 * bytes and the literals, then one copy of the text to `out`.  All device memory of the call is transient.
 * Refusals as fz_batch_derive's: a column that is no live batch handle of this context, columns with different numbers of
 * sequences (the column is named), several devices or a communicator, a search in flight, a text of 2^48 bytes or more. */
#define FZ_FORMAT_MAX_COLUMNS 8u
#define FZ_FORMAT_MAX_LITERAL 255u
#define FZ_FORMAT_NO_CHECK 0xffffffffu
typedef struct {
    uint64_t n_records, text_bytes, longest_record, bad_record;
    uint32_t bad_reason;
} fz_format_info;

int fz_batch_format(fz_ctx *ctx, fz_seq *const *columns, uint32_t n_columns, const uint8_t *literals, const uint32_t *literal_lens,
                    uint32_t equal_a, uint32_t equal_b, uint8_t *out, uint64_t cap, fz_format_info *info);
/* Test hooks.  fz_debug_format_plan: no device; the measure step and the scan on the host through the function the kernel
 * runs (fz_device.h: fz_format_record).  offs[c] = column c's n + 1 offsets (the same pointer twice: a column twice); at[]
 * (n + 1 entries: the records' starts in the text, its length last) is the caller's; the verdict as above, in *info.
 * fz_debug_format_ms: device and host spans of the context's last fz_batch_format, milliseconds: {the descriptor's H2D copy,
 * measure + scan, the gather (hipEvents on the stream), the D2H of the text (host clock, started once the gather has
 * finished), whole call}.  With timing off (fz_set_timing) the first four are 0 and the call does not wait for the gather
 * on its own. */
int fz_debug_format_plan(const uint64_t *const *offs, uint32_t n_columns, uint64_t n, const uint32_t *literal_lens,
                         uint32_t equal_a, uint32_t equal_b, uint64_t *at, fz_format_info *info);
int fz_debug_format_ms(fz_ctx *ctx, double *ms5);

/* has_near_match_* (substitutions_only.py:139-145, :218-233; generic_search.py:240-253): *found = 1 iff the
 * corresponding search would return at least one record.  Nothing is ordered or copied, and device work that starts
 * after the first record has been counted is skipped (workgroups of the scan, hits of the automaton kernel). */
int fz_subs_ngrams_any(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, int *found);
int fz_subs_lp_any(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, int *found);
int fz_generic_ngrams_any(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m,
                          uint32_t max_subs, uint32_t max_ins, uint32_t max_dels, uint32_t max_l, int *found);

/* The reference's linear-programming fallbacks, used by its dispatchers when
 * len(subsequence) // (k + 1) < 3 (short patterns).  Whole-sequence candidate automata, tiled by
 * start position on the GPU; ordered emission lists exactly as the reference yields them.
 *   fz_lev_lp     <->  find_near_matches_levenshtein_linear_programming   levenshtein.py:52-148
 *   fz_subs_lp    <->  _find_near_matches_substitutions_lp                substitutions_only.py:82-136
 *   fz_generic_lp <->  _find_near_matches_generic_linear_programming      generic_search.py:57-177 */
int fz_lev_lp(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n);
int fz_subs_lp(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n);
int fz_generic_lp(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m,
                  uint32_t max_subs, uint32_t max_ins, uint32_t max_dels, uint32_t max_l,
                  fz_match **out, uint64_t *n);

/* RCCL over xGMI without PyTorch (the reference's only scale-out analogue is the chunk loop of
 * __init__.py:129-171).  A context that joined a communicator searches COLLECTIVELY: fz_lev_ngrams and
 * fz_lev_ngrams_begin / _end must be called by every rank in the same order, every rank scans the shard(s) it
 * holds (fz_seq_upload_shard / fz_seq_add_shard), the ranks' record lists are exchanged by ONE ncclAllGather of
 * device buffers per search (capacity follows the counts) and every rank receives the merged stream of the whole
 * sequence in the reference's order.  With _begin / _end the all-gather of search i runs on its own stream next to
 * the scan of search i + 1.
 *   one process per GPU:   rank 0 calls fz_comm_unique_id and hands the FZ_COMM_ID_BYTES bytes to the other ranks
 *                          (file, socket, MPI: not this library's business), every rank calls fz_comm_init_rank on
 *                          its single-device context;
 *   one process, N GPUs:   fz_comm_init_all on the multi-device context (ncclCommInitAll; every device = one rank).
 * fz_comm_allgather / fz_comm_max_f64 / fz_comm_barrier serve load-time exchanges (halo bytes) and the job's clock.
 * fz_comm_set_collective(ctx, 0) makes the searches of the context local again (the communicator stays). */
#define FZ_COMM_ID_BYTES 128
int  fz_comm_unique_id(void *id, uint64_t id_bytes);
int  fz_comm_init_rank(fz_ctx *ctx, const void *id, int world, int rank);
int  fz_comm_init_all(fz_ctx *ctx);
int  fz_comm_info(fz_ctx *ctx, int *world, int *rank, int *collective);
int  fz_comm_set_collective(fz_ctx *ctx, int on);
int  fz_comm_allgather(fz_ctx *ctx, const void *send, uint64_t nbytes, void *recv);
int  fz_comm_max_f64(fz_ctx *ctx, double *value);
int  fz_comm_barrier(fz_ctx *ctx);
void fz_comm_destroy(fz_ctx *ctx);
/* Host time (ms) of the exchange step of the collective search collected last on this context: from "every local
 * shard has finished" to "every rank's records are on this host" (all-gather + D2H copy + parsing the ranks' blocks). */
int  fz_comm_gather_ms(fz_ctx *ctx, double *ms);
/* Which collective library fz_comm_* would use (loads it): 0 none found (fz_comm_* answer FZ_EUNSUPPORTED), 1 RCCL,
 * 2 the test suite's stand-in (tests/mock_rccl.cpp named by FZ_RCCL_LIB: the only one that accepts several ranks on
 * one device — fz_comm_init_all then accepts a context that lists a device more than once). */
int  fz_comm_backend(void);

/* consolidate_overlapping_matches: overlap groups -> best (dist, -len) per group -> sorted by
 * (start, end, dist).  Ties inside a group (the reference breaks them by set iteration order, i.e.
 * by PYTHONHASHSEED) are broken deterministically: smallest start. */
int fz_consolidate(const fz_match *in, uint64_t n, fz_match **out, uint64_t *n_out);

/* Best match of every overlap group in the reference's group-LIST order (group_matches appends new
 * groups and re-appends merged ones at the end, common.py:161-177) — the order that
 * substitutions_only.py:279-282 exposes.  Input order matters. */
int fz_group_best(const fz_match *in, uint64_t n, fz_match **out, uint64_t *n_out);

/* Multi-process jobs (one rank per GPU): merge the raw streams of `world` ranks,
 * each already in reference order (block-major, index ascending) and owning an ascending index range,
 * into the global reference order: for every block, the ranks' segments of that block back to back.
 * No sort, O(total) copies.  parts[r] / counts[r] = rank r's records; block_counts[r * nb + g] = how
 * many of them belong to block g.  `out` must hold sum(counts) records.  Needs no device. */
int fz_merge_ranks(const fz_match *const *parts, const uint64_t *counts, const uint64_t *block_counts,
                   uint32_t world, uint32_t nb, fz_match *out);

/* Wire format of one rank's contribution to the all-gather of match lists (16-byte rows so that the
 * collective and the D2H copy move 2/3 of the bytes of raw fz_match rows):
 *   header, FZ_WIRE_HEADER_ROWS rows: u64 count, u64 nblocks, u32 per_block_count[256]
 *   then `count` rows: i64 start, u32 end - start, u16 dist, u16 block   (at most cap_rows are stored)
 * fz_wire_pack fills `dst` (>= FZ_WIRE_HEADER_ROWS + cap_rows rows) from a stream in reference order.
 * fz_wire_merge reads `world` such blocks, each rows_per_rank rows apart, and writes the merged stream
 * (global reference order, like fz_merge_ranks) to `out`; *n_out = total.  If some rank stored fewer
 * rows than its count (count > cap), nothing is written and *max_count tells the capacity needed. */
#define FZ_WIRE_HEADER_ROWS 65
int fz_wire_pack(const fz_match *in, uint64_t n, uint64_t cap_rows, void *dst);
int fz_wire_merge(const void *recv, uint32_t world, uint64_t rows_per_rank, uint64_t cap_rows,
                  fz_match *out, uint64_t out_cap, uint64_t *n_out, uint64_t *max_count);

/* find_near_matches_in_file as a pipeline (replaces the chunk loops of __init__.py:129-171 and :174-200).
 * The reference searches every chunk of the file as an INDEPENDENT sequence, so results depend on the
 * chunk geometry; the stream reproduces it: chunk ("segment") j covers the items
 *     [j * seg_stride - seg_pre, (j + 1) * seg_stride + seg_post)   clipped to the file,
 * binary files: seg_stride = _chunk_size - keep, seg_pre = 0, seg_post = keep; text files: seg_stride =
 * _chunk_size, seg_pre = keep, seg_post = 0 (keep = len(subsequence) - 1 + extra_items_for_chunked_search).
 * Many chunks cross PCIe as one batch from pinned, double-buffered staging memory and are searched by one
 * launch with per-chunk clamps while the caller fills the next staging buffer.
 *   mode 0 exact (search_exact per chunk), 1 Levenshtein n-grams (k = max_l_dist), 2 substitutions-only
 *   n-grams (k = max_substitutions), 3 generic n-grams (k = max_l_dist + the three limits).
 * Protocol: fz_stream_buffer -> where to put the next bytes and how many fit; fz_stream_submit(n, last)
 * after writing n of them (a launch happens whenever whole chunks are available); or fz_stream_read_fd,
 * which drives both from a file descriptor until end of file: `threads` readers (0: half the cores, at most 32)
 * live for the whole call and take 1 MiB pieces of the current batch from a shared counter.
 * fz_stream_finish -> the raw match stream of the whole file in the reference's order (chunk by chunk,
 * each chunk in its in-memory order, file coordinates) and the chunk number of every record.
 * Requires seg_pre + seg_post <= seg_stride / 2 (FZ_EUNSUPPORTED otherwise: use per-chunk searches). */
typedef struct fz_stream fz_stream;
int  fz_stream_open(fz_ctx *ctx, uint32_t mode, const uint8_t *p, uint32_t m, uint32_t max_subs, uint32_t max_ins,
                    uint32_t max_dels, uint32_t k, uint64_t seg_stride, uint32_t seg_pre, uint32_t seg_post,
                    uint64_t batch_bytes, fz_stream **out);
int  fz_stream_buffer(fz_stream *st, uint8_t **host, uint64_t *capacity);
int  fz_stream_submit(fz_stream *st, uint64_t nbytes, int last);
int  fz_stream_read_fd(fz_stream *st, int fd, int64_t offset, int threads, uint64_t *total);
int  fz_stream_finish(fz_stream *st, fz_match **out, uint32_t **seg, uint64_t *n);
void fz_stream_close(fz_stream *st);

/* Test hook: the library reads its FZ_* environment switches (none is needed to use it) once,
 * on first use; this reads them again.  For tests that flip a switch inside one process; nothing may be in flight.
 * What a reload reaches: every switch that is consulted per search (routing, queue sizes, the scan grid's taper,
 * FZ_COMM_TIMEOUT_MS).  What it does NOT reach: the collective library (FZ_NO_RCCL / FZ_RCCL_LIB: loaded once per
 * process) and what a context took over when it was created (fz_create: the generic search's kernel choice, the worker
 * threads) — create a new context, or a new process, for those. */
void fz_debug_reload_switches(void);

/* Test hook (no device needed): how the scan would split the n-gram blocks of pattern p (block
 * length L, blocks at 0, L, 2L, ...) into launches.  out[4i .. 4i+3] = first block, number of blocks,
 * hash multiplier, slot shift of launch i (at most `cap` launches are written); *n_launches = total. */
int fz_debug_launch_plan(const uint8_t *p, uint32_t m, uint32_t L, uint32_t *out, uint32_t cap, uint32_t *n_launches);

/* Test hook (no device needed): the host step that turns the device's unordered 24-byte records
 * {u64 key = block << 48 | hit index, u32 left, u32 right, u32 dist (0xffffffff: empty slot), u32 aux} into fz_match
 * rows in the reference's emission order (block ascending, hit index ascending; n-gram length L). */
int fz_debug_order_records(const void *recs, uint64_t n, uint32_t L, fz_match **out, uint64_t *n_out);
/* ... the same with the key ranges a search knows beforehand (hit index < idx_bound, block < blk_bound): the form the
 * searches use — no pass over the records for their ranges, empty slots dropped while the sort keys are built. */
int fz_debug_order_records_bounded(const void *recs, uint64_t n, uint32_t L, uint64_t idx_bound, uint32_t blk_bound,
                                   fz_match **out, uint64_t *n_out);
/* ... and the sharded form: recs = the shards' records one shard after the other (seg_ends[i] = end of shard i), shards
 * owning ascending index ranges; every shard is ordered on its own and the rows are merged block by block. */
int fz_debug_order_segments(const void *recs, const uint64_t *seg_ends, uint32_t n_segments, uint32_t L, fz_match **out, uint64_t *n_out);

/* Test hook, no device needed: the regions a scan launch of `grid` workgroups over `ntiles` tiles is cut into on a GPU
 * with `n_cus` compute units (fzhip.hip: plan_scan_regions — the last `wg_per_cu * n_cus` workgroups take `steps` groups of
 * shrinking tile shares, down to `fmin` of a full one).  table[4 r .. 4 r + 3] = {first workgroup, workgroups, first tile,
 * end tile} of region r, `*n_regions` of them (0: one region, every workgroup strides over all tiles; at most 8 rows).
 * tests/test_host_logic.py checks that the regions partition both ranges. */
int fz_debug_scan_regions(uint64_t ntiles, uint64_t grid, uint32_t n_cus, int steps, double fmin, int wg_per_cu, uint32_t *n_regions,
                          uint64_t *table);

/* Test hook, no device needed: the plan of the scan launches of a Levenshtein n-gram search (pattern p of m characters,
 * budget k) over an in-memory shard of `buf_len` bytes on a GPU with `n_cus` compute units (fzhip.hip: plan_scan).
 * shares_chip != 0: the search is launched while another one of the context is in flight and writes its records straight
 * to the host.  *grid = workgroups per launch, *form = FZ_FORM_* of fz_stats' verify_form, *overlapped = the launch runs
 * next to its predecessor (on the device's other stream), regions as in fz_debug_scan_regions (table: at most 8 rows). */
int fz_debug_scan_plan(const uint8_t *p, uint32_t m, uint32_t k, uint64_t buf_len, uint32_t n_cus, int shares_chip, uint32_t *grid,
                       uint32_t *form, int *overlapped, uint32_t *n_regions, uint64_t *table);

/* Test hook, no device needed: which scan-kernel instance every launch of a fused in-memory search over one sequence
 * would run (fzhip.hip: scan_is_lean).  mode = FZ_MODE_LEV (1) or FZ_MODE_SUBS (2), budget k, shard and GPU as in
 * fz_debug_scan_plan.  *n_launches = scan launches of the search; bit i of *lean_mask = launch i (i < 32) runs the lean
 * instance (no equal-n-gram slot sets, register bands for k <= 2 only), clear = the full one.  *form = FZ_FORM_* as in
 * fz_debug_scan_plan: only FZ_FORM_FUSED_BAND has lean instances.  A function of the arguments and the FZ_* switches. */
int fz_debug_scan_instance(uint32_t mode, const uint8_t *p, uint32_t m, uint32_t k, uint64_t buf_len, uint32_t n_cus,
                           uint32_t *n_launches, uint32_t *lean_mask, uint32_t *form);

/* Test hook, no device needed: the host twin of the scan kernel's tile walk (fz_device.h: fz_scan_walk, the function the
 * kernel itself calls).  `ntiles`, `grid` and the region table as fz_debug_scan_plan returns them (n_regions rows);
 * *tile = the tile of the buffer that workgroup `wg` reads in its iteration `iter` of a forward (reversed = 0) or a
 * reversed launch, ~0 when the workgroup has no such iteration. */
int fz_debug_scan_walk(uint64_t ntiles, uint32_t grid, uint32_t n_regions, const uint64_t *table, uint32_t wg, uint32_t iter,
                       int reversed, uint64_t *tile);

/* Test hook: *next_reversed = the next eligible scan launch of the context on the FIRST shard of `seq` (every shard keeps
 * its own direction bit; NULL: on a sequence not scanned yet) would run reversed (fz_set_scan_direction); *reversed_launches = reversed scan launches of the context so far. */
int fz_debug_scan_direction(fz_ctx *ctx, fz_seq *seq, int *next_reversed, uint64_t *reversed_launches);

/* Test hook (no device needed): the host half of the exchange step of a collective search (what follows the
 * ncclAllGather).  `blocks` = `world` blocks of 1024 + cap * 24 bytes, block r = what rank r contributed: 128 64-bit
 * counters (word 1 = records the rank produced) followed by min(count, cap) device records (see fz_debug_order_records);
 * own_lo[r] = first hit index rank r owns (NULL: ranks own ascending ranges in rank order), L = n-gram length.
 * Some rank produced more than `cap` records: *need_cap = the capacity the re-gather uses (every rank computes the same
 * value from the same headers) and no stream.  Else *need_cap = 0 and *out = the merged stream in the reference's order:
 * every rank's records ordered by (block, index), then block by block the ranks' runs in ascending order of own_lo. */
int fz_debug_gather_merge(const void *blocks, uint32_t world, uint64_t cap, const uint64_t *own_lo, uint32_t L, fz_match **out,
                          uint64_t *n_out, uint64_t *need_cap);

/* Statistics of the search collected last.  The *_ms fields are hipEvent spans read from that search's events by THIS
 * call (and by fz_device_ms), not by the search: they describe it until the next search of the context is launched
 * (its launch re-records the events; the fields then read 0). */
int  fz_stats(fz_ctx *ctx, fz_stats_t *out);
/* Device memory of the context: the smallest free / total byte counts over its devices (hipMemGetInfo).  The host layer
 * sizes its residency cache with it (fuzzysearch_amd/engine.py: the reference itself holds nothing between calls,
 * __init__.py:35-57). */
int  fz_mem_info(fz_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);
/* hipEvent timing of the kernels (filter_ms / verify_ms / device_ms of fz_stats, fz_device_ms): on by default.
 * Off, no events are recorded around the kernels and the *_ms fields read 0. */
int  fz_set_timing(fz_ctx *ctx, int on);
/* Streams the two-deep pipeline (fz_lev_ngrams_begin / fz_subs_ngrams_begin) uses per device.  2 (the default of a context
 * of one device state) = a search launched while another one is in flight — when its scan is fused, in memory, and writes
 * its records straight to the host — runs on the device's other stream with a counter block of its own and starts while
 * the older one drains; consecutive searches of a pipeline alternate between the two streams.  1 (the default of a
 * context of several device states) = both searches in flight on one stream, the younger scan starts when the older one
 * has finished.  Synchronous calls always run on the first stream.  Under overlap a kernel's own hipEvent span (filter_ms,
 * fz_device_ms) includes the time it shares the device with its neighbour, so it no longer measures the kernel alone. */
int  fz_set_streams(fz_ctx *ctx, int n);
/* Direction of the whole-buffer scans of a resident sequence.  0 (default; FZ_SCAN_DIR=alt) = every such launch starts at
 * the end of the buffer its shard's last whole scan stopped at, so consecutive scans alternate between walking forward and
 * walking back and the second re-reads what the first read last while it is still in the device's last-level cache;
 * 1 (FZ_SCAN_DIR=fwd) = always forward; 2 (FZ_SCAN_DIR=rev) = always reversed.  Batches, file streams, has_near_match_*
 * and the re-run of a search whose results outgrew their buffers always go forward.  No row depends on the direction. */
int  fz_set_scan_direction(fz_ctx *ctx, int mode);
/* hipEvent span of the filter kernel(s) of the search collected last, per device of the ctx (at most `cap` values
 * are written); returns the number of devices, or a negative FZ_E* code. */
int  fz_device_ms(fz_ctx *ctx, double *filter_ms, int cap);
void fz_free(void *p);

#ifdef __cplusplus
}
#endif
#endif /* FZHIP_H */
