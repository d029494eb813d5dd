// Host model of a whole multi-pattern group over a BATCH (fuzzysearch_amd/csrc/fz_device.h compiled with g++): the group's
// table (fz_mp_build), the filter's lookup at every byte offset of the packed bytes as fz_mp_filter_kernel does it — seams
// between sequences included, which is where it over-reports — then, per reported (offset, block-table entry), what
// fz_mp_batch_verify_kernel / fz_mp_batch_verify_subs_kernel do per lane: the sequence of the offset (fz_segment_ragged),
// the ragged acceptance and the window's bounds (fz_mp_rag_accept), the exact n-gram test and fz_verify_lev with the
// sequence's ends, or fz_mp_block_equal / fz_mp_verify_subs on the window staged as aligned dwords.
// tests/test_multi_batch_host.py holds the rows against the oracle run per (pattern, sequence).
//
// With -DMP_BATCH_EMUL_MAIN the file is a program of its own: random groups over random batches, both modes, held against
// the same functions run on every sequence ALONE (copied out, so that nothing of a neighbour is in reach) — the form that
// runs under -fsanitize=address,undefined.
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../fuzzysearch_amd/csrc/fz_device.h"

namespace {
struct HostScores {
    std::vector<uint16_t> v;
    uint32_t get(uint32_t i) const { return v[i]; }
    void set(uint32_t i, uint32_t x) { v[i] = (uint16_t)x; }
};
struct CheckedWindow {                                     // the bytes a lane staged: [wlo, whi) of the packed buffer
    const uint8_t *buf;
    uint64_t wlo, whi;
    bool *outside;
    uint8_t at(uint64_t g) const {
        if (g < wlo || g >= whi) { *outside = true; return 0xEEu; }
        return buf[g];
    }
};
struct StagedWindow {                                      // a lane's LDS column: dword j of the staged window
    const uint32_t *d;
    uint32_t dword(uint32_t j) const { return d[j]; }
};
struct Row { uint32_t pid, g; uint64_t seq, idx; int64_t start, end; uint32_t dist; };

// -> rows of every pattern in LOCAL coordinates, ordered by (pattern, sequence, block, index); < 0: see mp_batch_emul_group.
long long run_group(uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t npat, uint32_t k, uint32_t L, const uint8_t *t,
                    const uint64_t *seq_offs, uint64_t n_seqs, std::vector<Row> &rows) {
    rows.clear();
    if (npat == 0 || npat > FZ_MP_MAX_PATS || L < FZ_MP_MIN_L || (mode != FZ_MODE_LEV && mode != FZ_MODE_SUBS)) return -1;
    const bool subs = mode == FZ_MODE_SUBS;
    const uint8_t *pp[FZ_MP_MAX_PATS];
    uint32_t pm[FZ_MP_MAX_PATS], max_m = 0;
    for (uint32_t i = 0; i < npat; ++i) {
        pp[i] = pats + offs[i];
        pm[i] = (uint32_t)(offs[i + 1] - offs[i]);
        if (pm[i] > FZ_MP_MAX_M || pm[i] / (k + 1) != L) return -1;
        max_m = std::max(max_m, pm[i]);
    }
    std::vector<uint32_t> desc(FZ_MP_DESC_WORDS);
    const uint32_t nent = fz_mp_build(desc.data(), pp, pm, npat, L);
    if (nent == 0) return -1;
    const uint64_t n = seq_offs[n_seqs];
    // the resident layout: zero padding behind the data; the batch's tables as fz_batch_upload builds them
    std::vector<uint8_t> buf(((n + 3) & ~(uint64_t)3) + 16, 0);
    if (n) memcpy(buf.data(), t, n);
    const uint64_t ntiles = (n + ((1ull << FZ_RAG_TILE_BITS) - 1)) >> FZ_RAG_TILE_BITS;
    std::vector<uint32_t> first(ntiles + 1);
    fz_ragged_first(seq_offs + 1, n_seqs, ntiles, first.data());
    FzGeom geom;
    memset(&geom, 0, sizeof geom);
    geom.n = n; geom.buf_off = 0; geom.buf_len = n; geom.own_lo = 0; geom.own_hi = n;
    geom.seg_org = reinterpret_cast<uint64_t>(seq_offs + 1);
    geom.seg_j0 = reinterpret_cast<uint64_t>(first.data());
    geom.seg_j1 = n_seqs;
    const uint32_t *sig = desc.data(), *slots = desc.data() + FZ_MP_DESC_SLOTS, *ent = desc.data() + FZ_MP_DESC_ENT;
    const uint32_t *pmt = desc.data() + FZ_MP_DESC_M, *pat4 = desc.data() + FZ_MP_DESC_PAT;
    const uint8_t *patb = reinterpret_cast<const uint8_t *>(pat4);
    const uint32_t win_dwords = subs ? (max_m + 3) / 4 + 1 : (max_m + 2 * k + 6) / 4 + 1;      // mp_run_shard
    const uint32_t m_max = (win_dwords - 1) * 4;
    std::vector<uint32_t> win(win_dwords);
    HostScores sc;
    sc.v.assign(2 * FZ_MP_MAX_K + 4, 0);
    for (uint64_t idx = 0; idx + L <= n; ++idx) {
        const uint32_t h = fz_mp_hash_bytes(buf.data() + idx, L);
        if (!fz_mp_sig_test(sig, h)) continue;
        const uint32_t run = fz_mp_lookup(slots, h);
        for (uint32_t j = 0; j < (run >> 16); ++j) {
            const uint32_t blk = (run & 0xffffu) + j;
            const uint32_t e = ent[blk & (FZ_MP_MAX_BLOCKS - 1u)];
            const uint32_t pid = e & (FZ_MP_MAX_PATS - 1u), g = (e >> 8) & 0xffu, s = e >> 16;
            const uint32_t m = pmt[pid];
            bool valid = blk < nent && m != 0u;
            if (subs) valid = valid && m <= m_max && s + L <= m;
            if (!valid) continue;
            const FzSeg sg = fz_segment_ragged(fz_ragged(geom), n, idx);
            FzMpRagCand c;
            if (!fz_mp_rag_accept(mode, geom, sg, m, k, L, s, idx, c)) continue;
            if (c.wlo < sg.sa || c.whi > sg.se || c.whi < c.wlo) return -3;          // a window that leaves the sequence
            FzRec rec;
            if (subs) {
                const uint64_t i0 = idx - s, wbase = i0 & ~(uint64_t)3;
                if (i0 != c.wlo || i0 + m != c.whi) return -3;
                const uint32_t sh = (uint32_t)(i0 - wbase);
                const uint32_t nd = (uint32_t)((i0 + m - wbase + 3) >> 2);
                if (nd > win_dwords) return -2;
                for (uint32_t d = 0; d < win_dwords; ++d) {
                    uint32_t x = 0;
                    if (d < nd) memcpy(&x, buf.data() + wbase + 4u * d, 4);     // (up to 3 bytes of a neighbour come along)
                    win[d] = x;
                }
                const StagedWindow w{win.data()};
                const uint32_t *p4 = pat4 + pid * (FZ_MP_MAX_M / 4u);
                valid = fz_mp_block_equal(w, sh, p4, 1u, L, s);
                if (!fz_mp_verify_subs(w, sh, p4, 1u, m, m_max, k, L, s, valid, rec)) continue;
            } else {
                const uint64_t wbase = c.wlo & ~(uint64_t)3;
                if (((c.whi - wbase + 3) >> 2) > win_dwords) return -2;
                bool outside = false;
                const CheckedWindow w{buf.data(), c.wlo, c.whi, &outside};
                const uint8_t *p = patb + pid * FZ_MP_MAX_M;
                if (memcmp(p + s, buf.data() + idx, L) != 0) continue;            // the exact n-gram test (inside the window)
                if (idx < c.wlo || idx + L > c.whi) return -4;
                const bool ok = fz_verify_lev<FZ_REG_BAND_MAX>(sc, w, sg.sa, sg.se, p, m, k, L, s, idx, rec);
                if (outside) return -4;                                           // a byte outside the staged window was asked for
                if (!ok) continue;
            }
            const int64_t base = (int64_t)sg.sa;
            rows.push_back(Row{pid, g, sg.j, idx, (int64_t)idx - (int64_t)rec.l - base, (int64_t)(idx + L + rec.r) - base, rec.dist});
        }
    }
    std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) {
        if (a.pid != b.pid) return a.pid < b.pid;
        if (a.seq != b.seq) return a.seq < b.seq;
        if (a.g != b.g) return a.g < b.g;
        return a.idx < b.idx;
    });
    return (long long)rows.size();
}
}  // namespace

extern "C" {

// mode 1 = Levenshtein, 2 = substitutions only.  pats / offs: npat patterns back to back, all with len / (k + 1) == L and
// inside the batched domain.  t / seq_offs: n_seqs sequences back to back (seq_offs has n_seqs + 1 entries, seq_offs[0] = 0).
// Every row of every pattern is written to out as {pattern, sequence, block, start, end, dist} in the sequence's LOCAL
// coordinates, ordered by (pattern, sequence, block, index): at most cap rows; -> the number of rows, -1 when the group does
// not fit a table, -2 when a staged window would leave the window area, -3 when a window leaves the candidate's sequence,
// -4 when the verification asked for a byte outside its window.
long long mp_batch_emul_group(uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t npat, uint32_t k, uint32_t L, const uint8_t *t,
                              const uint64_t *seq_offs, uint64_t n_seqs, int64_t *out, long long cap) {
    std::vector<Row> rows;
    const long long rc = run_group(mode, pats, offs, npat, k, L, t, seq_offs, n_seqs, rows);
    if (rc < 0) return rc;
    long long c = 0;
    for (const Row &r : rows) {
        if (c < cap) {
            int64_t *o = out + 6 * c;
            o[0] = r.pid; o[1] = (int64_t)r.seq; o[2] = r.g; o[3] = r.start; o[4] = r.end; o[5] = r.dist;
        }
        ++c;
    }
    return c;
}
}

#ifdef MP_BATCH_EMUL_MAIN
namespace {
uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd(uint32_t below) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % below);
}
}

int main() {
    long long total = 0;
    for (int it = 0; it < 60; ++it) {
        const uint32_t mode = (it & 1) ? FZ_MODE_SUBS : FZ_MODE_LEV;
        static const uint32_t ks[5] = {1, 2, 3, 4, 8};
        const uint32_t k = ks[rnd(5)], L = 4 + rnd(k < 8 ? 9 : 4);
        static const uint32_t sigmas[4] = {2, 4, 20, 200};
        const uint32_t sigma = sigmas[rnd(4)], npat = 1 + rnd(12);
        std::vector<uint8_t> pats;
        std::vector<uint64_t> offs(1, 0);
        uint32_t blocks = 0;
        for (uint32_t i = 0; i < npat; ++i) {
            const uint32_t m = L * (k + 1) + rnd(k + 1);
            if (m > FZ_MP_MAX_M || blocks + m / L > FZ_MP_MAX_BLOCKS) break;
            blocks += m / L;
            for (uint32_t q = 0; q < m; ++q) pats.push_back((uint8_t)(1 + rnd(sigma)));
            offs.push_back(pats.size());
        }
        const uint32_t np = (uint32_t)offs.size() - 1;
        if (!np) continue;
        // sequences of 0 .. 300 bytes, one of them longer than a tile; copies of patterns at their ends and across seams
        const uint32_t n_seqs = 1 + rnd(it % 5 == 0 ? 2 : 120);
        const uint32_t big = rnd(n_seqs);
        std::vector<uint8_t> t;
        std::vector<uint64_t> so(1, 0);
        for (uint32_t j = 0; j < n_seqs; ++j) {
            const uint32_t kind = rnd(10);
            uint32_t len = kind == 0 ? 0 : kind < 3 ? rnd(L + 2) : kind < 5 ? L * (k + 1) - k - 1 + rnd(2 * k + 3) : 40 + rnd(260);
            if (j == big && it % 3 == 0) len = (1u << FZ_RAG_TILE_BITS) + rnd(300);
            const size_t at = t.size();
            for (uint32_t q = 0; q < len; ++q) t.push_back((uint8_t)(1 + rnd(sigma)));
            const uint32_t pi = rnd(np), m = (uint32_t)(offs[pi + 1] - offs[pi]);
            if (len >= m) {
                const uint32_t where = rnd(3) == 0 ? 0 : rnd(2) ? len - m : rnd(len - m + 1);
                memcpy(t.data() + at + where, pats.data() + offs[pi], m);
                if (rnd(2)) t[at + where + rnd(m)] = (uint8_t)(1 + rnd(sigma));
            }
            so.push_back(t.size());
        }
        for (uint32_t j = 1; j < n_seqs; ++j) {                // a copy cut in two by the seam in front of sequence j
            if (rnd(3)) continue;
            const uint32_t pi = rnd(np), m = (uint32_t)(offs[pi + 1] - offs[pi]), cut = 1 + rnd(m - 1);
            if (so[j] - so[j - 1] >= cut && so[j + 1] - so[j] >= m - cut) memcpy(t.data() + so[j] - cut, pats.data() + offs[pi], m);
        }
        t.push_back(0);                                        // (data() of an empty vector may be null)
        std::vector<Row> got, want, one;
        const long long rc = run_group(mode, pats.data(), offs.data(), np, k, L, t.data(), so.data(), n_seqs, got);
        if (rc < 0) { fprintf(stderr, "iteration %d: the group model answered %lld\n", it, rc); return 1; }
        for (uint32_t j = 0; j < n_seqs; ++j) {                // every sequence alone, copied out: a batch of one
            std::vector<uint8_t> alone(t.begin() + (ptrdiff_t)so[j], t.begin() + (ptrdiff_t)so[j + 1]);
            alone.push_back(0);
            const uint64_t o1[2] = {0, so[j + 1] - so[j]};
            const long long r1 = run_group(mode, pats.data(), offs.data(), np, k, L, alone.data(), o1, 1, one);
            if (r1 < 0) { fprintf(stderr, "iteration %d, sequence %u alone: %lld\n", it, j, r1); return 1; }
            for (Row r : one) { r.seq = j; want.push_back(r); }
        }
        std::stable_sort(want.begin(), want.end(), [](const Row &a, const Row &b) { return a.pid < b.pid; });
        bool same = got.size() == want.size();
        for (size_t i = 0; same && i < got.size(); ++i)
            same = got[i].pid == want[i].pid && got[i].seq == want[i].seq && got[i].g == want[i].g && got[i].start == want[i].start &&
                   got[i].end == want[i].end && got[i].dist == want[i].dist;
        if (!same) { fprintf(stderr, "iteration %d (mode %u, k %u, L %u): %zu rows in the batch, %zu alone\n", it, mode, k, L, got.size(), want.size()); return 1; }
        total += (long long)got.size();
    }
    printf("mp_batch_emul: %lld rows agree\n", total);
    return total > 200 ? 0 : 1;
}
#endif
