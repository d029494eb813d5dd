// Host model of a whole multi-pattern group with symbol classes (fuzzysearch_amd/csrc/fz_device.h compiled with g++): the
// class table (fz_mp_build_cls), the filter's lookup at every byte offset as fz_mp_filter_kernel does it, then — per reported
// (offset, block-table entry), as fz_mp_verify_cls_kernel does it per lane — the block's hit range (fz_block_range), the
// window staged as aligned dwords, the class-exact n-gram test (fz_mp_block_match_cls) and the class mismatches outside the
// block (fz_mp_verify_cls), the pattern and mask rows read with the descriptor's stride.
// tests/test_multi_classes_host.py holds the rows against a brute-force model.
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../fuzzysearch_amd/csrc/fz_device.h"

namespace {
struct StagedWindow {                                      // a lane's LDS column: dword j of the staged window
    const uint32_t *d;
    uint32_t dword(uint32_t j) const { return d[j]; }
};
struct Row { uint32_t pid, g; uint64_t idx; int64_t start, end; uint32_t dist; };
}

extern "C" {

// pats / offs: npat patterns back to back, all with len / (k + 1) == L and inside the batched domain; pmask / tmask: the
// class tables.  Every row of every pattern is written to out as {pattern, block, start, end, dist} in the order the filter
// and the table produce them (NOT sorted, not deduplicated: a duplicate would be the table's fault and must show): at most
// cap rows; -> the number of rows, -1 when the group does not fit a table, -2 when a staged read would leave the window area.
// pad: what lies in the bytes behind the text (the staging of the last windows brings up to 3 of them along).
long long mp_cls_emul_group(const uint8_t *pats, const uint64_t *offs, uint32_t npat, uint32_t k, uint32_t L, const uint8_t *pmask,
                            const uint8_t *tmask, const uint8_t *t, uint64_t n, uint8_t pad, int64_t *out, long long cap,
                            uint32_t *n_entries) {
    if (npat == 0 || npat > FZ_MP_MAX_PATS || L < FZ_MP_MIN_L) return -1;
    const uint8_t *pp[FZ_MP_MAX_PATS];
    uint32_t pm[FZ_MP_MAX_PATS], max_m = 0;
    for (uint32_t i = 0; i < npat; ++i) {
        pp[i] = pats + offs[i];
        pm[i] = (uint32_t)(offs[i + 1] - offs[i]);
        if (pm[i] > FZ_MP_MAX_M || pm[i] / (k + 1) != L) return -1;
        max_m = std::max(max_m, pm[i]);
    }
    std::vector<uint32_t> desc(FZ_MP_CLS_DESC_WORDS);
    const uint32_t nent = fz_mp_build_cls(desc.data(), pp, pm, npat, L, pmask, tmask);
    if (nent == 0) return -1;
    if (n_entries) *n_entries = nent;
    std::vector<uint8_t> store(((n + 3) & ~(uint64_t)3) + 16, pad);
    uint8_t *buf = store.data();
    if (n) memcpy(buf, t, n);
    const uint32_t *sig = desc.data(), *slots = desc.data() + FZ_MP_DESC_SLOTS, *ent = desc.data() + FZ_MP_DESC_ENT;
    const uint32_t *pmt = desc.data() + FZ_MP_DESC_M, *pat4 = desc.data() + FZ_MP_DESC_PAT, *msk4 = desc.data() + FZ_MP_CLS_DESC_MASK;
    const uint8_t *tm = reinterpret_cast<const uint8_t *>(desc.data() + FZ_MP_CLS_DESC_TMASK);
    const uint32_t win_dwords = (max_m + 3) / 4 + 1, m_max = (win_dwords - 1) * 4;
    std::vector<uint32_t> win(win_dwords);
    std::vector<Row> rows;
    for (uint64_t idx = 0; idx + L <= n; ++idx) {
        const uint32_t h = fz_mp_hash_bytes(buf + idx, L);
        if (!fz_mp_sig_test(sig, h)) continue;
        const uint32_t run = fz_mp_lookup(slots, h);
        for (uint32_t j = 0; j < (run >> 16); ++j) {
            const uint32_t e = ent[(run & 0xffffu) + j];
            const uint32_t pid = e & (FZ_MP_MAX_PATS - 1u), g = (e >> 8) & 0xffu, s = e >> 16;
            const uint32_t m = pmt[pid];
            uint32_t lo_rel, hi_sub;
            fz_block_range(FZ_MODE_SUBS, m, k, L, s, lo_rel, hi_sub);
            bool valid = m != 0u && m <= m_max && s + L <= m && idx >= lo_rel && n >= hi_sub && idx + L <= n - hi_sub;
            if (!valid) continue;
            const uint64_t i0 = idx - s, wbase = i0 & ~(uint64_t)3;
            const uint32_t sh = (uint32_t)(i0 - wbase);
            uint32_t nd = (uint32_t)((i0 + m - wbase + 3) >> 2);
            if (nd > win_dwords) return -2;
            for (uint32_t d = 0; d < win_dwords; ++d) {
                uint32_t x = 0;
                if (d < nd) memcpy(&x, buf + wbase + 4u * d, 4);
                win[d] = x;
            }
            const StagedWindow w{win.data()};
            const uint32_t *p4 = pat4 + pid * (FZ_MP_MAX_M / 4u), *k4 = msk4 + pid * (FZ_MP_MAX_M / 4u);
            valid = fz_mp_block_match_cls(w, sh, p4, k4, 1u, tm, L, s);
            FzRec rec;
            if (!fz_mp_verify_cls(w, sh, p4, k4, 1u, tm, m, m_max, k, L, s, valid, rec)) continue;
            rows.push_back(Row{pid, g, idx, (int64_t)idx - (int64_t)rec.l, (int64_t)(idx + L + rec.r), rec.dist});
        }
    }
    long long c = 0;
    for (const Row &r : rows) {
        if (c < cap) { out[5 * c] = r.pid; out[5 * c + 1] = r.g; out[5 * c + 2] = r.start; out[5 * c + 3] = r.end; out[5 * c + 4] = r.dist; }
        ++c;
    }
    return c;
}

// The distinct hashes over the spellings of one block (fz_mp_cls_block_hashes) -> their number (cap + 1: more than cap).
uint32_t mp_cls_emul_block_hashes(const uint8_t *w, uint32_t L, const uint8_t *pmask, const uint8_t *tmask, uint32_t *hs, uint32_t cap) {
    return fz_mp_cls_block_hashes(w, L, pmask, tmask, hs, cap);
}

uint32_t mp_cls_emul_hash(const uint8_t *w, uint32_t L) { return fz_mp_hash_bytes(w, L); }
}
