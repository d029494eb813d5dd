// Host model of a whole substitutions-only multi-pattern group (fuzzysearch_amd/csrc/fz_device.h compiled with g++): the
// group's table (fz_mp_build), the filter's lookup at every byte offset as fz_mp_filter_kernel does it, then — per reported
// (offset, block-table entry), as fz_mp_verify_subs_kernel does it per lane — the block's hit range (fz_block_range), the
// window staged as aligned dwords, the exact n-gram test (fz_mp_block_equal) and the mismatch count outside the block
// (fz_mp_verify_subs).  tests/test_multi_subs_host.py holds the rows against the oracle's stream for every pattern.
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

// pats / offs: npat patterns back to back, all with len / (k + 1) == L and inside the batched domain.  Every row of every
// pattern is written to out as {pattern, block, start, end, dist}, ordered by (pattern, block, index): at most cap rows;
// -> the number of rows, -1 when the group does not fit a table, -2 when a staged read would leave the window area.
long long mp_subs_emul_group(const uint8_t *pats, const uint64_t *offs, uint32_t npat, uint32_t k, uint32_t L, const uint8_t *t,
                             uint64_t n, int64_t *out, long long cap) {
    if (npat == 0 || npat > FZ_MP_MAX_PATS || L < FZ_MP_MIN_L) return -1;
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
    // the resident layout: zero padding behind the data (halo loads and the last dword of a window read into it)
    std::vector<uint8_t> buf(((n + 3) & ~(uint64_t)3) + 16, 0);
    if (n) memcpy(buf.data(), t, n);
    const uint32_t *sig = desc.data(), *slots = desc.data() + FZ_MP_DESC_SLOTS, *ent = desc.data() + FZ_MP_DESC_ENT;
    const uint32_t *pmt = desc.data() + FZ_MP_DESC_M, *pat4 = desc.data() + FZ_MP_DESC_PAT;
    const uint32_t win_dwords = (max_m + 3) / 4 + 1, m_max = (win_dwords - 1) * 4;          // mp_run_shard / the kernel
    std::vector<uint32_t> win(win_dwords);
    std::vector<Row> rows;
    for (uint64_t idx = 0; idx + L <= n; ++idx) {
        const uint32_t h = fz_mp_hash_bytes(buf.data() + idx, L);
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
                if (d < nd) memcpy(&x, buf.data() + wbase + 4u * d, 4);
                win[d] = x;
            }
            const StagedWindow w{win.data()};
            const uint32_t *p4 = pat4 + pid * (FZ_MP_MAX_M / 4u);
            valid = fz_mp_block_equal(w, sh, p4, 1u, L, s);
            FzRec rec;
            if (!fz_mp_verify_subs(w, sh, p4, 1u, m, m_max, k, L, s, valid, rec)) continue;
            rows.push_back(Row{pid, g, idx, (int64_t)idx - (int64_t)rec.l, (int64_t)(idx + L + rec.r), rec.dist});
        }
    }
    std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) {
        if (a.pid != b.pid) return a.pid < b.pid;
        if (a.g != b.g) return a.g < b.g;
        return a.idx < b.idx;
    });
    long long c = 0;
    for (const Row &r : rows) {
        if (c < cap) { out[5 * c] = r.pid; out[5 * c + 1] = r.g; out[5 * c + 2] = r.start; out[5 * c + 3] = r.end; out[5 * c + 4] = r.dist; }
        ++c;
    }
    return c;
}
}
