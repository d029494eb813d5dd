// Host model of fz_overlap_kernel (fuzzysearch_amd/csrc/fz_device.h compiled with g++): the kernel's control flow around the
// very functions its lanes run.  Per launch the tables of a chunk of patterns (lengths, rows, and for Levenshtein the two
// Peq tables per pattern, word by word through fz_overlap_peq_word); per wave of 64 reads the tails staged a dword at a time
// into the lane-transposed window (dword d of lane l at win[d * 64 + l]: fz_overlap_stage, fz_overlap_stage_copy), then
// fz_overlap_lane per lane, the maximum over the launches per read, and fz_overlap_row.  The packed reads lie in an
// allocation of exactly their size rounded up to a dword, filled behind the data with a byte that the patterns also hold, so
// that a sanitizer build sees a load beyond it and a compared padding byte shows as a wrong answer.
// A stand-alone program: overlap_emul <cases> reads groups of
//   u32 mode, k, min_overlap, n_pats, n_reads, pad byte; n_pats x (u32 m, m bytes); n_reads x u32 length; the packed reads
// and prints one line "pattern overlap dist start" per read.  Exit status 0 unless the file is malformed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../fuzzysearch_amd/csrc/fz_device.h"

namespace {
bool take(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

template <uint32_t MODE>
void run_group(const std::vector<std::vector<uint8_t>> &pats, const std::vector<uint64_t> &offs, const uint8_t *buf, uint64_t buf_len,
               uint32_t k, uint32_t o, std::vector<uint64_t> &table) {
    const uint32_t n_pats = (uint32_t)pats.size(), chunk = fz_overlap_chunk(MODE);
    const uint64_t n_seqs = offs.size() - 1;
    for (uint32_t p0 = 0; p0 < n_pats; p0 += chunk) {
        const uint32_t npat = n_pats - p0 < chunk ? n_pats - p0 : chunk;
        std::vector<uint32_t> pm(npat), rows(npat * (FZ_OVL_ROW_BYTES / 4u), 0u);
        std::vector<uint64_t> peq(MODE == FZ_MODE_LEV ? npat * 512u : 0u);
        uint32_t tmax = 0;
        for (uint32_t i = 0; i < npat; ++i) {
            const std::vector<uint8_t> &p = pats[p0 + i];
            pm[i] = (uint32_t)p.size();
            memcpy(reinterpret_cast<uint8_t *>(rows.data()) + i * FZ_OVL_ROW_BYTES, p.data(), p.size());
            const uint32_t t = fz_overlap_tail(MODE, pm[i], k);
            if (t > tmax) tmax = t;
            for (uint32_t w = 0; w < (uint32_t)peq.size() / npat; ++w)
                peq[i * 512u + w] = fz_overlap_peq_word(reinterpret_cast<const uint8_t *>(rows.data()) + i * FZ_OVL_ROW_BYTES, pm[i], w & 255u, w >> 8);
        }
        const FzOvlTabs tb{pm.data(), rows.data(), peq.data()};
        const uint32_t win_dwords = fz_overlap_win_dwords(tmax);
        std::vector<uint32_t> win(win_dwords * 64u);
        for (uint64_t g = 0; g < n_seqs; g += 64u) {
            FzOvlStage st[64];
            for (uint32_t lane = 0; lane < 64u && g + lane < n_seqs; ++lane) {
                st[lane] = fz_overlap_stage(offs[g + lane], offs[g + lane + 1], tmax, buf_len);
                fz_overlap_stage_copy(buf, st[lane], win_dwords, win.data() + lane, 64u);
            }
            for (uint32_t lane = 0; lane < 64u && g + lane < n_seqs; ++lane) {
                const uint32_t n = (uint32_t)(offs[g + lane + 1] - offs[g + lane]);
                const uint64_t key = fz_overlap_lane<MODE>(tb, win.data() + lane, 64u, st[lane], n, p0, npat, k, o);
                if (key > table[g + lane]) table[g + lane] = key;
            }
        }
    }
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: overlap_emul <cases>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t head[6];
    while (fread(head, 1, sizeof head, f) == sizeof head) {
        const uint32_t mode = head[0], k = head[1], o = head[2], n_pats = head[3], n_reads = head[4], pad = head[5];
        std::vector<std::vector<uint8_t>> pats(n_pats);
        for (auto &p : pats) {
            uint32_t m = 0;
            if (!take(f, &m, 4) || m == 0 || m > FZ_OVL_MAX_M) { fprintf(stderr, "bad pattern\n"); return 2; }
            p.resize(m);
            if (!take(f, p.data(), m)) { fprintf(stderr, "short file\n"); return 2; }
        }
        std::vector<uint32_t> lens(n_reads);
        if (!take(f, lens.data(), 4ull * n_reads)) { fprintf(stderr, "short file\n"); return 2; }
        std::vector<uint64_t> offs(n_reads + 1, 0);
        for (uint32_t j = 0; j < n_reads; ++j) offs[j + 1] = offs[j] + lens[j];
        const uint64_t total = offs[n_reads], padded = (total + 3u) & ~(uint64_t)3;
        uint8_t *buf = static_cast<uint8_t *>(malloc(padded ? padded : 1u));
        if (!take(f, buf, total)) { fprintf(stderr, "short file\n"); return 2; }
        memset(buf + total, (int)pad, padded - total);
        std::vector<uint64_t> table(n_reads, 0);
        if (mode == FZ_MODE_LEV) run_group<FZ_MODE_LEV>(pats, offs, buf, total, k, o, table);
        else run_group<FZ_MODE_SUBS>(pats, offs, buf, total, k, o, table);
        for (uint32_t j = 0; j < n_reads; ++j) {
            const FzOverlapRow r = fz_overlap_row(table[j], lens[j]);
            printf("%u %u %u %u\n", (unsigned)r.pattern, (unsigned)r.overlap, (unsigned)r.dist, (unsigned)r.start);
        }
        free(buf);
    }
    fclose(f);
    return 0;
}
