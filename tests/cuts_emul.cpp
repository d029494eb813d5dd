// Host model of fz_cuts_kernel (fuzzysearch_amd/csrc/fz_device.h compiled with g++): the kernel's control flow around the
// very functions its lanes run.  Per wave of 64 reads and per requested side the lanes begin (fz_cuts_begin); while any of
// them is live, every lane stages its next piece a dword at a time into the lane-transposed window (dword d of lane l at
// win[d * 64 + l]: fz_cuts_piece, fz_stage_copy<false>) and then walks it (fz_cuts_lane); fz_cuts_row makes the row.  The
// window is filled with a poison dword before every piece, so a lane that read a dword it had not staged would score it.
// The packed reads lie in an allocation of exactly their size rounded up to a dword, filled behind the data with a byte that
// the tables give their highest score, so that a sanitizer build sees a load beyond it and a scored padding byte shows as
// a wrong answer.  Every group is run twice: with the bounded exit (s + remaining * wmax <= best), as the kernel runs, and
// with the bound disabled.
// A stand-alone program: cuts_emul <cases> reads groups of
//   u32 sides (bit 0: 3', bit 1: 5'), flags, rate_num, rate_den, n_reads, pad byte; per requested side 256 x i16;
//   n_reads x u32 length; the packed reads
// and prints one line "start end start_unbounded end_unbounded" per read.  Exit status 0 unless the file is malformed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../fuzzysearch_amd/csrc/fz_device.h"

namespace {
bool take(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

void run_group(const int16_t *tabs, uint32_t sides, uint32_t flags, uint32_t num, uint32_t den, const std::vector<uint64_t> &offs,
               const uint8_t *buf, uint64_t buf_len, uint32_t bounded, std::vector<FzCutRow> &rows) {
    const uint64_t n_seqs = offs.size() - 1;
    std::vector<uint32_t> win(FZ_CUT_PIECE_DWORDS * 64u);
    for (uint64_t g = 0; g < n_seqs; g += 64u) {
        const uint32_t lanes = n_seqs - g < 64u ? (uint32_t)(n_seqs - g) : 64u;
        uint32_t trim[2][64] = {};
        for (uint32_t side = 0; side < 2u; ++side) {
            if (!((sides >> side) & 1u)) continue;
            const int16_t *w = tabs + 256u * side;
            int32_t wmax = w[0];
            for (uint32_t c = 1; c < 256u; ++c)
                if (w[c] > wmax) wmax = w[c];
            if (wmax <= 0) continue;                        // (the call walks no such side)
            const FzCutRule r = fz_cuts_rule(side, flags, num, den, wmax, bounded);
            FzCutState st[64];
            FzOvlStage piece[64];
            bool any = false;
            for (uint32_t lane = 0; lane < lanes; ++lane) {
                st[lane] = fz_cuts_begin((uint32_t)(offs[g + lane + 1] - offs[g + lane]), r);
                any = any || st[lane].live;
            }
            while (any) {                                   // the wave's ballot
                for (uint32_t &x : win) x = 0xa5a5a5a5u;
                for (uint32_t lane = 0; lane < lanes; ++lane) {
                    piece[lane] = fz_cuts_piece(st[lane], offs[g + lane], offs[g + lane + 1], side, buf_len);
                    if (piece[lane].nd > FZ_CUT_PIECE_DWORDS) { fprintf(stderr, "a piece of %u dwords\n", piece[lane].nd); exit(3); }
                    fz_stage_copy<false>(buf, piece[lane], FZ_CUT_PIECE_DWORDS, win.data() + lane, 64u);
                }
                any = false;
                for (uint32_t lane = 0; lane < lanes; ++lane) {
                    const uint32_t before = st[lane].walked, was_live = st[lane].live;
                    fz_cuts_lane(st[lane], w, win.data() + lane, 64u, piece[lane], (uint32_t)(offs[g + lane + 1] - offs[g + lane]), side, r);
                    if (was_live && st[lane].live && st[lane].walked == before) { fprintf(stderr, "a live lane that does not move\n"); exit(3); }
                    any = any || st[lane].live;
                }
            }
            for (uint32_t lane = 0; lane < lanes; ++lane) trim[side][lane] = st[lane].trim;
        }
        for (uint32_t lane = 0; lane < lanes; ++lane)
            rows[g + lane] = fz_cuts_row((uint32_t)(offs[g + lane + 1] - offs[g + lane]), trim[0][lane], trim[1][lane], sides);
    }
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: cuts_emul <cases>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t head[6];
    while (fread(head, 1, sizeof head, f) == sizeof head) {
        const uint32_t sides = head[0], flags = head[1], num = head[2], den = head[3], n_reads = head[4], pad = head[5];
        if (sides == 0 || sides > 3u) { fprintf(stderr, "bad sides\n"); return 2; }
        int16_t tabs[512] = {};
        for (uint32_t side = 0; side < 2u; ++side)
            if (((sides >> side) & 1u) && !take(f, tabs + 256u * side, 512)) { fprintf(stderr, "short file\n"); return 2; }
        std::vector<uint32_t> lens(n_reads);
        if (!take(f, lens.data(), 4ull * n_reads)) { fprintf(stderr, "short file\n"); return 2; }
        std::vector<uint64_t> offs(n_reads + 1, 0);
        for (uint32_t j = 0; j < n_reads; ++j) offs[j + 1] = offs[j] + lens[j];
        const uint64_t total = offs[n_reads], padded = (total + 3u) & ~(uint64_t)3;
        uint8_t *buf = static_cast<uint8_t *>(malloc(padded ? padded : 1u));
        if (!take(f, buf, total)) { fprintf(stderr, "short file\n"); return 2; }
        memset(buf + total, (int)pad, padded - total);
        std::vector<FzCutRow> bounded(n_reads), unbounded(n_reads);
        run_group(tabs, sides, flags, num, den, offs, buf, total, 1u, bounded);
        run_group(tabs, sides, flags, num, den, offs, buf, total, 0u, unbounded);
        for (uint32_t j = 0; j < n_reads; ++j)
            printf("%u %u %u %u\n", (unsigned)bounded[j].start, (unsigned)bounded[j].end, (unsigned)unbounded[j].start, (unsigned)unbounded[j].end);
        free(buf);
    }
    fclose(f);
    return 0;
}
