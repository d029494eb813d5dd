// Host model of fz_format_gather_kernel (fuzzysearch_amd/csrc/fz_device.h compiled with g++): the destination cut into 16-byte
// pieces, every piece's record found by the search over at[] and its segment by the walk (fz_format_seek), a piece inside
// one column segment filled by ONE 16-byte load at the address rule's position (fz_format_run, fz_format_run_lo), every
// other piece filled byte by byte under the moving cursor (fz_format_settle, fz_format_byte_src) — the kernel's control
// flow, statement by statement.  Every load from a column goes through a checked accessor: a byte outside the sequence
// of the record it is loaded for is an error, whatever lies there, as if guard bytes stood around every sequence; and every
// column's bytes lie in an allocation of exactly their size, so that a sanitizer build sees a load beyond them too.
// A stand-alone program: for C = 1 .. 3 columns, literal lengths 0, 1, 3 and 17 in every rotation, every source alignment
// 0 .. 15, every destination alignment 0 .. 15 and segment lengths 0 .. 40, the text equals the three-line model's join.
// Exit status 0 and "ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../fuzzysearch_amd/csrc/fz_device.h"

namespace {
struct Column {
    uint8_t *alloc = nullptr;                              // shift + total bytes, exactly
    uint8_t *bytes = nullptr;                              // alloc + shift: the source alignment
    std::vector<uint64_t> offs;
};

long long g_bad = 0;

// cnt bytes at p for record j of column c: inside that sequence, or an error.
void load(const FzFmtDesc &d, uint32_t c, uint64_t j, const uint8_t *p, uint32_t cnt, uint8_t *dst) {
    const uint8_t *lo = d.col[c].bytes + d.col[c].offs[j], *hi = d.col[c].bytes + d.col[c].offs[j + 1];
    if (p < lo || p + cnt > hi) { ++g_bad; memset(dst, 0xEE, cnt); return; }
    memcpy(dst, p, cnt);
}

// The kernel over one destination: at[] (n + 1 entries) -> text[0 .. total).
void gather(const FzFmtDesc &sd, const std::vector<uint64_t> &at, uint64_t n, std::vector<uint8_t> &text) {
    const uint64_t total = at[n];
    const uint64_t *ends = at.data() + 1;
    text.assign((total + 15u) / 16u * 16u, 0xCC);
    for (uint64_t p0 = 0; p0 < total; p0 += 16u) {
        uint64_t p = p0, lo = 0, hi = n - 1u;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (ends[mid] > p) hi = mid; else lo = mid + 1u;
        }
        uint64_t j = lo;
        FzFmtCur g = fz_format_seek(sd, j, p - at[j]);
        if (fz_format_run(g, 16u)) {
            load(sd, g.seg >> 1, j, sd.col[g.seg >> 1].bytes + fz_format_run_lo(sd, j, g), 16u, text.data() + p);
        } else {
            const uint64_t pe = p + 16u < total ? p + 16u : total;
            for (; p < pe; ++p) {
                fz_format_settle(sd, j, g);
                const uint8_t *src = fz_format_byte_src(sd, j, g);
                if (g.seg & 1u) load(sd, g.seg >> 1, j, src, 1u, &text[p]);
                else if (src < sd.lits || src >= sd.lits + sd.lit_off[sd.n_cols + 1u]) { ++g_bad; text[p] = 0xEE; }
                else text[p] = *src;
                ++g.off;
            }
        }
    }
}
}  // namespace

int main() {
    static const uint32_t LITS[4] = {0u, 1u, 3u, 17u};
    long long cases = 0, failures = 0;
    for (uint32_t C = 1; C <= 3; ++C)
        for (uint32_t rot = 0; rot < 4; ++rot)
            for (uint32_t sa = 0; sa < 16; ++sa)
                for (uint32_t da = 0; da < 16; ++da)
                    for (uint32_t len = 0; len <= 40; ++len) {
                        const uint64_t n = 3;
                        const long long before = g_bad;
                        // three records: one that sets the destination alignment, the one under test, a ragged last one
                        const uint64_t lens[3][3] = {{da, 2u, 0u}, {len, (len + 7u) % 41u, (len + 14u) % 41u}, {21u, 0u, 33u}};
                        FzFmtDesc d;
                        memset(&d, 0, sizeof d);
                        d.n_cols = C; d.equal_a = d.equal_b = FZ_FMT_NO_CHECK;
                        uint32_t lat = 0;
                        for (uint32_t c = 0; c <= C; ++c) {
                            d.lit_off[c] = lat;
                            for (uint32_t i = 0; i < LITS[(rot + c) % 4u]; ++i) d.lits[lat++] = (uint8_t)(0x80u + c * 31u + i);
                        }
                        d.lit_off[C + 1u] = lat;
                        Column cols[3];
                        for (uint32_t c = 0; c < C; ++c) {
                            Column &k = cols[c];
                            k.offs = {0u, lens[0][c], lens[0][c] + lens[1][c], lens[0][c] + lens[1][c] + lens[2][c]};
                            const uint32_t shift = (sa + 5u * c) % 16u;
                            const uint64_t exact = shift + k.offs[3];          // (malloc's start is 16-byte aligned)
                            k.alloc = static_cast<uint8_t *>(malloc(exact ? exact : 1u));
                            k.bytes = k.alloc + shift;
                            for (uint64_t i = 0; i < k.offs[3]; ++i) k.bytes[i] = (uint8_t)(i * 37u + 11u + c * 3u);
                            d.col[c].bytes = k.bytes;
                            d.col[c].offs = k.offs.data();
                        }
                        std::vector<uint64_t> at(n + 1, 0);
                        std::vector<uint8_t> want, got;
                        for (uint64_t j = 0; j < n; ++j) {
                            at[j] = want.size();
                            const FzFmtRec r = fz_format_record(d, j);
                            for (uint32_t c = 0; c <= C; ++c) {
                                want.insert(want.end(), d.lits + d.lit_off[c], d.lits + d.lit_off[c + 1u]);
                                if (c < C) want.insert(want.end(), cols[c].bytes + cols[c].offs[j], cols[c].bytes + cols[c].offs[j + 1]);
                            }
                            if (at[j] + r.len != want.size()) ++g_bad;         // the measure's length is the join's
                        }
                        at[n] = want.size();
                        if (at[n]) gather(d, at, n, got);
                        ++cases;
                        const bool differ = at[n] && memcmp(want.data(), got.data(), want.size()) != 0;
                        if (g_bad != before || differ) {
                            if (++failures <= 10)
                                fprintf(stderr, "C=%u rot=%u sa=%u da=%u len=%u: %lld loads outside their sequence, bytes %s\n", C, rot, sa, da, len,
                                        g_bad - before, differ ? "differ" : "equal");
                        }
                        for (uint32_t c = 0; c < C; ++c) free(cols[c].alloc);
                    }
    if (failures || g_bad) { fprintf(stderr, "%lld of %lld cases failed\n", failures, cases); return 1; }
    printf("ok %lld\n", cases);
    return 0;
}
