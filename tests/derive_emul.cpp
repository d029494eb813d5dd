// Host model of fz_derive_gather_kernel (fuzzysearch_amd/csrc/fz_device.h compiled with g++): the destination cut into 16-byte
// pieces, every piece's output found by the search over at[], a piece inside one output filled by ONE 16-byte load at the
// address rule's position (fz_derive_piece_lo), turned round by fz_derive_rev16 and sent through fz_derive_xlat4, a piece
// across an output's end filled byte by byte (fz_derive_byte_src) — the kernel's control flow, statement by statement.
// Every load goes through a checked accessor: a byte outside [src[j], src[j] + len) of the output it is loaded for is an
// error, whatever lies there.  A stand-alone program: for every source alignment 0..15, output alignment 0..15, length 0..48,
// both directions, with and without a table, the packed bytes equal the three-line model's.  Exit status 0 and "ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../fuzzysearch_amd/csrc/fz_device.h"

namespace {
struct Checked {
    const std::vector<uint8_t> &raw;
    uint64_t lo = 0, hi = 0;                               // the source range of the output being filled
    long long bad = 0;
    void load(uint64_t pos, uint32_t cnt, uint8_t *dst) {
        if (pos < lo || pos + cnt > hi || pos + cnt > raw.size()) { ++bad; memset(dst, 0xEE, cnt); return; }
        memcpy(dst, raw.data() + pos, cnt);
    }
};

// The kernel over one destination: at[] (n + 1 entries), src[] (n entries) -> packed[0 .. total).
long long gather(const std::vector<uint8_t> &raw, const std::vector<uint64_t> &src, const std::vector<uint64_t> &at, bool rev,
                 const uint8_t *table, std::vector<uint8_t> &packed) {
    const uint64_t n_seqs = src.size(), total = at[n_seqs];
    const uint64_t *ends = at.data() + 1;
    Checked mem{raw};
    packed.assign((total + 15u) / 16u * 16u, 0xCC);
    for (uint64_t p0 = 0; p0 < total; p0 += 16u) {
        uint64_t p = p0, lo = 0, hi = n_seqs - 1u;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (ends[mid] > p) hi = mid; else lo = mid + 1u;
        }
        uint64_t j = lo;
        if (p + 16u <= ends[j]) {
            const uint64_t len = ends[j] - at[j];
            mem.lo = src[j]; mem.hi = src[j] + len;
            uint32_t v[4];
            uint8_t b[16];
            mem.load(fz_derive_piece_lo(src[j], len, p - at[j], 16u, rev), 16u, b);
            memcpy(v, b, 16);
            if (rev) fz_derive_rev16(v[0], v[1], v[2], v[3]);
            if (table) for (uint32_t &w : v) w = fz_derive_xlat4(table, w);
            memcpy(packed.data() + p, v, 16);
        } else {
            const uint64_t pe = p + 16u < total ? p + 16u : total;
            for (; p < pe; ++p) {
                while (ends[j] <= p) ++j;
                const uint64_t len = ends[j] - at[j];
                mem.lo = src[j]; mem.hi = src[j] + len;
                uint8_t c;
                mem.load(fz_derive_byte_src(src[j], len, p - at[j], rev), 1u, &c);
                packed[p] = table ? table[c] : c;
            }
        }
    }
    return mem.bad;
}
}  // namespace

int main() {
    uint8_t table[256];
    for (uint32_t c = 0; c < 256; ++c) table[c] = (uint8_t)(c * 7u + 3u);     // a permutation of the bytes
    long long cases = 0, failures = 0;
    for (uint32_t sa = 0; sa < 16; ++sa)
        for (uint32_t da = 0; da < 16; ++da)
            for (uint32_t len = 0; len <= 48; ++len) {
                // the parent's bytes: a neighbour of 40 + sa bytes, the item, a neighbour of 40; every byte its own value
                std::vector<uint8_t> raw(40u + sa + len + 40u);
                for (size_t i = 0; i < raw.size(); ++i) raw[i] = (uint8_t)(i * 37u + 11u);
                // three outputs: da bytes of the first neighbour, the item, 21 bytes of the second (its end is a ragged piece)
                const std::vector<uint64_t> src = {3u, 40u + sa, 40u + sa + len + 5u};
                const std::vector<uint64_t> lens = {da, len, 21u};
                std::vector<uint64_t> at = {0u, da, (uint64_t)da + len, (uint64_t)da + len + 21u};
                for (int rev = 0; rev < 2; ++rev)
                    for (int xl = 0; xl < 2; ++xl) {
                        std::vector<uint8_t> want, got;
                        for (size_t j = 0; j < src.size(); ++j)
                            for (uint64_t q = 0; q < lens[j]; ++q) {
                                const uint8_t c = raw[src[j] + (rev ? lens[j] - 1u - q : q)];
                                want.push_back(xl ? table[c] : c);
                            }
                        const long long bad = gather(raw, src, at, rev != 0, xl ? table : nullptr, got);
                        ++cases;
                        if (bad || want.size() != at[3] || memcmp(want.data(), got.data(), want.size()) != 0) {
                            if (++failures <= 10)
                                fprintf(stderr, "sa=%u da=%u len=%u rev=%d xlat=%d: %lld loads outside the item, bytes %s\n", sa, da, len, rev, xl,
                                        bad, memcmp(want.data(), got.data(), want.size()) ? "differ" : "equal");
                        }
                    }
            }
    if (failures) { fprintf(stderr, "%lld of %lld cases failed\n", failures, cases); return 1; }
    printf("ok %lld\n", cases);
    return 0;
}
