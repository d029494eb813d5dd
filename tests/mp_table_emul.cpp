// Host model of the multi-pattern filter's table (fuzzysearch_amd/csrc/fz_device.h: fz_mp_*): the very functions the
// HIP kernel runs per byte offset — window hash, signature bit, slot lookup — compiled with g++ and driven over a text
// offset by offset, the way fz_mp_filter_kernel does.  tests/test_multi_host.py holds the result against a plain
// comparison of every block of every pattern at every offset: no occurrence may be missing.
#include <cstddef>
#include <cstring>
#include <vector>

#include "../fuzzysearch_amd/csrc/fz_device.h"

extern "C" {

// pats / offs: npat patterns back to back (all inside the batched domain for this L).  Every (offset, entry) the filter
// reports for text t is written to out as {offset, pattern, block}: at most cap triples; -> the number reported, or -1
// when the group does not fit a table.
long long mp_emul_scan(const uint8_t *pats, const uint64_t *offs, uint32_t npat, uint32_t L, const uint8_t *t, uint64_t n,
                       uint64_t *out, long long cap) {
    if (npat > FZ_MP_MAX_PATS || L < FZ_MP_MIN_L) return -1;
    const uint8_t *pp[FZ_MP_MAX_PATS];
    uint32_t pm[FZ_MP_MAX_PATS];
    for (uint32_t i = 0; i < npat; ++i) { pp[i] = pats + offs[i]; pm[i] = (uint32_t)(offs[i + 1] - offs[i]); }
    std::vector<uint32_t> desc(FZ_MP_DESC_WORDS);
    const uint32_t nent = fz_mp_build(desc.data(), pp, pm, npat, L);
    if (nent == 0) return -1;
    // the resident layout: zero padding behind the data (the kernel's halo loads read into it)
    std::vector<uint8_t> buf(n + 16, 0);
    if (n) memcpy(buf.data(), t, n);
    const uint32_t *sig = desc.data(), *slots = desc.data() + FZ_MP_DESC_SLOTS, *ent = desc.data() + FZ_MP_DESC_ENT;
    long long cnt = 0;
    for (uint64_t i = 0; i + L <= n; ++i) {
        const uint32_t h = fz_mp_hash_bytes(buf.data() + i, L);
        if (!fz_mp_sig_test(sig, h)) continue;
        const uint32_t e = fz_mp_lookup(slots, h);
        for (uint32_t j = 0; j < (e >> 16); ++j) {
            const uint32_t en = ent[(e & 0xffffu) + j];
            if (cnt < cap) { out[3 * cnt] = i; out[3 * cnt + 1] = en & 0xffu; out[3 * cnt + 2] = (en >> 8) & 0xffu; }
            ++cnt;
        }
    }
    return cnt;
}

// The block start an entry carries must be block * L, and the pattern table must hold the patterns: -> 0 when it does.
int mp_emul_check_tables(const uint8_t *pats, const uint64_t *offs, uint32_t npat, uint32_t L) {
    const uint8_t *pp[FZ_MP_MAX_PATS];
    uint32_t pm[FZ_MP_MAX_PATS];
    if (npat > FZ_MP_MAX_PATS) return -1;
    for (uint32_t i = 0; i < npat; ++i) { pp[i] = pats + offs[i]; pm[i] = (uint32_t)(offs[i + 1] - offs[i]); }
    std::vector<uint32_t> desc(FZ_MP_DESC_WORDS);
    const uint32_t nent = fz_mp_build(desc.data(), pp, pm, npat, L);
    if (nent == 0) return -1;
    for (uint32_t j = 0; j < nent; ++j) {
        const uint32_t en = desc[FZ_MP_DESC_ENT + j], pid = en & 0xffu, g = (en >> 8) & 0xffu, s = en >> 16;
        if (pid >= npat || s != g * L || s + L > pm[pid]) return 1;
    }
    for (uint32_t i = 0; i < npat; ++i) {
        if (desc[FZ_MP_DESC_M + i] != pm[i]) return 2;
        if (memcmp(reinterpret_cast<const uint8_t *>(desc.data() + FZ_MP_DESC_PAT) + i * FZ_MP_MAX_M, pp[i], pm[i]) != 0) return 3;
    }
    return 0;
}
}
