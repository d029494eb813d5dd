// Host run of the scan kernel's tile walk (fuzzysearch_amd/csrc/fz_device.h compiled with g++): fz_scan_walk / fz_walk_tile,
// the very functions fz_scan_kernel and fz_debug_scan_walk call.  A stand-alone program: scan_walk_emul <cases> reads lines
//   ntiles grid n_regions {first workgroup, workgroups, first tile, end tile} x n_regions
// (a plan as fz_debug_scan_plan returns it) and walks every workgroup of the grid forward and reversed.  Per case it checks
// that every tile of the buffer is read by exactly one (workgroup, iteration) in each direction, that the reversed walk is
// the mirror of the forward one step by step, and that no workgroup has more iterations than a queue code can carry; the
// owner tables have exactly `ntiles` entries, so a sanitizer build sees a tile outside the buffer as a store out of bounds.
// Prints one line "ntiles grid steps max_iterations" per case.  Exit status 0 unless a check fails or the file is malformed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../fuzzysearch_amd/csrc/fz_device.h"

namespace {
constexpr uint32_t kTiterMax = (1u << (32 - 14 - FZ_BLK_BITS)) - 1;     // fz_kernels.h: FZ_TITER_MAX (FZ_TILE_BITS = 14)

int fail(const char *what, uint64_t ntiles, uint32_t grid, uint64_t a, uint64_t b) {
    fprintf(stderr, "ntiles %llu grid %u: %s (%llu, %llu)\n", (unsigned long long)ntiles, grid, what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: scan_walk_emul <cases>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    unsigned long long ntiles_in;
    unsigned grid_in, nreg_in;
    while (fscanf(f, "%llu %u %u", &ntiles_in, &grid_in, &nreg_in) == 3) {
        if (nreg_in > FZ_MAX_REGIONS || grid_in == 0) { fprintf(stderr, "malformed case\n"); return 2; }
        const uint64_t ntiles = ntiles_in;
        const uint32_t grid = grid_in, nreg = nreg_in;
        uint32_t wg0[FZ_MAX_REGIONS] = {0}, nwg[FZ_MAX_REGIONS] = {0};
        uint64_t tile0[FZ_MAX_REGIONS] = {0}, end[FZ_MAX_REGIONS] = {0};
        for (uint32_t r = 0; r < nreg; ++r) {
            unsigned long long v[4];
            if (fscanf(f, "%llu %llu %llu %llu", &v[0], &v[1], &v[2], &v[3]) != 4) { fprintf(stderr, "malformed region\n"); return 2; }
            wg0[r] = (uint32_t)v[0]; nwg[r] = (uint32_t)v[1]; tile0[r] = v[2]; end[r] = v[3];
        }
        std::vector<uint8_t> seen_fwd(ntiles, 0), seen_rev(ntiles, 0);
        uint64_t steps = 0;
        uint32_t most = 0;
        for (uint32_t wg = 0; wg < grid; ++wg) {
            const FzWalk fw = fz_scan_walk(nreg, wg0, nwg, tile0, end, grid, ntiles, wg, false);
            const FzWalk rv = fz_scan_walk(nreg, wg0, nwg, tile0, end, grid, ntiles, wg, true);
            for (uint32_t it = 0;; ++it) {
                const uint64_t a = fz_walk_tile(fw, it), b = fz_walk_tile(rv, it);
                if ((a == ~0ull) != (b == ~0ull)) return fail("the directions differ in their iterations", ntiles, grid, wg, it);
                if (a == ~0ull) break;
                if (a >= ntiles || b >= ntiles) return fail("a tile outside the buffer", ntiles, grid, a, b);
                if (b != ntiles - 1 - a) return fail("the reversed step is not the mirror", ntiles, grid, a, b);
                if (it >= kTiterMax) return fail("more iterations than a queue code carries", ntiles, grid, wg, it);
                if (seen_fwd[a]++ || seen_rev[b]++) return fail("a tile read twice", ntiles, grid, a, b);
                ++steps;
                if (it + 1 > most) most = it + 1;
            }
        }
        if (steps != ntiles) return fail("tiles never read", ntiles, grid, steps, ntiles);
        printf("%llu %u %llu %u\n", (unsigned long long)ntiles, grid, (unsigned long long)steps, most);
    }
    fclose(f);
    return 0;
}
