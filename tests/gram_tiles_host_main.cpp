// Host-only check of csrc/grf_gram_tiles.h (built and run by tests/test_gram_tiles_host.py): both locate forms
// against a band-by-band enumeration of the tile order.  Prints one line per group of shapes and "ok" at the end;
// the first disagreement is printed and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "grf_gram_tiles.h"

using grf::GramTiles;
using grf::GramTiles32;

static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// rows of band J, restated: every row in full mode, the rows of the bands <= J in symmetric mode
static int64_t band_rows(bool sym, int64_t rows, int64_t W, int64_t J) {
    if (!sym) return rows;
    return (J + 1) * W < rows ? (J + 1) * W : rows;
}

static void fail(const char *what, const GramTiles &tl, int64_t t, int64_t J, int64_t r, int64_t gJ, int64_t gr) {
    printf("MISMATCH %s: rows=%lld W=%lld nb=%lld sym=%d J_off=%lld tile %lld: want (%lld, %lld) got (%lld, %lld)\n",
           what, (long long)tl.rows, (long long)tl.W, (long long)tl.nb, (int)tl.sym, (long long)tl.J_off,
           (long long)t, (long long)J, (long long)r, (long long)gJ, (long long)gr);
    exit(1);
}

// tile t must be (J, r) in the generic form and, where t32 is given, in the 32-bit form -- with the host's
// square root and with estimates 0.4 below and above it (locate_est's stated tolerance is 1/2)
static void check_tile(const GramTiles &tl, const GramTiles32 *t32, int64_t t, int64_t J, int64_t r) {
    int64_t gJ, gr;
    tl.locate(t, gJ, gr);
    if (gJ != J || gr != r) fail("generic", tl, t, J, r, gJ, gr);
    if (!t32) return;
    uint32_t j, q;
    t32->locate((uint32_t)t, j, q);
    if ((int64_t)j != J || (int64_t)q != r) fail("32-bit", tl, t, J, r, j, q);
    const float s = (uint32_t)t < t32->tri_end ? sqrtf(GramTiles32::root_arg(t32->rW.div((uint32_t)t))) : 0.f;
    for (float ds : {-0.4f, 0.4f}) {
        t32->locate_est((uint32_t)t, s + ds, j, q);
        if ((int64_t)j != J || (int64_t)q != r) fail("32-bit, perturbed root", tl, t, J, r, j, q);
    }
}

static GramTiles make_tiles(int64_t rows, int64_t W, int64_t nb, bool sym, int64_t J_off) {
    GramTiles tl{rows, W, nb, sym, 0, 0x7fffffff};
    tl.J_off = J_off;
    return tl;
}

// every tile of the launch, cut into n_parts launches as grf_gram_sparse_upper cuts them
static int64_t enumerate_all(const GramTiles &tl, int64_t n_total, int n_parts) {
    int64_t total = 0;
    for (int64_t J = 0; J < tl.nb; ++J) total += band_rows(tl.sym, tl.rows, tl.W, J);
    if (tl.total() != total) fail("total", tl, -1, total, 0, tl.total(), 0);
    int64_t t = 0, J = 0, r = 0, checked = 0;
    for (int p = 0; p < n_parts; ++p) {
        const int64_t t0 = total * p / n_parts, t1 = total * (p + 1) / n_parts;
        if (t1 <= t0) continue;
        GramTiles32 t32;
        if (!grf::gram_tiles32(tl, n_total, t0, t1, t32)) fail("32-bit form refused", tl, t0, 0, 0, 0, 0);
        if (t32.J_off != (uint32_t)tl.J_off) fail("J_off", tl, t0, tl.J_off, 0, t32.J_off, 0);
        for (; t < t1; ++t) {
            while (r >= band_rows(tl.sym, tl.rows, tl.W, J)) {
                r = 0;
                ++J;
            }
            check_tile(tl, &t32, t, J, r);
            ++r;
            ++checked;
        }
    }
    if (checked != total) fail("enumeration", tl, t, total, 0, checked, 0);
    return checked;
}

// a large launch: the tiles within 2 of every band boundary and 10^4 seeded random tiles, each against the
// band starts summed band by band; use32: whether the whole launch must qualify for the 32-bit form
static int64_t check_large(int64_t n, int64_t W, bool use32) {
    const GramTiles tl = make_tiles(n, W, cdiv(n, W), true, 0);
    std::vector<int64_t> start(tl.nb + 1, 0);
    for (int64_t J = 0; J < tl.nb; ++J) start[J + 1] = start[J] + band_rows(true, n, W, J);
    const int64_t total = start[tl.nb];
    if (tl.total() != total) fail("total", tl, -1, total, 0, tl.total(), 0);
    GramTiles32 t32;
    const bool got32 = grf::gram_tiles32(tl, n, 0, total, t32);
    if (got32 != use32) fail(use32 ? "32-bit form refused" : "32-bit form chosen past 2^31 tiles", tl, total, 0, 0, 0, 0);
    int64_t checked = 0;
    auto one = [&](int64_t t) {
        if (t < 0 || t >= total) return;
        int64_t lo = 0, hi = tl.nb - 1;  // the band with start[J] <= t < start[J + 1]
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) / 2;
            if (start[mid] <= t) lo = mid;
            else hi = mid - 1;
        }
        check_tile(tl, use32 ? &t32 : nullptr, t, lo, t - start[lo]);
        ++checked;
    };
    for (int64_t J = 0; J <= tl.nb; ++J)
        for (int64_t d = -2; d <= 2; ++d) one(start[J] + d);
    uint64_t x = 0x9e3779b97f4a7c15ull ^ (uint64_t)n;  // (xorshift64: a fixed sequence per size)
    for (int i = 0; i < 10000; ++i) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        one((int64_t)(x % (uint64_t)total));
    }
    if (!use32) {
        // the launches such a call is cut into: those ending below 2^31 qualify, the others do not
        const int64_t lim = (int64_t)1 << 31;
        GramTiles32 part;
        if (!grf::gram_tiles32(tl, n, lim - 1000, lim, part)) fail("32-bit form refused below 2^31", tl, lim, 0, 0, 0, 0);
        for (int64_t t = lim - 1000; t < lim; ++t) {
            int64_t J, r;
            tl.locate(t, J, r);
            uint32_t j, q;
            part.locate((uint32_t)t, j, q);
            if ((int64_t)j != J || (int64_t)q != r) fail("32-bit, last tiles below 2^31", tl, t, J, r, j, q);
        }
        if (grf::gram_tiles32(tl, n, lim - 5, lim + 5, part)) fail("32-bit form chosen across 2^31", tl, lim, 0, 0, 0, 0);
    }
    return checked;
}

int main() {
    const int64_t rows_list[] = {1, 63, 64, 65, 129, 4095, 4096, 4097, 8193, 12289};
    const int64_t W_list[] = {64, 128, 4096};
    const int parts_list[] = {1, 3, 7};
    int64_t checked = 0;
    for (int64_t rows : rows_list)
        for (int64_t W : W_list)
            for (int sym = 0; sym < 2; ++sym)
                for (int64_t J_off : {0, 2})
                    for (int n_parts : parts_list) {
                        // the square case, and two more bands than rows / W (column blocks: bands of `rows` rows)
                        for (int64_t extra : {0, 2}) {
                            const GramTiles tl = make_tiles(rows, W, cdiv(rows, W) + extra, sym != 0, J_off);
                            checked += enumerate_all(tl, (cdiv(rows, W) + extra) * W, n_parts);
                        }
                    }
    printf("enumerated %lld tiles\n", (long long)checked);
    checked = check_large(1000000, 4096, true) + check_large(3000000, 4096, true);
    printf("large 32-bit launches: %lld tiles\n", (long long)checked);
    checked = check_large(5000000, 4096, false);  // 3.05e9 tiles
    printf("launch past 2^31 tiles: %lld tiles\n", (long long)checked);
    printf("ok\n");
    return 0;
}
