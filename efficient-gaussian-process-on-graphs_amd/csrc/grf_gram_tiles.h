// grf_gram_tiles.h -- the band-major tile order of a sparse Gram launch (grf_gram.hip) and the two ways a
// workgroup finds its tile in it.  Plain C++: the host planner, the kernels and a host-only test program
// (tests/test_gram_tiles_host.py) read the same code.
//
// GramTiles: the order itself and the generic 64-bit locate (divisions, an fp64 square root, search loops).
// GramTiles32: what is uniform over a launch, worked out once on the host (gram_tiles32), so that a workgroup
// finds (band, row) with two multiply-shifts, one fp32 square-root estimate and one exact integer correction.
// The host chooses it only when the launch's last tile index, n_total and rows fit in 31 bits; every other
// launch takes the generic form.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GRF_TILES_HD __host__ __device__
#else
#define GRF_TILES_HD
#endif

namespace grf {

// Tiles of one Gram call in band-major order: band J holds count(J) tiles, the local rows
// 0 .. count(J)-1 (full mode: all rows; symmetric mode, whole K: the rows of bands <= J).
struct GramTiles {
    int64_t rows, W, nb;
    bool sym;
    int32_t k_begin, k_end;  // only the nonzeros Phi[i, k] with k in [k_begin, k_end) contribute
    int64_t J_off = 0;       // the launch's bands are the global bands J_off .. J_off + nb - 1
    int64_t t_rows = -1;     // rows of the transposed matrix (< 0: n_total, the square case)
    bool add_k = false;      // write-out adds to K (which holds the dense hub-column part: grf_gram_sparse_upper_add)
    GRF_TILES_HD int64_t count(int64_t J) const {
        if (!sym) return rows;
        const int64_t c = (J + 1) * W;
        return c < rows ? c : rows;
    }
    // tiles before band J
    GRF_TILES_HD int64_t before(int64_t J) const {
        if (!sym) return J * rows;
        const int64_t full = (rows + W - 1) / W - 1;  // bands J < full hold (J + 1) W rows
        return J <= full ? W * J * (J + 1) / 2 : W * full * (full + 1) / 2 + (J - full) * rows;
    }
    GRF_TILES_HD int64_t total() const { return before(nb); }
    // band and local row of tile t
    GRF_TILES_HD void locate(int64_t t, int64_t &J, int64_t &r) const {
        if (!sym) {
            J = t / rows;
        } else {
            J = (int64_t)((sqrt(8.0 * (double)(t / W) + 1.0) - 1.0) * 0.5);
            if (J > nb - 1) J = nb - 1;
            while (J > 0 && before(J) > t) --J;
            while (J < nb - 1 && before(J + 1) <= t) ++J;
        }
        r = t - before(J);
    }
};

// floor(x / d) for 0 <= x < 2^31 as (x * mul) >> sh (Granlund & Montgomery, N = 31): with l = ceil(log2 d) and
// mul = floor(2^(31 + l) / d) + 1 the error mul d - 2^(31 + l) lies in (0, 2^l], which is exact for every x < 2^31;
// mul < 2^32 for d < 2^31.
struct GramRecip {
    uint32_t mul, sh;
    GRF_TILES_HD uint32_t div(uint32_t x) const { return (uint32_t)(((uint64_t)x * mul) >> sh); }
};

inline GramRecip gram_recip(uint32_t d) {
    uint32_t l = 0;
    while (((uint64_t)1 << l) < d) ++l;
    return {(uint32_t)((((uint64_t)1 << (31 + l)) / d) + 1), 31 + l};
}

// A launch's tile order as 32-bit host constants.  Symmetric mode: the tiles before tri_end lie in the bands
// J < full of (J + 1) W rows each -- tile t of them is in the band J with J (J + 1) / 2 <= t / W -- and the others
// in bands of `rows` rows from band `full` on.  Full mode: tri_end = 0 and full = 0, every band holds `rows`.
struct GramTiles32 {
    uint32_t rows, W;
    uint32_t full;     // first band of `rows` rows
    uint32_t tri_end;  // tiles before band `full`: W full (full + 1) / 2
    GramRecip rW, rR;  // / W, / rows
    uint32_t J_off;    // the launch's first global band

    // (band, row) of tile t < 2^31 from s, an estimate of sqrt(8 (t / W) + 1).  The band is floor((root - 1) / 2),
    // so any s within 1/2 of the root gives the true band or a neighbour, and one exact integer step settles it.
    // W >= 64 keeps t / W < 2^25 and the root below 2^14.5: the fp32 square root of the fp32-rounded argument, even
    // one a few ulp off, is within 2^-8 of it.
    GRF_TILES_HD void locate_est(uint32_t t, float s, uint32_t &J, uint32_t &r) const {
        if (t >= tri_end) {
            const uint32_t u = t - tri_end, q = rR.div(u);
            J = full + q;
            r = u - q * rows;
            return;
        }
        const uint32_t q = rW.div(t);
        int32_t j = (int32_t)((s - 1.0f) * 0.5f);
        if (j < 0) j = 0;
        uint32_t b = (uint32_t)j;
        if (b * (b + 1) / 2 > q) --b;
        else if ((b + 1) * (b + 2) / 2 <= q) ++b;
        J = b;
        r = t - W * (b * (b + 1) / 2);
    }
    GRF_TILES_HD static float root_arg(uint32_t q) { return (float)(8u * q + 1u); }
    GRF_TILES_HD void locate(uint32_t t, uint32_t &J, uint32_t &r) const {
        float s = 0.f;
        if (t < tri_end) {
#if defined(__HIP_DEVICE_COMPILE__)
            s = __builtin_amdgcn_sqrtf(root_arg(rW.div(t)));  // one v_sqrt_f32 (1 ulp): locate_est needs no more
#else
            s = sqrtf(root_arg(rW.div(t)));
#endif
        }
        locate_est(t, s, J, r);
    }
};

// The 32-bit form of the tiles [t_first, t_last) of tl over n_total columns; false: take the generic locate.
inline bool gram_tiles32(const GramTiles &tl, int64_t n_total, int64_t t_first, int64_t t_last, GramTiles32 &o) {
    const int64_t lim = (int64_t)1 << 31;
    if (t_last <= t_first || t_last - 1 >= lim || n_total >= lim || tl.rows >= lim || tl.rows < 1 || tl.W < 64 ||
        tl.W >= lim || tl.J_off < 0 || tl.J_off + tl.nb >= lim)
        return false;
    const int64_t full = tl.sym ? (tl.rows + tl.W - 1) / tl.W - 1 : 0;
    const int64_t tri_end = tl.sym ? tl.before(full < tl.nb ? full : tl.nb) : 0;
    // (tri_end <= before(nb) = the tile count whenever full < nb; a launch with fewer bands never leaves the triangle)
    o.rows = (uint32_t)tl.rows;
    o.W = (uint32_t)tl.W;
    o.full = (uint32_t)(full < tl.nb ? full : tl.nb);
    o.tri_end = (uint32_t)(tri_end < lim ? tri_end : lim);
    o.rW = gram_recip(o.W);
    o.rR = gram_recip(o.rows);
    o.J_off = (uint32_t)tl.J_off;
    return true;
}

}  // namespace grf
