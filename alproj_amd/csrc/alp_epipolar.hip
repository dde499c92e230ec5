// libalproj_hip.so -- the geometric match filter and the grid thinning that the reference's image_match runs between its matcher
// and set_gcp (src/alproj/gcp.py:507-544: _filter_geometric with outlier_filter="fundamental", then _filter_spatial).
//
// cv2's USAC (its random stream, PROSAC, SPRT, MAGSAC scoring) cannot be restated, so the filter is an algorithm of this project's
// own: hypothesise and verify outright.  H minimal samples of 8 matches -> H fundamental matrices by the normalised 8-point
// solve -> the inlier count of every one of them over all n matches -> the best one, refitted on its inliers while that strictly
// grows the count; or, least median of squares, the one with the smallest rank-th error, refitted while that value falls.  The
// four filters (fundamental or essential, RANSAC or LMedS) are one host driver, epi_filter.  Everything is float64, and the unit
// is compiled with -ffp-contract=off: the error of a match under F is written in the order include/alproj_hip.h gives, so that
// numpy reproduces it bit for bit.
//
//   epi_pack_kernel       p1, p2 -> (x1, y1, x2, y2), 32 B per match
//   epi_norm_kernel       one workgroup: Hartley's normalisation of both images from all n points (centroid, mean distance sqrt 2)
//   epi_hypotheses.h      epi_samples_kernel, epi_solve_kernel, epi_solve5_kernel, epi_essential_kernel: H minimal samples and the
//                         matrices of each (the 8-point solve: one; the five-point solver: up to 10 slots, NaN = unused)
//   epi_score_kernel      the inlier count of every hypothesis over one split of the match tiles (epi_walk_tiles: a workgroup = 256
//                         hypotheses, one per lane, x a tile of 512 matches in LDS); one division per error (epi_error1)
//   epi_merge_kernel      a thread per hypothesis: the sum of its partial counts over the splits (no atomics)
//   epi_choose_kernel     one workgroup: the highest count, the lowest index on a tie; the run begins in the state record (epi_begin)
//   epi_accum_kernel, epi_refit_kernel, epi_count_kernel, epi_decide_kernel
//                         one refit: the upper triangle of sum a a^T over the inliers of the current F (45 sums per lane, wave and
//                         workgroup reduction, fixed order), its smallest eigenvector by Jacobi rotations in one wave, rank 2,
//                         the count of the candidate, and the decision (epi_accept).  All of them read `stopped` and the bound
//                         from the state record and return at once when it is set: the host enqueues `refits` rounds and never looks.
//   epi_mask_kernel       mask and error of every match under the state record's F at its bound
//   epi_select_kernel, epi_select_merge_kernel
//                         the LMedS filter: the rank-th smallest error of every hypothesis, exactly, without an H x n array: a
//                         radix select on the 64 bits of the error, the most significant 4-bit digit first, 16 passes.  The
//                         walk is the score kernel's; in every pass a lane forms its errors again and, for each one whose
//                         higher digits equal the prefix found so far, bumps one of 16 counters in LDS (counter d of lane l at
//                         d * 256 + l: a lane's own column, no bank conflict).  The merge adds the splits' counters in order
//                         (integers), finds the digit at which they reach the remaining rank and extends the prefix.
//   epi_lmeds_choose_kernel, epi_errs_kernel, epi_lmeds_eval_kernel
//                         the smallest value, the lowest index on a tie; the errors of one F (the chosen one, a refit's candidate)
//                         as an array; and one workgroup that selects the value of that array (8-bit digits, integer LDS
//                         atomics, 8 passes), forms the bound, counts the inliers and decides by epi_accept on values
//   thin_*_kernel         alp_grid_thin: atomic minima on (distance bits) and then on the index, per cell
#include "alp_sampler.h"

#include <climits>
#include <cmath>

namespace {

using namespace alp;

#include "epi_dev.h"

__global__ __launch_bounds__(256) void epi_pack_kernel(const double2 *__restrict__ p1, const double2 *__restrict__ p2, int n,
                                                       double4 *__restrict__ pts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double2 a = p1[i], b = p2[i];
    pts[i] = make_double4(a.x, a.y, b.x, b.y);
}

__global__ __launch_bounds__(256) void epi_norm_kernel(const double4 *__restrict__ pts, int n, EpiState *__restrict__ st) {
    __shared__ double buf[4];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256) {
        const double4 q = pts[i];
        s[0] += q.x, s[1] += q.y, s[2] += q.z, s[3] += q.w;
    }
    double c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = block_sum256(s[k], buf) / (double)n;
    double m1 = 0.0, m2 = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double4 q = pts[i];
        const double ax = q.x - c[0], ay = q.y - c[1], bx = q.z - c[2], by = q.w - c[3];
        m1 += sqrt(ax * ax + ay * ay);
        m2 += sqrt(bx * bx + by * by);
    }
    m1 = block_sum256(m1, buf) / (double)n;
    m2 = block_sum256(m2, buf) / (double)n;
    if (threadIdx.x == 0) {
        st->T[0] = c[0], st->T[1] = c[1], st->T[2] = 1.4142135623730951 / m1;
        st->T[3] = c[2], st->T[4] = c[3], st->T[5] = 1.4142135623730951 / m2;
    }
}

#include "epi_hypotheses.h"

// The walk of the score and select kernels: a workgroup = 256 hypotheses (one per lane, F in registers) x one split of the
// match tiles.  A tile of 512 matches is staged in LDS and every lane walks it: all lanes read the same address (a broadcast).
// visit(f, q) is called with the lane's matrix and every match of the split in order.  (f goes through as an argument: a visitor
// that captures it compiles to another operand order in the inner loop than the loop written out.)
template <class Visit>
__device__ __forceinline__ void epi_walk_tiles(const double4 *__restrict__ pts, int n, int splits, int split, long long match_tiles,
                                               double4 *tile, const double (&f)[9], Visit visit) {
    int64_t tb, te;
    match_split_range(match_tiles, splits, split, &tb, &te);
    for (long long t = tb; t < te; ++t) {
        const int base = (int)(t * EPI_MATCH_TILE);
        const int cnt = n - base < EPI_MATCH_TILE ? n - base : EPI_MATCH_TILE;
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += EPI_HYP_TILE) tile[i] = pts[base + i];
        __syncthreads();
#pragma unroll 4
        for (int m = 0; m < cnt; ++m) visit(f, tile[m]);
    }
}

__global__ __launch_bounds__(EPI_HYP_TILE) void epi_score_kernel(const double4 *__restrict__ pts, int n, const double *__restrict__ F, int H,
                                                                 double t2, int splits, long long match_tiles, long long h_pad,
                                                                 int *__restrict__ partial) {
    __shared__ double4 tile[EPI_MATCH_TILE];
    const long long htile = blockIdx.x / (unsigned)splits;
    const int split = (int)(blockIdx.x % (unsigned)splits);
    const long long h = htile * EPI_HYP_TILE + threadIdx.x;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = h < H ? F[(size_t)h * 9 + k] : nan64();
    int count = 0;                      // stays in a register
    epi_walk_tiles(pts, n, splits, split, match_tiles, tile, f,
                   [&](const double (&m)[9], const double4 q) { count += epi_error1(m, q) <= t2 ? 1 : 0; });
    partial[(size_t)split * h_pad + h] = count;
}

__global__ __launch_bounds__(256) void epi_merge_kernel(const int *__restrict__ partial, int splits, long long h_pad, int H,
                                                        int *__restrict__ counts) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    int c = 0;
    for (int s = 0; s < splits; ++s) c += partial[(size_t)s * h_pad + h];
    counts[h] = c;
}

// the highest count, the lowest index on a tie: the largest key count << 32 | ~index
// min_count: the size of a minimal sample; a best count below it keeps every match.  t2: the bound of the whole run
__global__ __launch_bounds__(256) void epi_choose_kernel(const int *__restrict__ counts, int H, const double *__restrict__ F, int min_count,
                                                         double t2, EpiState *__restrict__ st) {
    __shared__ u64 best[4];
    u64 key = 0;
    for (int h = threadIdx.x; h < H; h += 256) {
        const u64 k = (u64)(unsigned)counts[h] << 32 | (u64)(0xffffffffu - (unsigned)h);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), o, 64);
        const u64 k = (u64)hi << 32 | lo;
        key = k > key ? k : key;
    }
    if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) key = best[w] > key ? best[w] : key;
        const int count = (int)(key >> 32);
        epi_begin(st, F, (int)(0xffffffffu - (unsigned)key), count, count < min_count);
        st->bound2 = t2;
    }
}

__global__ __launch_bounds__(EPI_REDUCE_BLOCK) void epi_accum_kernel(const double4 *__restrict__ pts, int n, const EpiState *__restrict__ st,
                                                                     double *__restrict__ sym) {
    __shared__ double red[4 * EPI_SYM];
    if (st->stopped) return;
    const double t2 = st->bound2;
    double f[9], T[6], acc[EPI_SYM];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = st->Fcur[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) T[k] = st->T[k];
#pragma unroll
    for (int k = 0; k < EPI_SYM; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * EPI_REDUCE_BLOCK + threadIdx.x; i < n; i += gridDim.x * EPI_REDUCE_BLOCK) {
        const double4 q = pts[i];
        if (!(epi_error(f, q) <= t2)) continue;
        const double x1 = (q.x - T[0]) * T[2], y1 = (q.y - T[1]) * T[2], x2 = (q.z - T[3]) * T[5], y2 = (q.w - T[4]) * T[5];
        const double a[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
        int k = 0;
#pragma unroll
        for (int r = 0; r < 9; ++r)
#pragma unroll
            for (int c = r; c < 9; ++c) acc[k++] += a[r] * a[c];
    }
#pragma unroll
    for (int k = 0; k < EPI_SYM; ++k) {
        const double v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * EPI_SYM + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < EPI_SYM)
        sym[(size_t)blockIdx.x * EPI_SYM + threadIdx.x] =
            (red[threadIdx.x] + red[EPI_SYM + threadIdx.x]) + (red[2 * EPI_SYM + threadIdx.x] + red[3 * EPI_SYM + threadIdx.x]);
}

// one wave: the 45 sums over the workgroups of epi_accum_kernel in order, then the eigenvector of the smallest eigenvalue of the
// 9 x 9 matrix by Jacobi rotations, four disjoint pairs at a time (matrix and vectors in LDS: they are indexed by the rotation's
// pair), and on lane 0 rank 2 and T2^T f T1
__global__ __launch_bounds__(64) void epi_refit_kernel(const double *__restrict__ sym, int blocks, EpiState *__restrict__ st) {
    __shared__ double S[EPI_SYM], M[81], V[81];
    if (st->stopped) return;
    if (threadIdx.x < EPI_SYM) {
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += sym[(size_t)b * EPI_SYM + threadIdx.x];
        S[threadIdx.x] = s;
    }
    __syncthreads();
    const int i = threadIdx.x;          // lanes 0..8 own index i of every rotation; all lanes walk the pairs together
    for (int e = i; e < 81; e += 64) {
        const int r = e / 9, c = e % 9, lo_rc = r < c ? r : c, hi_rc = r < c ? c : r;
        M[e] = S[lo_rc * 9 - lo_rc * (lo_rc - 1) / 2 + (hi_rc - lo_rc)];
        V[e] = r == c ? 1.0 : 0.0;
    }
    __syncthreads();
    // round-robin order: 9 rounds of 4 disjoint pairs cover the 36 pairs once (the circle method over 9 indices and a bye); the 4
    // rotations of a round touch different rows and columns, so M <- J^T M J is their columns, a barrier, their rows.  Lane
    // 9 k + e turns element e of pair k.
    const int pair = i / 9, e = i % 9;
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
        for (int round = 0; round < 9; ++round) {
            const int a = (round + pair + 1) % 9, b = (round + 8 - pair) % 9;
            const int p = a < b ? a : b, q = a < b ? b : a;
            bool rot = false;
            double c = 1.0, s = 0.0;
            if (pair < 4) {
                const double apq = M[p * 9 + q], app = M[p * 9 + p], aqq = M[q * 9 + q];
                rot = apq != 0.0 && fabs(apq) > 1e-17 * sqrt(fabs(app) * fabs(aqq));
                if (rot) {
                    const double zeta = (aqq - app) / (2.0 * apq);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                }
            }
            rotated = rotated || __any(rot);           // (the workgroup is one wave)
            __syncthreads();
            if (rot) {                                 // columns p, q of M and of V
                const double mp = M[e * 9 + p], mq = M[e * 9 + q], vp = V[e * 9 + p], vq = V[e * 9 + q];
                M[e * 9 + p] = c * mp - s * mq, M[e * 9 + q] = s * mp + c * mq;
                V[e * 9 + p] = c * vp - s * vq, V[e * 9 + q] = s * vp + c * vq;
            }
            __syncthreads();
            if (rot) {                                 // rows p, q
                const double mp = M[p * 9 + e], mq = M[q * 9 + e];
                M[p * 9 + e] = c * mp - s * mq, M[q * 9 + e] = s * mp + c * mq;
            }
            __syncthreads();
            if (rot && e == 0) M[p * 9 + q] = M[q * 9 + p] = 0.0;
            __syncthreads();
        }
        if (!rotated) break;
    }
    if (i != 0) return;
    int lo = 0;
    for (int i = 1; i < 9; ++i)
        if (M[i * 9 + i] < M[lo * 9 + lo]) lo = i;
    double f[9], out[9], T[6];
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = V[i * 9 + lo];
#pragma unroll
    for (int i = 0; i < 6; ++i) T[i] = st->T[i];
    rank2_denorm(f, T, st->essential != 0, out);
#pragma unroll
    for (int i = 0; i < 9; ++i) st->Fcand[i] = out[i];
}

__global__ __launch_bounds__(EPI_REDUCE_BLOCK) void epi_count_kernel(const double4 *__restrict__ pts, int n, const EpiState *__restrict__ st,
                                                                     int *__restrict__ cpart) {
    __shared__ int red[EPI_REDUCE_BLOCK / 64];
    if (st->stopped) return;
    const double t2 = st->bound2;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = st->Fcand[k];
    int c = 0;
    for (int i = blockIdx.x * EPI_REDUCE_BLOCK + threadIdx.x; i < n; i += gridDim.x * EPI_REDUCE_BLOCK)
        c += epi_error(f, pts[i]) <= t2 ? 1 : 0;
    c = block_count<EPI_REDUCE_BLOCK / 64>(c, red);
    if (threadIdx.x == 0) cpart[blockIdx.x] = c;
}

// the candidate is kept while it strictly grows the count
__global__ void epi_decide_kernel(const int *__restrict__ cpart, int blocks, int round, EpiState *__restrict__ st) {
    if (threadIdx.x != 0 || st->stopped) return;
    int c = 0;
    for (int b = 0; b < blocks; ++b) c += cpart[b];
    epi_accept(st, round, c, c > st->count);
}

// mask and error of every match under the state's current matrix at its bound; keep_all turns every mask entry into 1
__global__ __launch_bounds__(256) void epi_mask_kernel(const double4 *__restrict__ pts, int n, const EpiState *__restrict__ st,
                                                       unsigned char *__restrict__ mask, double *__restrict__ err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = st->Fcur[k];
    const double e = epi_error(f, pts[i]);
    err[i] = e;
    mask[i] = (e <= st->bound2 || st->keep_all) ? 1 : 0;
}

// ------------------------------------------------------------------ the LMedS filter
// One pass: `shift` is the place of the pass' digit (60 in the first pass, 0 in the last).  prefix[h]: the digits above it
// (not read in the first pass); hist: the counters of this split, [16][h_pad] from its base.
__global__ __launch_bounds__(EPI_HYP_TILE) void epi_select_kernel(const double4 *__restrict__ pts, int n, const double *__restrict__ F, int H,
                                                                  int splits, long long match_tiles, long long h_pad,
                                                                  const u64 *__restrict__ prefix, int shift, unsigned *__restrict__ hist) {
    __shared__ double4 tile[EPI_MATCH_TILE];
    __shared__ unsigned cnt[EPI_SELECT_DIGITS * EPI_HYP_TILE];
    const long long htile = blockIdx.x / (unsigned)splits;
    const int split = (int)(blockIdx.x % (unsigned)splits);
    const long long h = htile * EPI_HYP_TILE + threadIdx.x;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = h < H ? F[(size_t)h * 9 + k] : nan64();
    const bool first = shift == 64 - EPI_SELECT_BITS;
    const u64 pre = first ? 0 : prefix[h];
    const u64 above = first ? 0 : ~(u64)0 << (shift + EPI_SELECT_BITS);
    unsigned *const mine = cnt + threadIdx.x;         // counter d at mine[d * 256]: no other lane touches it
#pragma unroll
    for (int d = 0; d < EPI_SELECT_DIGITS; ++d) mine[d * EPI_HYP_TILE] = 0;
    epi_walk_tiles(pts, n, splits, split, match_tiles, tile, f, [&](const double (&m)[9], const double4 q) {
        const u64 k = epi_key_of(epi_error1(m, q));
        if (((k ^ pre) & above) == 0) atomicAdd(mine + (int)((k >> shift) & (EPI_SELECT_DIGITS - 1)) * EPI_HYP_TILE, 1u);
    });
    unsigned *const out = hist + (size_t)split * EPI_SELECT_DIGITS * h_pad + h;
#pragma unroll
    for (int d = 0; d < EPI_SELECT_DIGITS; ++d) out[(size_t)d * h_pad] = mine[d * EPI_HYP_TILE];
}

// a thread per padded hypothesis: the counters of the splits added in order, the digit at which they reach the remaining rank,
// the prefix extended by it and the rank reduced by what lies below it; after the last pass the prefix is the value
__global__ __launch_bounds__(256) void epi_select_merge_kernel(const unsigned *__restrict__ hist, int splits, long long h_pad, int H, int shift,
                                                               int rank0, u64 *__restrict__ prefix, int *__restrict__ rank,
                                                               double *__restrict__ value) {
    const long long h = (long long)blockIdx.x * 256 + threadIdx.x;
    if (h >= h_pad) return;
    const bool first = shift == 64 - EPI_SELECT_BITS;
    const unsigned r = (unsigned)(first ? rank0 : rank[h]);
    unsigned below = 0;
    int digit = EPI_SELECT_DIGITS - 1;
    for (int d = 0; d < EPI_SELECT_DIGITS; ++d) {
        unsigned c = 0;
        for (int s = 0; s < splits; ++s) c += hist[((size_t)s * EPI_SELECT_DIGITS + d) * h_pad + h];
        if (below + c >= r) {
            digit = d;
            break;
        }
        below += c;
    }
    const u64 p = (first ? 0 : prefix[h]) | (u64)digit << shift;
    prefix[h] = p;
    rank[h] = (int)(r - below);
    if (shift == 0 && h < H) value[h] = __longlong_as_double((long long)p);
}

// one workgroup: the smallest value, the lowest index on a tie (value and index do not pack into one 64-bit key: a
// lexicographic compare); the state of the filter from it
__global__ __launch_bounds__(256) void epi_lmeds_choose_kernel(const double *__restrict__ value, int H, const double *__restrict__ F, int rank,
                                                               double scale2, double floor2, EpiState *__restrict__ st) {
    __shared__ u64 bkey[256];
    __shared__ int bidx[256];
    u64 key = ~(u64)0;
    int idx = INT_MAX;
    for (int h = threadIdx.x; h < H; h += 256) {          // ascending h: a strict compare keeps the lowest index
        const u64 k = (u64)__double_as_longlong(value[h]);
        if (k < key) key = k, idx = h;
    }
    bkey[threadIdx.x] = key, bidx[threadIdx.x] = idx;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int t = 1; t < 256; ++t)
        if (bkey[t] < key || (bkey[t] == key && bidx[t] < idx)) key = bkey[t], idx = bidx[t];
    const double v = __longlong_as_double((long long)key);
    epi_begin(st, F, idx, 0, !(key < EPI_KEY_INF));      // (the count at the bound follows from epi_lmeds_eval_kernel)
    for (int k = 0; k < EPI_LMEDS_STATS; ++k) st->stats[k] = nan64();
    st->rank = rank, st->scale2 = scale2, st->floor2 = floor2;
    const double sv = scale2 * v;
    st->value = v, st->bound2 = sv > floor2 ? sv : floor2;
    st->stats[S_CHOSEN_VALUE] = st->stats[S_FINAL_VALUE] = v, st->stats[S_BOUND2] = st->bound2;
}

// the keys of the errors of every match under the current F (candidate == 0) or the refit's candidate, with the mask
// kernel's arithmetic
__global__ __launch_bounds__(256) void epi_errs_kernel(const double4 *__restrict__ pts, int n, const EpiState *__restrict__ st, int candidate,
                                                       u64 *__restrict__ keys) {
    if (st->stopped) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = candidate ? st->Fcand[k] : st->Fcur[k];
    keys[i] = epi_key_of(epi_error(f, pts[i]));
}

// One workgroup over the keys of one F.  round < 0: the chosen hypothesis, whose value is known: the count of its inliers.
// Otherwise the candidate of refit `round`: its value by a radix select on the array (8-bit digits, integer LDS atomics: the
// counts do not depend on their order), its bound, its count, and the decision: it replaces the current F only when its value is
// strictly smaller, otherwise the loop stops.  A value that is not finite counts no inliers.
__global__ __launch_bounds__(EPI_SELECT1_BLOCK) void epi_lmeds_eval_kernel(const u64 *__restrict__ keys, int n, int round, EpiState *__restrict__ st) {
    __shared__ unsigned hist[256];
    __shared__ u64 s_prefix;
    __shared__ unsigned s_rank;
    __shared__ int red[EPI_SELECT1_BLOCK / 64];
    if (st->stopped) return;
    u64 vkey = (u64)__double_as_longlong(st->value);
    if (round >= 0) {
        u64 pre = 0;
        unsigned r = (unsigned)st->rank;
        for (int pass = 0; pass < EPI_SELECT1_PASSES; ++pass) {
            const int shift = 56 - 8 * pass;
            const u64 above = pass == 0 ? 0 : ~(u64)0 << (shift + 8);
            __syncthreads();
            if (threadIdx.x < 256) hist[threadIdx.x] = 0;
            __syncthreads();
            for (int i = threadIdx.x; i < n; i += EPI_SELECT1_BLOCK) {
                const u64 k = keys[i];
                if (((k ^ pre) & above) == 0) atomicAdd(hist + (int)((k >> shift) & 255), 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned below = 0;
                int digit = 255;
                for (int d = 0; d < 256; ++d) {
                    if (below + hist[d] >= r) {
                        digit = d;
                        break;
                    }
                    below += hist[d];
                }
                s_prefix = pre | (u64)digit << shift, s_rank = r - below;
            }
            __syncthreads();
            pre = s_prefix, r = s_rank;
        }
        vkey = pre;
    }
    const bool finite = vkey < EPI_KEY_INF;
    const double v = __longlong_as_double((long long)vkey);
    const double sv = st->scale2 * v, floor2 = st->floor2;
    const double b2 = sv > floor2 ? sv : floor2;
    const u64 bkey = (u64)__double_as_longlong(b2);           // b2 >= 0: e <= b2 is key <= its key (a NaN e has the key of +inf, and b2 is below it whenever v is finite and scale2 * v does not overflow)
    int c = 0;
    if (finite)
        for (int i = threadIdx.x; i < n; i += EPI_SELECT1_BLOCK) c += (keys[i] <= bkey && keys[i] < EPI_KEY_INF) ? 1 : 0;
    c = block_count<EPI_SELECT1_BLOCK / 64>(c, red);
    if (threadIdx.x != 0) return;
    if (round < 0) {
        st->count = c;
        st->info[I_CHOSEN_COUNT] = st->info[I_FINAL_COUNT] = c;
        return;
    }
    st->stats[S_REFIT_VALUE0 + round] = v;
    if (epi_accept(st, round, c, v < st->value)) {
        st->value = v, st->bound2 = b2;
        st->stats[S_FINAL_VALUE] = v, st->stats[S_BOUND2] = b2;
    }
}

// ------------------------------------------------------------------ alp_grid_thin
__global__ __launch_bounds__(256) void thin_dist_kernel(const long long *__restrict__ cell, const double *__restrict__ dist, long long n,
                                                        long long lo, u64 *__restrict__ best) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    atomicMin(best + (cell[i] - lo), (u64)__double_as_longlong(dist[i] + 0.0));       // (+ 0.0: a -0.0 orders as 0.0)
}
__global__ __launch_bounds__(256) void thin_index_kernel(const long long *__restrict__ cell, const double *__restrict__ dist, long long n,
                                                         long long lo, const u64 *__restrict__ best, u64 *__restrict__ first) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long c = cell[i] - lo;
    if (!dist || (u64)__double_as_longlong(dist[i] + 0.0) == best[c]) atomicMin(first + c, (u64)i);
}
__global__ __launch_bounds__(256) void thin_mask_kernel(const long long *__restrict__ cell, long long n, long long lo,
                                                        const u64 *__restrict__ first, unsigned char *__restrict__ mask) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    mask[i] = first[cell[i] - lo] == (u64)i ? 1 : 0;
}

// ------------------------------------------------------------------ host side
// H rows of `width` distinct indices below n: EPI_SAMPLE or EPI_SAMPLE5, each on a stream word of its own
void epi_launch_samples(int width, int64_t n, int64_t H, uint64_t seed, int *samples) {
    const auto kernel = width == EPI_SAMPLE ? epi_samples_kernel<EPI_SAMPLE, EPI_STREAM> : epi_samples_kernel<EPI_SAMPLE5, EPI_STREAM5>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, ctx().stream, (int)n, (int)H, (unsigned)seed,
                       (unsigned)(seed >> 32), samples);
}

struct EpiCall {
    host::EpiPlan p;
    DeviceBuffer<char> dev;
    char *d = nullptr;
    double4 *pts() const { return (double4 *)(d + p.off_pts); }
    int *samples() const { return (int *)(d + p.off_samples); }
    double *F() const { return (double *)(d + p.off_F); }
    int *partial() const { return (int *)(d + p.off_partial); }
    int *counts() const { return (int *)(d + p.off_counts); }
    EpiState *state() const { return (EpiState *)(d + p.off_state); }
    double *sym() const { return (double *)(d + p.off_sym); }
    int *cpart() const { return (int *)(d + p.off_cpart); }
    unsigned char *mask() const { return (unsigned char *)(d + p.off_mask); }
    double *err() const { return (double *)(d + p.off_err); }

    unsigned *hist() const { return (unsigned *)(d + p.off_hist); }
    u64 *prefix() const { return (u64 *)(d + p.off_prefix); }
    int *rank() const { return (int *)(d + p.off_rank); }
    double *value() const { return (double *)(d + p.off_value); }

    // with_select: the plan of the LMedS filter, which has the select's arrays after all the others
    int reserve(int64_t n, int64_t H, int splits, bool with_select = false) {
        p = with_select ? host::epi_select_plan(n, H, splits, ctx().cu_count) : host::epi_plan(n, H, splits, ctx().cu_count);
        if (int rc = dev.reserve(p.scratch_bytes)) return rc;
        d = dev;
        return ALP_OK;
    }
    // p1, p2 -> the packed matches and (with_norm) the normalisation in the state record
    hipError_t upload(const double *p1, const double *p2, int64_t n, bool with_norm) {
        hipStream_t st = ctx().stream;
        hipError_t e = hipMemcpyAsync(d + p.off_raw1, p1, (size_t)n * 16, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d + p.off_raw2, p2, (size_t)n * 16, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(state(), 0, EPI_STATE_BYTES, st);
        if (e != hipSuccess) return e;
        KTimeScope kt;
        hipLaunchKernelGGL(epi_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double2 *)(d + p.off_raw1),
                           (const double2 *)(d + p.off_raw2), (int)n, pts());
        if (with_norm) hipLaunchKernelGGL(epi_norm_kernel, dim3(1), dim3(256), 0, st, (const double4 *)pts(), (int)n, state());
        return hipGetLastError();
    }
    // the essential filter: the call is planned for 10 H hypothesis slots, so the sample block holds the H rows of 5 and, from
    // byte 32 H on, the H solution counts
    int *nsol(int64_t H) const { return (int *)(d + p.off_samples + (size_t)H * 32); }
    // the hypotheses of the H samples: K == NULL the 8-point solve of rows of 8, else the five-point solver on rows of 5 with K
    // in the state record
    void launch_solver(int64_t H, const double *K) {
        if (K) {
            hipLaunchKernelGGL(epi_essential_kernel, dim3(1), dim3(64), 0, ctx().stream, K[0], K[1], K[2], state());
            hipLaunchKernelGGL(epi_solve5_kernel, dim3((unsigned)((H + EPI_SOLVE_BLOCK - 1) / EPI_SOLVE_BLOCK)), dim3(EPI_SOLVE_BLOCK), 0, ctx().stream,
                               (const double4 *)pts(), (const int *)samples(), (int)H, (const EpiState *)state(), F(), nsol(H));
        } else {
            hipLaunchKernelGGL(epi_solve_kernel, dim3((unsigned)p.solve_blocks), dim3(EPI_SOLVE_BLOCK), 0, ctx().stream, (const double4 *)pts(),
                               (const int *)samples(), (int)H, (const EpiState *)state(), F());
        }
    }
    // the plan as six words of an info array; the sixth is the caller's (the match tiles, or the blocks of the refit's reductions)
    void plan_info(int64_t *w, int64_t sixth) const {
        w[0] = p.hyp_tile, w[1] = p.match_tile, w[2] = p.splits, w[3] = p.workgroups, w[4] = (int64_t)p.scratch_bytes, w[5] = sixth;
    }
    void launch_score(int64_t n, int64_t H, double t2) {
        hipLaunchKernelGGL(epi_score_kernel, dim3((unsigned)p.workgroups), dim3(EPI_HYP_TILE), 0, ctx().stream, (const double4 *)pts(), (int)n,
                           (const double *)F(), (int)H, t2, p.splits, (long long)p.match_tiles, (long long)p.h_pad, partial());
        hipLaunchKernelGGL(epi_merge_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, ctx().stream, (const int *)partial(), p.splits,
                           (long long)p.h_pad, (int)H, counts());
    }
    // value()[h] = the rank-th smallest error of hypothesis h: the passes of the select, each followed by its merge
    void launch_select(int64_t n, int64_t H, int rank) {
        for (int pass = 0; pass < p.passes; ++pass) {
            const int shift = 64 - EPI_SELECT_BITS * (pass + 1);
            hipLaunchKernelGGL(epi_select_kernel, dim3((unsigned)p.workgroups), dim3(EPI_HYP_TILE), 0, ctx().stream, (const double4 *)pts(), (int)n,
                               (const double *)F(), (int)H, p.splits, (long long)p.match_tiles, (long long)p.h_pad, (const u64 *)prefix(), shift, hist());
            hipLaunchKernelGGL(epi_select_merge_kernel, dim3((unsigned)(p.h_pad / 256)), dim3(256), 0, ctx().stream, (const unsigned *)hist(), p.splits,
                               (long long)p.h_pad, (int)H, shift, rank, prefix(), this->rank(), value());
        }
    }
};

// slots: hypotheses scored per sample (10 for the five-point solver, whose samples need 5 matches and not 8)
int epi_check_points(const char *fn, const double *p1, const double *p2, int64_t n, int64_t H, int slots = 1) {
    if (!p1 || !p2) return fail(ALP_EINVAL, "%s: NULL input", fn);
    const int64_t min_n = slots == 1 ? EPI_MIN_N : EPI_SAMPLE5, max_h = EPI_MAX_H / slots;
    if (n < min_n || n > EPI_MAX_N) return fail(ALP_EINVAL, "%s: n = %lld, must be %lld..2^20", fn, (long long)n, (long long)min_n);
    if (H < 1 || H > max_h) return fail(ALP_EINVAL, "%s: H = %lld, must be 1..%s", fn, (long long)H, slots == 1 ? "2^20" : "2^20 / 10");
    if (!host::epi_caps_ok(n, H * slots, min_n)) return fail(ALP_EINVAL, "%s: H * n = %lld * %lld passes 2^35 error evaluations", fn, (long long)H, (long long)n);
    return ALP_OK;
}

int epi_check_samples(const char *fn, const int32_t *samples, int64_t H, int64_t n, int width = EPI_SAMPLE) {
    for (int64_t i = 0; i < H * width; ++i)
        if (samples[i] < 0 || samples[i] >= n)
            return fail(ALP_EINVAL, "%s: sample %lld of hypothesis %lld is %d, outside 0..%lld", fn, (long long)(i % width),
                        (long long)(i / width), samples[i], (long long)(n - 1));
    return ALP_OK;
}

int epi_check_splits(const char *fn, int splits, int64_t n) {
    const int64_t tiles = (n + EPI_MATCH_TILE - 1) / EPI_MATCH_TILE;
    if (splits < 0) return fail(ALP_EINVAL, "%s: splits is negative", fn);
    if (splits > tiles)
        return fail(ALP_EINVAL, "%s: splits = %d, but %lld matches are only %lld tiles of %d", fn, splits, (long long)n, (long long)tiles,
                    EPI_MATCH_TILE);
    return ALP_OK;
}

int epi_check_K(const char *fn, const double *K) {
    if (!K) return fail(ALP_EINVAL, "%s: NULL K", fn);
    if (!(std::isfinite(K[0]) && K[0] > 0.0)) return fail(ALP_EINVAL, "%s: the focal length must be finite and positive", fn);
    if (!(std::isfinite(K[1]) && std::isfinite(K[2]))) return fail(ALP_EINVAL, "%s: the principal point must be finite", fn);
    return ALP_OK;
}

int epi_finish(const char *fn, hipError_t e) {
    const hipError_t es = hipStreamSynchronize(ctx().stream);          // before the device block and the caller's arrays go away
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(ALP_EHIP, "%s: %s", fn, hipGetErrorString(e));
    return ALP_OK;
}

// what the select adds to epi_check_points: the work of its passes, and the rank
int epi_check_select(const char *fn, int64_t n, int64_t H, int slots, int64_t rank) {
    if (!host::epi_select_caps_ok(n, H * slots, slots == 1 ? EPI_MIN_N : EPI_SAMPLE5))
        return fail(ALP_EINVAL, "%s: %d passes * H * n = %d * %lld * %lld pass 2^35 error evaluations", fn, EPI_SELECT_PASSES, EPI_SELECT_PASSES,
                    (long long)(H * slots), (long long)n);
    if (rank < 1 || rank > n) return fail(ALP_EINVAL, "%s: rank = %lld, must be 1..n = %lld", fn, (long long)rank, (long long)n);
    return ALP_OK;
}

// alp_epipolar_samples (width 8) and alp_epipolar_samples5 (width 5)
int epi_samples(const char *fn, int width, int64_t n, int64_t H, uint64_t seed, int32_t *samples) {
    if (int rc = require_init()) return rc;
    if (!samples) return fail(ALP_EINVAL, "%s: NULL output", fn);
    if (!(n >= width && n <= EPI_MAX_N)) return fail(ALP_EINVAL, "%s: n must be %d..2^20", fn, width);
    if (!(H >= 1 && H <= EPI_MAX_H)) return fail(ALP_EINVAL, "%s: H must be 1..2^20", fn);
    DeviceBuffer<int> dev;
    if (int rc = dev.reserve((size_t)H * width * 4)) return rc;
    hipError_t e;
    {
        KTimeScope kt;
        epi_launch_samples(width, n, H, seed, (int *)dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(samples, (int *)dev, (size_t)H * width * 4, hipMemcpyDeviceToHost, ctx().stream);
    return epi_finish(fn, e);
}

// How a filter judges a matrix, the one thing epi_filter branches on.  RANSAC: by the count of its inliers at e <= threshold^2,
// the more the better.  LMedS: by its value, the rank-th smallest error, the smaller the better; the value sets the bound
// max(scale2 * value, floor2) at which its inliers are then counted.
struct EpiCriterion {
    bool lmeds;
    double threshold;
    int64_t rank;
    double scale2, floor2;
    static EpiCriterion count(double threshold) { return {false, threshold, 0, 0.0, 0.0}; }
    static EpiCriterion value(int64_t rank, double scale2, double floor2) { return {true, 0.0, rank, scale2, floor2}; }
};

// The whole filter in one device loop.  K == NULL: the fundamental one on samples of 8; else the essential one on samples of 5
// with 10 hypothesis slots each.  Everything is enqueued at once; what a refit round does is decided on the device
// (EpiState::stopped), the host never looks.
int epi_filter(const char *fn, const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed, const double *K,
               const EpiCriterion &cr, int refits, int splits, double F[9], uint8_t *mask, int64_t info[24], double stats[12]) {
    if (int rc = require_init()) return rc;
    const int slots = K ? EPI_SLOTS5 : 1, width = K ? EPI_SAMPLE5 : EPI_SAMPLE;
    if (int rc = epi_check_points(fn, p1, p2, n, H, slots)) return rc;
    if (cr.lmeds)
        if (int rc = epi_check_select(fn, n, H, slots, cr.rank)) return rc;
    if (K)
        if (int rc = epi_check_K(fn, K)) return rc;
    if (cr.lmeds) {
        if (!(std::isfinite(cr.scale2) && cr.scale2 >= 0.0)) return fail(ALP_EINVAL, "%s: scale2 must be finite and not negative", fn);
        if (!(std::isfinite(cr.floor2) && cr.floor2 >= 0.0)) return fail(ALP_EINVAL, "%s: floor2 must be finite and not negative", fn);
    } else if (!(std::isfinite(cr.threshold) && cr.threshold >= 0.0)) {
        return fail(ALP_EINVAL, "%s: threshold must be finite and not negative", fn);
    }
    if (!(refits >= 0 && refits <= EPI_MAX_REFITS)) return fail(ALP_EINVAL, "%s: refits must be 0..8", fn);
    if (int rc = epi_check_splits(fn, splits, n)) return rc;
    if (samples)
        if (int rc = epi_check_samples(fn, samples, H, n, width)) return rc;
    const int64_t HS = H * slots;       // hypothesis slots that are judged
    EpiCall c;
    if (int rc = c.reserve(n, HS, splits, cr.lmeds)) return rc;
    hipStream_t st = ctx().stream;
    EpiState host_state;
    hipError_t e = c.upload(p1, p2, n, !K);
    if (e == hipSuccess && samples) e = hipMemcpyAsync(c.samples(), samples, (size_t)H * width * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        const double4 *pts = c.pts();
        EpiState *state = c.state();
        u64 *keys = (u64 *)c.err();     // LMedS: the error keys of one matrix, until the mask kernel writes the errors there
        const unsigned rb = (unsigned)c.p.reduce_blocks, nb = (unsigned)((n + 255) / 256);
        // LMedS judges the current matrix (round < 0, its value known: only the count) or the candidate of a refit round
        auto lmeds_eval = [&](int round) {
            hipLaunchKernelGGL(epi_errs_kernel, dim3(nb), dim3(256), 0, st, pts, (int)n, (const EpiState *)state, round < 0 ? 0 : 1, keys);
            hipLaunchKernelGGL(epi_lmeds_eval_kernel, dim3(1), dim3(EPI_SELECT1_BLOCK), 0, st, (const u64 *)keys, (int)n, round, state);
        };
        if (!samples) epi_launch_samples(width, n, H, seed, c.samples());
        c.launch_solver(H, K);
        if (cr.lmeds) {
            c.launch_select(n, HS, (int)cr.rank);
            hipLaunchKernelGGL(epi_lmeds_choose_kernel, dim3(1), dim3(256), 0, st, (const double *)c.value(), (int)HS, (const double *)c.F(), (int)cr.rank,
                               cr.scale2, cr.floor2, state);
            lmeds_eval(-1);
        } else {
            const double t2 = cr.threshold * cr.threshold;
            c.launch_score(n, HS, t2);
            hipLaunchKernelGGL(epi_choose_kernel, dim3(1), dim3(256), 0, st, (const int *)c.counts(), (int)HS, (const double *)c.F(), width, t2, state);
        }
        for (int r = 0; r < refits; ++r) {
            hipLaunchKernelGGL(epi_accum_kernel, dim3(rb), dim3(EPI_REDUCE_BLOCK), 0, st, pts, (int)n, (const EpiState *)state, c.sym());
            hipLaunchKernelGGL(epi_refit_kernel, dim3(1), dim3(64), 0, st, (const double *)c.sym(), (int)rb, state);
            if (cr.lmeds) {
                lmeds_eval(r);
            } else {
                hipLaunchKernelGGL(epi_count_kernel, dim3(rb), dim3(EPI_REDUCE_BLOCK), 0, st, pts, (int)n, (const EpiState *)state, c.cpart());
                hipLaunchKernelGGL(epi_decide_kernel, dim3(1), dim3(64), 0, st, (const int *)c.cpart(), (int)rb, r, state);
            }
        }
        hipLaunchKernelGGL(epi_mask_kernel, dim3(nb), dim3(256), 0, st, pts, (int)n, (const EpiState *)state, c.mask(), c.err());
        e = hipGetLastError();
    }
    if (e == hipSuccess && mask) e = hipMemcpyAsync(mask, c.mask(), (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&host_state, c.state(), sizeof(EpiState), hipMemcpyDeviceToHost, st);
    if (int rc = epi_finish(fn, e)) return rc;
    if (F) memcpy(F, host_state.Fcur, 72);
    if (info) {
        for (int k = 0; k < EPI_INFO; ++k) info[k] = host_state.info[k];
        c.plan_info(info + I_HYP_TILE, c.p.reduce_blocks);
        if (cr.lmeds) {
            info[I_PASSES] = c.p.passes, info[I_PASSES1] = EPI_SELECT1_PASSES, info[I_MATCH_TILES] = c.p.match_tiles;
            info[I_HIST_BYTES] = (int64_t)c.p.hist_bytes;
        }
    }
    if (stats) memcpy(stats, host_state.stats, sizeof(host_state.stats));
    return ALP_OK;
}

}  // namespace

extern "C" int alp_epipolar_samples(int64_t n, int64_t H, uint64_t seed, int32_t *samples) {
    return epi_samples(__func__, EPI_SAMPLE, n, H, seed, samples);
}

extern "C" int alp_epipolar_samples5(int64_t n, int64_t H, uint64_t seed, int32_t *samples) {
    return epi_samples(__func__, EPI_SAMPLE5, n, H, seed, samples);
}

extern "C" int alp_epipolar_ransac(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed,
                                   double threshold, int refits, int splits, double F[9], uint8_t *mask, int64_t info[24]) {
    return epi_filter(__func__, p1, p2, n, samples, H, seed, nullptr, EpiCriterion::count(threshold), refits, splits, F, mask, info, nullptr);
}

extern "C" int alp_essential_ransac(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed,
                                    const double K[3], double threshold, int refits, int splits, double F[9], uint8_t *mask, int64_t info[24]) {
    if (!K) return fail(ALP_EINVAL, "%s: NULL K", __func__);
    return epi_filter(__func__, p1, p2, n, samples, H, seed, K, EpiCriterion::count(threshold), refits, splits, F, mask, info, nullptr);
}

extern "C" int alp_epipolar_lmeds(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed, int64_t rank,
                                  double scale2, double floor2, int refits, int splits, double F[9], uint8_t *mask, int64_t info[24],
                                  double stats[12]) {
    return epi_filter(__func__, p1, p2, n, samples, H, seed, nullptr, EpiCriterion::value(rank, scale2, floor2), refits, splits, F, mask, info, stats);
}

extern "C" int alp_essential_lmeds(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed,
                                   const double K[3], int64_t rank, double scale2, double floor2, int refits, int splits, double F[9],
                                   uint8_t *mask, int64_t info[24], double stats[12]) {
    if (!K) return fail(ALP_EINVAL, "%s: NULL K", __func__);
    return epi_filter(__func__, p1, p2, n, samples, H, seed, K, EpiCriterion::value(rank, scale2, floor2), refits, splits, F, mask, info, stats);
}

extern "C" int alp_epipolar_solve8(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, double *F) {
    if (int rc = require_init()) return rc;
    if (int rc = epi_check_points(__func__, p1, p2, n, H)) return rc;
    ALP_REQUIRE(samples && F, "NULL samples or output");
    if (int rc = epi_check_samples(__func__, samples, H, n)) return rc;
    EpiCall c;
    if (int rc = c.reserve(n, H, 1)) return rc;
    hipStream_t st = ctx().stream;
    hipError_t e = c.upload(p1, p2, n, true);
    if (e == hipSuccess) e = hipMemcpyAsync(c.samples(), samples, (size_t)H * EPI_SAMPLE * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        c.launch_solver(H, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(F, c.F(), (size_t)H * 72, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}

extern "C" int alp_epipolar_score(const double *p1, const double *p2, int64_t n, const double *F, int64_t H, double threshold, int splits,
                                  int32_t *counts, int64_t info[6]) {
    if (int rc = require_init()) return rc;
    if (int rc = epi_check_points(__func__, p1, p2, n, H)) return rc;
    ALP_REQUIRE(F && counts, "NULL F or output");
    ALP_REQUIRE(std::isfinite(threshold) && threshold >= 0.0, "threshold must be finite and not negative");
    if (int rc = epi_check_splits(__func__, splits, n)) return rc;
    EpiCall c;
    if (int rc = c.reserve(n, H, splits)) return rc;
    if (info) c.plan_info(info, c.p.match_tiles);
    hipStream_t st = ctx().stream;
    hipError_t e = c.upload(p1, p2, n, false);
    if (e == hipSuccess) e = hipMemcpyAsync(c.F(), F, (size_t)H * 72, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        c.launch_score(n, H, threshold * threshold);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(counts, c.counts(), (size_t)H * 4, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}

extern "C" int alp_epipolar_mask(const double *p1, const double *p2, int64_t n, const double F[9], double threshold, uint8_t *mask,
                                 double *err) {
    if (int rc = require_init()) return rc;
    if (int rc = epi_check_points(__func__, p1, p2, n, 1)) return rc;
    ALP_REQUIRE(F, "NULL F");
    ALP_REQUIRE(std::isfinite(threshold) && threshold >= 0.0, "threshold must be finite and not negative");
    EpiCall c;
    if (int rc = c.reserve(n, 1, 1)) return rc;
    hipStream_t st = ctx().stream;
    hipError_t e = c.upload(p1, p2, n, false);
    // F and the bound go into the state record that upload() zeroed: Fcur and bound2 lie side by side, keep_all is 0
    double fb[10];
    memcpy(fb, F, 72);
    fb[9] = threshold * threshold;
    static_assert(offsetof(EpiState, bound2) == offsetof(EpiState, Fcur) + 72, "Fcur and bound2 are uploaded as one block");
    if (e == hipSuccess) e = hipMemcpyAsync(c.state()->Fcur, fb, sizeof(fb), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        hipLaunchKernelGGL(epi_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double4 *)c.pts(), (int)n,
                           (const EpiState *)c.state(), c.mask(), c.err());
        e = hipGetLastError();
    }
    if (e == hipSuccess && mask) e = hipMemcpyAsync(mask, c.mask(), (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && err) e = hipMemcpyAsync(err, c.err(), (size_t)n * 8, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}

extern "C" int alp_epipolar_select(const double *p1, const double *p2, int64_t n, const double *F, int64_t H, int64_t rank, int splits,
                                   double *value, int64_t info[8]) {
    if (int rc = require_init()) return rc;
    if (int rc = epi_check_points(__func__, p1, p2, n, H)) return rc;
    if (int rc = epi_check_select(__func__, n, H, 1, rank)) return rc;
    ALP_REQUIRE(F && value, "NULL F or output");
    if (int rc = epi_check_splits(__func__, splits, n)) return rc;
    EpiCall c;
    if (int rc = c.reserve(n, H, splits, true)) return rc;
    if (info) {
        c.plan_info(info, c.p.match_tiles);
        info[6] = c.p.passes, info[7] = (int64_t)c.p.hist_bytes;
    }
    hipStream_t st = ctx().stream;
    hipError_t e = c.upload(p1, p2, n, false);
    if (e == hipSuccess) e = hipMemcpyAsync(c.F(), F, (size_t)H * 72, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        c.launch_select(n, H, (int)rank);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(value, c.value(), (size_t)H * 8, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}

extern "C" int alp_epipolar_solve5(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, const double K[3],
                                   double *F, int32_t *nsol) {
    if (int rc = require_init()) return rc;
    if (int rc = epi_check_points(__func__, p1, p2, n, H, EPI_SLOTS5)) return rc;
    ALP_REQUIRE(samples && F && nsol, "NULL samples or output");
    if (int rc = epi_check_K(__func__, K)) return rc;
    if (int rc = epi_check_samples(__func__, samples, H, n, EPI_SAMPLE5)) return rc;
    EpiCall c;
    if (int rc = c.reserve(n, H * EPI_SLOTS5, 1)) return rc;
    hipStream_t st = ctx().stream;
    hipError_t e = c.upload(p1, p2, n, false);
    if (e == hipSuccess) e = hipMemcpyAsync(c.samples(), samples, (size_t)H * EPI_SAMPLE5 * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        c.launch_solver(H, K);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(F, c.F(), (size_t)H * EPI_SLOTS5 * 72, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(nsol, c.nsol(H), (size_t)H * 4, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}

extern "C" int alp_grid_thin(const int64_t *cell_id, const double *dist, int64_t n, uint8_t *mask) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(n >= 0 && n <= THIN_MAX_N, "n must be 0..2^30");
    if (n == 0) return ALP_OK;
    ALP_REQUIRE(cell_id && mask, "NULL input or output");
    int64_t lo = cell_id[0], hi = cell_id[0];
    for (int64_t i = 1; i < n; ++i) lo = std::min(lo, cell_id[i]), hi = std::max(hi, cell_id[i]);
    // (unsigned: the difference of two int64 may pass INT64_MAX)
    if ((uint64_t)hi - (uint64_t)lo >= (uint64_t)THIN_MAX_SPAN)
        return fail(ALP_EINVAL, "alp_grid_thin: cell ids span %lld..%lld, more than 2^26 cells", (long long)lo, (long long)hi);
    if (dist)
        for (int64_t i = 0; i < n; ++i)
            if (!(dist[i] >= 0.0)) return fail(ALP_EINVAL, "alp_grid_thin: dist[%lld] is negative or NaN", (long long)i);
    const size_t span = (size_t)(hi - lo) + 1;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) / 256 * 256;
        return o;
    };
    const size_t off_cell = take((size_t)n * 8), off_dist = take(dist ? (size_t)n * 8 : 0), off_tables = take(span * 16), off_mask = take((size_t)n);
    DeviceBuffer<char> dev;
    if (int rc = dev.reserve(at)) return rc;
    char *d = dev;
    long long *cell_dev = (long long *)(d + off_cell);
    double *dist_dev = dist ? (double *)(d + off_dist) : nullptr;
    u64 *best = (u64 *)(d + off_tables), *first = best + span;
    hipStream_t st = ctx().stream;
    hipError_t e = hipMemcpyAsync(cell_dev, cell_id, (size_t)n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && dist) e = hipMemcpyAsync(dist_dev, dist, (size_t)n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(best, 0xff, span * 16, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        const dim3 grid((unsigned)((n + 255) / 256));
        if (dist) hipLaunchKernelGGL(thin_dist_kernel, grid, dim3(256), 0, st, (const long long *)cell_dev, (const double *)dist_dev, (long long)n, (long long)lo, best);
        hipLaunchKernelGGL(thin_index_kernel, grid, dim3(256), 0, st, (const long long *)cell_dev, (const double *)dist_dev, (long long)n, (long long)lo,
                           (const u64 *)best, first);
        hipLaunchKernelGGL(thin_mask_kernel, grid, dim3(256), 0, st, (const long long *)cell_dev, (long long)n, (long long)lo, (const u64 *)first,
                           (unsigned char *)(d + off_mask));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(mask, d + off_mask, (size_t)n, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}
