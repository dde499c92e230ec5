// Part of alp_epipolar.hip (one translation unit, included inside its anonymous namespace; not a stand-alone header): what
// every stage of the match filters shares -- the state record of the device loop and its two transitions, the error of a
// match under F, and the workgroup reductions.
#pragma once

typedef unsigned long long u64;

struct EpiState {
    double T[6];                  // cx1, cy1, s1, cx2, cy2, s2: x' = (x - c) * s
    // the current matrix and the squared bound in force: a match is an inlier iff e <= bound2.  RANSAC: threshold^2, written
    // once by its choose kernel; LMedS: what the value of Fcur sets.  (Side by side: alp_epipolar_mask uploads both at once.)
    double Fcur[9], bound2;
    double Fcand[9];
    long long info[EPI_INFO];
    int count, stopped, keep_all; // count: the inliers of Fcur at bound2
    int essential;                // T is K twice over (cx, cy, 1 / f) and a fitted matrix is projected onto the essential ones
    // the LMedS filter (alp_epipolar_lmeds / alp_essential_lmeds)
    int rank;                     // 1-based, the order statistic that is a hypothesis' value
    double scale2, floor2;        // bound2 = max(scale2 * value, floor2)
    double value;                 // of Fcur
    double stats[EPI_LMEDS_STATS];
};
static_assert(sizeof(EpiState) <= EPI_STATE_BYTES, "the state record outgrew its slot");

// info words of the four filters; those from I_PASSES on are the LMedS ones', past the refit counts
enum { I_CHOSEN = 0, I_CHOSEN_COUNT, I_FINAL_COUNT, I_REFITS_RUN, I_REFITS_KEPT, I_KEEP_ALL, I_HYP_TILE, I_MATCH_TILE, I_SPLITS,
       I_WORKGROUPS, I_BYTES, I_REDUCE_BLOCKS, I_REFIT_COUNT0, I_PASSES = 20, I_PASSES1, I_MATCH_TILES, I_HIST_BYTES };
enum { S_CHOSEN_VALUE = 0, S_FINAL_VALUE, S_BOUND2, S_REFIT_VALUE0 };         // stats words
static_assert(I_REFIT_COUNT0 + EPI_MAX_REFITS <= I_PASSES && I_HIST_BYTES < EPI_INFO && S_REFIT_VALUE0 + EPI_MAX_REFITS <= EPI_LMEDS_STATS,
              "info or stats too short");

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000ll); }

// A run begins: hypothesis idx of F is the current matrix, with `count` inliers; keep_all: no hypothesis is good enough, every
// match is kept and no refit runs.  Whoever calls this sets bound2 and its own info and stats words.
__device__ void epi_begin(EpiState *__restrict__ st, const double *__restrict__ F, int idx, int count, bool keep_all) {
    for (int k = 0; k < 9; ++k) st->Fcur[k] = F[(size_t)idx * 9 + k], st->Fcand[k] = nan64();
    for (int k = 0; k < EPI_INFO; ++k) st->info[k] = 0;
    for (int k = 0; k < EPI_MAX_REFITS; ++k) st->info[I_REFIT_COUNT0 + k] = -1;
    st->count = count;
    st->keep_all = st->stopped = keep_all ? 1 : 0;
    st->info[I_CHOSEN] = idx, st->info[I_CHOSEN_COUNT] = st->info[I_FINAL_COUNT] = count, st->info[I_KEEP_ALL] = st->keep_all;
}

// Refit `round` gave a candidate with c inliers: when it is better it becomes the current matrix, otherwise the loop stops.
__device__ bool epi_accept(EpiState *__restrict__ st, int round, int c, bool better) {
    st->info[I_REFIT_COUNT0 + round] = c;
    st->info[I_REFITS_RUN] = round + 1;
    if (better) {
        for (int k = 0; k < 9; ++k) st->Fcur[k] = st->Fcand[k];
        st->count = c;
        st->info[I_FINAL_COUNT] = c;
        st->info[I_REFITS_KEPT] += 1;
    } else {
        st->stopped = 1;
    }
    return better;
}

// the three quantities of the error expression, in the header's order
__device__ __forceinline__ void epi_terms(const double (&F)[9], double x1, double y1, double x2, double y2, double &ss, double &d2,
                                          double &d1) {
    const double l20 = (F[0] * x1 + F[1] * y1) + F[2];
    const double l21 = (F[3] * x1 + F[4] * y1) + F[5];
    const double l22 = (F[6] * x1 + F[7] * y1) + F[8];
    const double l10 = (F[0] * x2 + F[3] * y2) + F[6];
    const double l11 = (F[1] * x2 + F[4] * y2) + F[7];
    const double s = (x2 * l20 + y2 * l21) + l22;
    ss = s * s;
    d2 = l20 * l20 + l21 * l21;
    d1 = l10 * l10 + l11 * l11;
}

// e as written: the larger of the two quotients, NaN when either is
__device__ __forceinline__ double epi_error(const double (&F)[9], const double4 q) {
    double ss, d2, d1;
    epi_terms(F, q.x, q.y, q.z, q.w, ss, d2, d1);
    const double e2 = ss / d2, e1 = ss / d1;
    return e2 != e2 ? e2 : e1 != e1 ? e1 : e2 > e1 ? e2 : e1;
}

// e with one division (the score and select kernels): the larger quotient is the one by the smaller divisor, s2 / min(a, b) =
// max(s2 / a, s2 / b) bit for bit, since a correctly rounded quotient is monotone in its divisor.  Where the two differ, one
// is NaN and the other +inf (s2 = inf over one infinite divisor), which no compare and no key tells apart.
__device__ __forceinline__ double epi_error1(const double (&F)[9], const double4 q) {
    double ss, d2, d1;
    epi_terms(F, q.x, q.y, q.z, q.w, ss, d2, d1);
    double dm = d1 < d2 ? d1 : d2;
    if (d1 != d1) dm = d1;
    return ss / dm;
}

// An error is a non-negative double or +inf once a NaN counts as +inf, so errors order as their bit patterns do as unsigned
// integers: the key of an error.
constexpr u64 EPI_KEY_INF = 0x7ff0000000000000ull;
__device__ __forceinline__ u64 epi_key_of(double e) { return e != e ? EPI_KEY_INF : (u64)__double_as_longlong(e); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the sum of v over a workgroup of 256, the same value in every thread (buf: 4 doubles of LDS)
__device__ __forceinline__ double block_sum256(double v, double *buf) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    return (buf[0] + buf[1]) + (buf[2] + buf[3]);
}

// the sum of c over a workgroup of WAVES waves, in thread 0 alone (red: WAVES ints of LDS)
template <int WAVES>
__device__ __forceinline__ int block_count(int c, int *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    c = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < WAVES; ++w) c += red[w];
    return c;
}
