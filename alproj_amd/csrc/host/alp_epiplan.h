// Launch planning of the geometric match filter (alp_epipolar.hip: alp_epipolar_samples / _solve8 / _score / _mask / _ransac):
// the hypothesis tile of a workgroup, the match tile it stages in LDS, how the match tiles are divided among the splits, the
// blocks of the refit's reductions, the offsets of every array in the call's one device block, and the caps.
// Integer arithmetic on (n, H, forced splits, cu_count) alone; the caller allocates and launches.
// Included by host/alp_host.h after host/alp_matchplan.h; no HIP header.  host/alp_host_selfcheck.cpp sweeps it (check_epi_plan).
#pragma once

#include <cstddef>
#include <cstdint>

namespace alp {

constexpr int EPI_SAMPLE = 8;                  // matches of a minimal sample of the fundamental filter
constexpr int EPI_SAMPLE5 = 5;                 // and of the essential filter,
constexpr int EPI_SLOTS5 = 10;                 // whose every sample fills up to ten hypothesis slots: it is planned as H' = 10 H
constexpr int EPI_HYP_TILE = 256;              // hypotheses of a workgroup of the score kernel: one per lane
constexpr int EPI_MATCH_TILE = 512;            // matches staged in LDS at a time, 32 B each
constexpr int EPI_SOLVE_BLOCK = 64;            // hypotheses of a workgroup of the solve kernel: one per lane, its 8 x 9 matrix in LDS
constexpr int EPI_REDUCE_BLOCK = 256;          // threads of a workgroup of the refit's reductions over the matches
constexpr int EPI_REDUCE_MAX_BLOCKS = 256;
constexpr int EPI_SYM = 45;                    // entries of the upper triangle of the refit's 9 x 9 matrix
constexpr int EPI_MAX_REFITS = 8;
constexpr int EPI_INFO = 24;                   // int64 words of alp_epipolar_ransac's info
constexpr int EPI_STATE_BYTES = 1024;          // the device loop's state record
constexpr int64_t EPI_MIN_N = 8, EPI_MAX_N = (int64_t)1 << 20, EPI_MAX_H = (int64_t)1 << 20;
// H * n error evaluations of one call: a count is at most n <= 2^20 and fits int32 whatever H; 2^35 evaluations are a fraction
// of a second of the score kernel
constexpr int64_t EPI_MAX_WORK = (int64_t)1 << 35;
// the LMedS filter's select over the hypotheses: a radix select on the 64 bits of an error, 4 bits a pass
constexpr int EPI_SELECT_BITS = 4, EPI_SELECT_DIGITS = 1 << EPI_SELECT_BITS, EPI_SELECT_PASSES = 64 / EPI_SELECT_BITS;
constexpr int EPI_SELECT1_BLOCK = 1024;        // threads of the one workgroup that selects over the error array of one F,
constexpr int EPI_SELECT1_PASSES = 8;          // 8 bits a pass
constexpr int EPI_LMEDS_STATS = 12;            // doubles of alp_epipolar_lmeds' stats
constexpr int64_t THIN_MAX_N = (int64_t)1 << 30;
constexpr int64_t THIN_MAX_SPAN = (int64_t)1 << 26;      // cells of alp_grid_thin's table

namespace host {

struct EpiPlan {
    int hyp_tile = EPI_HYP_TILE, match_tile = EPI_MATCH_TILE;
    int splits = 0;
    int reduce_blocks = 0;                // workgroups of the refit's accumulation and count
    int64_t hyp_tiles = 0, match_tiles = 0;
    int64_t h_pad = 0;                    // hypotheses rounded up to whole tiles: the row length of the partial counts
    int64_t workgroups = 0;               // hyp_tiles * splits
    int64_t solve_blocks = 0;
    // byte offsets in the call's device block (each a multiple of 256) and its size
    size_t off_raw1 = 0, off_raw2 = 0, off_pts = 0, off_samples = 0, off_F = 0, off_partial = 0, off_counts = 0, off_state = 0,
           off_sym = 0, off_cpart = 0, off_mask = 0, off_err = 0, scratch_bytes = 0;
    // epi_select_plan alone: the passes of the select over the hypotheses and its arrays, after all of the above
    int passes = 0;
    size_t hist_bytes = 0, off_hist = 0, off_prefix = 0, off_rank = 0, off_value = 0;
};

// n in [8, 2^20] (min_n = 5: the essential filter), H in [1, 2^20], H * n <= 2^35: what every entry point of the unit requires
// before it plans
inline bool epi_caps_ok(int64_t n, int64_t H, int64_t min_n = EPI_MIN_N) {
    return n >= min_n && n <= EPI_MAX_N && H >= 1 && H <= EPI_MAX_H && H <= EPI_MAX_WORK / n;
}

// splits: as many as bring the grid to four workgroups per CU, at most one per match tile; `forced` > 0 replaces the choice (the
// caller has refused forced > match_tiles)
inline EpiPlan epi_plan(int64_t n, int64_t H, int forced, int cu_count) {
    EpiPlan p;
    p.hyp_tiles = (H + EPI_HYP_TILE - 1) / EPI_HYP_TILE;
    p.match_tiles = (n + EPI_MATCH_TILE - 1) / EPI_MATCH_TILE;
    p.h_pad = p.hyp_tiles * EPI_HYP_TILE;
    if (forced > 0) p.splits = forced;
    else {
        const int64_t aim = 4 * (int64_t)(cu_count > 0 ? cu_count : 1);
        int64_t s = p.hyp_tiles > 0 ? (aim + p.hyp_tiles - 1) / p.hyp_tiles : 1;
        if (s > p.match_tiles) s = p.match_tiles;
        p.splits = (int)(s < 1 ? 1 : s);
    }
    p.workgroups = p.hyp_tiles * p.splits;
    p.solve_blocks = (H + EPI_SOLVE_BLOCK - 1) / EPI_SOLVE_BLOCK;
    const int64_t rb = (n + EPI_REDUCE_BLOCK - 1) / EPI_REDUCE_BLOCK;
    p.reduce_blocks = (int)(rb > EPI_REDUCE_MAX_BLOCKS ? EPI_REDUCE_MAX_BLOCKS : rb < 1 ? 1 : rb);
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) / 256 * 256;
        return o;
    };
    p.off_raw1 = take((size_t)n * 16);
    p.off_raw2 = take((size_t)n * 16);
    p.off_pts = take((size_t)n * 32);
    p.off_samples = take((size_t)H * EPI_SAMPLE * 4);
    p.off_F = take((size_t)H * 72);
    p.off_partial = take((size_t)p.splits * p.h_pad * 4);
    p.off_counts = take((size_t)H * 4);
    p.off_state = take(EPI_STATE_BYTES);
    p.off_sym = take((size_t)p.reduce_blocks * EPI_SYM * 8);
    p.off_cpart = take((size_t)p.reduce_blocks * 4);
    p.off_mask = take((size_t)n);
    p.off_err = take((size_t)n * 8);
    p.scratch_bytes = at;
    return p;
}

// passes * H * n <= 2^35 on top of epi_caps_ok: every pass of the select forms every error again
inline bool epi_select_caps_ok(int64_t n, int64_t H, int64_t min_n = EPI_MIN_N) {
    return epi_caps_ok(n, H, min_n) && H <= EPI_MAX_WORK / EPI_SELECT_PASSES / n;
}

// epi_plan with the arrays of the LMedS select appended: every offset of epi_plan stays what it is.  The partial histograms are
// [splits][16][h_pad] counters, counter d of hypothesis h in split s at (s * 16 + d) * h_pad + h; prefix and rank have a word per
// padded hypothesis (the lanes past H run on all-NaN matrices), value one per hypothesis.
inline EpiPlan epi_select_plan(int64_t n, int64_t H, int forced, int cu_count) {
    EpiPlan p = epi_plan(n, H, forced, cu_count);
    size_t at = p.scratch_bytes;
    auto take = [&at](size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) / 256 * 256;
        return o;
    };
    p.passes = EPI_SELECT_PASSES;
    p.hist_bytes = (size_t)p.splits * EPI_SELECT_DIGITS * p.h_pad * 4;
    p.off_hist = take(p.hist_bytes);
    p.off_prefix = take((size_t)p.h_pad * 8);
    p.off_rank = take((size_t)p.h_pad * 4);
    p.off_value = take((size_t)H * 8);
    p.scratch_bytes = at;
    return p;
}

}  // namespace host
}  // namespace alp
