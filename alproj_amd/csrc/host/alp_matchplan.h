// Launch planning of the descriptor matcher (alp_match.hip: alp_match_knn2): the K steps of the int8 MFMA a descriptor length
// pads to, the query tile of a workgroup, the train tiles and how they are divided among the splits, the padded arrays and the
// offsets of every array in the call's one device block.
// Integer arithmetic on (n_query, n_train, len, element size, forced splits, cu_count) alone; the caller allocates and launches.
// Included by host/alp_host.h after host/alp_fold.h (ALP_HD); no HIP header.  host/alp_host_selfcheck.cpp sweeps it (check_match_plan).
#pragma once

#include <cstddef>
#include <cstdint>

namespace alp {

constexpr int MATCH_K = 32;               // bytes of one descriptor that one 32x32x32 MFMA contracts
constexpr int MATCH_TRAIN_TILE = 32;      // train rows of one MFMA: the accumulator's rows
constexpr int MATCH_GROUP = 32;           // queries of one MFMA: the accumulator's columns, one per lane of a half wave
constexpr int MATCH_WAVES = 4;            // waves of a workgroup, each with its own query groups
constexpr int MATCH_MAX_LEN = 512;
constexpr int64_t MATCH_MAX_PACKED = (int64_t)1 << 31;      // bytes of one padded descriptor array
// the K-step counts the walk kernel is instantiated for: a length pads to the first one that holds it
constexpr int MATCH_KSTEPS[] = {1, 2, 3, 4, 6, 8, 12, 16};
constexpr int MATCH_PAD_NORM = 1 << 30;   // the "squared norm" of a padding train row: far above 2 * 512 * 128^2, far below 2^31

// train tiles [begin, end) of split s of S: contiguous, in order, sizes that differ by at most one, none empty when S <= tiles
ALP_HD inline void match_split_range(int64_t tiles, int S, int s, int64_t *begin, int64_t *end) {
    *begin = tiles * s / S;
    *end = tiles * (s + 1) / S;
}

namespace host {

inline int match_ksteps(int len) {
    for (int ks : MATCH_KSTEPS)
        if (ks * MATCH_K >= len) return ks;
    return 0;
}

// query groups per wave: two while the queries' fragments are few registers (each train fragment then feeds two accumulators)
inline int match_groups_per_wave(int ksteps) { return ksteps <= 4 ? 2 : 1; }

struct MatchPlan {
    int ksteps = 0, groups = 0;           // MFMA K steps per tile; query groups per wave
    int padded_len = 0;                   // ksteps * 32
    int query_tile = 0, train_tile = MATCH_TRAIN_TILE;
    int splits = 0;
    int64_t query_tiles = 0, train_tiles = 0;
    int64_t nq_pad = 0, nt_pad = 0;       // rows of the packed arrays
    int64_t workgroups = 0;               // query_tiles * splits
    // byte offsets in the call's device block (each a multiple of 256) and its size
    size_t off_raw_q = 0, off_raw_t = 0, off_pack_q = 0, off_pack_t = 0, off_norm_q = 0, off_norm_t = 0, off_partial = 0,
           off_idx = 0, off_dist2 = 0, off_dist = 0, off_good = 0, off_flags = 0, scratch_bytes = 0;
};

// splits: as many as bring the grid to two workgroups per CU, at most one per train tile; `forced` > 0 replaces the choice (the
// caller has refused forced > train_tiles)
inline MatchPlan match_plan(int64_t n_query, int64_t n_train, int len, int esize, int forced, int cu_count) {
    MatchPlan p;
    p.ksteps = match_ksteps(len);
    p.groups = match_groups_per_wave(p.ksteps);
    p.padded_len = p.ksteps * MATCH_K;
    p.query_tile = MATCH_WAVES * p.groups * MATCH_GROUP;
    p.query_tiles = (n_query + p.query_tile - 1) / p.query_tile;
    p.train_tiles = (n_train + MATCH_TRAIN_TILE - 1) / MATCH_TRAIN_TILE;
    p.nq_pad = p.query_tiles * p.query_tile;
    p.nt_pad = p.train_tiles * MATCH_TRAIN_TILE;
    if (forced > 0) p.splits = forced;
    else {
        const int64_t aim = 2 * (int64_t)(cu_count > 0 ? cu_count : 1);
        int64_t s = p.query_tiles > 0 ? (aim + p.query_tiles - 1) / p.query_tiles : 1;
        if (s > p.train_tiles) s = p.train_tiles;
        p.splits = (int)(s < 1 ? 1 : s);
    }
    p.workgroups = p.query_tiles * p.splits;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) / 256 * 256;
        return o;
    };
    p.off_raw_q = take((size_t)n_query * len * esize);
    p.off_raw_t = take((size_t)n_train * len * esize);
    p.off_pack_q = take((size_t)p.nq_pad * p.padded_len);
    p.off_pack_t = take((size_t)p.nt_pad * p.padded_len);
    p.off_norm_q = take((size_t)p.nq_pad * 4);
    p.off_norm_t = take((size_t)p.nt_pad * 4);
    p.off_partial = take((size_t)p.splits * p.nq_pad * 16);
    p.off_idx = take((size_t)n_query * 8);
    p.off_dist2 = take((size_t)n_query * 8);
    p.off_dist = take((size_t)n_query * 8);
    p.off_good = take((size_t)n_query);
    p.off_flags = take(32);               // n_good, the lowest offending index of the queries, of the train rows
    p.scratch_bytes = at;
    return p;
}

// where byte k of row `row` lies in a packed array: tile by tile, K step by K step, the 16 bytes of lane (k / 16 % 2) * 32 + row % 32
inline size_t match_packed_offset(int64_t row, int k, int ksteps) {
    const int64_t tile = row / MATCH_GROUP;
    const int lane = (k / 16 % 2) * 32 + (int)(row % MATCH_GROUP);
    return (((size_t)tile * ksteps + k / MATCH_K) * 64 + lane) * 16 + k % 16;
}

}  // namespace host
}  // namespace alp
