// libalproj_hip.so -- descriptor matching: the exact brute-force 2-nearest-neighbour search and Lowe's ratio test of the
// reference's built-in matchers (src/alproj/gcp.py:55-70: cv2.BFMatcher() with its default NORM_L2, knnMatch(k = 2), then
// m.distance < ratio * n.distance).
//
// AKAZE descriptors are bytes and OpenCV's SIFT descriptors are float32 holding the integers 0..255, so every squared distance is
// an integer.  Both sides are shifted to signed bytes (a' = a - 128) and
//     |q - t|^2 = |q'|^2 + |t'|^2 - 2 q'.t'
// with the inner products on the int8 matrix cores (v_mfma_i32_32x32x32_i8, int32 accumulators); the length is padded to the MFMA's
// K step with the byte 128, which is 0 after the shift.  No floating point before the final square root, so the unit needs no
// -ffp-contract=off.
//
//   match_pack_kernel   raw rows (uint8, or float32 checked to be integers 0..255: the lowest offending flat index is kept by an
//                       atomic minimum) -> shifted bytes in fragment order + MINUS the squared norm per row.  Fragment order: tile
//                       of 32 rows by tile, K step by K step, the 16 bytes of lane l = 32 h + r are bytes 32 step + 16 h .. + 15 of
//                       row r (host/alp_matchplan.h: match_packed_offset), so that a wave reads one operand of one MFMA as one
//                       contiguous KiB.  Queries and train rows are packed alike: whatever k the hardware gives byte j of lane
//                       half h, it is the same k on the A and the B side, and a sum over k does not care about its order.
//   match_walk_kernel   a workgroup = 4 waves x G groups of 32 queries (its query tile) x one split of the train tiles.  B = the
//                       queries, kept in registers for the whole walk; A = one train tile after the other, read straight from
//                       global memory (the next tile's fragments are in flight during this tile's MFMAs).  In the C/D map
//                       col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) the query is the lane's, so each lane
//                       keeps the best two of ITS query over the rows it sees and no lane talks to another until the end.
//                       Per tile and lane: m = 2 q'.t' - |t'|^2 for its 16 rows (|q'|^2 is the same for all of them) and their
//                       maximum; only when some lane's maximum reaches its second best does the wave test the rows one by one
//                       and run, for a row that some lane needs, the two minimum-updates on the keys
//                       (uint64) d^2 << 32 | train index -- order by (d^2, index), the lower index first on a tie.  A padding
//                       row has "norm" 2^30 and an all-ones key.  At the end the two lane halves are merged by a lane exchange
//                       and (query, split) gets its best two keys.
//   match_merge_kernel  a thread per query: the best two over the splits, then idx, dist2, dist = the correctly rounded float32
//                       square root of (float) dist2, good = (double) dist[0] < ratio * (double) dist[1], and the count of good.
#include "alp_internal.h"

#include <climits>
#include <cmath>

namespace {

using namespace alp;

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr u64 KEY_NONE = ~0ull;

// one thread per 16 packed bytes.  negnorm (zeroed before) receives minus the sum of squares of the shifted bytes; a padding row
// receives -MATCH_PAD_NORM when pad_norm is set (the train side).  `bad`: the lowest flat index of a value that is not an integer
// in 0..255 (float32 input only).
template <typename T>
__global__ __launch_bounds__(256) void match_pack_kernel(const T *__restrict__ src, long long n, int len, int ksteps, long long chunks,
                                                         int pad_norm, v4i *__restrict__ packed, int *__restrict__ negnorm,
                                                         u64 *__restrict__ bad) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= chunks) return;
    const int lane = (int)(g & 63);
    const long long ts = g >> 6;
    const int step = (int)(ts % ksteps);
    const long long row = ts / ksteps * MATCH_GROUP + (lane & 31);
    const int k0 = step * MATCH_K + (lane >> 5) * 16;
    int w[4] = {0, 0, 0, 0}, sum = 0;
    if (row < n) {
        for (int j = 0; j < 16; ++j) {
            const int k = k0 + j;
            int v = 128;
            if (k < len) {
                const long long at = row * len + k;
                if constexpr (sizeof(T) == 1) v = (int)src[at];
                else {
                    const float f = (float)src[at];
                    if (f >= 0.0f && f <= 255.0f && f == truncf(f)) v = (int)f;
                    else atomicMin(bad, (u64)at);
                }
            }
            const int s = v - 128;
            sum += s * s;
            w[j >> 2] |= (s & 255) << (8 * (j & 3));
        }
        if (sum) atomicSub(negnorm + row, sum);
    } else if (pad_norm && step == 0 && lane < 32) {
        atomicSub(negnorm + row, MATCH_PAD_NORM);
    }
    v4i o;
    o.x = w[0], o.y = w[1], o.z = w[2], o.w = w[3];
    packed[g] = o;
}

__device__ __forceinline__ u64 exchange_half(u64 v) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, 32, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), 32, 64);
    return (u64)hi << 32 | lo;
}
__device__ __forceinline__ u64 min64(u64 a, u64 b) { return a < b ? a : b; }
__device__ __forceinline__ u64 max64(u64 a, u64 b) { return a < b ? b : a; }

// the best two of two best-two pairs (a0 <= a1, b0 <= b1; keys of real rows are distinct)
__device__ __forceinline__ void merge_pairs(u64 &a0, u64 &a1, u64 b0, u64 b1) {
    const u64 hi = min64(max64(a0, b0), min64(a1, b1));
    a0 = min64(a0, b0);
    a1 = hi;
}

template <int KS, int QG>
__global__ __launch_bounds__(256) void match_walk_kernel(const v4i *__restrict__ qp, const v4i *__restrict__ tp,
                                                         const int *__restrict__ qneg, const int *__restrict__ tneg, int n_train,
                                                         long long train_tiles, int splits, long long nq_pad, u64 *__restrict__ partial) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
    const long long qtile = blockIdx.x / (unsigned)splits;
    const int split = (int)(blockIdx.x % (unsigned)splits);
    const long long group0 = (qtile * MATCH_WAVES + wave) * QG;
    v4i b[QG][KS];
    int qn[QG], thr[QG];
    u64 best0[QG], best1[QG];
#pragma unroll
    for (int g = 0; g < QG; ++g) {
#pragma unroll
        for (int k = 0; k < KS; ++k) b[g][k] = qp[((group0 + g) * KS + k) * 64 + lane];
        qn[g] = -qneg[(group0 + g) * MATCH_GROUP + col];
        thr[g] = INT_MIN;
        best0[g] = best1[g] = KEY_NONE;
    }
    int64_t tb, te;
    match_split_range(train_tiles, splits, split, &tb, &te);
    v4i a[KS], an[KS];
    if (tb < te) {
#pragma unroll
        for (int k = 0; k < KS; ++k) a[k] = tp[(tb * KS + k) * 64 + lane];
    }
    for (long long t = tb; t < te; ++t) {
        const long long tnext = t + 1 < te ? t + 1 : t;       // the last tile once more: never past the array
#pragma unroll
        for (int k = 0; k < KS; ++k) an[k] = tp[(tnext * KS + k) * 64 + lane];
        v4i nt[4];                                            // minus the norms of rows 8 j + 4 half + 0..3 of the tile
#pragma unroll
        for (int j = 0; j < 4; ++j) nt[j] = ((const v4i *)tneg)[t * 8 + 2 * j + half];
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < KS; ++k) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[k], b[g][k], acc, 0, 0, 0);
            int m[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) m[r] = (acc[r] << 1) + nt[r >> 2][r & 3];
            int mx = m[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = max(mx, m[r]);
            if (__ballot(mx >= thr[g]) != 0) {
                // some lane has a row that may enter its best two.  Early in a walk that is most tiles (a lane's second best falls
                // as 1 / rows seen), so the rows are tested one by one and only those that some lane needs pay for the key
                u64 k0 = best0[g], k1 = best1[g];
                int th = thr[g];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (__ballot(m[r] >= th) == 0) continue;
                    const long long idx = t * MATCH_TRAIN_TILE + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const u64 key = idx < n_train ? (u64)(unsigned)(qn[g] - m[r]) << 32 | (u64)idx : KEY_NONE;
                    k1 = min64(k1, max64(k0, key));
                    k0 = min64(k0, key);
                    th = k1 == KEY_NONE ? INT_MIN : qn[g] - (int)(k1 >> 32);
                }
                best0[g] = k0, best1[g] = k1, thr[g] = th;
            }
        }
#pragma unroll
        for (int k = 0; k < KS; ++k) a[k] = an[k];
    }
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        u64 k0 = best0[g], k1 = best1[g];
        const u64 o0 = exchange_half(k0), o1 = exchange_half(k1);
        merge_pairs(k0, k1, o0, o1);
        if (half == 0) {
            u64 *out = partial + ((size_t)split * nq_pad + (group0 + g) * MATCH_GROUP + col) * 2;
            out[0] = k0, out[1] = k1;
        }
    }
}

__global__ __launch_bounds__(256) void match_merge_kernel(const u64 *__restrict__ partial, int splits, long long nq_pad, long long n_query,
                                                          double ratio, int *__restrict__ idx, int *__restrict__ dist2,
                                                          float *__restrict__ dist, unsigned char *__restrict__ good,
                                                          u64 *__restrict__ n_good) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    bool ok = false;
    if (q < n_query) {
        u64 k0 = KEY_NONE, k1 = KEY_NONE;
        for (int s = 0; s < splits; ++s) {
            const u64 *in = partial + ((size_t)s * nq_pad + q) * 2;
            merge_pairs(k0, k1, in[0], in[1]);
        }
        const int d0 = (int)(k0 >> 32), d1 = (int)(k1 >> 32);
        // the correctly rounded float32 root whatever the unit's flags: the float64 root (IEEE) rounded once more -- 53 bits are
        // at least 2 * 24 + 2, so the second rounding cannot change the result (the intrinsic of that name is the native approximation)
        const float r0 = (float)sqrt((double)(float)d0), r1 = (float)sqrt((double)(float)d1);
        ok = (double)r0 < ratio * (double)r1;
        idx[2 * q] = (int)(unsigned)k0, idx[2 * q + 1] = (int)(unsigned)k1;
        dist2[2 * q] = d0, dist2[2 * q + 1] = d1;
        dist[2 * q] = r0, dist[2 * q + 1] = r1;
        good[q] = ok ? 1 : 0;
    }
    const u64 mask = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(n_good, (u64)__popcll(mask));
}

template <int KS>
void walk_launch(const host::MatchPlan &p, hipStream_t st, const v4i *qp, const v4i *tp, const int *qneg, const int *tneg, int n_train,
                 u64 *partial) {
    constexpr int QG = KS <= 4 ? 2 : 1;
    hipLaunchKernelGGL((match_walk_kernel<KS, QG>), dim3((unsigned)p.workgroups), dim3(256), 0, st, qp, tp, qneg, tneg, n_train,
                       (long long)p.train_tiles, p.splits, (long long)p.nq_pad, partial);
}

template <typename T>
void pack_launch(hipStream_t st, const void *src, int64_t n, int64_t n_pad, int len, int ksteps, int pad_norm, v4i *packed, int *negnorm,
                 u64 *bad) {
    const long long chunks = (long long)n_pad * ksteps * 2;
    hipLaunchKernelGGL(match_pack_kernel<T>, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st, (const T *)src, (long long)n, len,
                       ksteps, chunks, pad_norm, packed, negnorm, bad);
}

}  // namespace

extern "C" int alp_match_knn2(const void *query, int64_t n_query, const void *train, int64_t n_train, int len, int dtype, double ratio,
                              int splits, int32_t *idx, int32_t *dist2, float *dist, uint8_t *good, int64_t *n_good, int64_t info[6]) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(n_query >= 0, "n_query is negative");
    ALP_REQUIRE(dtype == ALP_U8 || dtype == ALP_F32, "dtype must be ALP_U8, or ALP_F32 holding the integers 0..255");
    ALP_REQUIRE(len >= 1 && len <= MATCH_MAX_LEN, "len must be 1..512");
    ALP_REQUIRE(n_train >= 2, "n_train must be at least 2: there is no second neighbour otherwise");
    ALP_REQUIRE(std::isfinite(ratio), "ratio must be finite");
    ALP_REQUIRE(splits >= 0, "splits is negative");
    ALP_REQUIRE(train && (query || n_query == 0), "NULL input");
    const int esize = dtype == ALP_U8 ? 1 : 4;
    const int64_t train_tiles = (n_train + MATCH_TRAIN_TILE - 1) / MATCH_TRAIN_TILE;
    if (splits > train_tiles)
        return fail(ALP_EINVAL, "alp_match_knn2: splits = %d, but %lld train rows are only %lld tiles of %d", splits, (long long)n_train,
                    (long long)train_tiles, MATCH_TRAIN_TILE);
    const int padded = host::match_ksteps(len) * MATCH_K;
    // (the bound is taken before the plan multiplies anything: 2^31 bytes at one byte per padded element)
    ALP_REQUIRE(n_query <= MATCH_MAX_PACKED / padded - 256 && n_train <= MATCH_MAX_PACKED / padded - 256,
                "a padded descriptor array would pass 2^31 bytes");
    const host::MatchPlan p = host::match_plan(n_query, n_train, len, esize, splits, ctx().cu_count);
    ALP_REQUIRE(p.workgroups <= INT_MAX, "query tiles x splits pass 2^31 workgroups");
    if (info) {
        info[0] = p.query_tile, info[1] = p.train_tile, info[2] = p.splits, info[3] = p.padded_len, info[4] = p.workgroups;
        info[5] = (int64_t)p.scratch_bytes;
    }
    if (n_good) *n_good = 0;
    if (n_query == 0) return ALP_OK;

    DeviceBuffer<char> dev;
    if (int rc = dev.reserve(p.scratch_bytes)) return rc;
    char *d = dev;
    v4i *pack_q = (v4i *)(d + p.off_pack_q), *pack_t = (v4i *)(d + p.off_pack_t);
    int *norm_q = (int *)(d + p.off_norm_q), *norm_t = (int *)(d + p.off_norm_t);
    u64 *partial = (u64 *)(d + p.off_partial), *flags = (u64 *)(d + p.off_flags);
    int *idx_dev = (int *)(d + p.off_idx), *dist2_dev = (int *)(d + p.off_dist2);
    float *dist_dev = (float *)(d + p.off_dist);
    unsigned char *good_dev = (unsigned char *)(d + p.off_good);
    hipStream_t st = ctx().stream;
    const u64 flags0[3] = {0, KEY_NONE, KEY_NONE};
    u64 flags_host[3] = {0, 0, 0};
    // from here on every failure still waits for the stream: the copies read and write the caller's arrays and this call's device block
    hipError_t e = hipMemcpyAsync(d + p.off_raw_q, query, (size_t)n_query * len * esize, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + p.off_raw_t, train, (size_t)n_train * len * esize, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(flags, flags0, sizeof(flags0), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(norm_q, 0, p.off_partial - p.off_norm_q, st);        // both norm arrays: they are adjacent
    if (e == hipSuccess) {
        KTimeScope kt;
        if (dtype == ALP_U8) {
            pack_launch<unsigned char>(st, d + p.off_raw_q, n_query, p.nq_pad, len, p.ksteps, 0, pack_q, norm_q, flags + 1);
            pack_launch<unsigned char>(st, d + p.off_raw_t, n_train, p.nt_pad, len, p.ksteps, 1, pack_t, norm_t, flags + 2);
        } else {
            pack_launch<float>(st, d + p.off_raw_q, n_query, p.nq_pad, len, p.ksteps, 0, pack_q, norm_q, flags + 1);
            pack_launch<float>(st, d + p.off_raw_t, n_train, p.nt_pad, len, p.ksteps, 1, pack_t, norm_t, flags + 2);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess && dtype == ALP_F32) {        // nothing is computed from values that are not bytes
        e = hipMemcpyAsync(flags_host, flags, sizeof(flags_host), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess && (flags_host[1] != KEY_NONE || flags_host[2] != KEY_NONE)) {
            const bool in_query = flags_host[1] != KEY_NONE;
            return fail(ALP_EINVAL, "alp_match_knn2: %s value at flat index %llu is not an integer in 0..255", in_query ? "query" : "train",
                        in_query ? flags_host[1] : flags_host[2]);
        }
    }
    if (e == hipSuccess) {
        KTimeScope kt;
        switch (p.ksteps) {
        case 1: walk_launch<1>(p, st, pack_q, pack_t, norm_q, norm_t, (int)n_train, partial); break;
        case 2: walk_launch<2>(p, st, pack_q, pack_t, norm_q, norm_t, (int)n_train, partial); break;
        case 3: walk_launch<3>(p, st, pack_q, pack_t, norm_q, norm_t, (int)n_train, partial); break;
        case 4: walk_launch<4>(p, st, pack_q, pack_t, norm_q, norm_t, (int)n_train, partial); break;
        case 6: walk_launch<6>(p, st, pack_q, pack_t, norm_q, norm_t, (int)n_train, partial); break;
        case 8: walk_launch<8>(p, st, pack_q, pack_t, norm_q, norm_t, (int)n_train, partial); break;
        case 12: walk_launch<12>(p, st, pack_q, pack_t, norm_q, norm_t, (int)n_train, partial); break;
        default: walk_launch<16>(p, st, pack_q, pack_t, norm_q, norm_t, (int)n_train, partial); break;
        }
        hipLaunchKernelGGL(match_merge_kernel, dim3((unsigned)((n_query + 255) / 256)), dim3(256), 0, st, (const u64 *)partial, p.splits,
                           (long long)p.nq_pad, (long long)n_query, ratio, idx_dev, dist2_dev, dist_dev, good_dev, flags);
        e = hipGetLastError();
    }
    if (e == hipSuccess && idx) e = hipMemcpyAsync(idx, idx_dev, (size_t)n_query * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && dist2) e = hipMemcpyAsync(dist2, dist2_dev, (size_t)n_query * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && dist) e = hipMemcpyAsync(dist, dist_dev, (size_t)n_query * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && good) e = hipMemcpyAsync(good, good_dev, (size_t)n_query, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(flags_host, flags, 8, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);          // before `dev` and the host arrays above go away
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(ALP_EHIP, "alp_match_knn2: %s", hipGetErrorString(e));
    if (n_good) *n_good = (int64_t)flags_host[0];
    return ALP_OK;
}
