// Part of alp_raster.hip (one translation unit, included inside namespace alp BEFORE the kernels' headers; not a
// stand-alone header): the host side of the development switches.
//
// Timing / census / stage-skipping builds used while the kernels were tuned (tools/build_variant.sh; DESIGN.md
// section 5 quotes their results).  Several produce WRONG IMAGES by design, so none of them can get into a
// library by accident: each needs -DALP_DEV next to it, the library reports what it was built with through
// alp_build_flags(), and tests/test_abi_symbols.py requires the shipped one to report nothing.  The development
// environment overrides (ALP_NEAR_PX, ALP_GRID_LANES, ALP_PATCH_NEAR / _FAR) are read by ALP_DEV builds only.
// ALP_NO_GRID_DETECT, ALP_QUEUE_CAP, ALP_NO_VIS_CACHE, ALP_NO_TILE_CULL and ALP_NO_OCCLUSION stay: they select
// between paths that produce the same image and are how the tests reach the index kernels, the queue growth,
// the full-frame path and the exact path without its culling.
//
// The frame code (alp_raster.hip) calls the reports of the two instrumented builds through three hooks --
// dev_report_first_round, dev_report_tiles, dev_report_frame -- which are empty in every other build.
#pragma once

#if defined(ALP_WG_TIMING) || defined(ALP_RASTER_STATS) || defined(VIS_PLAIN_STORE) || defined(VIS_NEVER) || defined(PARK_NOATOMIC) || \
    defined(PARKED_SKIP_CELLS) || defined(PARKED_SKIP_COOP) || defined(PARKED_SKIP_COOP4) || defined(GRID_STOP_AFTER) ||               \
    defined(GRID_NO_XCD_SWIZZLE)
#define ALP_DEV_SWITCHES 1
#ifndef ALP_DEV
#error "development switch given without -DALP_DEV: this would build a library that renders wrong images"
#endif
#endif
// (before the kernels' headers give the tunables their defaults)
#if defined(INLINE_LOG2) || defined(FAST_MAX) || defined(COOP_MIN_W) || defined(COOP_MIN_PIX) || defined(GT_W_LOG2) || defined(GT_H_LOG2) || \
    defined(HIZ_SPAN) || defined(GRID_WAVES_PER_EU) || defined(PATCH_MIN_FAST) || defined(PATCH_WORDS_NEAR) || defined(PATCH_WORDS_FAR) ||    \
    defined(RASTER_BLOCKS_PER_CU) || defined(RESOLVE_BLOCKS_PER_CU)
#define ALP_DEV_TUNABLES 1
#ifndef ALP_DEV
#error "tuning parameter overridden without -DALP_DEV"
#endif
#endif

const char *raster_dev_flags() {
    return ""
#ifdef ALP_DEV
           "ALP_DEV,"
#endif
#ifdef ALP_DEV_TUNABLES
           "tunables-overridden,"
#endif
#ifdef ALP_WG_TIMING
           "ALP_WG_TIMING,"
#endif
#ifdef ALP_RASTER_STATS
           "ALP_RASTER_STATS,"
#endif
#ifdef VIS_PLAIN_STORE
           "VIS_PLAIN_STORE(wrong image),"
#endif
#ifdef VIS_NEVER
           "VIS_NEVER(wrong image),"
#endif
#ifdef PARK_NOATOMIC
           "PARK_NOATOMIC(wrong image),"
#endif
#if defined(PARKED_SKIP_CELLS) || defined(PARKED_SKIP_COOP) || defined(PARKED_SKIP_COOP4)
           "PARKED_SKIP_*(wrong image),"
#endif
#ifdef GRID_STOP_AFTER
           "GRID_STOP_AFTER(wrong image),"
#endif
#ifdef GRID_NO_XCD_SWIZZLE
           "GRID_NO_XCD_SWIZZLE,"
#endif
        ;
}

#ifdef ALP_DEV
static const char *dev_getenv(const char *name) { return getenv(name); }
#else
static const char *dev_getenv(const char *) { return nullptr; }
#endif

// development: ALP_PATCH_NEAR / ALP_PATCH_FAR override the patch sizes (words; 0 switches the patches off)
static int patch_words_env(const char *name, int dflt) {
    if (const char *e = dev_getenv(name)) {
        const long w = atol(e);
        if (w >= 0 && w <= 5632) return (int)w;
    }
    return dflt;
}

struct TileCull;

#if defined(ALP_WG_TIMING) || defined(ALP_RASTER_STATS)
// the reports read the kernels' instrumentation and rerun two of the kernels: the stages they need come first here (and
// are not included a second time by alp_raster.hip)
#include "raster_common.h"
#include "raster_parked.h"
#include "raster_index.h"
#include "raster_plan.h"
#endif

// ---- ALP_WG_TIMING: duration of every workgroup of the first round, after its raster_grid_kernel was launched
// (counts[0]: the length of the NEAR list)
#ifdef ALP_WG_TIMING
static int dev_report_first_round(hipStream_t st, const unsigned *counts) {
    ALP_HIP(hipStreamSynchronize(st));
    unsigned hc[4];
    ALP_HIP(hipMemcpy(hc, counts, sizeof(hc), hipMemcpyDeviceToHost));
    std::vector<unsigned long long> tt(8 * (size_t)hc[0]);
    ALP_HIP(hipMemcpyFromSymbol(tt.data(), HIP_SYMBOL(g_wgtime), tt.size() * 8));
    unsigned long long t0 = ~0ull, t1 = 0;
    std::vector<double> dur;
    double phase[4] = {0, 0, 0, 0};
    for (unsigned i = 0; i < hc[0] && i < 131072; ++i) {
        t0 = std::min(t0, tt[8 * i]);
        t1 = std::max(t1, tt[8 * i + 4]);
        dur.push_back((tt[8 * i + 4] - tt[8 * i]) / 100.0);
        for (int k = 0; k < 4; ++k) phase[k] += (tt[8 * i + k + 1] - tt[8 * i + k]) / 100.0;
    }
    std::vector<double> sorted = dur;
    std::sort(sorted.begin(), sorted.end());
    double sum = 0;
    for (double d : dur) sum += d;
    fprintf(stderr, "[wg timing] first round: %u workgroups, span %.1f us, sum of durations %.0f us (vertices %.0f, classify %.0f, fast %.0f, slow %.0f), "
                    "median %.1f, p90 %.1f, p99 %.1f, max %.1f us\n", hc[0], (t1 - t0) / 100.0, sum, phase[0], phase[1], phase[2], phase[3],
            sorted[sorted.size() / 2], sorted[sorted.size() * 9 / 10], sorted[sorted.size() * 99 / 100], sorted.back());
    std::vector<unsigned> idx(dur.size());
    for (unsigned i = 0; i < idx.size(); ++i) idx[i] = i;
    std::partial_sort(idx.begin(), idx.begin() + std::min<size_t>(8, idx.size()), idx.end(), [&](unsigned a, unsigned b) { return dur[a] > dur[b]; });
    for (size_t k = 0; k < std::min<size_t>(8, idx.size()); ++k) {
        const unsigned i = idx[k];
        fprintf(stderr, "   wg %u: start +%.1f us, duration %.1f us = vertices %.1f + classify %.1f + fast %.1f + slow %.1f\n", i,
                (tt[8 * i] - t0) / 100.0, dur[i], (tt[8 * i + 1] - tt[8 * i]) / 100.0, (tt[8 * i + 2] - tt[8 * i + 1]) / 100.0,
                (tt[8 * i + 3] - tt[8 * i + 2]) / 100.0, (tt[8 * i + 4] - tt[8 * i + 3]) / 100.0);
    }
    return ALP_OK;
}
#else
static inline int dev_report_first_round(hipStream_t, const unsigned *) { return ALP_OK; }
#endif

#ifdef ALP_RASTER_STATS
// ---- ALP_RASTER_STATS, after the last raster launch of a grid frame: the lengths of the tile lists (counts: [0] near,
// [1] far, [2] far survivors) and, for a frame of two rounds, how many NEAR tiles an occlusion test against the FINISHED
// frame would drop (an upper bound for what more rounds could gain): full-frame pyramid, the NEAR list through
// tile_occlusion_kernel.
static int dev_report_tiles(alp_mesh *m, const View &v, const TileCull &cull, long long tiles, unsigned plan_grid, bool two_rounds,
                            unsigned *counts) {
    hipStream_t st = ctx().stream;
    unsigned *near_list = m->tile_lists, *second_list = near_list + 2 * tiles;
    unsigned hc[4];
    ALP_HIP(hipMemcpyAsync(hc, counts, sizeof(hc), hipMemcpyDeviceToHost, st));
    ALP_HIP(hipStreamSynchronize(st));
    fprintf(stderr, "[frame plan] tiles %lld: near %u, far %u of which %u survive the occlusion test\n", tiles, hc[0], hc[1], hc[2]);
    if (!two_rounds) return ALP_OK;
    const HizDims dm = hiz_dims(v.w, v.h);
    const unsigned full[4] = {65535u, (unsigned)v.w, 65535u, (unsigned)v.h}, zero = 0;
    ALP_HIP(hipMemcpy(counts + 4, full, sizeof(full), hipMemcpyHostToDevice));
    ALP_HIP(hipMemcpy(counts + 3, &zero, sizeof(zero), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(hiz_build_kernel, dim3((unsigned)dm.w[3], (unsigned)dm.h[3]), dim3(256), 0, st, m->vis, v.w, v.h, dm, m->hiz,
                       counts + 4);
    hipLaunchKernelGGL(tile_occlusion_kernel, dim3(plan_grid), dim3(256), 0, st, m->tile_bounds, cull, near_list, counts - 1, dm,
                       m->hiz, second_list, counts + 3);      // counts[-1 + 1] = the NEAR count
    unsigned left = 0;
    ALP_HIP(hipStreamSynchronize(st));
    ALP_HIP(hipMemcpy(&left, counts + 3, sizeof(left), hipMemcpyDeviceToHost));
    fprintf(stderr, "[frame plan] of the %u NEAR tiles %u survive a test against the finished frame\n", hc[0], left);
    return ALP_OK;
}

// ---- ALP_RASTER_STATS, after the resolve: the fragment / request census of the frame's kernels (g_rstat), then cleared
static int dev_report_frame(hipStream_t st) {
    unsigned long long hs[24 + 64], zero[24 + 64] = {0};
    ALP_HIP(hipStreamSynchronize(st));
    ALP_HIP(hipMemcpyFromSymbol(hs, HIP_SYMBOL(g_rstat), sizeof(hs)));
    ALP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_rstat), zero, sizeof(zero)));
    fprintf(stderr, "[raster stats] inline tris %llu | inline fragments by bbox width: 1px %llu, 2-3 %llu, 4-7 %llu, "
                    ">=8 %llu | coop tris %llu fragments %llu\n", hs[2], hs[3], hs[4], hs[5], hs[6], hs[8], hs[7]);
    static const char *bn[8] = {"<=512", "<=1K", "<=2K", "<=4K", "<=8K", "<=16K", "<=64K", ">64K"};
    for (int b = 0; b < 8; ++b)
        fprintf(stderr, "[footprint %6s px] tiles %7llu  area %10llu  cells FAST %9llu SLOW %9llu PARKED %8llu | box centres FAST %10llu "
                        "SLOW %10llu PARKED %10llu\n", bn[b], hs[24 + 8 * b], hs[25 + 8 * b], hs[26 + 8 * b], hs[27 + 8 * b], hs[28 + 8 * b],
                hs[29 + 8 * b], hs[30 + 8 * b], hs[31 + 8 * b]);
    fprintf(stderr, "[parked cells] %llu: box height <= 2: %llu, <= 4: %llu; width <= 4: %llu; centres in boxes %llu\n", hs[23], hs[19], hs[20],
            hs[21], hs[22]);
    fprintf(stderr, "[grid stats] (unused %llu) tiles drawn %llu | FAST cells %llu (wave rounds %llu) SLOW cells %llu (wave "
                    "rounds %llu)\n", hs[9], hs[10], hs[11], hs[13], hs[12], hs[14]);
    return ALP_OK;
}
#else
static inline int dev_report_tiles(alp_mesh *, const View &, const TileCull &, long long, unsigned, bool, unsigned *) { return ALP_OK; }
static inline int dev_report_frame(hipStream_t) { return ALP_OK; }
#endif
